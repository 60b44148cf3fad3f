"""GPU: sized batches -- cameras of different frame sizes in one detector batch.  Every comparison is integer or bit for bit:
  1. the sized ingest kernel (vc_frames_to_bgr_sized_host) against the NumPy definition (tests/yuv_ref.py) frame by frame, on random bytes,
     for one batch that mixes sizes, formats, geometries and alignments; the bytes of a cell beyond its frame keep the caller's pattern;
     a batch of equal sizes equals frames_to_bgr_kernel byte for byte;
  2. letterbox_frames_kernel (one launch, every frame its own geometry) against letterbox_kernel / letterbox_copy_kernel on each frame
     alone (vc_letterbox_host), fp32 and bf16, with and without the R / B swap, and in fp32 against the oracle;
  3. the crop kernel with the per-frame table against vc_embed + vc_embed_debug_input on each frame alone;
  4. staging: cells read back as the reference frames, the slot rules and refusals of vc_stream_stage_frames, dims that differ between
     stage / submit / run, a sized batch of uniform frames tracks like vc_stream_stage_frames + vc_stream_run_async_multi, and uniform
     and sized batches that take turns in every slot (one table pair per slot serves both) stage the reference frames;
  5. run_streams(mixed_sizes=True) over four cameras of four sizes equals, per camera, run_stream of that camera alone."""
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import yuv_ref  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from oracle import imageops as oi  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource, YuvFrameSource  # noqa: E402
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC = 8
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
VC_ERR_ARG, VC_ERR_STATE, VC_ERR_CAPACITY = 1, 3, 4
FILL = 0x5A


def geometry(kind, fmt, h, w):
    """tests/test_gpu_frame_table.py::geometry: tight; padded: 16-byte aligned pitches, chroma beyond pitch * h; padded_odd: nothing aligned"""
    if kind == "tight":
        return {}
    align = lambda v, a: (v + a - 1) // a * a
    if kind == "padded":
        py = align(w, 256) + 256
        pc = py if fmt == "nv12" else py // 2
        geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * align(h + 5, 16))
    else:
        py = w + 7
        pc = (w if fmt == "nv12" else w // 2) + 3
        geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * h + 13)
    if fmt == "i420":
        geo["offset_v"] = geo["offset_c"] + pc * (h // 2) + (32 if kind == "padded" else 5)
    return geo


def cell_bytes(dims):
    return (max(h * w * 3 for h, w in dims) + 15) // 16 * 16


# ---- 1. ingest ---------------------------------------------------------------------------------------------------------------------
def build_batch(rng, specs):
    """specs: per frame (h, w, type = None (BGR) or (fmt, matrix, full range), geometry kind, host address mod 16), all frames carved out
    of ONE buffer of uniformly random bytes.  Returns (keep-alive buffer, frame list, dims, per-frame reference (h, w, 3))."""
    sizes = [h * w * 3 if typ is None else yuv_ref.batch_bytes(1, h, w, typ[0], **geometry(kind, typ[0], h, w)) for h, w, typ, kind, _ in specs]
    buf = rng.integers(0, 256, sum(sizes) + 32 * len(specs) + 16, dtype=np.uint8)
    frames, want, pos = [], [], 0
    for (h, w, typ, kind, mod), n in zip(specs, sizes):
        pos += (mod - (buf.ctypes.data + pos)) % 16                                       # the next address congruent to `mod`
        data = buf[pos:pos + n]
        assert data.ctypes.data % 16 == mod
        if typ is None:
            frames.append(E.frame_src("bgr_host", data.ctypes.data))
            want.append(data.reshape(h, w, 3))
        else:
            fmt, matrix, full = typ
            geo = geometry(kind, fmt, h, w)
            frames.append(E.frame_src("yuv_host", data.ctypes.data, E.yuv_desc(fmt, matrix, full, **geo)))
            want.append(yuv_ref.yuv_to_bgr(data, 1, h, w, fmt, matrix, full, **geo)[0])
        pos += n
    return buf, frames, [(h, w) for h, w, *_ in specs], want


def mixed_specs():
    """sizes 6x18 (a partial 16-pixel group), 48x64 (the 16-byte path), 36x64 and 38x66 x NV12 / I420 / BGR x tight / padded_odd x address = 0 / 5
    mod 16; the largest frame is neither first nor last, consecutive frames differ in size"""
    sizes = [(6, 18), (48, 64), (36, 64), (38, 66)]
    types_ = [("nv12", "bt601", False), ("i420", "bt709", True), None, ("i420", "bt601", False), ("nv12", "bt709", True)]
    out = []
    for i in range(24):
        h, w = sizes[i % 4]
        out.append((h, w, types_[i % 5], ("tight", "padded_odd")[(i // 4) % 2], (0, 5)[(i // 2) % 2]))
    return out


def test_sized_ingest_matches_the_definition_frame_by_frame():
    specs = mixed_specs()
    assert {(s[0], s[1]) for s in specs} == {(6, 18), (48, 64), (36, 64), (38, 66)} and {s[4] for s in specs} == {0, 5}
    assert any(s[2] is None for s in specs) and {s[2][0] for s in specs if s[2]} == {"nv12", "i420"} and {s[3] for s in specs} == {"tight", "padded_odd"}
    buf, frames, dims, want = build_batch(np.random.default_rng(2417), specs)
    off, total, cell, net = E.frames_layout_sized(frames, dims, 1)
    assert cell == cell_bytes(dims) == 48 * 64 * 3 and 38 * 66 * 3 % 16 != 0              # the largest frame; frames that end off a 16-byte boundary inside their cells
    cells = np.full(len(specs) * cell, FILL, np.uint8)
    E.frames_to_bgr_sized(frames, dims, cells)
    cells = cells.reshape(len(specs), cell)
    for f, (h, w) in enumerate(dims):
        np.testing.assert_array_equal(cells[f, : h * w * 3].reshape(h, w, 3), want[f], err_msg=f"frame {f}: {specs[f]}")
        assert (cells[f, h * w * 3:] == FILL).all(), f"frame {f}: the kernel wrote beyond the frame inside its cell"


def test_sized_ingest_of_equal_sizes_equals_the_uniform_kernel():
    h, w = 48, 64
    types_ = [("nv12", "bt601", False), None, ("i420", "bt709", True), ("nv12", "bt709", False), None]
    specs = [(h, w, types_[i % 5], ("tight", "padded_odd", "padded")[i % 3], (0, 5)[i % 2]) for i in range(10)]
    buf, frames, dims, want = build_batch(np.random.default_rng(4864), specs)
    old = E.frames_to_bgr(frames, h, w)
    cells = np.full(len(specs) * h * w * 3, FILL, np.uint8)                                # 9216-byte frames: the cells are the packed batch
    E.frames_to_bgr_sized(frames, dims, cells)
    np.testing.assert_array_equal(cells.reshape(old.shape), old)
    np.testing.assert_array_equal(old, np.stack(want))


# ---- 2. letterbox ------------------------------------------------------------------------------------------------------------------
LANDSCAPE = [(36, 64), (37, 64), (18, 32), (54, 96), (37, 65), (48, 64)]      # copy; copy, top 13 / bottom 14; x2 up; x2/3 down; odd, resize by a hair; copy
PORTRAIT = [(64, 36), (65, 37), (96, 54)]                                      # left padding 14


def random_frames(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


@pytest.fixture(scope="module")
def letterbox_alone():
    """vc_letterbox_host of every frame of the two batches alone, computed once: {(batch, precision, swap): [per frame (64, 64, 3)]}"""
    out = {}
    for name, sizes in (("landscape", LANDSCAPE), ("portrait", PORTRAIT)):
        frames = random_frames(sizes, len(sizes))
        for prec in ("f32", "bf16"):
            for swap in (False, True):
                out[name, prec, swap] = [E.letterbox(np.ascontiguousarray(f[:, :, ::-1]) if swap else f, 64, 64, prec) for f in frames]
        out[name] = frames
    return out


def test_letterbox_geometries_are_the_cases_they_claim():
    geo = {hw: oi.letterbox_geometry(*hw, 64, 64) for hw in LANDSCAPE + PORTRAIT}        # unpad_w, unpad_h, top, bottom, left, right
    assert geo[(36, 64)][:4] == (64, 36, 14, 14) and geo[(37, 64)][:4] == (64, 37, 13, 14) and geo[(48, 64)][:4] == (64, 48, 8, 8)
    assert geo[(18, 32)][:2] == (64, 36) and geo[(54, 96)][:2] == (64, 36) and geo[(37, 65)][:2] == (64, 36)
    assert all(geo[hw][4] == 14 for hw in PORTRAIT)


@pytest.mark.parametrize("batch", ["landscape", "portrait"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("swap", [False, True])
def test_letterbox_frames_equals_the_kernel_on_each_frame_alone(letterbox_alone, batch, prec, swap):
    frames = letterbox_alone[batch]
    got = E.letterbox_frames(frames, 64, 64, swap_rb=swap, precision=prec)
    for f, im in enumerate(frames):
        np.testing.assert_array_equal(got[f].view(np.uint32), letterbox_alone[batch, prec, swap][f].view(np.uint32), err_msg=f"frame {f} {im.shape}")
        if prec == "f32":                                                                  # tests/test_gpu_kernels.py::test_letterbox
            src = np.ascontiguousarray(im[:, :, ::-1]) if swap else im
            np.testing.assert_array_equal(got[f], oi.letterbox(src, 64, 64).astype(np.float32) / np.float32(255), err_msg=f"frame {f} {im.shape}")


def test_letterbox_frames_strides_over_a_long_batch(letterbox_alone):
    """more frames than the capped grid has room for in one sweep: every lane makes several items, frames repeat the six geometries"""
    frames = letterbox_alone["landscape"]
    order = [(7 * i) % 6 for i in range(1100)]
    got = E.letterbox_frames([frames[j] for j in order], 64, 64, swap_rb=True, precision="bf16")
    want = np.stack(letterbox_alone["landscape", "bf16", True])
    np.testing.assert_array_equal(got.view(np.uint32), want[order].view(np.uint32))


# ---- 3. crops ----------------------------------------------------------------------------------------------------------------------
def test_crop_table_equals_embed_on_each_frame_alone():
    sizes = [(90, 120), (121, 77), (64, 200)]
    frames = random_frames(sizes, 31)
    rng = np.random.default_rng(5)
    boxes, fob = [], []
    for f, (h, w) in enumerate(sizes):
        bx = [[w - 10.0, h / 2, 40.0, 30.0],                      # clamped at the frame's own right edge: x2 = w - 1
              [w / 2, h - 6.0, 33.0, 28.0],                       # ... and at its own bottom edge: y2 = h - 1
              [35.0, 32.0, 50.0, 50.0]]                           # exactly 50 x 50: no resize
        for _ in range(5):
            cw, ch = rng.uniform(8, w * 0.8), rng.uniform(8, h * 0.8)
            bx.append([rng.uniform(cw / 2, w - cw / 2), rng.uniform(ch / 2, h - ch / 2), cw, ch])
        boxes += bx
        fob += [f] * len(bx)
    boxes, fob = np.array(boxes), np.array(fob)
    order = rng.permutation(len(boxes))                            # boxes of the frames interleaved, as in no particular order
    boxes, fob = boxes[order], fob[order]
    got = E.crop_resize_frames(frames, fob, boxes)
    eng = E.Engine(None, synth_reid(1702), precision="f32", max_batch=1, max_frame_hw=(128, 200), max_crops=64, max_tracks=64, nn_budget_cap=10)
    try:
        for f, im in enumerate(frames):
            sel = np.flatnonzero(fob == f)
            eng.embed(im, boxes[sel])
            np.testing.assert_array_equal(got[sel].view(np.uint32), eng.embed_input(len(sel)).view(np.uint32), err_msg=f"frame {f} {im.shape}")
    finally:
        eng.close()
    assert np.isfinite(got).all() and got.std() > 0.1


# ---- 4. staging on an engine -------------------------------------------------------------------------------------------------------
B, H, W, NB = 4, 360, 640, 3
MAX_HW = (540, 960)


@pytest.fixture(scope="module")
def staged():
    import torch
    clip = synth_frames(B * NB, H, W, n_obj=8, seed=13)
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", num_classes=NC, max_batch=B, max_frame_hw=MAX_HW, max_crops=B * 300, max_tracks=2048, nn_budget_cap=60)
    trk = [eng.tracker_create(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
           for _ in range(NC)]
    s = types.SimpleNamespace(eng=eng, trk=trk, clip=clip, host_bgr=torch.from_numpy(clip).pin_memory(), dev_bgr=torch.from_numpy(clip).cuda())
    yield s
    eng.close()


def read_bytes(p, n):
    import torch
    view = types.SimpleNamespace(__cuda_array_interface__={"shape": (n,), "typestr": "|u1", "data": (p, False), "version": 2})
    return torch.as_tensor(view, device="cuda").clone().cpu().numpy()


def code_of(fn):
    with pytest.raises(L.VcError) as ei:
        fn()
    return ei.value.code


def four_sizes(clip):
    """four frames of four sizes that run at 384 x 640, from four kinds of source: (keep-alive, frames, dims, reference frames)"""
    import torch
    dims = [(360, 640), (180, 320), (362, 640), (540, 960)]
    rng = np.random.default_rng(44)
    nv12 = bgr_to_yuv420(clip[0:1], "nv12")[0]
    d0 = torch.zeros(nv12.size + 1, dtype=torch.uint8, device="cuda")                      # NV12 in device memory at an address = 1 mod 16
    d0[1:] = torch.from_numpy(nv12).cuda()
    geo = geometry("padded_odd", "i420", 180, 320)
    raw1 = rng.integers(0, 256, yuv_ref.batch_bytes(1, 180, 320, "i420", **geo), dtype=np.uint8)
    h1 = torch.from_numpy(raw1).pin_memory()                                               # padded I420, BT.709 full range, pinned host memory
    f2 = rng.integers(0, 256, (362, 640, 3), dtype=np.uint8)
    f3 = rng.integers(0, 256, (540, 960, 3), dtype=np.uint8)
    d2, h3 = torch.from_numpy(f2).cuda(), torch.from_numpy(f3).pin_memory()
    frames = [E.frame_src("yuv_dev", d0[1:].data_ptr(), E.yuv_desc("nv12")), E.frame_src("yuv_host", h1.data_ptr(), E.yuv_desc("i420", "bt709", True, **geo)),
              E.frame_src("bgr_dev", d2.data_ptr()), E.frame_src("bgr_host", h3.data_ptr())]
    want = [yuv_ref.yuv_to_bgr(nv12, 1, 360, 640, "nv12")[0], yuv_ref.yuv_to_bgr(raw1, 1, 180, 320, "i420", "bt709", True, **geo)[0], f2, f3]
    return (d0, h1, d2, h3), frames, dims, want


def test_staged_sized_batch_is_the_reference_frames_in_their_cells(staged):
    import torch
    eng, trk = staged.eng, staged.trk
    keep, frames, dims, want = four_sizes(staged.clip)
    cell = cell_bytes(dims)
    eng.stream_reset()
    for t in trk:
        eng.tracker_reset(t)
    p = eng.stream_stage_frames_sized(frames, dims)
    # other dims than the staged ones are refused, by submit and by run, and leave the batch where it was
    other = [dims[0], dims[1], dims[0], dims[3]]
    assert code_of(lambda: eng.stream_submit_sized(p, other)) == VC_ERR_ARG
    assert code_of(lambda: eng.stream_submit_sized(p, dims[:3])) == VC_ERR_ARG
    assert code_of(lambda: eng.stream_submit(p, B, *dims[3])) == VC_ERR_ARG
    eng.stream_submit_sized(p, dims)
    many = np.array([[eng.tracker_create(nn_budget=60) for _ in range(NC)] for _ in range(4)], np.int32)
    with pytest.raises(L.VcError, match="differ from those the batch was submitted with") as ei:
        eng.stream_run_async_multi_sized(many, [0, 1, 2, 3], p, other)
    assert ei.value.code == VC_ERR_ARG
    # two sizes for one camera inside a batch
    with pytest.raises(L.VcError, match="frame 1: camera 0 delivers 180x320") as ei:
        eng.stream_run_async_multi_sized(many, [0, 0, 1, 1], p, dims)
    assert ei.value.code == VC_ERR_ARG
    eng.stream_run_async_multi_sized(many, [0, 1, 2, 3], p, dims)
    rows, fidx, ndet = eng.stream_collect()
    torch.cuda.synchronize()
    got = read_bytes(p, B * cell).reshape(B, cell)
    for f, (h, w) in enumerate(dims):
        np.testing.assert_array_equal(got[f, : h * w * 3].reshape(h, w, 3), want[f], err_msg=f"frame {f}")
    assert ndet.shape == (B,) and len(rows) == len(fidx)
    for t in many.reshape(-1):
        eng.tracker_destroy(int(t))
    del keep


def test_sized_staging_follows_the_slot_rules(staged):
    eng, trk = staged.eng, staged.trk
    fb = H * W * 3
    kinds = ["bgr_host", "bgr_dev"]
    base = {"bgr_host": staged.host_bgr.data_ptr(), "bgr_dev": staged.dev_bgr.data_ptr()}
    sl = lambda i: slice(i * B, (i + 1) * B)
    uni = [(H, W)] * B

    def frames_of(i, b=B):
        return [E.frame_src(kinds[(i + j) % 2], base[kinds[(i + j) % 2]] + ((i * B + j) % (B * NB)) * fb) for j in range(b)]

    eng.stream_reset()
    # a fifth staged batch without a submit is refused, by whichever staging call; vc_stream_reset clears the staged batches
    for n in range(4):
        eng.stream_stage_frames_sized(frames_of(n), uni)
    assert code_of(lambda: eng.stream_stage_frames_sized(frames_of(4), uni)) == VC_ERR_STATE
    assert code_of(lambda: eng.stream_stage_frames(frames_of(4), H, W)) == VC_ERR_STATE
    assert code_of(lambda: eng.stream_stage_host(staged.host_bgr[sl(0)].data_ptr(), B, H, W)) == VC_ERR_STATE
    eng.stream_reset()
    # refusals come before a slot is taken: a bad descriptor in frame 2, a frame of another network shape, too many or too large frames
    bad = frames_of(0)
    bad[2] = E.frame_src("yuv_dev", staged.dev_bgr.data_ptr(), E.yuv_desc(pitch_y=W - 2))
    with pytest.raises(L.VcError, match="frame 2: pitch_y") as ei:
        eng.stream_stage_frames_sized(bad, uni)
    assert ei.value.code == VC_ERR_ARG
    with pytest.raises(L.VcError, match="frame 3: 480x640 runs at 480x640, frame 0 at 384x640") as ei:
        eng.stream_stage_frames_sized(frames_of(0), uni[:3] + [(480, 640)])
    assert ei.value.code == VC_ERR_ARG
    assert code_of(lambda: eng.stream_stage_frames_sized(frames_of(0, B + 1), [(H, W)] * (B + 1))) == VC_ERR_CAPACITY
    assert code_of(lambda: eng.stream_stage_frames_sized(frames_of(0), uni[:3] + [(720, 1280)])) == VC_ERR_CAPACITY
    for n in range(4):
        eng.stream_stage_frames_sized(frames_of(n), uni)
    assert code_of(lambda: eng.stream_stage_frames_sized(frames_of(4), uni)) == VC_ERR_STATE
    eng.stream_reset()

    tids = np.array([trk], np.int32)
    cams = np.zeros(B, np.int32)

    def run(sized_of):
        """stage(i + 2); submit(i + 1); run(i); collect(i - 1); batch i goes the sized way when sized_of(i)"""
        for t in trk:
            eng.tracker_reset(t)
        ptrs, got = {}, []
        stage = lambda i: ptrs.__setitem__(i, eng.stream_stage_frames_sized(frames_of(i), uni) if sized_of(i) else eng.stream_stage_frames(frames_of(i), H, W))
        submit = lambda i: eng.stream_submit_sized(ptrs[i], uni) if sized_of(i) else eng.stream_submit(ptrs[i], B, H, W)
        stage(0); stage(1)
        submit(0)
        for i in range(NB):
            if i + 2 < NB:
                stage(i + 2)
            if i + 1 < NB:
                submit(i + 1)
            if sized_of(i):
                eng.stream_run_async_multi_sized(tids, cams, ptrs[i], uni)
            else:
                eng.stream_run_async_multi(tids, cams, ptrs[i], B, H, W)
            if i > 0:
                got.append(eng.stream_collect())
        got.append(eng.stream_collect())
        return got

    uniform = run(lambda i: False)
    assert sum(len(r[0]) for r in uniform) > 20
    for name, got in {"sized": run(lambda i: True), "alternating": run(lambda i: i % 2 == 0)}.items():
        for (r0, f0, n0), (r1, f1, n1) in zip(uniform, got):
            np.testing.assert_array_equal(n0, n1, err_msg=name)
            np.testing.assert_array_equal(f0, f1, err_msg=name)
            np.testing.assert_array_equal(r0, r1, err_msg=name)


def test_uniform_and_sized_batches_share_the_slot_tables(staged):
    """Every ingest slot has ONE pinned / device table pair that serves both kinds of staged batch.  Twelve batches in the kinds
    u s s u  s u u s  u s s u (u: stream_stage_frames, s: stream_stage_frames_sized) go through stage i + 2, submit i + 1, run i,
    collect i - 1: with four slots, whatever the slot phase at entry, every slot holds u -> s -> u or s -> u -> s.  After each collect
    the slot's bytes are the reference frames (uniform tight, sized in their cells), and all rows equal those of the same twelve
    batches submitted as plain device batches of the reference frames (no staging, no table)."""
    import torch
    eng = staged.eng
    pattern = "ussusuusussu"
    nb = len(pattern)
    slots = [[pattern[i] for i in range(nb) if i % 4 == ph] for ph in range(4)]
    assert all(sl in (["u", "s", "u"], ["s", "u", "s"]) for sl in slots)
    keep, sized_frames, dims, sized_want = four_sizes(staged.clip)
    cell = cell_bytes(dims)
    uni = [(H, W)] * B
    fb = H * W * 3
    nv12 = bgr_to_yuv420(staged.clip, "nv12")
    host_nv12 = torch.from_numpy(nv12).pin_memory()
    ref_clip = staged.clip.copy()
    ref_clip[0::2] = yuv_ref.yuv_to_bgr(nv12, len(nv12), H, W, "nv12")[0::2]          # even frames arrive as NV12, odd ones as BGR
    # the uniform batches walk through the clip in order (and once more): B is even, so the parity of j is that of the clip index
    clip_idx = lambda i: [(pattern[:i].count("u") * B + j) % (B * NB) for j in range(B)]

    def uniform_frames(i):
        return [E.frame_src("yuv_host", host_nv12[k].data_ptr(), E.yuv_desc("nv12")) if k % 2 == 0 else E.frame_src("bgr_dev", staged.dev_bgr.data_ptr() + k * fb)
                for k in clip_idx(i)]

    # the reference batches in device memory: uniform ones tight, the sized one in its cells
    ref_uniform = {i: torch.from_numpy(ref_clip[clip_idx(i)]).cuda() for i in range(nb) if pattern[i] == "u"}
    cells = np.zeros((B, cell), np.uint8)
    for f, (h, w) in enumerate(dims):
        cells[f, : h * w * 3] = sized_want[f].reshape(-1)
    ref_sized = torch.from_numpy(cells).cuda()
    many = np.array([[eng.tracker_create(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
                      for _ in range(NC)] for _ in range(4)], np.int32)
    own_cam, one_cam = np.arange(B, dtype=np.int32), np.zeros(B, np.int32)

    def run(staging):
        eng.stream_reset()
        for t in many.reshape(-1):
            eng.tracker_reset(int(t))
        ptrs, got = {}, []

        def stage(i):
            if not staging:
                ptrs[i] = (ref_sized if pattern[i] == "s" else ref_uniform[i]).data_ptr()
            elif pattern[i] == "s":
                ptrs[i] = eng.stream_stage_frames_sized(sized_frames, dims)
            else:
                ptrs[i] = eng.stream_stage_frames(uniform_frames(i), H, W)

        submit = lambda i: eng.stream_submit_sized(ptrs[i], dims) if pattern[i] == "s" else eng.stream_submit(ptrs[i], B, H, W)

        def collect(i):
            got.append(eng.stream_collect())
            if not staging:
                return
            torch.cuda.synchronize()                                                    # the slot is restaged by stage(i + 4) at the earliest
            if pattern[i] == "s":
                slot = read_bytes(ptrs[i], B * cell).reshape(B, cell)
                for f, (h, w) in enumerate(dims):
                    np.testing.assert_array_equal(slot[f, : h * w * 3].reshape(h, w, 3), sized_want[f], err_msg=f"batch {i} (sized) frame {f}")
            else:
                np.testing.assert_array_equal(read_bytes(ptrs[i], B * fb).reshape(B, H, W, 3), ref_clip[clip_idx(i)], err_msg=f"batch {i} (uniform)")

        stage(0); stage(1)
        submit(0)
        for i in range(nb):
            if i + 2 < nb:
                stage(i + 2)
            if i + 1 < nb:
                submit(i + 1)
            if pattern[i] == "s":
                eng.stream_run_async_multi_sized(many, own_cam, ptrs[i], dims)
            else:
                eng.stream_run_async_multi(many, one_cam, ptrs[i], B, H, W)
            if i > 0:
                collect(i - 1)
        collect(nb - 1)
        return got

    plain, mixed = run(False), run(True)
    assert sum(len(r[0]) for i, r in enumerate(plain) if pattern[i] == "u") > 0          # not empty against empty
    for i, ((r0, f0, n0), (r1, f1, n1)) in enumerate(zip(plain, mixed)):
        np.testing.assert_array_equal(n0, n1, err_msg=f"batch {i} ({pattern[i]})")
        np.testing.assert_array_equal(f0, f1, err_msg=f"batch {i} ({pattern[i]})")
        np.testing.assert_array_equal(r0, r1, err_msg=f"batch {i} ({pattern[i]})")
    eng.stream_reset()
    for t in many.reshape(-1):
        eng.tracker_destroy(int(t))
    del keep


# ---- 5. run_streams ----------------------------------------------------------------------------------------------------------------
def whole_frame_zone(golden_dir, tmp_path, name, h, w):
    """tests/test_gpu_yuv_ingest.py::whole_frame_zone: cam_04's directions with the zone polygon widened to the frame"""
    with open(os.path.join(golden_dir, name)) as f:
        z = json.load(f)
    for sh in z["shapes"]:
        if sh["label"] == "zone":
            sh["points"] = [[0.0, 0.0], [float(w), 0.0], [float(w), float(h)], [0.0, float(h)]]
    path = str(tmp_path / f"zone_{h}x{w}.json")
    with open(path, "w") as f:
        json.dump(z, f)
    return path


def assert_same_output(got, want, case):
    """tests/test_gpu_yuv_ingest.py::assert_same_output: one dict per CSV line, all of it equal, and the counts"""
    rows, counts = got
    ref_rows, ref_counts = want
    assert len(rows) == len(ref_rows), case
    for r, q in zip(rows, ref_rows):
        assert set(r) == set(q), case
        for k in r:
            np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(q[k]), err_msg=f"{case}: {k}")
    assert counts == ref_counts, case


CAM2 = (12, 7, 6)       # frames, seed, objects of the 540x960 camera
CAM3 = (16, 5, 6)       # ... of the 362x640 camera


def four_cameras():
    """(sources, the BGR frames each camera's source decodes to, sizes): 360x640 BGR, 180x320 tight NV12, 540x960 padded I420 BT.709 full
    range, 362x640 BGR; 12..18 frames each.  The clips are chosen so that the reference pipeline alone (oracle.pipeline.run_video on the
    decoded frames, checked on the CPU) tracks >= 10 CSV rows per camera and clamps boxes of the 180x320 camera at x2 = 319 / y2 = 179."""
    sizes = [(360, 640), (180, 320), (540, 960), (362, 640)]
    c0 = synth_frames(18, 360, 640, n_obj=6, seed=3)
    nv12 = bgr_to_yuv420(synth_frames(14, 180, 320, n_obj=6, seed=3), "nv12")
    geo = geometry("padded", "i420", 540, 960)
    geo["frame_stride"] = yuv_ref.batch_bytes(1, 540, 960, "i420", **geo) + 4096
    big = synth_frames(CAM2[0], 180, 320, n_obj=CAM2[2], seed=CAM2[1]).repeat(3, axis=1).repeat(3, axis=2)      # a 180x320 scene at 540x960
    tight = bgr_to_yuv420(big, "i420", "bt709", True)
    i420 = pad_surfaces_i420(tight, 540, 960, geo)
    c3 = synth_frames(CAM3[0], 362, 640, n_obj=CAM3[2], seed=CAM3[1])
    sources = [FrameSource(c0), YuvFrameSource(nv12, 180, 320, fmt="nv12"),
               YuvFrameSource(i420, 540, 960, fmt="i420", matrix="bt709", full_range=True, pitch=geo["pitch_y"], pitch_c=geo["pitch_c"],
                              offset_c=geo["offset_c"], offset_v=geo["offset_v"], frame_stride=geo["frame_stride"]),
               FrameSource(c3)]
    expected = [c0, yuv_ref.yuv_to_bgr(nv12, 14, 180, 320, "nv12"), yuv_ref.yuv_to_bgr(i420, CAM2[0], 540, 960, "i420", "bt709", True, **geo), c3]
    return sources, expected, sizes


def pad_surfaces_i420(tight, h, w, geo):
    """tests/test_gpu_frame_table.py::pad_surfaces for I420: tightly packed frames (T, h * w * 3 / 2) laid out as `geo` (zero padding)"""
    t, py, pc, oc, ov, q = len(tight), geo["pitch_y"], geo["pitch_c"], geo["offset_c"], geo["offset_v"], h * w // 4
    surf = np.zeros((t, geo["frame_stride"]), np.uint8)
    surf[:, : py * h].reshape(t, h, py)[:, :, :w] = tight[:, : h * w].reshape(t, h, w)
    surf[:, oc: oc + pc * (h // 2)].reshape(t, h // 2, pc)[:, :, : w // 2] = tight[:, h * w: h * w + q].reshape(t, h // 2, w // 2)
    surf[:, ov: ov + pc * (h // 2)].reshape(t, h // 2, pc)[:, :, : w // 2] = tight[:, h * w + q:].reshape(t, h // 2, w // 2)
    return surf


def test_run_streams_of_mixed_sizes_equals_separate_runs(golden_dir, tmp_path):
    """fp32: conv numerics do not depend on the tile configuration a batch size selects (test_run_streams_of_mixed_cameras_equals_separate_runs)"""
    names = ["cam_00", "cam_01", "cam_02", "cam_03"]
    sources, expected, sizes = four_cameras()
    zones = [whole_frame_zone(golden_dir, tmp_path, "cam_04_halfres.json", h, w) for h, w in sizes]
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="f32", num_classes=NC, max_batch=5, max_frame_hw=MAX_HW, max_crops=5 * 300, max_tracks=4096, nn_budget_cap=60,
                   max_trackers=4 * NC)
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path))
    pipe = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": TRACK_CFG} for n in names + ["cam_04"]}}, engine=eng, class_names=[f"c{i}" for i in range(NC)])
    # a camera of another network shape is refused before any GPU work; without the opt-in the old rule holds
    with pytest.raises(ValueError, match="own call"):
        pipe.run_streams(sources + [FrameSource(synth_frames(2, 480, 640, n_obj=2, seed=4))], names + ["cam_04"], zones + [zones[0]], batch=4, mixed_sizes=True)
    with pytest.raises(ValueError, match="one size"):
        pipe.run_streams(sources, names, zones, batch=4, host_frames=True)
    want = [pipe.run_stream(FrameSource(expected[c]), names[c], zones[c], batch=4, asynchronous=True) for c in range(4)]
    for c in range(4):
        assert len(want[c][0]) >= 10, (c, len(want[c][0]))                                # no camera passes empty against empty
    # a clamp to the batch's largest frame (959 x 539) instead of the camera's own would differ here
    assert any(r["box"][2] == 319 or r["box"][3] == 179 for r in want[1][0])
    for batch in (4, 5):
        for host_frames in (False, True):
            got = pipe.run_streams(sources, names, zones, batch=batch, host_frames=host_frames, mixed_sizes=True)
            for c in range(4):
                assert_same_output(got[c], want[c], f"camera {c} batch={batch} host_frames={host_frames}")
    eng.close()
