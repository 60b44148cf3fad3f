"""GPU: multi-camera ingest -- one batch from per-frame sources of mixed formats (frames_to_bgr_kernel, vc_stream_stage_frames,
CountingPipeline.run_streams over per-camera clips).  The arithmetic is integer, so every comparison is bit for bit:
  * the kernel (vc_frames_to_bgr_host) against the NumPy definition (tests/yuv_ref.py) frame by frame, on uniformly random bytes, for
    batches that mix both formats, both matrices, both ranges and BGR copies, the 16-byte path and the generic one in ONE launch, and
    against yuv_to_bgr_kernel on a batch both can express;
  * a staged batch of four frames from four kinds of source is the four reference frames, and tracks like them;
  * the slot rules of vc_stream_stage_host hold, refusals take no slot, and the call mixes with the other staging calls;
  * run_streams over a BGR, a tight NV12 and a padded I420 camera of different lengths equals the separate single-camera runs."""
import ctypes as C
import itertools
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import yuv_ref  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource, YuvFrameSource  # noqa: E402
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC = 8
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
VC_ERR_ARG, VC_ERR_STATE, VC_ERR_CAPACITY = 1, 3, 4
GUARD = 4096
# the nine frame types: {nv12, i420} x {bt601, bt709} x {limited, full}, and a BGR frame (None)
TYPES = list(itertools.product(("nv12", "i420"), ("bt601", "bt709"), (False, True))) + [None]
KINDS = ("tight", "padded", "padded_odd")


# ---- kernel ------------------------------------------------------------------------------------------------------------------------
def geometry(kind, fmt, h, w):
    """tests/test_gpu_yuv_ingest.py::geometry: tight; padded: 16-byte aligned pitches, chroma beyond pitch * h, a gap between frames (a
    decoder surface); padded_odd: the same with nothing aligned (generic path at every width)."""
    if kind == "tight":
        return {}
    align = lambda v, a: (v + a - 1) // a * a
    if kind == "padded":
        py = align(w, 256) + 256
        pc = py if fmt == "nv12" else py // 2
        geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * align(h + 5, 16))
        gap = 4096
    else:
        py = w + 7
        pc = (w if fmt == "nv12" else w // 2) + 3
        geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * h + 13)
        gap = 101
    if fmt == "i420":
        geo["offset_v"] = geo["offset_c"] + pc * (h // 2) + (32 if kind == "padded" else 5)
    geo["frame_stride"] = yuv_ref.batch_bytes(1, h, w, fmt, **geo) + gap
    return geo


def build_batch(rng, h, w, specs):
    """specs: per frame (type, geometry kind, host address mod 16).  All frames are carved out of ONE buffer of uniformly random bytes
    (padding included).  Returns (keep-alive buffer, frame list, reference (b, h, w, 3))."""
    sizes = []
    for typ, kind, _ in specs:
        sizes.append(h * w * 3 if typ is None else yuv_ref.batch_bytes(1, h, w, typ[0], **geometry(kind, typ[0], h, w)))
    buf = rng.integers(0, 256, sum(sizes) + 32 * len(specs) + 16, dtype=np.uint8)
    frames, want, pos = [], [], 0
    for (typ, kind, mod), n in zip(specs, sizes):
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
    return buf, frames, np.stack(want)


def convert_with_guards(frames, h, w):
    """vc_frames_to_bgr_host writing into the middle of a larger host array: (images, guard bytes before, guard bytes after)."""
    n = len(frames) * h * w * 3
    out = np.full(n + 2 * GUARD, 0x5A, np.uint8)
    E.frames_to_bgr(frames, h, w, out=out[GUARD:GUARD + n])
    return out[GUARD:GUARD + n].reshape(len(frames), h, w, 3), out[:GUARD], out[GUARD + n:]


def kernel_cases():
    cases = {}
    # every frame a single active lane, consecutive frames of different types, more frames than a wavefront has lanes
    cases["2x2 b=70"] = (2, 2, [(TYPES[f % 9], KINDS[(f + f // 9) % 3], (5 * f) % 16) for f in range(70)])
    # the generic path with a partial 16-pixel group
    cases["6x18 b=9"] = (6, 18, [(TYPES[f], KINDS[(f + 1) % 3], (3 * f) % 16) for f in range(9)])
    # even frames: aligned address, tight or padded geometry -> the 16-byte path; odd frames: address = 1 mod 16 -> the generic path
    cases["48x64 b=9"] = (48, 64, [(TYPES[f], ("tight", "padded")[(f // 2) % 2], 0) if f % 2 == 0 else (TYPES[f], KINDS[(f // 2) % 3], 1) for f in range(9)])
    cases["360x640 b=3"] = (360, 640, [(("nv12", "bt601", False), "padded", 0), (None, "tight", 0), (("i420", "bt709", True), "tight", 0)])
    return cases


@pytest.mark.parametrize("name", list(kernel_cases()))
def test_kernel_matches_the_definition_frame_by_frame(name):
    h, w, specs = kernel_cases()[name]
    rng = np.random.default_rng([h, w, len(specs)])
    buf, frames, want = build_batch(rng, h, w, specs)
    got, before, after = convert_with_guards(frames, h, w)
    for f, spec in enumerate(specs):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{name} frame {f}: {spec}")
    assert (before == 0x5A).all() and (after == 0x5A).all(), name
    np.testing.assert_array_equal(E.frames_to_bgr(frames, h, w), want, err_msg=name)           # the wrapper that allocates its result


@pytest.mark.parametrize("h,w,kind", [(48, 64, "padded"), (48, 64, "tight"), (6, 18, "padded_odd")])
def test_kernel_equals_yuv_to_bgr_kernel_on_a_contiguous_batch(h, w, kind):
    """frames that all share one contiguous NV12 layout: what the existing kernel converts from one base and a stride"""
    b, rng = 5, np.random.default_rng([h, w])
    geo = geometry(kind, "nv12", h, w)
    stride = geo.get("frame_stride", h * w * 3 // 2)
    raw = rng.integers(0, 256, (b - 1) * stride + yuv_ref.batch_bytes(1, h, w, "nv12", **geo) + 16, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]                                                     # 16-byte aligned: the 16-byte path where the geometry allows
    desc = E.yuv_desc("nv12", "bt709", False, **geo)
    frames = [E.frame_src("yuv_host", buf.ctypes.data + f * stride, desc) for f in range(b)]
    old = E.yuv_to_bgr(buf, b, h, w, desc=desc)
    np.testing.assert_array_equal(E.frames_to_bgr(frames, h, w), old)
    np.testing.assert_array_equal(old, yuv_ref.yuv_to_bgr(buf, b, h, w, "nv12", "bt709", False, **geo))


# ---- staging on an engine ----------------------------------------------------------------------------------------------------------
B, H, W, NB = 4, 360, 640, 6


def pad_surfaces(tight, h, w, fmt, geo):
    """tightly packed 4:2:0 frames (T, h * w * 3 / 2) laid out as `geo` (zero padding): (T, frame_stride)"""
    t, py, pc, oc = len(tight), geo["pitch_y"], geo["pitch_c"], geo["offset_c"]
    surf = np.zeros((t, geo["frame_stride"]), np.uint8)
    surf[:, : py * h].reshape(t, h, py)[:, :, :w] = tight[:, : h * w].reshape(t, h, w)
    if fmt == "nv12":
        surf[:, oc: oc + pc * (h // 2)].reshape(t, h // 2, pc)[:, :, :w] = tight[:, h * w:].reshape(t, h // 2, w)
    else:
        ov, q = geo["offset_v"], h * w // 4
        surf[:, oc: oc + pc * (h // 2)].reshape(t, h // 2, pc)[:, :, : w // 2] = tight[:, h * w: h * w + q].reshape(t, h // 2, w // 2)
        surf[:, ov: ov + pc * (h // 2)].reshape(t, h // 2, pc)[:, :, : w // 2] = tight[:, h * w + q:].reshape(t, h // 2, w // 2)
    return surf


@pytest.fixture(scope="module")
def staged():
    """the engine of test_yuv_staging_follows_the_slot_rules, its trackers, and one clip in every place a frame can come from"""
    import torch
    clip = synth_frames(B * NB, H, W, n_obj=8, seed=13)
    yuv = bgr_to_yuv420(clip, "nv12")
    expected = yuv_ref.yuv_to_bgr(yuv, B * NB, H, W, "nv12")
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", num_classes=NC, max_batch=B, max_frame_hw=(H, W), max_crops=B * 64, max_tracks=2048, nn_budget_cap=60)
    trk = [eng.tracker_create(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
           for _ in range(NC)]
    s = types.SimpleNamespace(eng=eng, trk=trk, clip=clip, yuv=yuv, expected=expected,
                              host_yuv=torch.from_numpy(yuv).pin_memory(), host_bgr=torch.from_numpy(expected).pin_memory(),
                              dev_yuv=torch.from_numpy(yuv).cuda(), dev_bgr=torch.from_numpy(expected).cuda())
    yield s
    eng.close()


def read_back(p, b):
    import torch
    view = types.SimpleNamespace(__cuda_array_interface__={"shape": (b, H, W, 3), "typestr": "|u1", "data": (p, False), "version": 2})
    return torch.as_tensor(view, device="cuda").clone().cpu().numpy()


def test_staged_batch_of_four_kinds_is_the_reference_frames(staged):
    import torch
    eng, trk, clip = staged.eng, staged.trk, staged.clip
    # frame 0: NV12 surface in device memory at an address = 1 mod 16
    nv12 = bgr_to_yuv420(clip[0:1], "nv12")[0]
    d0 = torch.zeros(nv12.size + 1, dtype=torch.uint8, device="cuda")
    d0[1:] = torch.from_numpy(nv12).cuda()
    assert d0[1:].data_ptr() % 16 == 1
    # frame 1: padded I420, BT.709 full range, pinned host memory
    geo = geometry("padded", "i420", H, W)
    i420 = pad_surfaces(bgr_to_yuv420(clip[1:2], "i420", "bt709", True), H, W, "i420", geo)[0]
    h1 = torch.from_numpy(i420).pin_memory()
    # frame 2: BGR in device memory; frame 3: BGR in pinned host memory
    d2, h3 = torch.from_numpy(clip[2]).cuda(), torch.from_numpy(clip[3]).pin_memory()
    frames = [E.frame_src("yuv_dev", d0[1:].data_ptr(), E.yuv_desc("nv12")),
              E.frame_src("yuv_host", h1.data_ptr(), E.yuv_desc("i420", "bt709", True, **geo)),
              E.frame_src("bgr_dev", d2.data_ptr()), E.frame_src("bgr_host", h3.data_ptr())]
    want = np.stack([yuv_ref.yuv_to_bgr(nv12, 1, H, W, "nv12")[0], yuv_ref.yuv_to_bgr(i420, 1, H, W, "i420", "bt709", True, **geo)[0], clip[2], clip[3]])
    off, total = E.frames_layout(frames, H, W)
    assert off.tolist() == [-1, 0, -1, -1] and total == yuv_ref.batch_bytes(1, H, W, "i420", **geo)

    for t in trk:
        eng.tracker_reset(t)
    p = eng.stream_stage_frames(frames, H, W)
    eng.stream_submit(p, B, H, W)                                                         # the detector waits for the slot's event
    rows, fidx, ndet = eng.stream_run_packed(trk, p, B, H, W)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(read_back(p, B), want)
    # the same four frames from a plain device tensor track the same
    for t in trk:
        eng.tracker_reset(t)
    plain = torch.from_numpy(want).cuda()
    rows2, fidx2, ndet2 = eng.stream_run_packed(trk, plain.data_ptr(), B, H, W)
    assert len(rows2) >= 1
    np.testing.assert_array_equal(ndet, ndet2)
    np.testing.assert_array_equal(fidx, fidx2)
    np.testing.assert_array_equal(rows, rows2)


def test_stage_frames_follows_the_slot_rules(staged):
    eng, trk = staged.eng, staged.trk
    fb_yuv, fb_bgr = H * W * 3 // 2, H * W * 3
    order = ["yuv_host", "yuv_dev", "bgr_host", "bgr_dev"]
    base = {"yuv_host": (staged.host_yuv.data_ptr(), fb_yuv), "yuv_dev": (staged.dev_yuv.data_ptr(), fb_yuv),
            "bgr_host": (staged.host_bgr.data_ptr(), fb_bgr), "bgr_dev": (staged.dev_bgr.data_ptr(), fb_bgr)}
    sl = lambda i: slice(i * B, (i + 1) * B)

    def frames_of(i, b=B):
        """batch i with every frame from another kind of source: all of them give expected[i * B + j]"""
        out = []
        for j in range(b):
            k = order[(i + j) % 4]
            out.append(E.frame_src(k, base[k][0] + (i * B + j) * base[k][1]))
        return out

    def code_of(fn):
        with pytest.raises(L.VcError) as ei:
            fn()
        return ei.value.code

    eng.stream_reset()
    # a fifth staged batch without a submit is refused, by whichever staging call; vc_stream_reset clears the staged batches
    for n in range(4):
        eng.stream_stage_frames(frames_of(n), H, W)
    assert code_of(lambda: eng.stream_stage_frames(frames_of(4), H, W)) == VC_ERR_STATE
    assert code_of(lambda: eng.stream_stage_host(staged.host_bgr[sl(4)].data_ptr(), B, H, W)) == VC_ERR_STATE
    assert code_of(lambda: eng.stream_stage_yuv_dev(staged.dev_yuv[sl(4)].data_ptr(), B, H, W)) == VC_ERR_STATE
    eng.stream_reset()
    # a bad descriptor in frame 2 is refused before a slot is taken: four good calls still fit
    bad = frames_of(0)
    bad[2] = E.frame_src("yuv_dev", staged.dev_yuv.data_ptr(), E.yuv_desc(pitch_y=W - 2))
    with pytest.raises(L.VcError, match="frame 2: pitch_y") as ei:
        eng.stream_stage_frames(bad, H, W)
    assert ei.value.code == VC_ERR_ARG
    for n in range(4):
        eng.stream_stage_frames(frames_of(n), H, W)
    assert code_of(lambda: eng.stream_stage_frames(frames_of(4), H, W)) == VC_ERR_STATE
    eng.stream_reset()
    # a batch or a frame larger than the slot
    assert code_of(lambda: eng.stream_stage_frames(frames_of(0, B + 1), H, W)) == VC_ERR_CAPACITY
    assert code_of(lambda: eng.stream_stage_frames(frames_of(0), H + 2, W)) == VC_ERR_CAPACITY

    def run(stage_of):
        """stage(i + 2); submit(i + 1); run(i); collect(i - 1) with batch i staged by stage_of(i)."""
        for t in trk:
            eng.tracker_reset(t)
        ptrs, got = {}, []
        stage = lambda i: ptrs.__setitem__(i, stage_of(i))
        stage(0); stage(1)
        eng.stream_submit(ptrs[0], B, H, W)
        for i in range(NB):
            if i + 2 < NB:
                stage(i + 2)
            if i + 1 < NB:
                eng.stream_submit(ptrs[i + 1], B, H, W)
            eng.stream_run_async(trk, ptrs[i], B, H, W)
            if i > 0:
                got.append(eng.stream_collect())
        got.append(eng.stream_collect())
        return got

    bgr_dev = run(lambda i: staged.dev_bgr[sl(i)].data_ptr())
    assert sum(len(r[0]) for r in bgr_dev) > 20
    calls = [lambda i: eng.stream_stage_frames(frames_of(i), H, W),
             lambda i: eng.stream_stage_yuv_host(staged.host_yuv[sl(i)].data_ptr(), B, H, W),
             lambda i: eng.stream_stage_host(staged.host_bgr[sl(i)].data_ptr(), B, H, W)]
    runs = {"frames": run(calls[0]), "alternating": run(lambda i: calls[i % 3](i))}
    for name, got in runs.items():
        for (r0, f0, n0), (r1, f1, n1) in zip(bgr_dev, got):
            np.testing.assert_array_equal(n0, n1, err_msg=name)
            np.testing.assert_array_equal(f0, f1, err_msg=name)
            np.testing.assert_array_equal(r0, r1, err_msg=name)


# ---- run_streams -------------------------------------------------------------------------------------------------------------------
def whole_frame_zone(golden_dir, tmp_path, name, h, w):
    """tests/test_gpu_yuv_ingest.py::whole_frame_zone: cam_04's directions with the zone polygon widened to the frame, so that every
    tracked row reaches the CSV."""
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


def test_run_streams_of_mixed_cameras_equals_separate_runs(golden_dir, tmp_path):
    """fp32: conv numerics do not depend on the tile configuration a batch size selects (test_multi_camera_random_layouts_equal_separate_runs)"""
    zone = whole_frame_zone(golden_dir, tmp_path, "cam_04_halfres.json", H, W)
    names = ["cam_00", "cam_01", "cam_02"]
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="f32", num_classes=NC, max_batch=5, max_frame_hw=(H, W), max_crops=5 * 300, max_tracks=4096, nn_budget_cap=60,
                   max_trackers=3 * NC)
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path))
    pipe = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": TRACK_CFG} for n in names}}, engine=eng, class_names=[f"c{i}" for i in range(NC)])
    clip = synth_frames(18, H, W, n_obj=6, seed=3)
    # camera 0: the clip as BGR; camera 1: the clip backwards as tight NV12; camera 2: 14 frames mirrored as padded I420, BT.709 full range
    nv12 = bgr_to_yuv420(clip[::-1], "nv12")
    geo = geometry("padded", "i420", H, W)
    i420 = pad_surfaces(bgr_to_yuv420(clip[4:, :, ::-1], "i420", "bt709", True), H, W, "i420", geo)
    sources = [FrameSource(clip), YuvFrameSource(nv12, H, W, fmt="nv12"),
               YuvFrameSource(i420, H, W, fmt="i420", matrix="bt709", full_range=True, pitch=geo["pitch_y"], pitch_c=geo["pitch_c"],
                              offset_c=geo["offset_c"], offset_v=geo["offset_v"], frame_stride=geo["frame_stride"])]
    expected = [clip, yuv_ref.yuv_to_bgr(nv12, 18, H, W, "nv12"), yuv_ref.yuv_to_bgr(i420, 14, H, W, "i420", "bt709", True, **geo)]
    # a camera of another size is refused before any GPU work
    with pytest.raises(ValueError, match="one size"):
        pipe.run_streams(sources + [FrameSource(synth_frames(2, H, W - 64, n_obj=2, seed=4))], names + ["cam_00"], [zone] * 4, batch=4)
    want = [pipe.run_stream(FrameSource(expected[c]), names[c], zone, batch=4, asynchronous=True) for c in range(3)]
    for c in range(3):
        assert len(want[c][0]) >= 10, (c, len(want[c][0]))                                # no camera passes empty against empty
    for batch in (4, 5):
        for host_frames in (False, True):
            got = pipe.run_streams(sources, names, [zone] * 3, batch=batch, host_frames=host_frames)
            for c in range(3):
                assert_same_output(got[c], want[c], f"camera {c} batch={batch} host_frames={host_frames}")
    eng.close()
