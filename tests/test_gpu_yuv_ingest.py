"""GPU: 4:2:0 YUV ingest.  The arithmetic is integer, so every comparison is bit for bit (assert_array_equal):
  * yuv_to_bgr_kernel (vc_yuv_to_bgr_host) against the NumPy definition (tests/yuv_ref.py) on uniformly random bytes -- out-of-range luma
    and chroma included -- for both formats, both matrices, both ranges, the 16-byte path and the generic one, tight and padded geometry;
  * the stream path: on ONE engine run_stream(FrameSource(expected BGR)) and run_stream(YuvFrameSource(YUV)) give identical rows and
    counts in every mode (same-engine runs repeat exactly: tile choices are fixed per engine);
  * the slot rules of vc_stream_stage_host hold for the YUV staging calls, alone and mixed with BGR staging."""
import ctypes as C
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
VC_ERR_STATE, VC_ERR_CAPACITY = 3, 4
GUARD = 4096


# ---- kernel ------------------------------------------------------------------------------------------------------------------------
def geometry(kind, fmt, h, w):
    """tight; padded: 16-byte aligned pitches, chroma beyond pitch * h, a gap between frames (a decoder surface); padded_odd: the same
    with nothing aligned (generic path at every width)."""
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


def convert_with_guards(buf, b, h, w, desc):
    """vc_yuv_to_bgr_host writing into the middle of a larger host array: (image, guard bytes before, guard bytes after)."""
    n = b * h * w * 3
    out = np.full(n + 2 * GUARD, 0x5A, np.uint8)
    dst = C.cast(out.ctypes.data + GUARD, C.POINTER(C.c_uint8))
    L.check(L.lib().vc_yuv_to_bgr_host(C.byref(desc), L.ptr(buf, C.c_uint8), b, h, w, dst))
    return out[GUARD:GUARD + n].reshape(b, h, w, 3), out[:GUARD], out[GUARD + n:]


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_kernel_matches_the_definition_bit_for_bit(fmt, matrix, full_range):
    rng = np.random.default_rng([fmt == "nv12", matrix == "bt601", full_range])
    for h, w in ((2, 2), (6, 18), (640, 640), (720, 1280), (718, 1278)):
        for kind in ("tight", "padded", "padded_odd"):
            for b in (1, 3):
                geo = geometry(kind, fmt, h, w)
                buf = rng.integers(0, 256, yuv_ref.batch_bytes(b, h, w, fmt, **geo), dtype=np.uint8)      # padding bytes random too
                desc = E.yuv_desc(fmt, matrix, full_range, **geo)
                got, before, after = convert_with_guards(buf, b, h, w, desc)
                want = yuv_ref.yuv_to_bgr(buf, b, h, w, fmt, matrix, full_range, **geo)
                case = f"{fmt} {matrix} full={full_range} {h}x{w} {kind} b={b}"
                np.testing.assert_array_equal(got, want, err_msg=case)
                assert (before == 0x5A).all() and (after == 0x5A).all(), case
                np.testing.assert_array_equal(E.yuv_to_bgr(buf, b, h, w, desc=desc), want, err_msg=case)     # the numpy-in / numpy-out wrapper


def test_kernel_default_descriptor_and_capacity():
    rng = np.random.default_rng(1)
    buf = rng.integers(0, 256, 3 * 48 * 64 * 3 // 2, dtype=np.uint8)
    np.testing.assert_array_equal(E.yuv_to_bgr(buf, 3, 48, 64), yuv_ref.yuv_to_bgr(buf, 3, 48, 64))         # NV12, BT.601, limited, tight
    # the same kernel on the caller's device buffers (vc_yuv_to_bgr_dev, null stream)
    import torch
    src, dst = torch.from_numpy(buf).cuda(), torch.full((3 * 48 * 64 * 3 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    E.yuv_to_bgr_dev(src.data_ptr(), 3, 48, 64, dst.data_ptr() + 32)
    torch.cuda.synchronize()
    back = dst.cpu().numpy()
    np.testing.assert_array_equal(back[32:-32].reshape(3, 48, 64, 3), yuv_ref.yuv_to_bgr(buf, 3, 48, 64))
    assert (back[:32] == 0x5A).all() and (back[-32:] == 0x5A).all()
    # every value of every channel is reachable: all 2^24 (Y, U, V) triples of one matrix, as 4096 x 4096 pixels with a 2 x 2 block per triple
    # would be 64 MB -- the 256 x 256 (U, V) plane at 16 luma levels covers every chroma term against clamped and unclamped luma
    h = w = 512
    Y = np.repeat(np.array([0, 15, 16, 17, 64, 100, 127, 128, 129, 180, 200, 234, 235, 236, 254, 255], np.uint8), h * w).reshape(16, h, w)
    U = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (16, 256, 256))
    V = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (16, 256, 256))
    frames = np.concatenate([Y.reshape(16, -1), U.reshape(16, -1), V.reshape(16, -1)], axis=1)             # I420, tight
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            np.testing.assert_array_equal(E.yuv_to_bgr(frames, 16, h, w, "i420", matrix, full),
                                          yuv_ref.yuv_to_bgr(frames, 16, h, w, "i420", matrix, full), err_msg=f"{matrix} full={full}")


# ---- stream path -------------------------------------------------------------------------------------------------------------------
def whole_frame_zone(golden_dir, tmp_path, name, h, w):
    """cam_04's directions with the zone polygon widened to the frame: every tracked row reaches the CSV, so the comparison covers the
    tracker's complete output."""
    with open(os.path.join(golden_dir, name)) as f:
        z = json.load(f)
    for sh in z["shapes"]:
        if sh["label"] == "zone":
            sh["points"] = [[0.0, 0.0], [float(w), 0.0], [float(w), float(h)], [0.0, float(h)]]
    path = str(tmp_path / f"zone_{h}x{w}.json")
    with open(path, "w") as f:
        json.dump(z, f)
    return path


def make_pipe(precision, batch, h, w, nc, det_scale, obj_shift, tmp_path):
    ysd, rsd = synth_yolo("yolov5s", nc=nc, seed=1702, det_scale=det_scale, obj_shift=obj_shift), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision=precision, num_classes=nc, max_batch=batch, max_frame_hw=(h, w), max_crops=batch * 300, max_tracks=4096,
                   nn_budget_cap=60)                                                       # max_crops: max_det boxes in every frame
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path))
    pipe = CountingPipeline(args, cfg, {"cam": {"cam_04": {"tracking_config": TRACK_CFG}}}, engine=eng, class_names=[f"c{i}" for i in range(nc)])
    return eng, pipe


def assert_same_output(got, want, case):
    """rows = one dict per CSV line: frame, track id, label, box, direction, first / last point and frame -- all of it equal."""
    rows, counts = got
    ref_rows, ref_counts = want
    assert len(rows) == len(ref_rows), case
    for r, q in zip(rows, ref_rows):
        assert set(r) == set(q), case
        for k in r:
            np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(q[k]), err_msg=f"{case}: {k}")
    assert counts == ref_counts, case


# precision, h, w, frames, batch, zone file, then the detector / clip calibration of an existing test of that geometry:
# classes, det_scale, obj_shift, objects, clip seed
# (bench.py's 80-class head at 640 x 640 finds nothing once the clip's random textures have been through 4:2:0 -- an empty CSV on both sides;
# the 8-class head of the other tests keeps its boxes)
STREAM_CASES = [("bf16", 640, 640, 22, 8, "cam_04_halfres.json", 8, 4.0, 0.0, 12, 1702),      # bench.py's clip, test_gpu_pipeline.py's head; 8 + 8 + 6 frames: a short last batch
                ("bf16", 720, 1280, 11, 4, "cam_04.json", 8, 8.0, 1.0, 8, 21),                 # test_720p_stream_with_the_reference_zone_file; 4 + 4 + 3, letterbox resize
                ("f32", 360, 640, 18, 4, "cam_04_halfres.json", 8, 4.0, 0.0, 6, 3)]             # test_gpu_pipeline.py::test_csv_parity; 4 x 4 + 2


@pytest.mark.parametrize("precision,h,w,t,batch,zone_name,nc,det_scale,obj_shift,n_obj,seed", STREAM_CASES, ids=[f"{c[0]}_{c[2]}x{c[1]}" for c in STREAM_CASES])
def test_run_stream_yuv_source_equals_bgr_source(precision, h, w, t, batch, zone_name, nc, det_scale, obj_shift, n_obj, seed, golden_dir, tmp_path):
    zone = whole_frame_zone(golden_dir, tmp_path, zone_name, h, w)
    clip = synth_frames(t, h, w, n_obj=n_obj, seed=seed)
    eng, pipe = make_pipe(precision, batch, h, w, nc, det_scale, obj_shift, tmp_path)
    for fmt in ("nv12", "i420"):
        yuv = bgr_to_yuv420(clip, fmt)
        expected = yuv_ref.yuv_to_bgr(yuv, t, h, w, fmt)                                  # what the device must have produced
        assert np.abs(expected.astype(int) - clip).mean() < 8                             # and it still is the clip (chroma subsampled)
        want = pipe.run_stream(FrameSource(expected), "cam_04", zone, batch=batch, asynchronous=True)
        assert len(want[0]) >= 10, len(want[0])                                           # a populated CSV, not an empty-equals-empty pass
        for host_frames in (False, True):
            for asynchronous in (False, True):
                got = pipe.run_stream(YuvFrameSource(yuv, h, w, fmt=fmt), "cam_04", zone, batch=batch, asynchronous=asynchronous, host_frames=host_frames)
                assert_same_output(got, want, f"{precision} {h}x{w} {fmt} host_frames={host_frames} asynchronous={asynchronous}")
    # a padded NV12 surface (pitch 256 above the width, chroma below an aligned height, a gap between frames) and BT.709 full range
    geo = geometry("padded", "nv12", h, w)
    tight = bgr_to_yuv420(clip, "nv12", "bt709", True)
    stride = geo["frame_stride"]
    surf = np.zeros((t, stride), np.uint8)
    surf[:, : geo["pitch_y"] * h].reshape(t, h, -1)[:, :, :w] = tight[:, : h * w].reshape(t, h, w)
    surf[:, geo["offset_c"]: geo["offset_c"] + geo["pitch_c"] * (h // 2)].reshape(t, h // 2, -1)[:, :, :w] = tight[:, h * w:].reshape(t, h // 2, w)
    expected = yuv_ref.yuv_to_bgr(surf, t, h, w, "nv12", "bt709", True, **geo)
    np.testing.assert_array_equal(expected, yuv_ref.yuv_to_bgr(tight, t, h, w, "nv12", "bt709", True))
    want = pipe.run_stream(FrameSource(expected), "cam_04", zone, batch=batch, asynchronous=True)
    src = YuvFrameSource(surf, h, w, fmt="nv12", matrix="bt709", full_range=True, pitch=geo["pitch_y"], offset_c=geo["offset_c"], frame_stride=stride)
    for host_frames in (False, True):
        got = pipe.run_stream(src, "cam_04", zone, batch=batch, asynchronous=True, host_frames=host_frames)
        assert_same_output(got, want, f"{precision} {h}x{w} padded surface host_frames={host_frames}")
    eng.close()


# ---- slot rules --------------------------------------------------------------------------------------------------------------------
def test_yuv_staging_follows_the_slot_rules():
    import torch
    B, H, W, NB = 4, 360, 640, 6
    clip = synth_frames(B * NB, H, W, n_obj=8, seed=13)
    yuv = bgr_to_yuv420(clip, "nv12")
    expected = yuv_ref.yuv_to_bgr(yuv, B * NB, H, W, "nv12")
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", num_classes=NC, max_batch=B, max_frame_hw=(H, W), max_crops=B * 64, max_tracks=2048, nn_budget_cap=60)
    trk = [eng.tracker_create(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
           for _ in range(NC)]
    host_yuv, host_bgr = torch.from_numpy(yuv).pin_memory(), torch.from_numpy(expected).pin_memory()
    dev_yuv, dev_bgr = torch.from_numpy(yuv).cuda(), torch.from_numpy(expected).cuda()
    sl = lambda i: slice(i * B, (i + 1) * B)

    def code_of(fn):
        with pytest.raises(L.VcError) as ei:
            fn()
        return ei.value.code

    # a fifth staged batch without a submit is refused, by either call; vc_stream_reset clears staged YUV batches
    for n in range(4):
        stage = eng.stream_stage_yuv_host if n % 2 == 0 else eng.stream_stage_yuv_dev
        stage((host_yuv if n % 2 == 0 else dev_yuv)[sl(n)].data_ptr(), B, H, W)
    assert code_of(lambda: eng.stream_stage_yuv_host(host_yuv[sl(4)].data_ptr(), B, H, W)) == VC_ERR_STATE
    assert code_of(lambda: eng.stream_stage_yuv_dev(dev_yuv[sl(4)].data_ptr(), B, H, W)) == VC_ERR_STATE
    assert code_of(lambda: eng.stream_stage_host(host_bgr[sl(4)].data_ptr(), B, H, W)) == VC_ERR_STATE
    eng.stream_reset()
    for n in range(4):
        eng.stream_stage_yuv_host(host_yuv[sl(n)].data_ptr(), B, H, W)
    assert code_of(lambda: eng.stream_stage_yuv_host(host_yuv[sl(4)].data_ptr(), B, H, W)) == VC_ERR_STATE
    eng.stream_reset()
    # a batch or a frame larger than the slot
    assert code_of(lambda: eng.stream_stage_yuv_host(host_yuv.data_ptr(), B + 1, H, W)) == VC_ERR_CAPACITY
    assert code_of(lambda: eng.stream_stage_yuv_dev(dev_yuv.data_ptr(), 1, H + 2, W)) == VC_ERR_CAPACITY
    # geometry errors come first and take no slot
    assert code_of(lambda: eng.stream_stage_yuv_host(host_yuv.data_ptr(), B, H, W, E.yuv_desc(pitch_y=W - 2))) == 1

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

    bgr_dev = run(lambda i: dev_bgr[sl(i)].data_ptr())
    assert sum(len(r[0]) for r in bgr_dev) > 20
    kinds = {"bgr_host": lambda i: eng.stream_stage_host(host_bgr[sl(i)].data_ptr(), B, H, W),
             "yuv_host": lambda i: eng.stream_stage_yuv_host(host_yuv[sl(i)].data_ptr(), B, H, W),
             "yuv_dev": lambda i: eng.stream_stage_yuv_dev(dev_yuv[sl(i)].data_ptr(), B, H, W)}
    order = ["bgr_host", "yuv_host", "yuv_dev"]
    runs = {"yuv_host": run(kinds["yuv_host"]), "yuv_dev": run(kinds["yuv_dev"]),
            "alternating": run(lambda i: kinds[order[i % 3]](i)),                         # BGR and YUV staging mixed on one engine
            "alternating2": run(lambda i: kinds[order[(i + 1) % 2]](i))}
    for name, got in runs.items():
        for (r0, f0, n0), (r1, f1, n1) in zip(bgr_dev, got):
            np.testing.assert_array_equal(n0, n1, err_msg=name)
            np.testing.assert_array_equal(f0, f1, err_msg=name)
            np.testing.assert_array_equal(r0, r1, err_msg=name)
    # the staged address is an ordinary BGR frame buffer: read it back
    p = eng.stream_stage_yuv_dev(dev_yuv[sl(2)].data_ptr(), B, H, W)
    eng.stream_submit(p, B, H, W)                                                         # the detector waits for the conversion
    eng.stream_run_packed(trk, p, B, H, W)
    torch.cuda.synchronize()
    view = types.SimpleNamespace(__cuda_array_interface__={"shape": (B, H, W, 3), "typestr": "|u1", "data": (p, False), "version": 2})
    back = torch.as_tensor(view, device="cuda").clone()
    np.testing.assert_array_equal(back.cpu().numpy(), expected[sl(2)])
    eng.close()
