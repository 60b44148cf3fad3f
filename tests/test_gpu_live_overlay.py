"""GPU: the live overlay (csrc/live_overlay.hip) -- the build kernels in one launch each against the definition on the case table of
tests/live_overlay_cases.py; attached to an engine: the lists of every batch equal overlay.LiveVisualizer fed the collected rows, rows
and counts are what they are without it, and a batch without a single box still numbers and draws its frames; CountingPipeline.run_stream / run_streams(annotate=sink): every output byte equals the
existing Renderer.submit given the host-built lists of the same batches; refusals leave the state as it was; a counter without the
overlay launches what it launched before."""
import json
import os
import types

import numpy as np
import pytest

import live_overlay_cases as OC
from vehicle_counting_amd import overlay as ov

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", OC.CASES, ids=[c.name for c in OC.CASES])
def test_one_launch_parity_with_the_definition(case):
    OC.check(case, host=False)


# ---- attached to an engine: the scenario of tests/test_gpu_live_count.py, restated ------------------------------------------------------
H, W, B, T, NL = 64, 96, 4, 24, 2
TRACK_KW = dict(max_dist=0.2, min_confidence=0.25, nms_max_overlap=1.0, max_iou_distance=0.7, max_age=2, n_init=1, nn_budget=8)
ZONE = [[0.0, 0.0], [60.0, 0.0], [60.0, 64.0], [0.0, 64.0]]
RIGHT, DOWN, LEFT = [10.0, 32.0, 80.0, 32.0], [48.0, 5.0, 48.0, 60.0], [80.0, 50.0, 10.0, 50.0]
CAM_LINES = [[RIGHT, DOWN], [RIGHT, DOWN, LEFT]]
CAM_KEYS = [["01", "02"], ["01", "02", "10"]]
CAM_DIRS = [{k: [l[:2], l[2:]] for k, l in zip(keys, lines)} for keys, lines in zip(CAM_KEYS, CAM_LINES)]
OBJECTS = [
    [(0, 0, 23, 5, 8, 2.0, 0.0, 14, 12), (0, 0, 7, 72, 40, -3.0, 0.0, 14, 12), (1, 0, 23, 20, 4, 0.0, 1.5, 12, 14),
     (1, 5, 12, 75, 30, 0.0, 0.0, 14, 12), (0, 12, 18, 28, 42, 2.0, 0.0, 14, 12)],
    [(0, 0, 23, 8, 46, 1.0, 0.0, 14, 12), (1, 0, 23, 38, 18, 0.0, 0.0, 12, 14), (0, 2, 9, 56, 6, -2.0, 0.0, 14, 12),
     (1, 14, 23, 22, 26, 0.0, 1.0, 12, 14)],
]
VC_ERR_ARG, VC_ERR_STATE = 1, 3


def clip(cam):
    rng = np.random.default_rng(100 + cam)
    bg = rng.integers(60, 120, (H, W, 3), dtype=np.uint8)
    tex = [rng.integers(0, 256, (o[8], o[7], 3), dtype=np.uint8) for o in OBJECTS[cam]]
    frames = np.repeat(bg[None], T, 0).copy()
    boxes = []
    for t in range(T):
        bl = []
        for k, (label, t0, t1, x, y, vx, vy, w, h) in enumerate(OBJECTS[cam]):
            if t0 <= t <= t1:
                x1, y1 = int(round(x + vx * (t - t0))), int(round(y + vy * (t - t0)))
                frames[t, y1:y1 + h, x1:x1 + w] = tex[k]
                bl.append((x1, y1, w, h, label))
        boxes.append(bl)
    return frames, boxes


@pytest.fixture(scope="module")
def eng():
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd.weights import synth_reid, synth_yolo
    e = E.Engine(synth_yolo("yolov5s", nc=NL, seed=1702, det_scale=4.0, obj_shift=-2.0), synth_reid(1702), precision="f32", num_classes=NL,
                 max_batch=B, max_frame_hw=(H, W), max_crops=B * 16, max_tracks=64, nn_budget_cap=8, max_trackers=32)
    yield e
    e.close()


def per_frame(rows, fidx, b):
    return [rows[fidx == f] for f in range(b)]


def run_clip(eng, cams, overlay, multi):
    """The clips of `cams` interleaved frame by frame, one batch of B frames at a time on new trackers with a live counter -- through
    run_async_multi + collect (multi) or the blocking stream_run.  Returns per batch (rows, fidx), the counts after it, and with
    `overlay` the lists read back after it next to those of a LiveVisualizer fed the collected rows."""
    import torch
    import vehicle_counting_amd.engine as E
    clips = [clip(c) for c in cams]
    order = [(k, t) for t in range(T) for k in range(len(cams))]
    dev = torch.from_numpy(np.stack([clips[k][0][t] for k, t in order])).cuda()
    nmax = max(len(b) for k in range(len(cams)) for b in clips[k][1])
    det, cnt = np.zeros((len(order), nmax, 6), np.float32), np.zeros(len(order), np.int32)
    for g, (k, t) in enumerate(order):
        for i, (x, y, w, h, label) in enumerate(clips[k][1][t]):
            det[g, i] = (x, y, x + w, y + h, 0.9, label)
        cnt[g] = len(clips[k][1][t])
    tids = np.array([[eng.tracker_create(**TRACK_KW) for _ in range(NL)] for _ in cams], np.int32)
    live = E.LiveCounter(eng, tids, [ZONE] * len(cams), [CAM_LINES[c] for c in cams])
    lv = ov.LiveVisualizer([ZONE] * len(cams), [CAM_DIRS[c] for c in cams], NL)
    if overlay:
        live.enable_overlay([CAM_KEYS[c] for c in cams], max_batch=B, max_rows_per_frame=16, depth=2)
    out = []
    try:
        for f0 in range(0, len(order), B):
            eng.stream_inject(det[f0:f0 + B], cnt[f0:f0 + B])
            if multi:
                eng.stream_submit(dev[f0:f0 + B].data_ptr(), B, H, W)
                eng.stream_run_async_multi(tids, [k for k, _ in order[f0:f0 + B]], dev[f0:f0 + B].data_ptr(), B, H, W, cap_rows=32)
                rows, fidx, _ = eng.stream_collect()
            else:
                rows, fidx, _ = eng.stream_run_packed(tids[0], dev[f0:f0 + B].data_ptr(), B, H, W, cap_rows=32)
            rec = dict(rows=rows.copy(), fidx=fidx.copy(), counts=live.counts())
            if overlay:
                rec["got"] = live.overlay_lists()
                rec["want"] = lv.batch_prims([k for k, _ in order[f0:f0 + B]], [t + 1 for _, t in order[f0:f0 + B]], per_frame(rows, fidx, B), (H, W))
            out.append(rec)
    finally:
        eng.stream_inject(None)
        eng.stream_reset()
        live.close()
        for t in tids.reshape(-1):
            eng.tracker_destroy(int(t))
    return out


@pytest.fixture(scope="module")
def attached_runs(eng):
    return {(multi, overlay): run_clip(eng, [0, 1] if multi else [0], overlay, multi) for multi in (True, False) for overlay in (True, False)}


@pytest.mark.parametrize("multi", [True, False], ids=["two cameras, run_async_multi", "one camera, stream_run"])
def test_lists_of_every_batch_equal_the_definition_fed_the_collected_rows(attached_runs, multi):
    run = attached_runs[multi, True]
    assert len(run) == (2 if multi else 1) * T // B and sum(len(r["rows"]) for r in run) > (100 if multi else 50)
    with_text = 0
    for k, r in enumerate(run):
        (prims, first), (want_prims, want_first) = r["got"], r["want"]
        print(f"batch {k}: {len(r['rows'])} rows, {first[-1]} primitives")
        np.testing.assert_array_equal(first, want_first, err_msg=f"batch {k}")
        np.testing.assert_array_equal(prims, want_prims, err_msg=f"batch {k}")
        with_text += bool((prims[:, 6] == 0xFFFFFF).any())                   # white glyphs: the count text
    assert with_text == len(run) - 1                                          # none in the first batch (no frame before it), then always


@pytest.mark.parametrize("multi", [True, False], ids=["two cameras", "one camera"])
def test_rows_and_counts_are_untouched_by_the_overlay(attached_runs, multi):
    a, b = attached_runs[multi, True], attached_runs[multi, False]
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x["rows"], y["rows"])
        np.testing.assert_array_equal(x["fidx"], y["fidx"])
        np.testing.assert_array_equal(x["counts"], y["counts"])
    assert a[-1]["counts"].sum() >= 3


def test_a_batch_without_a_box_still_numbers_and_draws_its_frames(eng):
    """track_enqueue's path for a batch that steps no tracker, with a counter and its overlay attached: two cameras x two labels, three
    batches of four frames, the middle one without a single box.  It gives no row, its frames take their cameras' next numbers (the
    third batch's lists carry frames 5 and 6), its lists are the definition's for frames without rows, and the rows of the batches
    around it are the oracle's VideoTracker.run per camera, which is never called for a frame without boxes (Q1)."""
    import torch
    import vehicle_counting_amd.engine as E
    from oracle import deepsort as od
    from oracle import reid as orr
    from oracle import yolov5 as oy
    from vehicle_counting_amd.weights import synth_reid
    NB = 3
    clips = [clip(0), clip(1)]
    order = [(k, t) for t in range(NB * B // 2) for k in range(2)]
    dev = torch.from_numpy(np.stack([clips[k][0][t] for k, t in order])).cuda()
    nmax = max(len(clips[k][1][t]) for k, t in order)
    assert nmax <= 8
    det, cnt = np.zeros((len(order), nmax, 6), np.float32), np.zeros(len(order), np.int32)
    for g, (k, t) in enumerate(order):
        if B <= g < 2 * B:
            continue
        for i, (x, y, w, h, label) in enumerate(clips[k][1][t]):
            det[g, i] = (x, y, x + w, y + h, 0.9, label)
        cnt[g] = len(clips[k][1][t])
    cfg = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=1.0, MAX_IOU_DISTANCE=0.7, MAX_AGE=2, N_INIT=1, NN_BUDGET=8)     # TRACK_KW
    oracle = [od.VideoTrackerOracle(NL, cfg, orr.make_embedder(synth_reid(1702))) for _ in range(2)]
    want_rows = []
    for g, (k, t) in enumerate(order):
        if cnt[g] == 0:
            want_rows.append(np.zeros((0, 6), np.int64))
            continue
        m = oy.marshal_like_reference(det[g, :cnt[g]])
        res = oracle[k].run(clips[k][0][t], m["bboxes"], m["classes"], m["scores"])
        want_rows.append(np.array([list(b) + [tr, lb] for b, tr, lb in zip(res["boxes"], res["tracks"], res["labels"])], dtype=np.int64).reshape(-1, 6))
    tids = np.array([[eng.tracker_create(**TRACK_KW) for _ in range(NL)] for _ in range(2)], np.int32)
    live = E.LiveCounter(eng, tids, [ZONE] * 2, CAM_LINES)
    lv = ov.LiveVisualizer([ZONE] * 2, CAM_DIRS, NL)
    live.enable_overlay(CAM_KEYS, max_batch=B, max_rows_per_frame=16, depth=2)
    try:
        for n in range(NB):
            sl = slice(n * B, (n + 1) * B)
            eng.stream_inject(det[sl], cnt[sl])
            eng.stream_submit(dev[sl].data_ptr(), B, H, W)
            eng.stream_run_async_multi(tids, [k for k, _ in order[sl]], dev[sl].data_ptr(), B, H, W, cap_rows=32)
            rows, fidx, _ = eng.stream_collect()
            got = per_frame(rows, fidx, B)
            print(f"batch {n}: {len(rows)} rows")
            assert (len(rows) == 0) == (n == 1)
            for f in range(B):
                np.testing.assert_array_equal(got[f], want_rows[n * B + f], err_msg=f"batch {n}, frame {f}")
            assert live.counts(with_frames=True)[1].tolist() == [(n + 1) * B // 2] * 2
            prims, first = live.overlay_lists()
            want_prims, want_first = lv.batch_prims([k for k, _ in order[sl]], [t + 1 for _, t in order[sl]], got, (H, W))
            np.testing.assert_array_equal(first, want_first, err_msg=f"batch {n}")
            np.testing.assert_array_equal(prims, want_prims, err_msg=f"batch {n}")
    finally:
        eng.stream_inject(None)
        eng.stream_reset()
        live.close()
        for t in tids.reshape(-1):
            eng.tracker_destroy(int(t))


@pytest.fixture()
def one_camera(eng):
    """camera 0's trackers with a counter attached; batches of B frames of its clip through the blocking stream_run"""
    import torch
    import vehicle_counting_amd.engine as E
    frames, boxes = clip(0)
    dev = torch.from_numpy(frames).cuda()
    nmax = max(len(b) for b in boxes)
    det, cnt = np.zeros((T, nmax, 6), np.float32), np.zeros(T, np.int32)
    for t in range(T):
        for i, (x, y, w, h, label) in enumerate(boxes[t]):
            det[t, i] = (x, y, x + w, y + h, 0.9, label)
        cnt[t] = len(boxes[t])
    tids = np.array([eng.tracker_create(**TRACK_KW) for _ in range(NL)], np.int32)
    live = E.LiveCounter(eng, [tids], [ZONE], [CAM_LINES[0]])

    def run(n):
        eng.stream_inject(det[n * B:(n + 1) * B], cnt[n * B:(n + 1) * B])
        return eng.stream_run_packed(tids, dev[n * B:(n + 1) * B].data_ptr(), B, H, W, cap_rows=32)

    yield types.SimpleNamespace(tids=tids, live=live, run=run, dev=dev)
    eng.stream_inject(None)
    eng.stream_reset()
    live.close()
    for t in tids:
        eng.tracker_destroy(int(t))


def test_refusals_leave_the_state_as_it_was(eng, one_camera):
    import torch
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd._lib import VcError
    c = one_camera
    lv = ov.LiveVisualizer([ZONE], [CAM_DIRS[0]], NL)
    c.live.enable_overlay([CAM_KEYS[0]], max_batch=B, max_rows_per_frame=16, depth=1)
    out = torch.zeros(B * H * W * 3 // 2, dtype=torch.uint8, device="cuda")
    with E.Renderer(eng, max_batch=B, max_hw=(H, W), depth=2) as rnd:
        def refused(call, code):
            with pytest.raises(VcError) as ei:
                call()
            assert ei.value.code == code, ei.value

        refused(lambda: rnd.submit_live(c.live, c.dev[:B].data_ptr(), B, H, W, out.data_ptr(), kind="bgr_dev", out_is_dev=True), VC_ERR_STATE)   # nothing pending
        refused(lambda: c.live.overlay_lists(), VC_ERR_STATE)
        refused(lambda: c.live.enable_overlay([CAM_KEYS[0]], max_batch=B, max_rows_per_frame=16, depth=1), VC_ERR_STATE)                  # enable called twice
        rows, fidx, _ = c.run(0)
        want0 = lv.batch_prims([0] * B, range(1, B + 1), per_frame(rows, fidx, B), (H, W))
        counts = c.live.counts()
        refused(lambda: c.run(1), VC_ERR_STATE)                                  # depth 1: the only buffer holds batch 0's lists
        np.testing.assert_array_equal(c.live.counts(), counts)                   # nothing of the refused run was enqueued
        for b, h, w in ((B - 1, H, W), (B, H - 2, W), (B, H, W - 2)):            # not the batch's own b / h / w
            refused(lambda: rnd.submit_live(c.live, c.dev[:B].data_ptr(), b, h, w, out.data_ptr(), kind="bgr_dev", out_is_dev=True), VC_ERR_ARG)
        assert rnd.outstanding == 0
        prims, first = c.live.overlay_lists()                                    # the refusals consumed nothing: batch 0's lists are still the oldest
        np.testing.assert_array_equal(first, want0[1])
        np.testing.assert_array_equal(prims, want0[0])
        rows, fidx, _ = c.run(1)                                                 # and the stream goes on where it was
        want1 = lv.batch_prims([0] * B, range(B + 1, 2 * B + 1), per_frame(rows, fidx, B), (H, W))
        prims, first = c.live.overlay_lists()
        np.testing.assert_array_equal(first, want1[1])
        np.testing.assert_array_equal(prims, want1[0])
        # a sized batch builds no list: submit_live after it finds nothing
        eng.stream_inject(None)
        dims = [(H, W)] * B
        ptr = eng.stream_stage_frames_sized([E.frame_src("bgr_dev", c.dev[2 * B + i].data_ptr()) for i in range(B)], dims)
        eng.stream_submit_sized(ptr, dims)
        eng.stream_run_async_multi_sized([c.tids], [0] * B, ptr, dims, cap_rows=32)
        eng.stream_collect()
        refused(lambda: rnd.submit_live(c.live, c.dev[:B].data_ptr(), B, H, W, out.data_ptr(), kind="bgr_dev", out_is_dev=True), VC_ERR_STATE)
        assert c.live.counts(with_frames=True)[1].tolist() == [3 * B]            # the sized batch still advanced the counter


def test_a_counter_without_the_overlay_launches_what_it_did(eng, one_camera):
    """overlay_lists() without enable_overlay is VC_ERR_STATE; the profile's tracker launches of one batch equal those of the same batch
    on a counter-only run, and the enabled overlay adds exactly one (its build launches are profiled as a launch of their own)."""
    from vehicle_counting_amd._lib import PROF_TRACK, VcError
    c = one_camera
    with pytest.raises(VcError) as ei:
        c.live.overlay_lists()
    assert ei.value.code == VC_ERR_STATE
    eng.profile(True)
    try:
        launches = []
        for n in range(3):
            if n == 2:
                c.live.enable_overlay([CAM_KEYS[0]], max_batch=B, max_rows_per_frame=16, depth=2)
            eng.profile_reset()
            c.run(n)
            launches.append(eng.profile_read(PROF_TRACK)["launches"])
    finally:
        eng.profile(False)
    print("tracker launches per batch: counter only", launches[:2], "with the overlay", launches[2])
    assert launches[0] == launches[1] and launches[2] == launches[0] + 1


# ---- the pipeline: one pass from frames to annotated encoder surfaces ---------------------------------------------------------------------
PH, PW, PT, PB, PNC = 360, 640, 18, 4, 8          # tests/test_gpu_pipeline.py::test_csv_parity's geometry and detector calibration
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)


def pipe_zone(golden_dir, tmp_path):
    with open(os.path.join(golden_dir, "cam_04_halfres.json")) as f:
        z = json.load(f)
    for sh in z["shapes"]:
        if sh["label"] == "zone":                   # the whole frame, as tests/test_gpu_yuv_ingest.py::whole_frame_zone: every tracked row is drawn
            sh["points"] = [[0.0, 0.0], [float(PW), 0.0], [float(PW), float(PH)], [0.0, float(PH)]]
    path = str(tmp_path / "overlay_zone.json")
    with open(path, "w") as f:
        json.dump(z, f)
    return path


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd.pipeline import CountingPipeline
    from vehicle_counting_amd.weights import synth_reid, synth_yolo
    e = E.Engine(synth_yolo("yolov5s", nc=PNC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702), precision="f32", num_classes=PNC, max_batch=PB,
                 max_frame_hw=(PH, PW), max_crops=PB * 300, max_tracks=4096, nn_budget_cap=60)
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path_factory.mktemp("overlay_out")))
    p = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": TRACK_CFG} for n in ("cam_a", "cam_b")}}, engine=e, class_names=[f"c{i}" for i in range(PNC)])
    yield p
    e.close()


class Recorder:
    """the (rows, frame index) every collect of the engine hands to the pipeline, batch by batch"""

    def __init__(self, eng):
        self.eng, self.batches = eng, []
        self.saved = (eng.stream_collect, eng.stream_run_packed)
        eng.stream_collect = lambda: self.keep(self.saved[0]())
        eng.stream_run_packed = lambda *a, **k: self.keep(self.saved[1](*a, **k))

    def keep(self, res):
        self.batches.append((res[0].copy(), res[1].copy()))
        return res

    def close(self):
        del self.eng.stream_collect, self.eng.stream_run_packed


def rendered_by_submit(eng, frames_bgr, lists, sink_kw, batch):
    """the existing path: Renderer.submit with host-built lists, batch by batch, into a pinned sink of the same layout"""
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd.pipeline import YuvFrameSink
    sink = YuvFrameSink(PH, PW, n_frames=len(frames_bgr), **sink_kw)
    with E.Renderer(eng, max_batch=batch, max_hw=(PH, PW), depth=1) as rnd:
        for n, (prims, first) in enumerate(lists):
            b = len(first) - 1
            rnd.submit(np.ascontiguousarray(frames_bgr[n * batch:n * batch + b]), b, PH, PW, sink.address(n * batch), kind="bgr_host", prims=prims, first=first,
                       out_desc=sink.desc)
            rnd.collect()
    return sink.data.copy()


SINKS = [("nv12", False, False), ("i420", False, True), ("nv12", True, True), ("i420", True, False)]


@pytest.mark.parametrize("fmt,device,asynchronous", SINKS, ids=[f"{f}-{'device' if d else 'pinned'}-{'async' if a else 'sync'}" for f, d, a in SINKS])
def test_run_stream_annotate_equals_submit_with_host_built_lists(pipe, golden_dir, tmp_path, fmt, device, asynchronous):
    import torch
    from vehicle_counting_amd.counting import load_zone_anno
    from vehicle_counting_amd.pipeline import FrameSource, YuvFrameSink
    from vehicle_counting_amd.synth import synth_frames
    zone = pipe_zone(golden_dir, tmp_path)
    frames = synth_frames(PT, PH, PW, n_obj=6, seed=3)
    plain = pipe.run_stream(FrameSource(frames), "cam_a", zone, batch=PB, asynchronous=asynchronous)
    live = pipe.open_live(["cam_a"], [zone])
    sink_kw = dict(fmt=fmt, matrix="bt709" if fmt == "i420" else "bt601", full_range=fmt == "i420")
    surf = torch.zeros(PT * PH * PW * 3 // 2, dtype=torch.uint8, device="cuda") if device else None
    sink = YuvFrameSink(PH, PW, n_frames=PT, device_ptr=surf.data_ptr() if device else None, **sink_kw)
    rec = Recorder(pipe.engine)
    try:
        got = pipe.run_stream(FrameSource(frames), "cam_a", zone, batch=PB, asynchronous=asynchronous, live=live, annotate=sink)
    finally:
        rec.close()
    assert got == plain and len(got[0]) >= 10                                   # rows, counts and CSV are what they are without annotate
    polygon, directions = load_zone_anno(zone)
    lv = ov.LiveVisualizer([polygon], [directions], PNC)
    lists, drawn = [], 0
    for n, (rows, fidx) in enumerate(rec.batches):
        b = min(PB, PT - n * PB)
        lists.append(lv.batch_prims([0] * b, range(n * PB + 1, n * PB + b + 1), per_frame(rows, fidx, b), (PH, PW)))
        drawn += int((lists[-1][0][:, 0] == ov.RECT).sum())
    print(f"{len(lists)} batches, {drawn} boxes drawn, {len(got[0])} CSV rows")
    assert len(lists) == (PT + PB - 1) // PB and drawn == len(got[0])            # every CSV row is a box in the picture (rows outside a zone: the engine tests above)
    want = rendered_by_submit(pipe.engine, frames, lists, sink_kw, PB)
    data = surf.cpu().numpy().reshape(PT, -1) if device else sink.data
    for i in range(PT):
        np.testing.assert_array_equal(data[i], want[i], err_msg=f"frame {i + 1}")
    assert live.counts_of(0) == got[1]


def test_run_streams_annotate_returns_the_order_and_the_same_frames(pipe, golden_dir, tmp_path):
    from vehicle_counting_amd.counting import load_zone_anno
    from vehicle_counting_amd.pipeline import FrameSource, YuvFrameSink
    from vehicle_counting_amd.synth import synth_frames
    zone = pipe_zone(golden_dir, tmp_path)
    clip18 = synth_frames(PT, PH, PW, n_obj=6, seed=3)                           # two windows of the calibrated clip: 10 and 7 frames, 17 = 4 x 4 + 1
    clips = [np.ascontiguousarray(clip18[:10]), np.ascontiguousarray(clip18[8:15])]
    names, zones = ["cam_a", "cam_b"], [zone, zone]
    sources = [FrameSource(c) for c in clips]
    plain = pipe.run_streams(sources, names, zones, batch=PB)
    with pytest.raises(ValueError):
        pipe.run_streams(sources, names, zones, batch=PB, mixed_sizes=True, live=pipe.open_live(names, zones), annotate=YuvFrameSink(PH, PW, n_frames=17))
    with pytest.raises(ValueError):
        pipe.run_streams(sources, names, zones, batch=PB, annotate=YuvFrameSink(PH, PW, n_frames=17))            # no live counter
    live = pipe.open_live(names, zones)
    sink = YuvFrameSink(PH, PW, n_frames=17)
    rec = Recorder(pipe.engine)
    try:
        got, order = pipe.run_streams(sources, names, zones, batch=PB, live=live, annotate=sink)
    finally:
        rec.close()
    print("CSV rows per camera:", [len(r) for r, _ in got])
    assert got == plain and sum(len(r) for r, _ in got) >= 1
    assert order == [(c, t + 1) for t in range(10) for c in range(2) if t < len(clips[c])] and len(order) == 17
    polygon, directions = load_zone_anno(zone)
    lv = ov.LiveVisualizer([polygon] * 2, [directions] * 2, PNC)
    lists = []
    for n, (rows, fidx) in enumerate(rec.batches):
        part = order[n * PB:(n + 1) * PB]
        lists.append(lv.batch_prims([c for c, _ in part], [f for _, f in part], per_frame(rows, fidx, len(part)), (PH, PW)))
    interleaved = np.stack([clips[c][f - 1] for c, f in order])
    want = rendered_by_submit(pipe.engine, interleaved, lists, {}, PB)
    for i in range(17):
        np.testing.assert_array_equal(sink.data[i], want[i], err_msg=f"sink frame {i}: camera {order[i][0]} frame {order[i][1]}")
