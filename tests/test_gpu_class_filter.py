"""GPU: the class filter and label map (class_filter.hip) -- the two kernels on known input through vc_class_filter_nms_host, and the
engine's detect paths with a map set (vc_engine_set_class_map).

Kernels: rows bit-equal to the float32 oracle on the frames with the dropped candidates removed, the kept count and the stable positions
of the kept candidates equal (tests/class_filter_cases.py; its conditions are asserted on the CPU by tests/test_class_filter_cases.py).
Engine: against oracle.yolov5's non_max_suppression(classes=...) where max_det binds, and bit for bit against the same engine's
unfiltered result filtered on the host where no cap binds.  CSV: the per-video loop of the oracle with the filter and the relabel, in
four drivers, by the rules of tests/test_gpu_pipeline.py::test_csv_parity."""
import functools
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import class_filter_cases as F  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd._lib import PROF_DETECT_AUX, VcError  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource  # noqa: E402

NC = F.NC
VC_ERR_STATE = 3
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
H, W = F.CLIP["H"], F.CLIP["W"]


# ------------------------------------------------------------------------------------------------------------------- 1. kernels
def _run(case, table=None):
    fr = case.frames
    return E.class_filter_nms([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], case.counts, case.table if table is None else table,
                              iou=case.iou, max_det=case.max_det, max_cand=case.max_cand, geoms=case.geoms)


@pytest.mark.parametrize("name", sorted(F.filter_cases()))
def test_kernels_match_the_filtered_oracle(name):
    case, ref = F.filter_cases()[name], F.filter_ref(name)
    out, n_out, kept, kept_idx = _run(case)
    for f, (rows, pos) in enumerate(ref):
        assert kept[f] == len(pos), (name, f, kept[f], len(pos))
        np.testing.assert_array_equal(kept_idx[f, :kept[f]], pos, err_msg=f"{name} frame {f}")
        assert n_out[f] == len(rows), (name, f, n_out[f], len(rows))
        np.testing.assert_array_equal(out[f, :n_out[f]].view(np.uint32), rows.view(np.uint32), err_msg=f"{name} frame {f}")


def test_identity_map_is_the_plain_nms():
    for name in ("identity", "edges_interleaved", "geometry", "mixed"):
        case = F.filter_cases()[name]
        fr = case.frames
        want, want_n = E.nms_batch([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], case.counts, iou=case.iou, max_det=case.max_det, max_cand=case.max_cand, geoms=case.geoms)
        out, n_out, kept, kept_idx = _run(case, table=np.arange(NC))
        np.testing.assert_array_equal(kept, case.counts)
        np.testing.assert_array_equal(n_out, want_n)
        for f, n in enumerate(case.counts):
            np.testing.assert_array_equal(kept_idx[f, :n], np.arange(n))
            np.testing.assert_array_equal(out[f, :n_out[f]].view(np.uint32), want[f, :want_n[f]].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- 2. engine, max_det binds
def check_dets(dets, ref, atol_px=5e-2):
    """tests/test_gpu_configs.py::check_dets"""
    assert len(dets) == len(ref)
    for d, r in zip(dets, ref):
        assert len(d) == len(r), (len(d), len(r))
        if len(r):
            np.testing.assert_array_equal(d[:, 5], r[:, 5])
            np.testing.assert_allclose(d[:, :4], r[:, :4], rtol=0, atol=atol_px)
            np.testing.assert_allclose(d[:, 4], r[:, 4], rtol=0, atol=2e-4)


def test_engine_filters_in_front_of_the_max_det_cut():
    frames, ysd, _ = F.clip()
    ids = (6, 7, 11, 17)
    table = F.table_of(F.SWAP)
    ref, binds = [], 0
    for i in ids:
        full = F.clip_detect(i, classes=[3, 7], max_det=300)
        if len(full) > 10:                                           # the cut binds: the score gap across it is far above the conf tolerance
            gap = float(full[9, 4] - full[10, 4])
            print(f"frame {i}: {len(full)} rows of classes 3 / 7, score gap at the cut {gap:.4f}")
            assert gap > 2e-3, (i, gap)
            binds += 1
        ref.append(F.relabel_dets(F.clip_detect(i, classes=[3, 7], max_det=10), table))
    assert binds >= 2 and all(len(r) for r in ref)
    eng = E.Engine(ysd, None, precision="f32", num_classes=NC, max_batch=4, max_frame_hw=(H, W), max_det=10)
    eng.set_class_map(F.SWAP)
    assert eng.num_labels == 2
    np.testing.assert_array_equal(eng.class_map, table)
    dets = eng.detect([frames[i][:, :, ::-1] for i in ids])
    check_dets(dets, ref)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------- 3. no cap binds
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_map_equals_host_filter_where_no_cap_binds(precision):
    frames, ysd, _ = F.clip()
    imgs = [frames[i][:, :, ::-1] for i in range(8)]
    eng = E.Engine(ysd, None, precision=precision, num_classes=NC, max_batch=8, max_frame_hw=(H, W), max_det=300)
    assert eng.num_labels == NC
    np.testing.assert_array_equal(eng.class_map, np.arange(NC))
    plain = eng.detect(imgs)
    assert sum(len(d) for d in plain) > 50 and max(len(d) for d in plain) < 300
    for mapping in (F.SWAP, F.MERGE, F.SPARSE):
        eng.set_class_map(mapping)
        table = F.table_of(mapping)
        assert eng.num_labels == int(table.max()) + 1
        got = eng.detect(imgs)
        want = [F.relabel_dets(d, table) for d in plain]
        assert sum(len(d) for d in want) > 10
        for g, w_ in zip(got, want):
            assert g.shape == w_.shape, (mapping, g.shape, w_.shape)
            np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32))
    eng.set_class_map(None)
    again = eng.detect(imgs)
    for a, p in zip(again, plain):
        np.testing.assert_array_equal(a.view(np.uint32), p.view(np.uint32))
    # a map adds two launch scopes to the detector's tail (the filter, the relabel); without one the pass launches what it always did
    def aux_launches(mapping):
        eng.set_class_map(mapping)
        eng.profile_reset()
        eng.detect(imgs)
        return eng.profile_read(PROF_DETECT_AUX)["launches"]
    eng.profile(True)
    n_plain, n_map, n_cleared = aux_launches(None), aux_launches(list(range(NC))), aux_launches(None)
    eng.profile(False)
    assert n_plain > 0 and n_map == n_plain + 2 and n_cleared == n_plain, (n_plain, n_map, n_cleared)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------- 4. CSV
def key(rows):
    return [(r["label"], r["track_id"], r["frame_id"], r["direction"], r["fframe"], r["lframe"]) for r in rows]


def _zone(golden_dir):
    return os.path.join(golden_dir, "cam_04_halfres.json")


@functools.lru_cache(maxsize=None)
def csv_ref(zone, which):
    return F.run_video_classes(F.clip()[2], TRACK_CFG, zone, {"swap": F.SWAP, "merge": F.MERGE}[which])


def _trackers(eng, n):
    return [eng.tracker_create(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60) for _ in range(n)]


def _stream_counts(eng, frames, n_trackers, batch=8):
    """the clip through the stream path on fresh trackers: (detections per frame, boxes that reached the ReID stage)"""
    import torch
    eng.stream_reset()
    trk = _trackers(eng, n_trackers)
    dev = torch.from_numpy(frames).cuda()
    nd = []
    for f0 in range(0, len(frames), batch):
        b = min(batch, len(frames) - f0)
        eng.stream_submit(dev[f0:f0 + b].data_ptr(), b, H, W)
        nd.extend(eng.stream_run_packed(trk, dev[f0:f0 + b].data_ptr(), b, H, W)[2].tolist())
    boxes = eng.stream_crop_stats()[0]
    for t in trk:
        eng.tracker_destroy(t)
    return nd, boxes


@pytest.mark.parametrize("which,mode", [("swap", "loop"), ("swap", "stream"), ("swap", "stream_async_host"), ("swap", "frame_sharded"), ("merge", "stream")])
def test_csv_with_a_class_map(golden_dir, tmp_path, which, mode):
    frames, ysd, rsd = F.clip()
    zone = _zone(golden_dir)
    mapping = {"swap": F.SWAP, "merge": F.MERGE}[which]
    ref_rows, ref_counts, n_det = csv_ref(zone, which)
    print(f"{which}: {len(ref_rows)} CSV rows, {sum(n_det)} detections")
    assert len(ref_rows) > 10 and sum(n_det) > 50
    assert key(csv_ref(zone, "swap")[0]) != key(csv_ref(zone, "merge")[0])                 # merged is not swapped
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path))
    cam_cfg = {"cam": {"cam_04": {"tracking_config": TRACK_CFG}}}
    eng = E.Engine(ysd, rsd, precision="f32", num_classes=NC, max_batch=8, max_frame_hw=(H, W), max_crops=512, max_tracks=1024, nn_budget_cap=60)
    names = [f"c{i}" for i in range(NC)]
    pipe = CountingPipeline(args, cfg, cam_cfg, engine=eng, class_names=names, classes=mapping)
    assert pipe.class_names == (["c7", "c3"] if which == "swap" else ["c3"])
    src = FrameSource(frames)
    if mode == "loop":
        rows, counts = pipe.run(src, "cam_04", zone)
    elif mode == "frame_sharded":
        rows, counts = pipe.run_frame_sharded(src, "cam_04", zone, chunk=4)
    else:
        rows, counts = pipe.run_stream(src, "cam_04", zone, batch=4 if "async" in mode else 8, asynchronous="async" in mode, host_frames=mode.endswith("_host"))
    assert key(rows) == key(ref_rows), mode
    for r, q in zip(rows, ref_rows):
        assert np.abs(np.array(r["box"]) - np.array(q["box"])).max() <= 1, (mode, r, q)
        assert np.abs(np.array(r["fpoint"]) - np.array(q["fpoint"])).max() <= 0.5
        assert np.abs(np.array(r["lpoint"]) - np.array(q["lpoint"])).max() <= 0.5
    assert counts == ref_counts, mode
    assert all(len(v) == len(pipe.class_names) for v in counts.values())
    if mode == "stream":
        # only the kept classes reach the ReID stage: boxes seen = detections returned, fewer than the same engine sends without a map
        nd, boxes = _stream_counts(eng, frames, eng.num_labels)
        assert boxes == sum(nd) > 0
        eng.set_class_map(None)
        nd_all, boxes_all = _stream_counts(eng, frames, NC)
        assert boxes_all == sum(nd_all) and sum(nd) < sum(nd_all), (sum(nd), sum(nd_all))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------- 5. state rule
def test_set_class_map_is_refused_while_a_submission_is_pending():
    import torch
    frames, ysd, rsd = F.clip()
    eng = E.Engine(ysd, rsd, precision="f32", num_classes=NC, max_batch=4, max_frame_hw=(H, W), max_crops=256, max_tracks=512, nn_budget_cap=60)
    trk = _trackers(eng, NC)
    dev = torch.from_numpy(frames[:8]).cuda()
    eng.stream_submit(dev[:4].data_ptr(), 4, H, W)
    for attempt in (F.SWAP, None):
        with pytest.raises(VcError) as ei:
            eng.set_class_map(attempt)
        assert ei.value.code == VC_ERR_STATE
    rows0, _, nd0 = eng.stream_run_packed(trk, dev[:4].data_ptr(), 4, H, W)               # the pending batch ran without a map
    assert eng.num_labels == NC and nd0.sum() > 0
    eng.set_class_map(F.SWAP)                                                             # nothing pending any more
    assert eng.num_labels == 2
    eng.stream_submit(dev[4:8].data_ptr(), 4, H, W)
    rows1, _, nd1 = eng.stream_run_packed(trk[:2], dev[4:8].data_ptr(), 4, H, W)
    assert 0 < nd1.sum() and set(rows1[:, 5].tolist()) <= {0, 1}
    assert nd1.sum() == sum(len(d) for d in eng.detect([frames[i][:, :, ::-1] for i in range(4, 8)]))   # the blocking path under the same map
    eng.close()
