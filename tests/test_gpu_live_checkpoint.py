"""GPU: the live checkpoint (csrc/live_ckpt.hip, format csrc/live_ckpt.h) -- a counter and its trackers packed on the device behind an
uncollected batch, restored onto a counter of ANOTHER engine (other max_tracks, larger nn_budget_cap, a partly occupied pool) and fed
the rest of the stream: rows, frame numbers, counts, stats, overlay lists and tracker states equal the uninterrupted run exactly.  The
blob against vc_tracker_snapshot field by field; checkpoint -> restore -> checkpoint; one camera migrating through cam_map; every refusal
leaving the counter as it was; no effect when unused; CountingPipeline.run_streams(checkpoint_every=) + open_live(resume=).

Shapes: 2 cameras x 2 labels, 64 x 96 frames, 24 frames per camera interleaved, batches of 3, max_age 2, n_init 1, nn_budget 3; the cut
is behind batch 8 of 16 (camera 0 has had 14 frames, camera 1 13)."""
import struct

import numpy as np
import pytest

import live_ckpt_cases as K
from test_gpu_live_count import CAM_DIRS, H, NL, W, ZONE

pytestmark = pytest.mark.gpu

T, B, CUT = 24, 3, 8
TRACK_KW = dict(max_dist=0.2, min_confidence=0.25, nms_max_overlap=1.0, max_iou_distance=0.7, max_age=2, n_init=1, nn_budget=3)
DIR_KEYS = [[1, 2], [1, 2, 3]]
# per camera: (label, first frame, last frame, x, y, vx, vy, w, h).  The zone is x <= 60.  At the cut (camera 0 frame 13, camera 1 frame 12):
#   camera 0, label 0: A lives through the clip in the zone (wrapped ring, open LiveSlot); B never enters the zone and is deleted early;
#                      C ends at frame 9 and is deleted at frame 12, INSIDE the cut batch (freed there, its LiveSlot folded into base);
#                      D is born in the very last frame before the cut: tentative
#   camera 0, label 1: E through the clip; F outside the zone, deleted at frame 8; G born at frame 9 into a slot a deleted track gave back
#   camera 1, label 0: H through the clip; I in the zone, deleted at frame 7; J outside the zone from frame 8, last seen at frame 11: alive, closed LiveSlot
#   camera 1, label 1: nothing until frame 16: a tracker without a track (it has never been stepped)
OBJECTS = [
    [(0, 0, 23, 5, 8, 2.0, 0.0, 14, 12), (0, 0, 3, 72, 40, 0.0, 0.0, 14, 12), (0, 6, 9, 20, 46, 2.0, 0.0, 14, 12), (0, 13, 23, 30, 28, 1.0, 0.0, 14, 12),
     (1, 0, 23, 20, 4, 0.0, 1.5, 12, 14), (1, 2, 5, 75, 30, 0.0, 0.0, 14, 12), (1, 9, 23, 44, 44, -1.0, 0.0, 12, 14)],
    [(0, 0, 23, 8, 46, 1.0, 0.0, 14, 12), (0, 1, 4, 56, 6, -2.0, 0.0, 14, 12), (0, 8, 11, 70, 20, 0.0, 0.0, 14, 12), (1, 16, 23, 22, 26, 0.0, 1.0, 12, 14)],
]
ORDER = [(c, t) for t in range(T) for c in range(2)]
N_BATCHES = len(ORDER) // B
POOL_A = 8                            # max_tracks of the first engine: fewer slots than tracks created before the cut, so slots are reused


def clip(cam):
    rng = np.random.default_rng(300 + cam)
    bg = rng.integers(60, 120, (H, W, 3), dtype=np.uint8)
    tex = [rng.integers(0, 256, (o[8], o[7], 3), dtype=np.uint8) for o in OBJECTS[cam]]
    frames = np.repeat(bg[None], T, 0).copy()
    boxes = []
    for t in range(T):
        bl = []
        for k, (label, t0, t1, x, y, vx, vy, w, h) in enumerate(OBJECTS[cam]):
            if t0 <= t <= t1:
                x1, y1 = int(round(x + vx * (t - t0))), int(round(y + vy * (t - t0)))
                assert 0 <= x1 and x1 + w < W and 0 <= y1 and y1 + h < H
                frames[t, y1:y1 + h, x1:x1 + w] = tex[k]
                bl.append((x1, y1, w, h, label))
        boxes.append(bl)
    return frames, boxes


class Feed:
    """frames of `order` (camera, frame) on the device with their injected detections; batch k = frames [k * B, (k + 1) * B)"""

    def __init__(self, order, cam_index=None):
        import torch
        clips = [clip(0), clip(1)]
        self.order = order
        self.cams = [c if cam_index is None else cam_index[c] for c, _ in order]
        self.dev = torch.from_numpy(np.stack([clips[c][0][t] for c, t in order])).cuda()
        nmax = max(len(b) for c in range(2) for b in clips[c][1])
        self.det, self.cnt = np.zeros((len(order), nmax, 6), np.float32), np.zeros(len(order), np.int32)
        for g, (c, t) in enumerate(order):
            for i, (x, y, w, h, label) in enumerate(clips[c][1][t]):
                self.det[g, i] = (x, y, x + w, y + h, 0.9, label)
            self.cnt[g] = len(clips[c][1][t])
        self.n_batches = (len(order) + B - 1) // B

    def run(self, eng, tids, k):
        f0, f1 = k * B, min((k + 1) * B, len(self.order))
        eng.stream_inject(self.det[f0:f1], self.cnt[f0:f1])
        eng.stream_submit(self.dev[f0:f1].data_ptr(), f1 - f0, H, W)
        eng.stream_run_async_multi(tids, self.cams[f0:f1], self.dev[f0:f1].data_ptr(), f1 - f0, H, W, cap_rows=32)


def make_engine(max_tracks, nn_budget_cap):
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd.weights import synth_reid, synth_yolo
    return E.Engine(synth_yolo("yolov5s", nc=NL, seed=1702, det_scale=4.0, obj_shift=-2.0), synth_reid(1702), precision="f32", num_classes=NL,
                    max_batch=B, max_frame_hw=(H, W), max_crops=B * 16, max_tracks=max_tracks, nn_budget_cap=nn_budget_cap, max_trackers=32)


class Cams:
    """trackers [n_cam][NL] and their counter on an engine; cams: which of the two cameras' zones"""

    def __init__(self, eng, cams=(0, 1), overlay=True, ckpt_bytes=1 << 20, **kw):
        import vehicle_counting_amd.engine as E
        self.eng = eng
        self.tids = np.array([[eng.tracker_create(**dict(TRACK_KW, **kw)) for _ in range(NL)] for _ in cams], np.int32)
        self.live = E.LiveCounter(eng, self.tids, [ZONE for _ in cams], [CAM_DIRS[c] for c in cams])
        self.overlay = overlay
        if overlay:
            self.live.enable_overlay([DIR_KEYS[c] for c in cams], max_batch=B, max_rows_per_frame=16, depth=2)
        if ckpt_bytes:
            self.live.enable_checkpoint(ckpt_bytes)

    def observe(self):
        counts, done = self.live.counts(with_frames=True)
        return dict(counts=counts, frames_done=done, stats=self.live.stats(), state=[self.eng.tracker_state(int(t)) for t in self.tids.reshape(-1)])

    def step(self, feed, k, after_run=None):
        """batch k: run, (after_run), collect, and what the counter and the trackers say behind it"""
        feed.run(self.eng, self.tids, k)
        if after_run is not None:
            after_run()
        rows, fidx, nd = self.eng.stream_collect()
        rec = dict(rows=rows.copy(), fidx=fidx.copy(), nd=nd.copy(), **self.observe())
        if self.overlay:
            rec["lists"] = self.live.overlay_lists()
        return rec

    def close(self):
        self.eng.stream_inject(None)
        self.eng.stream_reset()
        self.live.close()
        for t in self.tids.reshape(-1):
            self.eng.tracker_destroy(int(t))


def same_state(a, b, where):
    for f in ("ids", "state", "hits", "age", "tsu", "gallery", "mean", "cov"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{where}: {f}")


def same_batch(a, b, where, lists=True):
    for f in ("rows", "fidx", "nd", "counts", "frames_done"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{where}: {f}")
    assert a["stats"] == b["stats"], where
    for i, (x, y) in enumerate(zip(a["state"], b["state"])):
        same_state(x, y, f"{where}, tracker {i}")
    if lists:
        np.testing.assert_array_equal(a["lists"][0], b["lists"][0], err_msg=f"{where}: prims")
        np.testing.assert_array_equal(a["lists"][1], b["lists"][1], err_msg=f"{where}: frame_first")


def unchanged(cams, before, where):
    now = cams.observe()
    np.testing.assert_array_equal(now["counts"], before["counts"], err_msg=where)
    np.testing.assert_array_equal(now["frames_done"], before["frames_done"], err_msg=where)
    assert now["stats"] == before["stats"], where
    for i, (x, y) in enumerate(zip(now["state"], before["state"])):
        same_state(x, y, f"{where}, tracker {i}")


def refused(call, code, where):
    from vehicle_counting_amd._lib import VcError
    with pytest.raises(VcError) as ei:
        call()
    assert ei.value.code == code, (where, str(ei.value))


@pytest.fixture(scope="module")
def runs():
    """Everything that runs on the GPU, once: A straight through; B with a checkpoint behind the uncollected cut batch (then to the end);
    D with a staging buffer that is too small and a blob whose nn_budget exceeds the engine's cap; E with too few free slots; C on a second engine from the blob, with the
    refusals in front of its first batch; M: camera 1 alone."""
    import vehicle_counting_amd.engine as E
    out = {}
    feed = Feed(ORDER)
    eng_a, eng_c = make_engine(POOL_A, 3), make_engine(32, 6)
    try:
        # ---- A
        a = Cams(eng_a, ckpt_bytes=0)
        out["A"] = [a.step(feed, k) for k in range(N_BATCHES)]
        a.close()
        # ---- B
        b = Cams(eng_a)
        rec_b, extra = [], {}
        for k in range(N_BATCHES):
            rec_b.append(b.step(feed, k, after_run=b.live.checkpoint_begin if k == CUT else None))
            if k == CUT:
                refused(b.live.checkpoint_begin, 3, "begin twice")
                extra["refused_begin_twice"] = True
                out["blob"] = b.live.checkpoint_end()
                refused(b.live.checkpoint_end, 3, "end without begin")
                extra["refused_end_without_begin"] = True
                out["snapshots"] = [eng_a.tracker_snapshot(int(t)) for t in b.tids.reshape(-1)]         # drained: allowed for attached trackers
                out["blob_drained"] = b.live.checkpoint()
        out["B"], out["B_extra"] = rec_b, extra
        b.close()
        # ---- a blob whose trackers have nn_budget 5, made where that fits
        c5 = Cams(eng_c, overlay=False, nn_budget=5)
        out["blob_budget5"] = c5.live.checkpoint()
        c5.close()
        # ---- D: max_bytes below the state; then the refusals of the small engine
        d = Cams(eng_a, overlay=False, ckpt_bytes=K.tracks_off(2, 3, NL) + 4 * 704)
        rec_d = []
        for k in range(6):
            rec_d.append(d.step(feed, k, after_run=d.live.checkpoint_begin if k == 2 else None))
            if k == 2:
                refused(d.live.checkpoint_end, 4, "max_bytes smaller than the state")
                refused(d.live.checkpoint_end, 3, "the overflowed checkpoint is dropped")
            if k == 3:
                before = d.observe()
                refused(lambda: d.live.restore(out["blob_budget5"]), 4, "nn_budget above the cap")
                unchanged(d, before, "nn_budget above the cap")
        out["D"] = rec_d
        d.close()
        # ---- E: too few free slots -- the pool mostly taken by an unrelated tracker, a counter without tracks
        spare = eng_a.tracker_create(**TRACK_KW)
        eng_a.tracker_step(spare, np.array([[5 + 20 * i, 5, 10, 10] for i in range(4)], np.float64), np.full(4, 0.9),
                           np.random.default_rng(5).normal(size=(4, 512)).astype(np.float32))
        e = Cams(eng_a, overlay=False, ckpt_bytes=0)
        before = e.observe()
        assert POOL_A - 4 < K.parse(out["blob"])["header"]["n_tracks"]
        refused(lambda: e.live.restore(out["blob"]), 4, "too few free slots")
        unchanged(e, before, "too few free slots")
        assert len(eng_a.tracker_state(spare)["ids"]) == 4
        eng_a.tracker_destroy(spare)
        # ... and a restore while a batch is enqueued but not collected: refused, nothing touched, the batch's rows as ever
        out["E"] = [e.step(feed, 0, after_run=lambda: refused(lambda: e.live.restore(out["blob"]), 3, "restore with a batch outstanding")), e.step(feed, 1)]
        e.close()
        # ---- C: second engine, pool partly occupied by an unrelated tracker, trackers created with OTHER parameters
        other = eng_c.tracker_create(**TRACK_KW)
        rng = np.random.default_rng(6)
        eng_c.tracker_step(other, np.array([[5, 5, 10, 10], [40, 5, 10, 10], [70, 30, 10, 10]], np.float64), np.full(3, 0.9), rng.normal(size=(3, 512)).astype(np.float32))
        other_before = eng_c.tracker_state(other)
        c = Cams(eng_c, max_age=30, n_init=3, nn_budget=6, min_confidence=0.5)
        blob = out["blob"]
        fresh = c.observe()
        zone_off = K.camera_off(1, 3, NL) + K.CAMERA.fields["polygon"][1] + 16
        one_label = E.LiveCounter(eng_c, [[eng_c.tracker_create(**TRACK_KW)], [eng_c.tracker_create(**TRACK_KW)]], [ZONE, ZONE], CAM_DIRS)
        for where, call, code in [("truncated blob", lambda: c.live.restore(blob[:-2048]), 1), ("truncated to nothing", lambda: c.live.restore(blob[:10]), 1),
                                  ("wrong magic", lambda: c.live.restore(b"VCTRK01\0" + blob[8:]), 1),
                                  ("changed zone", lambda: c.live.restore(K.apply_patch(blob, zone_off, struct.pack("<d", 61.0))), 1),
                                  ("zones swapped by cam_map", lambda: c.live.restore(blob, cam_map=[1, 0]), 1),
                                  ("n_labels mismatch", lambda: one_label.restore(blob), 1)]:
            refused(call, code, where)
            unchanged(c, fresh, where)
        one_label.close()
        c.live.restore(blob)
        out["C_restored"] = c.observe()
        out["blob_again"] = c.live.checkpoint()
        for where, call in [("truncated blob", lambda: c.live.restore(blob[:-16])), ("wrong magic", lambda: c.live.restore(b"X" + blob[1:])),
                            ("changed zone", lambda: c.live.restore(K.apply_patch(blob, zone_off, struct.pack("<d", 61.0))))]:
            refused(call, 1, where)
            unchanged(c, out["C_restored"], where + " (restored counter)")
        out["C"] = [c.step(feed, k) for k in range(CUT + 1, N_BATCHES)]
        same_state(eng_c.tracker_state(other), other_before, "the unrelated tracker")
        c.close()
        # ---- M: camera 1 of the blob into camera 0 of a one-camera counter
        m = Cams(eng_c, cams=(1,), overlay=False)
        m.live.restore(blob, cam_map=[-1, 0])
        done1 = int(out["B"][CUT]["frames_done"][1])
        feed1 = Feed([(1, t) for t in range(done1, T)], cam_index={1: 0})
        out["M"] = [m.step(feed1, k) for k in range(feed1.n_batches)]
        out["M_first_frame"] = done1
        m.close()
        eng_c.tracker_destroy(other)
    finally:
        eng_a.close()
        eng_c.close()
    return out


def test_the_clip_reaches_the_cases(runs):
    a, p = runs["A"], K.parse(runs["blob"])
    tracks = [t["tracks"] for t in p["trackers"]]
    everything = np.concatenate(tracks)
    nn = TRACK_KW["nn_budget"]
    assert any(r["rec"]["gal_count"] == nn and r["rec"]["gal_head"] != 0 for r in everything), "a wrapped ring"
    ids_before = [set(s["ids"].tolist()) for s in a[CUT - 1]["state"]]
    ids_at = [set(s["ids"].tolist()) for s in a[CUT]["state"]]
    assert any(x - y for x, y in zip(ids_before, ids_at)), "a track freed in the batch before the cut"
    assert a[CUT]["stats"][1] > a[CUT - 1]["stats"][1], "... whose LiveSlot was folded into base there"
    created = sum(int(t["params"]["next_id"]) - 1 for t in p["trackers"])
    assert created > POOL_A >= len(everything), "a reused slot: more tracks were created than the pool has slots"
    assert any(r["rec"]["state"] == K.TENTATIVE for r in everything), "a tentative track at the cut"
    assert any(len(t) == 0 for t in tracks), "a tracker with no tracks"
    done = [int(c["frames_done"]) for c, _ in p["cameras"]]
    assert done == a[CUT]["frames_done"].tolist() and done[0] != done[1] and done == [14, 13], "cameras with different frames_done"
    assert any(r["slot"]["open"] == 1 for r in everything) and any(r["slot"]["open"] == 0 for r in everything), "open and closed LiveSlots"
    assert p["retired"] == a[CUT]["stats"][1] and a[CUT]["stats"][0] == sum(int(r["slot"]["open"]) for r in everything)
    assert CUT < N_BATCHES - 1 and sum(len(r["rows"]) for r in a[CUT + 1:]) > 30


def test_continuation_on_a_second_engine(runs):
    a, c = runs["A"], runs["C"]
    assert len(c) == N_BATCHES - CUT - 1
    np.testing.assert_array_equal(runs["C_restored"]["counts"], a[CUT]["counts"])
    np.testing.assert_array_equal(runs["C_restored"]["frames_done"], a[CUT]["frames_done"])
    assert runs["C_restored"]["stats"] == a[CUT]["stats"]
    for i, (x, y) in enumerate(zip(runs["C_restored"]["state"], a[CUT]["state"])):
        same_state(x, y, f"right after the restore, tracker {i}")
    for k, rec in enumerate(c):
        same_batch(rec, a[CUT + 1 + k], f"batch {CUT + 1 + k}")
    assert c[-1]["counts"].sum() > runs["C_restored"]["counts"].sum()


def test_blob_equals_tracker_snapshot(runs):
    """every tracker's section against vc_tracker_snapshot of that tracker at the cut, field by field and gallery row by row"""
    p = K.parse(runs["blob"])
    assert runs["blob"] == runs["blob_drained"]                        # packed behind the uncollected batch = packed on the drained engine
    for t, (tk, snap) in enumerate(zip(p["trackers"], runs["snapshots"])):
        magic, feat_dim, n_tracks, next_id, max_dist, min_conf, nms, max_iou, max_age, n_init, nn_budget, _ = struct.unpack_from("<8siiqddddiiii", snap, 0)
        assert magic == b"VCTRK01\0" and feat_dim == 512
        k = tk["params"]
        assert (n_tracks, next_id, max_dist, min_conf, nms, max_iou, max_age, n_init, nn_budget) == tuple(
            k[f].item() for f in ("n_tracks", "next_id", "max_dist", "min_confidence", "nms_max_overlap", "max_iou_distance", "max_age", "n_init", "nn_budget")), t
        o = 72
        for i in range(n_tracks):
            rec = struct.unpack_from("<qiiiiii", snap, o)
            assert rec == tuple(tk["tracks"][i]["rec"][f].item() for f in K.REC.names), (t, i)
            assert snap[o + 40:o + 40 + 576] == tk["tracks"][i]["mean"].tobytes() + tk["tracks"][i]["cov"].tobytes(), (t, i)
            rows = min(rec[5], nn_budget)
            o += 616
            for r in range(rows):
                assert snap[o + r * 2048:o + (r + 1) * 2048] == tk["gallery"][i][r].tobytes(), (t, i, r)
            o += rows * 2048
        assert o == len(snap)


def test_round_trip(runs):
    assert runs["blob_again"] == runs["blob"]
    from vehicle_counting_amd import _lib as L
    buf = runs["blob"]
    assert L.lib().vc_live_ckpt_validate_host(buf, len(buf)) == 0 and L.lib().vc_live_ckpt_validate_host(buf, len(buf) - 1) == 1


def test_one_camera_migrates_through_cam_map(runs):
    a, m, first = runs["A"], runs["M"], runs["M_first_frame"]
    want = {}                                                          # camera 1's rows of run A per frame
    for k, rec in enumerate(a):
        for f in range(B):
            cam, t = ORDER[k * B + f]
            if cam == 1:
                want[t] = (rec["rows"][rec["fidx"] == f], rec["nd"][f])
    n = 0
    for k, rec in enumerate(m):
        for f in range(len(rec["nd"])):
            t = first + k * B + f
            np.testing.assert_array_equal(rec["rows"][rec["fidx"] == f], want[t][0], err_msg=f"camera 1, frame {t}")
            assert rec["nd"][f] == want[t][1]
            n += len(want[t][0])
        assert rec["frames_done"].tolist() == [min(first + (k + 1) * B, T)]
        for ra in a:                                                   # the batches of A behind which camera 1 had had as many frames
            if ra["frames_done"][1] == rec["frames_done"][0]:
                np.testing.assert_array_equal(rec["counts"][0], ra["counts"][1], err_msg=f"camera 1 after {rec['frames_done'][0]} frames")
                for x, y in zip(rec["state"], ra["state"][NL:]):
                    same_state(x, y, f"camera 1 after {rec['frames_done'][0]} frames")
    assert n > 10
    np.testing.assert_array_equal(m[-1]["counts"][0], a[-1]["counts"][1])


def test_refusals_leave_everything_unchanged(runs):
    """the refusals themselves, and the state behind each, are asserted where they happen (the `runs` fixture); here: the streams they
    happened in went on to the same rows as A"""
    assert runs["B_extra"] == {"refused_begin_twice": True, "refused_end_without_begin": True}
    for k, rec in enumerate(runs["D"]):                                # max_bytes too small at batch 2; nn_budget above the cap at batch 3
        same_batch(rec, runs["A"][k], f"run D, batch {k}", lists=False)
    for k, rec in enumerate(runs["E"]):                                # too few free slots, in front of the first batch
        same_batch(rec, runs["A"][k], f"run E, batch {k}", lists=False)
    for k, rec in enumerate(runs["C"]):                                # truncated / magic / zone / n_labels refusals in front of and behind the restore
        same_batch(rec, runs["A"][CUT + 1 + k], f"run C, batch {CUT + 1 + k}")


def test_no_effect_when_unused_or_used(runs):
    """A never enabled checkpoints; B enabled them and took two at the cut: bit-equal rows, counts, states and overlay lists throughout"""
    assert len(runs["B"]) == len(runs["A"]) == N_BATCHES
    for k, (x, y) in enumerate(zip(runs["B"], runs["A"])):
        same_batch(x, y, f"batch {k}")


def test_pipeline_checkpoint_every_and_resume(golden_dir, tmp_path):
    """run_streams(live=, checkpoint_every=2) to the end; then the first part again on new sources cut at a checkpoint and a second call with
    open_live(resume=blob) on the rest: the concatenated rows equal the uninterrupted call's, frame numbers continue, final counts equal."""
    import types

    import test_gpu_mixed_sizes as MS
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource
    from vehicle_counting_amd.weights import synth_reid, synth_yolo
    names = ["cam_00", "cam_01"]
    sources, _, sizes = MS.four_cameras()
    h, w = sizes[0]
    clips = [sources[0].frames[:12], sources[0].frames[:12][::-1].copy()]          # two cameras of one size: a clip and the same clip backwards
    zone_paths = [MS.whole_frame_zone(golden_dir, tmp_path, "cam_04_halfres.json", h, w)] * 2
    e = E.Engine(synth_yolo("yolov5s", nc=MS.NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702), precision="f32", num_classes=MS.NC, max_batch=4,
                 max_frame_hw=MS.MAX_HW, max_crops=4 * 300, max_tracks=2048, nn_budget_cap=60, max_trackers=4 * MS.NC)
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path))
    pipe = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": MS.TRACK_CFG} for n in names}}, engine=e, class_names=[f"c{i}" for i in range(MS.NC)])
    batch = 4

    def srcs(lo, hi):
        return [FrameSource(c[lo:hi], name=n + ".mp4") for c, n in zip(clips, names)]

    try:
        plain = pipe.open_live(names, zone_paths)
        want = pipe.run_streams(srcs(0, 12), names, zone_paths, batch=batch, live=plain)
        want_counts = plain.counts()
        ckpts = []
        live = pipe.open_live(names, zone_paths, on_checkpoint=lambda n, blob, done: ckpts.append((n, blob, np.array(done))), checkpoint_bytes=64 << 20)
        got = pipe.run_streams(srcs(0, 12), names, zone_paths, batch=batch, live=live, checkpoint_every=2)
        assert [n for n, _, _ in ckpts] == [1, 3, 5] and [d.tolist() for _, _, d in ckpts] == [[4, 4], [8, 8], [12, 12]]
        # every batch: batch n + 1 runs before batch n is collected, one checkpoint is in flight at a time
        each, each1 = [], []
        live1 = pipe.open_live(names, zone_paths, on_checkpoint=lambda n, blob, done: each.append((n, blob, done.tolist())), checkpoint_bytes=64 << 20)
        got1 = pipe.run_streams(srcs(0, 12), names, zone_paths, batch=batch, live=live1, checkpoint_every=1)
        assert [(n, d) for n, _, d in each] == [(n, [2 * n + 2] * 2) for n in range(6)] and each[3][1] == ckpts[1][1]
        live1 = pipe.open_live(names[:1], zone_paths[:1], on_checkpoint=lambda n, blob, done: each1.append((n, done.tolist())), checkpoint_bytes=64 << 20)
        one = pipe.run_stream(srcs(0, 12)[0], names[0], zone_paths[0], batch=batch, asynchronous=True, live=live1, checkpoint_every=1)
        assert each1 == [(n, [4 * n + 4]) for n in range(3)]
        key = lambda rows: sorted((r["frame_id"], r["track_id"], r["label"], tuple(r["box"])) for r in rows)
        for c in range(2):                                             # checkpointing does not perturb the stream
            assert len(want[c][0]) >= 10 and key(got[c][0]) == key(want[c][0]) and got[c][1] == want[c][1]
            assert key(got1[c][0]) == key(want[c][0]) and got1[c][1] == want[c][1]
        assert key(one[0]) == key(want[0][0]) and one[1] == want[0][1]
        np.testing.assert_array_equal(live.counts(), want_counts)
        _, blob, done = ckpts[1]                                       # resume behind frame 8 of both cameras
        resumed = pipe.open_live(names, zone_paths, resume=blob)
        rest = pipe.run_streams(srcs(8, 12), names, zone_paths, batch=batch, live=resumed)
        for c in range(2):                                             # (direction, fpoint, fframe ... of the resumed part cover that part alone)
            head = [r for r in want[c][0] if r["frame_id"] <= 8]
            assert len(rest[c][0]) >= 3 and min(r["frame_id"] for r in rest[c][0]) == 9
            assert key(head + rest[c][0]) == key(want[c][0])
        np.testing.assert_array_equal(resumed.counts(), want_counts)
    finally:
        e.close()
