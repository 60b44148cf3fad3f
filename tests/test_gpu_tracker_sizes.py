"""GPU: the tracker kernels on the large side of their size switches (tests/tracker_size_cases.py; tests/test_tracker_size_cases.py shows
on the CPU that every scene gets there): galleries of 64, 65 and 100 samples whose nearest sample lies past ring position 64, more than
64 detections in a step, a tracker that outgrows the LDS state copy, the LDS cost rows and the LDS work arrays inside one launch, a
launch in which one tracker's appearance table fits the arena and another's does not, and the three capacity stops.

Against oracle.deepsort at the project's tolerances for these kernels (tests/test_gpu_tracker.py): ids, hits, age, time since update,
state, gallery sizes and emitted rows exact, means to 1e-9, cosine rows to 2e-6 with identical gate decisions, IoU rows to 1e-14."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tracker_size_cases as C  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from oracle import deepsort as od  # noqa: E402
from vehicle_counting_amd.weights import synth_reid  # noqa: E402

VC_ERR_CAPACITY = 4
ARENA_DEFAULT_MB = 1024
KEYS = ("ids", "state", "hits", "age", "tsu", "gallery")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(None, synth_reid(1702), precision="f32", max_crops=128, max_frame_hw=(720, 1280), max_tracks=512, nn_budget_cap=100)
    yield e
    e.close()


@pytest.fixture(params=[None, 0], ids=["tables", "inwalk"])
def arena(request, eng):
    """None: the default arena, every tracker has its table (track_batch_kernel<8, true>); 0: no arena, every row is computed inside
    the walk (track_batch_kernel<4, false>)."""
    eng.set_option("dot_arena_mb", ARENA_DEFAULT_MB if request.param is None else request.param)
    yield request.param
    eng.set_option("dot_arena_mb", ARENA_DEFAULT_MB)


def small_engine(**kw):
    return E.Engine(None, synth_reid(1702), precision="f32", max_crops=8, max_frame_hw=(64, 64), **kw)


def create(e, p):
    return e.tracker_create(max_dist=p["max_dist"], min_confidence=p.get("min_confidence", 0.3), nms_max_overlap=p.get("nms_max_overlap", 1.0),
                            max_iou_distance=p["max_iou_distance"], max_age=p["max_age"], n_init=p["n_init"], nn_budget=p["budget"])


def feed(e, tid, dets):
    e.tracker_step(tid, np.array([d["tlwh"] for d in dets]).reshape(-1, 4), np.array([d["conf"] for d in dets]),
                   np.array([d["feature"] for d in dets], dtype=np.float32).reshape(-1, 512))


def check_state(s, want, mean, where):
    for k, w in zip(KEYS, want):
        np.testing.assert_array_equal(s[k], np.asarray(w, dtype=s[k].dtype), err_msg=f"{k}, {where}")
    np.testing.assert_allclose(s["mean"], mean, rtol=1e-9, atol=1e-9, err_msg=f"mean, {where}")


def check_tracker(e, tid, trk, where):
    check_state(e.tracker_state(tid, with_cov=False), C.state_of(trk), np.array([k.mean for k in trk.tracks]).reshape(-1, 8), where)


def same_bits(a, b, where):
    for k in KEYS + ("mean", "cov"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k}, {where}")


@functools.lru_cache(maxsize=None)
def oracle_frames(name):
    """The oracle's side of a single-tracker scene, computed once: per frame the cost matrices the step matched on (as
    test_hot_kernel_cost_rows_match_the_oracle takes them) and the state after it."""
    sc = C.scene(name)
    ref = C.Probe(sc["p"])
    out = []
    for dets in sc["frames"]:
        ref.predict()
        conf = [i for i, k in enumerate(ref.tracks) if k.state == od.CONFIRMED]
        cand = [i for i, k in enumerate(ref.tracks) if not (k.state == od.CONFIRMED and k.tsu != 1)]
        cols = list(range(len(dets)))
        app = od.TrackerState._appearance_cost(ref, dets, conf, cols) if dets and conf else None
        iou = ref._iou_cost(dets, cand, cols) if dets and cand else None
        T = len(ref.tracks)
        ref.update(dets)
        out.append({"conf": conf, "cand": cand, "app": app, "iou": iou, "T": T, "state": C.state_of(ref),
                    "mean": np.array([k.mean for k in ref.tracks]).reshape(-1, 8)})
    return out


def check_costs(e, o, D, where):
    """-> (open appearance entries, gated ones, IoU entries) compared"""
    app, iou = e.tracker_debug_costs(cap=1 << 14)
    assert app.shape == (o["T"], D), (where, app.shape)
    n = [0, 0, 0]
    if o["app"] is not None:
        got, open_ = app[o["conf"]], o["app"] != od.GATED_COST
        np.testing.assert_array_equal(got == od.GATED_COST, ~open_, err_msg=f"gate, {where}")
        np.testing.assert_allclose(got[open_], o["app"][open_], rtol=0, atol=2e-6, err_msg=f"cosine, {where}")
        n[0], n[1] = int(open_.sum()), int((~open_).sum())
    if o["iou"] is not None:
        np.testing.assert_allclose(iou[o["cand"]], o["iou"], rtol=0, atol=1e-14, err_msg=f"iou, {where}")
        n[2] = o["iou"].size
    return n


def run_scene(e, name, tids, frames=None, first=0):
    """Feeds the scene's frames [first, ...) to every tracker of `tids` and holds each to the oracle after every frame: state, and the
    cost rows of the step."""
    sc, orc = C.scene(name), oracle_frames(name)
    total = np.zeros(3, np.int64)
    for t in range(first, len(sc["frames"]) if frames is None else frames):
        for tid in tids:
            feed(e, tid, sc["frames"][t])
            total += check_costs(e, orc[t], len(sc["frames"][t]), f"{name} frame {t}")
            check_state(e.tracker_state(tid, with_cov=False), orc[t]["state"], orc[t]["mean"], f"{name} frame {t}")
    return total


# ------------------------------------------------------------------------------------------------ galleries past 64, detections past 64
@pytest.mark.parametrize("name", ["deep_gallery_64", "deep_gallery_65", "deep_gallery_100", "deep_gallery_wide", "many_dets"])
def test_every_frame_matches_the_oracle(eng, arena, name):
    """Per frame: state and the kernel's own cost rows.  Without the arena the deep galleries run the second sample pass of
    appearance_row_wave (D <= 12) and appearance_row_dev (deep_gallery_wide); with it, appearance_row_table's repeated unroll over rows that
    track_plan_kernel numbered past 64 per slot; many_dets runs appearance_row_table's second detection pass."""
    tid = create(eng, C.scene(name)["p"])
    try:
        n_open, n_gated, n_iou = run_scene(eng, name, [tid])
    finally:
        eng.tracker_destroy(tid)
    assert n_open > 100 and n_gated > 100 and n_iou > 100, (n_open, n_gated, n_iou)


def test_snapshot_across_a_wrapped_ring(eng, arena):
    """deep_gallery(100) after the first wrap (gal_head != 0, more than 64 samples held): snapshot, restore into a second tracker of the
    engine, and both continue to the end like the oracle."""
    name, cut = "deep_gallery_100", 130
    assert max(oracle_frames(name)[cut - 1]["state"][2]) > 100                  # hits: the ring has wrapped, its head is not at 0
    tid, tid2 = create(eng, C.scene(name)["p"]), create(eng, dict(C.P_DEEP, budget=7, n_init=1))
    try:
        run_scene(eng, name, [tid], frames=cut)
        blob = eng.tracker_snapshot(tid)
        eng.tracker_restore(tid2, blob)
        assert eng.tracker_snapshot(tid2) == blob
        run_scene(eng, name, [tid, tid2], first=cut)
        same_bits(eng.tracker_state(tid), eng.tracker_state(tid2), "after the clip")
    finally:
        eng.tracker_destroy(tid); eng.tracker_destroy(tid2)


# ------------------------------------------------------------------------------------------------ one launch, several trackers
def launch(e, tids, frames, hw=C.FRAME_HW, cap_rows=512):
    import torch
    rows7, feat = C.walk_rows(frames)
    dev = torch.from_numpy(feat).cuda()
    torch.cuda.synchronize()
    return e.videotracker_run_features(tids, rows7, dev.data_ptr(), hw[0], hw[1], cap_rows=cap_rows)


def check_rows(got, want, where):
    assert [k for k, _ in got] == list(range(1, len(want) + 1)), where
    for (k, rows), w in zip(got, want):
        np.testing.assert_array_equal(rows, w, err_msg=f"{where}, frame key {k}")


def test_growing_walk_in_one_launch(eng, arena):
    """A tracker that starts empty and grows to 120 tracks inside one videotracker_run_features call: the host planned for no track, so
    the walk goes from the LDS state copy to the pool (T > 64), from LDS cost rows to the scratch (T * D > 512) and from LDS work arrays
    to the scratch (T + D > cap) on the way; a light tracker shares the launch."""
    sc = C.scene("growing_walk")
    trk, want = C.run_walk(sc["params"], sc["frames"])
    tids = [create(eng, p) for p in sc["params"]]
    try:
        got = launch(eng, tids, sc["frames"])
        check_rows(got, want, "growing_walk")
        assert sum(len(w) for w in want) > 250
        for c, tid in enumerate(tids):
            check_tracker(eng, tid, trk[c], f"growing_walk, tracker {c}")
    finally:
        for tid in tids:
            eng.tracker_destroy(tid)


def run_mixed_on(e, sc):
    tids = [create(e, p) for p in sc["params"]]
    try:
        for tid, b in zip(tids, sc["build"]):
            for d in b:
                feed(e, tid, d)
        got = launch(e, tids, sc["frames"])
        return got, [e.tracker_state(tid) for tid in tids]
    finally:
        for tid in tids:
            e.tracker_destroy(tid)


def test_mixed_table_fit(eng):
    """dot_arena_mb = 1: the light tracker's table fits, the heavy one's does not (track_batch_kernel<4, false> with use_table set for one
    workgroup and clear for the other -- or for both, when the heavy tracker's reservation comes first: an atomic decides).  Rows and
    states equal the oracle's, and, bit for bit, those of the same clip on fresh trackers under the default arena."""
    sc = C.scene("mixed_fit")
    trk, want, _ = C.run_mixed(sc)
    try:
        eng.set_option("dot_arena_mb", C.MIXED_ARENA_MB)
        got, states = run_mixed_on(eng, sc)
    finally:
        eng.set_option("dot_arena_mb", ARENA_DEFAULT_MB)
    check_rows(got, want, "mixed_fit")
    assert sum(len(w) for w in want) > 100
    for c, s in enumerate(states):
        check_state(s, C.state_of(trk[c]), np.array([k.mean for k in trk[c].tracks]).reshape(-1, 8), f"mixed_fit, tracker {c}")
    got2, states2 = run_mixed_on(eng, sc)
    for (k, rows), (k2, rows2) in zip(got, got2):
        assert k == k2
        np.testing.assert_array_equal(rows, rows2, err_msg=f"frame key {k}: 1 MB arena against the default")
    for c in range(2):
        same_bits(states[c], states2[c], f"tracker {c}: 1 MB arena against the default")


# ------------------------------------------------------------------------------------------------ capacity stops
def raises_capacity(call, *words):
    with pytest.raises(E.L.VcError) as ei:
        call()
    assert ei.value.code == VC_ERR_CAPACITY, ei.value
    for w in words:
        assert w in str(ei.value), ei.value
    return str(ei.value)


def test_pool_exhausted_stops_one_tracker_and_spares_the_other():
    """TERR_POOL: a pool of eight slots, A's third frame asks for the eighth and ninth.  The call fails naming A; B, which shared the
    launch, stepped every frame; A stays stopped until its reset; after both resets all eight slots are back (one of them came through
    the freed list and merge_free_kernel) and A runs a new scene like a fresh tracker."""
    clip = C.pool_clip()
    trk, _ = C.run_walk(clip["params"], clip["frames"])
    e = small_engine(max_tracks=C.POOL_SLOTS, nn_budget_cap=4)
    try:
        a, b = (create(e, p) for p in clip["params"])
        msg = raises_capacity(lambda: launch(e, [a, b], clip["frames"]), "track pool exhausted", "stopped until vc_tracker_reset")
        assert f"tracker {a & 0xffff}:" in msg, msg
        check_tracker(e, b, trk[1], "B after the launch that stopped A")
        raises_capacity(lambda: feed(e, a, clip["after"][0]), "track pool exhausted")
        check_tracker(e, b, trk[1], "B after A's refused step")
        e.tracker_reset(a); e.tracker_reset(b)
        feed(e, a, clip["eight"])
        s = e.tracker_state(a)
        np.testing.assert_array_equal(s["ids"], np.arange(1, C.POOL_SLOTS + 1))
        raises_capacity(lambda: feed(e, b, clip["after"][0][:1]), "track pool exhausted")      # ... and not one slot more
        e.tracker_reset(a); e.tracker_reset(b)
        ref = C.Probe(clip["params"][0])
        for t, d in enumerate(clip["after"]):
            ref.predict(); ref.update(d)
            feed(e, a, d)
            check_tracker(e, a, ref, f"A after the reset, frame {t}")
        assert len(ref.tracks) == 4 and all(k.state == od.CONFIRMED for k in ref.tracks)
    finally:
        e.close()


def build_lingering(e, groups, per, seed, extra):
    frames, new, dets = C.lingering(groups, per, seed, extra=extra)
    tid = create(e, C.P_LINGER)
    for d in frames:
        feed(e, tid, d)
    return tid, frames, new, dets


@pytest.fixture(scope="module")
def cap_eng():
    e = small_engine(max_tracks=1024, nn_budget_cap=1)
    yield e
    e.close()


def refused_step_leaves_the_tracker_alone(e, tid, dets, frames):
    before = e.tracker_state(tid)
    raises_capacity(lambda: feed(e, tid, dets), "per-tracker capacity", "stopped until vc_tracker_reset")
    same_bits(before, e.tracker_state(tid), "after the refused step")
    raises_capacity(lambda: feed(e, tid, dets[:1]), "per-tracker capacity")                   # stopped: a step that would fit is refused too
    same_bits(before, e.tracker_state(tid), "after the second refused step")
    e.tracker_reset(tid)
    ref = C.Probe(C.P_LINGER)
    for t, d in enumerate(frames[:3]):
        ref.predict(); ref.update(d)
        feed(e, tid, d)
        check_tracker(e, tid, ref, f"after the reset, frame {t}")


def test_track_cap_hard_limit(cap_eng):
    """TERR_TRACK_CAP at TC_HARD_CAP: 300 lingering confirmed tracks (held to the oracle) and 213 detections.  The refused step leaves
    ids, counters, means and covariances bit for bit as they were."""
    tid, frames, new, _ = build_lingering(cap_eng, 6, 50, 5001, 213)
    try:
        check_tracker(cap_eng, tid, C.run_single(C.P_LINGER, frames), "300 lingering tracks")
        assert len(cap_eng.tracker_state(tid, with_cov=False)["ids"]) + len(new) == C.TC_HARD_CAP + 1
        refused_step_leaves_the_tracker_alone(cap_eng, tid, new, frames)
    finally:
        cap_eng.tracker_destroy(tid)


def test_track_cap_tracks_per_tracker():
    """TERR_TRACK_CAP at the engine's tracks_per_tracker = 16 (the a.list_cap arm of the check): 10 tracks + 6 detections are taken,
    16 tracks + 1 detection are refused."""
    e = small_engine(max_tracks=64, nn_budget_cap=1, tracks_per_tracker=16)
    try:
        tid, frames, new, _ = build_lingering(e, 2, 5, 5002, 7)
        feed(e, tid, new[:6])
        assert len(e.tracker_state(tid, with_cov=False)["ids"]) == 16
        refused_step_leaves_the_tracker_alone(e, tid, new[6:], frames)
    finally:
        e.close()


def test_rows_beyond_the_callers_room(cap_eng):
    """TERR_ROWS.  From the row arena: 150 confirmed rows in one frame against cap_rows = 2 (the arena holds 2 * 2 + 128): the tracker is
    stopped, a reset brings it back.  From the per-frame room: 6 rows against cap_rows = 2 fit the arena, the host refuses the frame when
    it hands the rows out; the step has run, the tracker goes on."""
    tid, frames, _, dets = build_lingering(cap_eng, 6, 50, 5001, 0)
    try:
        seen = C._walk_frame(np.random.default_rng(1), [dets(range(50, 200), len(frames))])
        raises_capacity(lambda: launch(cap_eng, [tid], [seen], hw=C.LINGER_WH, cap_rows=2), "more output rows than the caller's buffers hold (cap_rows)",
                        "stopped until vc_tracker_reset")
        raises_capacity(lambda: feed(cap_eng, tid, frames[0][:1]), "cap_rows")
        cap_eng.tracker_reset(tid)
        ref = C.Probe(C.P_LINGER)
        for t, d in enumerate(frames[:2]):
            ref.predict(); ref.update(d)
            feed(cap_eng, tid, d)
            check_tracker(cap_eng, tid, ref, f"after the reset, frame {t}")
    finally:
        cap_eng.tracker_destroy(tid)
    tid, frames, _, dets = build_lingering(cap_eng, 1, 6, 5003, 0)
    try:
        seen = C._walk_frame(np.random.default_rng(2), [dets(range(6), len(frames))])
        trk, want = C.run_walk([C.P_LINGER], [seen], states=[C.run_single(C.P_LINGER, frames)], hw=C.LINGER_WH)
        assert len(want[0]) == 6
        raises_capacity(lambda: launch(cap_eng, [tid], [seen], hw=C.LINGER_WH, cap_rows=2), "frame 0 needs room for 6 rows")
        check_tracker(cap_eng, tid, trk[0], "after the frame whose rows found no room")
        got = launch(cap_eng, [tid], [C._walk_frame(np.random.default_rng(3), [dets(range(6), len(frames) + 1)])], hw=C.LINGER_WH, cap_rows=6)
        assert len(got) == 1 and len(got[0][1]) == 6
    finally:
        cap_eng.tracker_destroy(tid)
