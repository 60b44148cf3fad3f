"""CPU: the scenes of tests/tracker_size_cases.py reach the regimes tests/test_gpu_tracker_sizes.py relies on, shown with oracle.deepsort
alone -- so a GPU test cannot pass because a scene quietly stayed on the small side of a switch -- and every scene meets the margin
condition (appearance costs perturbed by +-1e-5 leave every id and FSM counter of every frame unchanged)."""
import numpy as np
import pytest

import tracker_size_cases as C


@pytest.mark.parametrize("budget", [64, 65, 100])
def test_deep_gallery_fills_and_wraps_its_ring(budget):
    r = C.regime(f"deep_gallery_{budget}")
    assert r["gallery"] == budget and r["wraps"] >= 2           # every ring fills and its head comes round twice
    assert budget == 64 or budget % 16 != 0                     # ... at a position that is no multiple of the table rows' 16-entry unroll
    assert r["max_D"] <= C.VC_SMALL_D                           # without a table: appearance_row_wave
    assert 4 <= r["max_T"] <= 8
    if budget == 64:
        assert r["deep_any_steps"] == 0                         # the last length with one pass over the samples
    else:
        assert r["deep_steps"] >= 10, r["deep_steps"]          # minimum at ring position >= 64, runner-up >= 1e-3 farther
    assert r["margin_ok"]


def test_deep_gallery_wide_is_past_the_small_detection_count():
    r = C.regime("deep_gallery_wide")
    assert r["gallery"] == 100 and r["wraps"] >= 1
    assert (r["D"] > C.VC_SMALL_D).all()                        # without a table: appearance_row_dev in every step
    assert r["deep_steps"] >= 10, r["deep_steps"]
    assert r["margin_ok"]


def test_many_dets_has_more_than_a_wavefront_of_detections():
    r = C.regime("many_dets")
    assert int((r["D"] > 64).sum()) >= 5 and r["gallery"] == 5 and r["wraps"] >= 1
    assert r["max_T_plus_D"] <= C.TC_HARD_CAP
    assert r["margin_ok"]


def test_growing_walk_changes_side_inside_the_launch():
    r = C.regime("growing_walk")
    T, D = r["T"], r["D"]
    assert T[0] == 0                                            # an empty tracker: the host plans with known_tracks = 0
    assert r["cap"] == C.walk_cap(int(D.max())) == 128
    assert C.crosses(T <= C.VC_STEP_STATE)                      # use_st: true, then false
    assert C.crosses(T * D <= C.SMALL_COST)                     # small_cost: true, then false
    assert C.crosses(T + D <= r["cap"])                         # w_lds, then w_glb
    assert r["max_T_plus_D"] <= C.TC_HARD_CAP
    # on the large side of all three at once, a whole group comes back after a gap: matched on appearance or not at all
    assert ((r["reid"] >= C.WALK_GROUP) & (T > C.VC_STEP_STATE) & (T * D > C.SMALL_COST) & (T + D > r["cap"])).any()
    light = r["others"][0]
    assert light["max_T"] == 2 and light["max_D"] == 2
    assert r["margin_ok"]


def test_growing_walk_with_small_groups_stays_small():
    """The claims above are about the scene, not about the checker: groups of three never leave the small side."""
    r = C.regime_of(C.growing_walk(group=3))
    assert not C.crosses(r["T"] <= C.VC_STEP_STATE) and not C.crosses(r["T"] + r["D"] <= r["cap"])


def test_mixed_fit_has_one_table_that_fits_and_one_that_does_not():
    sc, r = C.scene("mixed_fit"), C.regime("mixed_fit")
    arena = sc["arena_floats"]
    assert arena == 262144
    assert r["device_need"][0] > arena and r["host_need"][0] > arena        # the heavy tracker: no table, on the device's count and the host's bound
    assert r["device_need"][1] * 100 < arena and r["host_need"][1] * 100 < arena
    assert r["launch"]["max_D"] > C.VC_SMALL_D                              # its rows come from appearance_row_dev
    assert r["margin_ok"]


def test_capacity_scenes_stand_where_the_stops_are():
    frames, extra, _ = C.lingering(6, 50, 5001, extra=213)
    trk = C.run_single(C.P_LINGER, frames)
    assert len(trk.tracks) == 300 and all(t.state == C.od.CONFIRMED for t in trk.tracks)
    assert len(trk.tracks) + len(extra) == C.TC_HARD_CAP + 1
    frames, extra, _ = C.lingering(2, 5, 5002, extra=7)
    assert len(C.run_single(C.P_LINGER, frames).tracks) == 10 and len(extra) == 7
    clip = C.pool_clip()
    trk, _ = C.run_walk(clip["params"], clip["frames"])
    born = [k.next_id - 1 for k in trk]                                     # slots taken: every track ever started
    assert born == [7, 2] and sum(born) == C.POOL_SLOTS + 1
    assert [s["T"] for s in trk[0].steps] == [0, 2, 4]                      # the clutter track died in frame 1: its slot is on the freed list
    assert all(s["T"] + s["D"] <= C.POOL_SLOTS for s in trk[0].steps)       # no step is refused for its size: the pool is what runs out
    assert len(clip["eight"]) == C.POOL_SLOTS and all(len(d) * 2 == C.POOL_SLOTS for d in clip["after"])


def test_walk_cap_follows_the_planner():
    assert [C.walk_cap(d) for d in (0, 8, 9, 24, 25, 56, 57, 300)] == [32, 32, 64, 64, 128, 128, 192, 512]
    assert C.walk_cap(2, known_tracks=100) == 256
