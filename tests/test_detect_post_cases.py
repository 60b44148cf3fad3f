"""CPU: the conditions the inputs of tests/test_gpu_detect_post.py are built to satisfy (tests/detect_post_cases.py).  They make every
comparison of that file well defined without leaving a candidate out: no score near the confidence threshold, no near-tie between class
scores, and NMS inputs on which the float32 oracle and a float64 walk keep the same boxes."""
import numpy as np
import pytest
import torch

import detect_post_cases as D
from oracle import yolov5 as oy

DECODE = sorted(D.decode_cases())
NMS = sorted(D.nms_cases())


@pytest.mark.parametrize("name", DECODE)
def test_decode_logits_are_on_the_grid_and_clear_of_conf(name):
    case, ref = D.decode_cases()[name], D.decode_ref(name)
    no = case.nc + 5
    for level, lg in enumerate(case.logits):
        ny, nx = case.shapes[level]
        assert lg.dtype == np.float32 and lg.shape == (case.B, ny, nx, D.lcs_of(case.nc))
        assert np.array_equal(lg * 4, np.round(lg * 4))                                     # multiples of 0.25
        assert np.array_equal(torch.from_numpy(lg).bfloat16().float().numpy(), lg)            # bf16-representable
        assert not lg[..., 3 * no:].any()
        a = case.anchors(level)
        outside = np.abs(a) > 8                                                             # only the planted sigmoid -> 0 width / height logits
        assert not outside[..., :2].any() and not outside[..., 4:].any() and (name == "edges" or not outside.any())
        assert (a[outside] == -200).all()
        assert a[..., 4].min() >= -4
        assert (np.abs(ref["obj"][level] - D.CONF) > D.MARGIN).all()
        assert (np.abs(ref["best"][level] - D.CONF) > D.MARGIN).all()
        # two class scores of an anchor: from equal logits, or more than CLS_GAP apart
        cl = np.sort(a[..., 5:].astype(np.float64), -1)
        sc = D._sig(cl) * D._sig(a[..., 4].astype(np.float64))[..., None]
        step = np.diff(sc, axis=-1)
        assert (step[np.diff(cl, axis=-1) > 0] > D.CLS_GAP).all()


def test_decode_cases_hold_what_they_were_built_for():
    cases = D.decode_cases()
    count = lambda name: [len(f["idx"]) for f in D.decode_ref(name)["frames"]]
    gathered = lambda name: [len(g) for g in D.decode_ref(name)["gathered"]]
    # tiny: every anchor of every frame a candidate, 63 per frame -> a 128-anchor run spans three frames
    assert cases["tiny"].B == 9 and count("tiny") == [63] * 9 and gathered("tiny") == [144, 36, 9]
    # ragged: one frame without a candidate, one with every pixel gathered, about 30 % of the pixels in the others
    c = count("ragged")
    assert c[1] == 0 and min(c[0], c[2], c[3], c[4]) > 0
    ppf = [12 * 20, 6 * 10, 3 * 5]
    for level, g in enumerate(D.decode_ref("ragged")["gathered"]):
        per = np.bincount(g // ppf[level], minlength=5)
        assert per[1] == 0 and per[3] == ppf[level]
        if level == 0:
            assert all(0.2 < per[f] / ppf[0] < 0.4 for f in (0, 2, 4))
    assert [D.lcs_of(nc) // 8 for nc in (3, 59, 80, 123, 251)] == [3, 24, 32, 48, 96]
    # passes: every pixel gathered, 3 anchors each; 16 * 1024 anchors per pass, at most 8 passes per round
    assert gathered("passes4") == [8 * 1600, 8 * 400, 8 * 100] and -(-3 * sum(gathered("passes4")) // (16 * 1024)) == 4
    assert 3 * sum(gathered("round2")) == 201600 > 8 * 16 * 1024
    for name in ("passes4", "round2"):
        assert 0 < min(count(name)) and max(count(name)) < cases[name].max_cand // 4
    # ties: the planted anchors are candidates of the smaller class
    ref = D.decode_ref("ties")["frames"]
    assert len(cases["ties"].planted) == 32 and {v for v in cases["ties"].planted.values()} == {0, 3, 5, 15, 17}
    for (frame, idx), cls in cases["ties"].planted.items():
        assert ref[frame]["cls"][list(ref[frame]["idx"]).index(idx)] == cls
    # edges: passing objectness with a failing class is no candidate; the far-negative logits give (near) zero extent
    e, p = D.decode_ref("edges")["frames"][0], cases["edges"].planted
    assert not set(p["class_fails"]) & set(e["idx"]) and set(p["zero_w"]) <= set(e["idx"]) and len(e["idx"]) == 63 - 2
    for idx in p["class_fails"]:
        level, a, y, x = cases["edges"].locate(idx)
        assert D.decode_ref("edges")["obj"][level][0, a, y, x] > D.CONF
    box = {i: b for i, b in zip(e["idx"], e["box"])}
    assert all(box[i][2] - box[i][0] < 1e-80 for i in p["zero_w"]) and all(box[i][3] - box[i][1] < 1e-80 for i in p["zero_h"])
    assert box[5][2] - box[5][0] < 1e-4 and box[21][2] - box[21][0] > 39.9                  # width logits -8 and +8 (anchor 10 px)
    # overflow: 10, exactly max_cand, more
    assert count("overflow") == [10, 64, 70] and cases["overflow"].max_cand == 64


@pytest.mark.parametrize("name", NMS)
def test_nms_inputs_are_exact_in_float32_and_both_walks_agree(name):
    case = D.nms_cases()[name]
    assert case.max_cand % 64 == 0 and max(case.counts) <= case.max_cand
    for f, frame in enumerate(case.frames):
        boxes, conf, cls = frame
        assert np.array_equal(boxes * 4, np.round(boxes * 4)) and 0 <= cls.min(initial=0) and cls.max(initial=0) <= 79
        wh = boxes[:, 2:] - boxes[:, :2]
        assert (wh >= 0).all() and (wh <= 200).all()
        assert np.array_equal(D.offset_boxes(boxes, cls).astype(np.float64), boxes.astype(np.float64) + cls[:, None] * 4096.0)
        keep32 = D.nms_ref(name)[f][0]
        np.testing.assert_array_equal(keep32, D.nms_keep64(frame, case.iou), err_msg=f"{name} frame {f}")


def _ranks(frame):
    order = np.argsort(-frame[1], kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank


def test_nms_cases_hold_what_they_were_built_for():
    cases = D.nms_cases()
    c = cases["counts_mc8192"]
    assert tuple(c.counts) == D.COUNT_EDGES and c.max_det == 300
    kept = {n: len(k) for n, (k, _) in zip(c.counts, D.nms_ref(c.name))}
    assert all(kept[n] * 2 <= n for n in (4096, 4097, 8192))                                # at least half suppressed
    assert kept[512] > 300 and kept[513] > 300 and kept[4096] > 300                         # the max_det cut acts ...
    assert kept[4097] < 300 and kept[8192] < 300                                            # ... and the walk runs to the last candidate
    k4097, k8192 = D.nms_ref(c.name)[8][0], D.nms_ref(c.name)[9][0]
    assert _ranks(c.frames[8])[k4097].max() < 4096                                          # candidate 4096 (second register word) is suppressed
    r = _ranks(c.frames[9])[k8192]
    assert 0 < (r >= 4096).sum() < 100                                                      # kept and suppressed candidates above 4096
    assert [cases[f"counts_mc{m}"].counts for m in (4096, 512, 64)] == [[0, 1, 63, 64, 65, 512, 513, 4096], [0, 1, 63, 64, 65, 512], [0, 1, 63, 64]]
    # max_det cut: nothing suppressed, the output is the first max_det in score order
    for md in (1, 63, 64, 65, 128):
        case = cases[f"maxdet{md}"]
        keep, rows = D.nms_ref(case.name)[0]
        assert len(keep) == 130 and len(rows) == md == case.max_det
        np.testing.assert_array_equal(rows[:, 4], np.sort(case.frames[0][1])[::-1][:md])
    # across words: the copies of the top box sit at the stated ranks, all vanish, nothing else changes
    case = cases["across_words"]
    keep = D.nms_ref(case.name)[0][0]
    rank = _ranks(case.frames[0])
    assert sorted(rank[case.notes["copies"]]) == list(D.ACROSS_RANKS) and len(keep) < case.max_det
    top = int(np.flatnonzero(rank == 0)[0])
    assert all(np.array_equal(case.frames[0][0][p], case.frames[0][0][top]) and case.frames[0][2][p] == case.frames[0][2][top] for p in case.notes["copies"])
    np.testing.assert_array_equal(keep, case.notes["plain_pos"][D.nms_keep32(case.notes["plain"], case.iou)])
    assert (rank[keep] >= 4096).any()
    # the small frames
    case, n = cases["small"], cases["small"].notes
    keeps = [k for k, _ in D.nms_ref("small")]
    assert list(keeps[n["chain"]]) == [0, 2]
    order = np.argsort(-case.frames[n["equal"]][1], kind="stable")
    assert list(order) == list(range(200)) and list(keeps[n["equal"]]) == sorted(keeps[n["equal"]]) and len(keeps[n["equal"]]) < 200
    q = case.frames[n["quantised"]][1]
    assert np.array_equal(q * 64, np.round(q * 64)) and len(np.unique(q)) < 60
    assert list(keeps[n["classes"]]) == [0, 1, 2, 3, 4, 5, 6, 7, 8]                         # ten identical boxes, nine classes: only the second 79 goes
    assert 0 < len(keeps[n["cls79"]]) < 200 and set(case.frames[n["cls79"]][2]) == {78, 79}
    assert list(keeps[n["degenerate"]]) == [0, 1, 2, 3]
    # threshold: IoU exactly 0.5 stays, one step above goes
    case = cases["threshold"]
    keep = set(D.nms_ref("threshold")[0][0])
    for p, kept_pair in enumerate(case.notes["pair_kept"]):
        assert 2 * p in keep and ((2 * p + 1) in keep) == kept_pair
    assert case.iou == 0.5 and sum(case.notes["pair_kept"]) == 4 == len(case.notes["pair_kept"]) // 2
    # geometry: every clamp acts in every frame
    case = cases["geometry"]
    for (keep, rows), g in zip(D.nms_ref("geometry"), case.geoms):
        assert len(rows) == len(keep) < case.max_det
        assert (rows[:, 0] == 0).any() and (rows[:, 1] == 0).any() and (rows[:, 2] == g[3]).any() and (rows[:, 3] == g[2]).any()
        assert (rows[:, 0] > 0).any() and (rows[:, 2] < g[3]).any()
        unscaled = D.nms_rows(case.frames[case.geoms.index(g)], keep, case.max_det)
        assert (unscaled[:, 0] < 0).any() and (unscaled[:, 1] < 0).any() and (unscaled[:, 2] > g[1]).any() and (unscaled[:, 3] > g[0]).any()
    assert case.geoms[-1][:2] == case.geoms[-1][2:]                                         # the identity
    assert oy.MAX_WH * 79 == 323584
