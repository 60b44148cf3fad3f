"""GPU: the kernels of detect_post.hip on known input, through the engine-free entry points vc_decode_host / vc_nms_batch_host.

Decode (decode_kernel<f32 | bf16>, head_compact_kernel + decode_sparse_kernel): the three modes bit-identical to one another, and against
the float64 reference of tests/detect_post_cases.py the same (frame, idx, cls) set exactly, boxes and scores within DECODE_ULPS (per field) float32
ulps of the field's scale -- max(|value|, stride * (nx + 2)) for a coordinate, 1 for a score -- and the gathered pixel lists equal, as
sets, to the pixels whose float64 objectness passes.  No candidate is left out: tests/test_detect_post_cases.py shows that none sits
near a threshold or a class tie that rounding could move.

NMS (rank_sort_kernel, nms_mask_kernel, nms_scan_kernel): bit-equal to oracle.yolov5.box_iou_greedy_nms + scale_coords, per frame."""
import numpy as np
import pytest

import detect_post_cases as D
import vehicle_counting_amd.engine as E

pytestmark = pytest.mark.gpu

# Worst deviation from the float64 reference per field (x1, y1, x2, y2, conf), measured on an MI355X over all cases and modes, in float32
# ulps of the field's scale.  Asserted: twice the measured worst, the margin for expf differences between ROCm releases.  The kernel's
# chain per field (one expf, an add and a divide per sigmoid, at most three multiplies and two adds) is of the order of ten ulps; float32
# NumPy in the same operation order gives 3.69 / 3.97 / 2.74 / 3.02 / 1.18.
MEASURED_ULPS = np.array([3.69, 3.69, 2.74, 3.02, 1.18])
DECODE_ULPS = 2 * MEASURED_ULPS
MODES = ("f32", "bf16", "sparse")


def _run_decode(case, mode, **kw):
    return E.decode(case.logits, case.nc, D.STRIDES, D.ANCHORS, conf=D.CONF, max_cand=case.max_cand, mode=mode, **kw)


def _sorted_frame(r, f, max_cand):
    n = min(int(r["cand_count"][f]), max_cand)
    order = np.argsort(r["idx"][f, :n], kind="stable")
    return {k: r[k][f, :n][order] for k in ("idx", "cls", "box", "conf")}


def _ulps(got, ref, scale):
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.float32(scale)).astype(np.float64)


def _check_against_ref(case, r, mode, frames=None):
    ref = D.decode_ref(case.name)
    worst = np.zeros(5)
    for f in range(case.B) if frames is None else frames:
        want, got = ref["frames"][f], _sorted_frame(r, f, case.max_cand)
        assert r["cand_count"][f] == len(want["idx"]) and not r["overflow"][f], (case.name, mode, f)
        np.testing.assert_array_equal(got["idx"], want["idx"], err_msg=f"{case.name} {mode} frame {f}")
        np.testing.assert_array_equal(got["cls"], want["cls"], err_msg=f"{case.name} {mode} frame {f}")
        if not len(want["idx"]):
            continue
        scale = np.maximum(np.abs(want["box"]), want["scale"][:, None])
        ub, uc = _ulps(got["box"], want["box"], scale), _ulps(got["conf"], want["conf"], np.ones(len(want["conf"])))
        worst = np.maximum(worst, np.append(ub.max(0), uc.max()))
    print(f"decode {case.name} {mode}: worst deviation x1 y1 x2 y2 conf = {np.round(worst, 2)} float32 ulps of the scale")
    assert (worst <= DECODE_ULPS).all(), (case.name, mode, worst, DECODE_ULPS)
    if mode == "sparse":
        for level in range(3):
            got = r["hc_lists"][level]
            assert len(got) == len(set(got.tolist())), "a pixel gathered twice"
            np.testing.assert_array_equal(np.sort(got), ref["gathered"][level], err_msg=f"{case.name} gathered level {level}")


@pytest.mark.parametrize("name", [n for n in sorted(D.decode_cases()) if n != "overflow"])
def test_decode_modes_agree_and_match_float64(name):
    case = D.decode_cases()[name]
    res = {mode: _run_decode(case, mode) for mode in MODES}
    for mode in MODES:
        _check_against_ref(case, res[mode], mode)
    for mode in MODES[1:]:                                            # the file's own claim: the same detections, bit for bit
        np.testing.assert_array_equal(res[mode]["cand_count"], res["f32"]["cand_count"])
        for f in range(case.B):
            a, b = _sorted_frame(res["f32"], f, case.max_cand), _sorted_frame(res[mode], f, case.max_cand)
            for k in a:
                np.testing.assert_array_equal(b[k], a[k], err_msg=f"{name} {mode} vs f32, frame {f}, {k}")
    if name == "ties":
        for (frame, idx), cls in case.planted.items():
            for mode in MODES:
                g = _sorted_frame(res[mode], frame, case.max_cand)
                assert g["cls"][list(g["idx"]).index(idx)] == cls, (mode, frame, idx)
    if name == "edges":
        for mode in MODES:
            g = _sorted_frame(res[mode], 0, case.max_cand)
            box = {int(i): b for i, b in zip(g["idx"], g["box"])}
            assert all(box[i][0] == box[i][2] for i in case.planted["zero_w"]) and all(box[i][1] == box[i][3] for i in case.planted["zero_h"])
            assert not set(case.planted["class_fails"]) & set(box)


def _nms_of_candidates(g, iou, max_det, geom):
    frame = D._frame(g["box"], g["conf"], g["cls"])
    return D.nms_rows(frame, D.nms_keep32(frame, iou), max_det, geom)


@pytest.mark.parametrize("mode", ("f32", "sparse"))
def test_overflow_flags_one_frame_and_the_chain_reports_it(mode):
    """max_cand = 64; 10, exactly 64 and 70 candidates: only the last frame is flagged, its count through the chain is -1 and the other
    frames come out as the oracle's NMS of their own candidates."""
    case = D.decode_cases()["overflow"]
    geoms = [(64, 64, 128, 128)] * 3
    r = _run_decode(case, mode, nms=dict(iou=0.45, max_det=300, geoms=geoms))
    assert list(r["overflow"]) == [0, 0, 1] and list(r["cand_count"][:2]) == [10, 64] and r["cand_count"][2] >= 65
    _check_against_ref(case, r, mode, frames=(0, 1))
    assert r["det_count"][2] == -1
    for f in (0, 1):
        want = _nms_of_candidates(_sorted_frame(r, f, case.max_cand), 0.45, 300, geoms[f])
        assert r["det_count"][f] == len(want) > 0
        np.testing.assert_array_equal(r["det"][f, :len(want)], want)


@pytest.mark.parametrize("mode", ("f32", "sparse"))
def test_decode_chained_into_nms_end_to_end(mode):
    """The ragged batch (a frame without candidates among them) through decode + NMS on the same device buffers, per-frame geometry."""
    case = D.decode_cases()["ragged"]
    geoms = [(96, 160, 270, 480), (96, 160, 96, 160), (96, 160, 180, 320), (96, 160, 540, 960), (96, 160, 100, 160)]
    r = _run_decode(case, mode, nms=dict(iou=0.45, max_det=100, geoms=geoms))
    _check_against_ref(case, r, mode)
    for f in range(case.B):
        want = _nms_of_candidates(_sorted_frame(r, f, case.max_cand), 0.45, 100, geoms[f])
        assert r["det_count"][f] == len(want)
        np.testing.assert_array_equal(r["det"][f, :len(want)], want, err_msg=f"frame {f}")
    assert r["det_count"][1] == 0 and r["det_count"][3] == 100          # the empty frame; the full frame meets the max_det cut


@pytest.mark.parametrize("name", sorted(D.nms_cases()))
def test_nms_bit_equal_to_the_float32_oracle(name):
    case, ref = D.nms_cases()[name], D.nms_ref(name)
    boxes, conf, cls = zip(*case.frames)
    out, n = E.nms_batch(boxes, conf, cls, case.counts, iou=case.iou, max_det=case.max_det, max_cand=case.max_cand, geoms=case.geoms)
    for f, (_, want) in enumerate(ref):
        assert n[f] == len(want), (name, f, case.counts[f], int(n[f]), len(want))
        np.testing.assert_array_equal(out[f, :len(want)], want, err_msg=f"{name} frame {f} ({case.counts[f]} candidates)")
