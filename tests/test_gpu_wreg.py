"""GPU: conv1x1_wreg_kernel (tile configurations 73 - 78), one launch at a time through vc_conv2d_view_host under VC_CONV_CFG = id and
VC_CONV_STRICT (the id's own kernel or an error), as tests/test_gpu_conv_views.py does for the ids before it; tests/wreg_cases.py holds the
cases.  Every run is
  (a) bit-equal, y and y2 whole, to the heuristic implicit-GEMM launch of the same view (VC_CONV_CFG unset);
  (b) untouched outside the written slice: every other element still holds the sentinel, and the entry point's guard blocks around y and y2
      are intact (it reports a broken guard as an error);
  (c) inside the project's bf16 gate (rtol 2^-7, atol 2e-3) against float64 on the rounded operands;
  (d) finite: every channel of x around the slice is NaN.
Every refusal raises VcError code 1 without a message under VC_CONV_STRICT and leaves y / y2 at the sentinel; without VC_CONV_STRICT it is
the heuristic launch bit for bit.  Last, the bf16 detector with the family forced wherever it applies against the heuristic tiles
everywhere: layers 6, 13, 17, 20 and the detections bit for bit."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import conv_view_cases as V  # noqa: E402
import wreg_cases as W  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402

_heuristic = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def set_env(mp, cfg=None, strict=False, slots=0):
    for name, val in (("VC_CONV_CFG", cfg), ("VC_CONV_STRICT", 1 if strict else None), ("VC_CONV_SLOTS", slots or None)):
        if val is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(val))


def launch(case):
    o = case.operands()
    x, xu, res, y, y2 = case.buffers()
    out = E.conv2d_view(x, o["w"], o["b"], y, view=case.v, x_up=xu, res=res, y2=y2, stride=case.stride, pad=case.pad, act=case.act,
                        res_mode=case.res_mode, precision=case.precision)
    return out if y2 is not None else (out, None)


def heuristic(case, mp):
    """the same view on the tile conv_heuristic picks: computed once per case, never modified"""
    if case.name not in _heuristic:
        set_env(mp)
        y, y2 = launch(case)
        for a in (y, y2):
            if a is not None:
                a.setflags(write=False)
        _heuristic[case.name] = (y, y2)
    return _heuristic[case.name]


@pytest.mark.parametrize("cfg", W.IDS)
def test_wreg_runs(cfg, monkeypatch):
    runs = [r for r in W.RUNS if r.cfg == cfg]
    assert runs
    for run in runs:
        case = run.case
        hy, hy2 = heuristic(case, monkeypatch)
        set_env(monkeypatch, cfg, strict=True, slots=run.slots)
        y, y2 = launch(case)
        got = case.written(y, y2)
        ref = V.rnd(case.reference().astype(np.float32), "bf16")
        err = np.abs(got - ref)
        print("%s: max |err| %.3g, max err / (atol + rtol |ref|) %.3f" % (run.name, err.max(), (err / (2e-3 + 2 ** -7 * np.abs(ref))).max()))
        assert (case.untouched(y, y2) == V.SENTINEL).all(), run.name + ": an element outside the written slice changed"          # (b)
        assert np.isfinite(got).all(), run.name + ": a non-operand element reached the result"                                  # (d)
        np.testing.assert_array_equal(bits(y), bits(hy), err_msg=run.name + ": differs from the heuristic launch")               # (a)
        if y2 is not None:
            np.testing.assert_array_equal(bits(y2), bits(hy2), err_msg=run.name + ": y2 differs from the heuristic launch")
        np.testing.assert_allclose(got, ref, err_msg=run.name, **V.GATE["bf16"])                                                # (c)


@pytest.mark.parametrize("cfg,case,why", W.REFUSALS, ids=[c.tag for _, c, _ in W.REFUSALS])
def test_wreg_refuses(cfg, case, why, monkeypatch):
    set_env(monkeypatch, cfg, strict=True)
    with pytest.raises(L.VcError) as ei:
        launch(case)
    assert ei.value.code == 1, why
    assert str(ei.value).endswith("status 1: "), why + ": not the launcher's own quiet refusal: " + str(ei.value)
    for buf in ei.value.outputs:
        assert buf is None or (buf == V.SENTINEL).all(), why + ": a refused launch wrote"
    set_env(monkeypatch, cfg)
    y, y2 = launch(case)
    hy, hy2 = heuristic(case, monkeypatch)
    np.testing.assert_array_equal(bits(y), bits(hy), err_msg=why + ": the fall-back differs from the heuristic launch")
    if y2 is not None:
        np.testing.assert_array_equal(bits(y2), bits(hy2), err_msg=why)
    assert (case.untouched(y, y2) == V.SENTINEL).all() and np.isfinite(case.written(y, y2)[:case.rows]).all(), why


def test_wreg_in_the_detector(monkeypatch):
    """bf16 YOLOv5s, 2 frames of 640 x 640: VC_TUNE_WREG = 1 (the family's id wherever it applies, the heuristic's tile elsewhere, launch_conv's
    fall-back on) against VC_TUNE_WREG = 0 (the heuristic's tile everywhere)."""
    from vehicle_counting_amd.synth import synth_frames
    from vehicle_counting_amd.weights import synth_yolo
    set_env(monkeypatch)
    sd = synth_yolo("yolov5s", nc=8, seed=1702, det_scale=4.0, obj_shift=0.0)
    imgs = [f[:, :, ::-1] for f in synth_frames(2, 640, 640, n_obj=6, seed=5)]
    out = {}
    for force in (1, 0):
        monkeypatch.setenv("VC_TUNE_WREG", str(force))
        eng = E.Engine(sd, None, precision="bf16", num_classes=8, max_batch=2, max_frame_hw=(640, 640))
        eng.profile(True)
        dets = eng.detect(imgs)
        ids = [int(m) for m in re.findall(r"cfg=(-?\d+)", eng.profile_ops())]
        out[force] = (dets, [eng.debug_layer(l, batch=2) for l in (6, 13, 17, 20)], ids)
        eng.close()
    used = sorted(set(i for i in out[1][2] if i in W.IDS))
    print("ids of the family in the forced pass:", used, "launches:", sum(i in W.IDS for i in out[1][2]))
    assert len(used) >= 2 and not any(i in W.IDS for i in out[0][2])
    assert sum(len(d) for d in out[1][0]) > 0
    for a, b in zip(out[1][0], out[0][0]):
        np.testing.assert_array_equal(bits(a), bits(b))
    for a, b in zip(out[1][1], out[0][1]):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(bits(a), bits(b))
