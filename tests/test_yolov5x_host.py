"""CPU: YOLOv5x (the fourth detector of the reference's utilities/utils.py weight list and configs.yaml `model_name`) below the GPU:
layer table against the oracle's graph and the published figures, checkpoint ingestion, what `Engine(model_name="yolov5x")` answers
with and without fp8, and the coded detector of vehicle_counting_amd/coded.py at the wider / deeper model's activations."""
import numpy as np
import pytest
import torch

import yolov5x_case as xc
import vehicle_counting_amd.engine as E
from oracle import yolov5 as oy
from vehicle_counting_amd._lib import VcError
from vehicle_counting_amd.checkpoint import load_yolov5_checkpoint
from vehicle_counting_amd.coded import coded_frames, coded_yolo
from vehicle_counting_amd.weights import fold_yolo_state_dict, synth_yolo, yolo_conv_table

X = xc.VARIANT
VC_ERR_ARG, VC_ERR_HIP = 1, 2          # include/vcount_hip.h
# stride of the map every conv of layer i writes (models/yolov5x.yaml: backbone P1 .. P5, head back up to P3 and down again)
STRIDE = {0: 2, 1: 4, 2: 4, 3: 8, 4: 8, 5: 16, 6: 16, 7: 32, 8: 32, 9: 32, 10: 32, 13: 16, 14: 16, 17: 8, 18: 16, 20: 16, 21: 32, 23: 32}


def test_conv_table_is_the_oracles_graph():
    specs = {n: (ci, co, k) for n, ci, co, k, s, p, act in oy.conv_specs(X, 80)}
    table = {n: (ci, co, k) for n, ci, co, k in yolo_conv_table(X, 80)}
    assert len(table) == len(yolo_conv_table(X, 80)) == 126          # 18 single convs + 8 C3 blocks of 3 + 2 n convs (n = 4, 8, 12, 4, 4, 4, 4, 4) + 3 heads
    assert sorted(table) == sorted(specs)
    for n in specs:
        assert table[n] == specs[n], n
    assert table["model.0.conv"] == (3, 80, 6) and table["model.8.cv3.conv"] == (1280, 1280, 1)
    assert sum(n.startswith("model.6.m.") for n in table) == 2 * 12


def test_params_and_gflops_match_the_published_release():
    """ultralytics v6.0 publishes 86.7 M parameters and 205.7 GFLOPs at 640 x 640 for yolov5x (the figures SURVEY.md 8c cross-checks for
    s / m / l): BN-fused weights + biases, and 2 M N K over every conv at the stride its layer runs at."""
    table = yolo_conv_table(X, 80)
    params = sum(ci * co * k * k + co for n, ci, co, k in table)
    flops = 0.0
    for n, ci, co, k in table:
        idx = int(n.split(".")[1])
        stride = (8, 16, 32)[int(n.rsplit(".", 1)[1])] if idx == 24 else STRIDE[idx]
        flops += 2.0 * (640 // stride) ** 2 * co * ci * k * k
    assert abs(params / 1e6 - 86.7) <= 0.01 * 86.7, params
    assert abs(flops / 1e9 - 205.7) <= 0.01 * 205.7, flops


def _save_state_dict(sd, path):
    torch.save({k: torch.from_numpy(v).half() for k, v in sd.items()}, path)          # upstream ships fp16


def test_checkpoint_round_trip_and_wrong_variant(tmp_path):
    nc = 8
    raw = synth_yolo(X, nc=nc, seed=3, fused=False)                   # upstream's un-fused names: conv.weight + bn.*
    path = tmp_path / "yolov5x.pt"
    _save_state_dict(raw, path)
    sd = load_yolov5_checkpoint(path, X)
    half = lambda a: torch.from_numpy(np.asarray(a, np.float32)).half().float().numpy()
    expect = fold_yolo_state_dict({k: half(v) for k, v in raw.items()})
    table = yolo_conv_table(X, nc)
    assert len(sd) == len(expect) == 2 * len(table)
    for name, ci, co, k in table:
        assert sd[name + ".weight"].shape == (co, ci, k, k) and sd[name + ".bias"].shape == (co,)
        np.testing.assert_array_equal(sd[name + ".weight"], expect[name + ".weight"])
        np.testing.assert_array_equal(sd[name + ".bias"], expect[name + ".bias"])
    with pytest.raises(ValueError, match=r"yolov5l .* needs \("):      # an x file offered as l ...
        load_yolov5_checkpoint(path, "yolov5l")
    lpath = tmp_path / "yolov5l.pt"
    _save_state_dict(synth_yolo("yolov5l", nc=nc, seed=3, fused=False), lpath)
    with pytest.raises(ValueError, match=r"model\.0\.conv\.weight is \(64, 3, 6, 6\), yolov5x \(nc=8\) needs \(80, 3, 6, 6\)"):   # ... and an l file as x
        load_yolov5_checkpoint(lpath, X)


def test_engine_accepts_the_variant_and_refuses_fp8():
    """No KeyError any more.  Where there is no GPU the engine fails as it does for every variant (VC_ERR_HIP, no device); fp8 is refused
    before any device or plan is touched, with or without a GPU."""
    assert E.YOLO_VARIANT_ID[X] == 3
    for precision in ("bf16", "f32"):
        try:
            E.Engine(None, None, precision=precision, model_name=X).close()    # (with a GPU: an engine without networks, created and destroyed)
        except VcError as err:
            assert err.code == VC_ERR_HIP, err
    with pytest.raises(VcError) as ei:
        E.Engine(None, None, precision="fp8", model_name=X)
    assert ei.value.code == VC_ERR_ARG and "fp8 path is not built for yolov5x" in str(ei.value)


def test_coded_detector_is_well_conditioned():
    """One coded frame at 320 x 320 under the oracle: fp32 and the bf16 restatement give the same detections (count, class, position),
    one per plate, and no objectness logit of any anchor lies within +-3 of the threshold's logit (log(0.25 / 0.75) = -1.1): no rounding
    error of a narrower precision decides a detection.  tests/golden/coded_x640.json depends on this."""
    nc = 8
    sd = coded_yolo(X, nc=nc)
    frames, truth = coded_frames(1, 320, 320, n_obj=8, seed=5, size=320)
    x, s0, s1 = oy.preprocess([f[:, :, ::-1] for f in frames], 320)
    assert s1 == [320, 320] and len(truth[0]) >= 6
    thr = float(np.log(0.25 / 0.75))
    dets = {}
    for bf16 in (False, True):
        pred, _, raw = oy.forward(sd, x, X, nc, return_layers=True, bf16=bf16)
        obj = np.concatenate([r.numpy().reshape(1, 3, nc + 5, -1)[:, :, 4].ravel() for r in raw])
        margin = float(np.abs(obj - thr).min())
        print(f"bf16={bf16}: closest objectness logit to the threshold {margin:.2f} away, {int((obj > thr).sum())} above it")
        assert margin > 3.0, (bf16, margin)
        d = oy.non_max_suppression(pred.numpy(), 0.25, 0.45, None, 300)[0]
        dets[bf16] = d[np.lexsort((d[:, 0], d[:, 1]))]
        # every detection is a plate's: its class, and the box the plate's bits decode to (the random term of the box logits: up to ~2 px)
        assert 0 < len(d) <= len(truth[0])
        for row in d:
            e = [max(abs(row[0] - x1), abs(row[1] - y1), abs(row[2] - x2), abs(row[3] - y2)) if int(row[5]) == lab else 1e9 for i, lab, x1, y1, x2, y2 in truth[0]]
            assert min(e) <= 2.5, (bf16, row, min(e))
    a, b = dets[False], dets[True]
    assert len(a) == len(b) >= 6
    np.testing.assert_array_equal(a[:, 5], b[:, 5])
    np.testing.assert_allclose(a[:, :4], b[:, :4], rtol=0, atol=1.0)            # the tolerance test_bf16_restatement_gives_the_same_csv holds boxes to
