"""GPU: every launch of the detector and ReID op plans against float64 on its own input (tests/graph_launch_cases.py), with the product's
default options, so every fusion is on.  One engine and one recorded pass per case.  The engine first runs the shape on OTHER frames
(the conv autotuner times its candidates there, and the buffers then hold values the recorded pass has to replace), then the recorded
pass; tests/graph_launch_cases.py says what a launch is held to.  Each case prints its worst gate ratio and the launch it belongs to
(profiles/graph_launches.md keeps one run's table)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_cases as A
import graph_launch_cases as G
import vehicle_counting_amd.engine as E
from oracle import reid as orr
from oracle.deepsort import crop_corners
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import synth_reid, synth_yolo

pytestmark = pytest.mark.gpu
NC = 8


def yolo_sd(variant):
    return synth_yolo(variant, nc=NC, seed=1702, det_scale=4.0)


def det_engine(variant, precision, hw, size, batch):
    return E.Engine(yolo_sd(variant), None, precision=precision, model_name=variant, num_classes=NC, img_size=size, max_batch=batch, max_frame_hw=hw,
                    max_crops=16, max_tracks=64, nn_budget_cap=10)


def report(tag, p, net, variant="yolov5s"):
    fails, table = p.verdict()
    fails += p.wiring(net, variant)
    w = max(table, key=lambda t: t[2])
    chains = [t for t, L in zip(table, p.launches) if sum(o["kind"] == "conv" for o in L["ops"]) > 1]
    print("%s: %d launches, ids %s; worst %.3f of the gate at %s; elements above the gate %d (fused launches: worst %.3f); fp8 convs: at most %.5f of a "
          "launch's outputs differ from the reference's rounding (those that store bf16, not judged by it: worst %.3f of the bf16 gate)"
          % (tag, len(table), [i for i in p.ids() if i >= 100], w[2], w[1], sum(t[3] for t in table), max([t[2] for t in chains], default=0.0), max(t[4] for t in table),
             max(t[5] for t in table)))
    assert not fails, fails
    return table


def frames_small(seed):
    return synth_frames(3, 83, 150, n_obj=6, seed=seed)


# ---- detector, small ragged geometry: 3 frames of 83 x 150 into 96 x 160 (P5 is 3 x 5: tiles span images) ---------------------------------
@pytest.mark.parametrize("variant,precision", [("yolov5s", "f32"), ("yolov5s", "bf16"), ("yolov5s", "fp8"), ("yolov5m", "bf16"), ("yolov5l", "bf16"),
                                               ("yolov5x", "bf16"), ("yolov5l", "fp8")])
def test_detector_launches_small(variant, precision):
    eng = det_engine(variant, precision, (83, 150), 160, 3)
    try:
        eng.detect([f[:, :, ::-1] for f in frames_small(4)])
        eng.record_arm("yolo")
        eng.detect([f[:, :, ::-1] for f in frames_small(3)])
        launches, arena = eng.record_read()
    finally:
        eng.close()
    p = G.Pass(launches, arena, G.Weights(yolo_sd(variant), nc=NC))
    report("%s %s 96x160" % (variant, precision), p, "yolo", variant)
    if precision == "bf16":
        assert 100 in p.ids() and any("up" in o for L in launches for o in L["ops"]) and any("m_dev" in o for L in launches for o in L["ops"])
        if variant == "yolov5s":
            assert {103, 105, 107} <= set(p.ids())


# ---- detector, the product's geometry: 2 frames of 360 x 640 into 384 x 640 ------------------------------------------------------------------
@pytest.mark.parametrize("path", ["detect", "stream"])
def test_detector_launches_product_geometry(path):
    warm, frames = synth_frames(2, 360, 640, n_obj=6, seed=4), synth_frames(2, 360, 640, n_obj=6, seed=3)
    eng = det_engine("yolov5s", "bf16", (360, 640), 640, 2)
    try:
        if path == "detect":
            eng.detect([f[:, :, ::-1] for f in warm])
            eng.record_arm("yolo")
            eng.detect([f[:, :, ::-1] for f in frames])
        else:
            dev = torch.as_tensor(np.ascontiguousarray(np.concatenate([warm, frames]))).cuda()
            eng.stream_submit(dev[:2].data_ptr(), 2, 360, 640)
            eng.sync()
            eng.stream_reset()
            eng.record_arm("yolo")
            eng.stream_submit(dev[2:].data_ptr(), 2, 360, 640)
            eng.sync()
        launches, arena = eng.record_read()
        if path == "stream":
            eng.stream_reset()
    finally:
        eng.close()
    p = G.Pass(launches, arena, G.Weights(yolo_sd("yolov5s"), nc=NC), frames if path == "stream" else None)
    report("yolov5s bf16 384x640 %s" % path, p, "yolo")
    ids = set(p.ids())
    ops = [o for L in launches for o in L["ops"]]
    if path == "stream":      # a silently disabled fusion fails here instead of narrowing the test
        assert 102 in ids or any(L["cfg"] == 100 and "u8" in L["ops"][0] for L in launches), ids
        assert any("u8" in o for o in ops)
    assert 103 in ids and (104 in ids or 105 in ids) and 107 in ids, ids
    assert any("up" in o for o in ops), "no folded upsample"
    assert sum(o["kind"] == "head_compact" for o in ops) == 3 and sum("m_dev" in o for o in ops) == 3, "no sparse head"
    assert any(int(G.Mem(L, arena, "after").b[L["ops"][0]["count"]["buf"]].reshape(-1)[L["ops"][0]["count"]["index"]]) > 0
               for L in launches if L["ops"][0]["kind"] == "head_compact"), "the sparse head gathered nothing: its conv ran on no row"


# ---- ReID --------------------------------------------------------------------------------------------------------------------------------------
def reid_boxes():
    """tests/test_gpu_round4.py::test_embed_random_boxes_odd_frame's frame and box list"""
    rng = np.random.default_rng(11)
    H, W = 271, 523
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = [[W - 3.0, H - 3.0, 6.0, 6.0], [2.0, 2.0, 5.0, 5.0], [W - 1.5, 100.0, 3.0, 40.0], [100.0, H - 1.5, 60.0, 3.0],
             [W / 2, H / 2, 2.0 * W, 2.0 * H], [W / 2, H / 2, W, 2.0], [W - 25.0, H - 25.0, 50.0, 50.0]]
    for _ in range(41):
        w, h = rng.uniform(2, 300), rng.uniform(2, 260)
        boxes.append([rng.uniform(-20, W + 20), rng.uniform(-20, H + 20), w, h])
    keep = [b for b in boxes if (lambda c: c[2] > c[0] and c[3] > c[1])(crop_corners(np.asarray(b), W, H))]
    return img, np.asarray(keep)


def reid_ref64(sd, x):
    """oracle.reid.reid_forward_bf16 with float64 convolutions, pooling and norm: the same rounding points"""
    sd = {k: torch.as_tensor(v) for k, v in sd.items()}
    r = lambda t: t.float().bfloat16().double()
    fold = lambda w, b, p: tuple(t for t in orr._fold(w, b, sd, p))
    x = r(torch.as_tensor(x, dtype=torch.float32))
    w, b = fold(sd["conv.0.weight"], sd["conv.0.bias"], "conv.1")
    y = r(F.relu(F.conv2d(x, r(w), b.double(), stride=1, padding=1)))
    y = F.max_pool2d(y, 3, 2, padding=1)
    for name, cin, cout, down in orr.BLOCKS:
        s = 2 if down else 1
        w, b = fold(sd[name + ".conv1.weight"], None, name + ".bn1")
        z = r(F.relu(F.conv2d(y, r(w), b.double(), stride=s, padding=1)))
        if down or cin != cout:
            w, b = fold(sd[name + ".downsample.0.weight"], None, name + ".downsample.1")
            y = r(F.conv2d(y, r(w), b.double(), stride=s))
        w, b = fold(sd[name + ".conv2.weight"], None, name + ".bn2")
        y = r(F.relu(F.conv2d(z, r(w), b.double(), stride=1, padding=1) + y))
    y = F.avg_pool2d(y, (4, 4), 1).view(len(x), -1)
    return (y / y.norm(p=2, dim=1, keepdim=True)).numpy()


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("entry,k", [("embed", 3), ("embed", 7), ("embed_tensor", 3)])
def test_reid_launches(precision, entry, k):
    sd = synth_reid(1702)
    img, boxes = reid_boxes()
    eng = E.Engine(None, sd, precision=precision, max_crops=16, max_tracks=64, nn_budget_cap=10, max_frame_hw=img.shape[:2])
    try:
        if entry == "embed":
            eng.embed(img, boxes[k:2 * k])
            eng.record_arm("reid")
            feat = eng.embed(img, boxes[:k])
        else:
            x = np.random.default_rng(k).standard_normal((2 * k, 3, 50, 50)).astype(np.float32)
            eng.embed_tensor(x[k:])
            eng.record_arm("reid")
            feat = eng.embed_tensor(x[:k])
        launches, arena = eng.record_read()
    finally:
        eng.close()
    p = G.Pass(launches, arena, G.Weights(None, sd))
    report("ReID %s %s k=%d" % (precision, entry, k), p, "reid")
    if precision == "bf16":
        assert {101, 106} <= set(p.ids()), p.ids()
    # the feature from the last block's recorded output: AvgPool + L2 in float64 at the tolerance of test_gpu_aux_kernels.py::test_avgpool_l2norm
    last = launches[-1]
    y = G.Mem(last, arena, "after").read(last["ops"][-1]["out"]).reshape(k, 4, 4, 512)
    err, bound = np.abs(feat.astype(np.float64) - A.avgpool_ref(y)), A.avgpool_bound(y)      # (a channel ReLU left at zero everywhere: error 0, bound 0)
    print("feature against AvgPool + L2 of the last recorded block: worst |error| / bound %.3f" % (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()


def test_reid_feature_whole_net_bf16():
    """The whole bf16 ReID net against the float64 restatement of oracle.reid.reid_forward_bf16 on the same crops: 1 - cos at most 4 x what
    the float32 restatement shows against that reference on those crops (one summation order of many)."""
    sd = synth_reid(1702)
    img, boxes = reid_boxes()
    boxes = boxes[:7]
    crops = [img[y1:y2, x1:x2] for x1, y1, x2, y2 in (crop_corners(b, img.shape[1], img.shape[0]) for b in boxes)]
    x = orr.preprocess_crops(crops)
    ref = reid_ref64(sd, x)
    emu = orr.reid_forward_bf16({k: torch.as_tensor(v) for k, v in sd.items()}, x).astype(np.float64)
    eng = E.Engine(None, sd, precision="bf16", max_crops=16, max_tracks=64, nn_budget_cap=10, max_frame_hw=img.shape[:2])
    try:
        feat = eng.embed(img, boxes).astype(np.float64)
    finally:
        eng.close()
    one_minus_cos = lambda a: 1.0 - (a * ref).sum(1) / np.sqrt((a * a).sum(1) * (ref * ref).sum(1))
    d_eng, d_emu = one_minus_cos(feat).max(), one_minus_cos(emu).max()
    print("1 - cos against the float64 restatement: engine %.3g, float32 restatement %.3g" % (d_eng, d_emu))
    assert d_eng <= 4 * d_emu, (d_eng, d_emu)


# ---- the recorder changes nothing ------------------------------------------------------------------------------------------------------------
def test_recorder_hygiene():
    """an armed pass returns bit for bit the detections, layers 1 - 23 and features of an unarmed pass of the same engine"""
    imgs, other = [f[:, :, ::-1] for f in synth_frames(2, 360, 640, n_obj=6, seed=3)], [f[:, :, ::-1] for f in synth_frames(2, 360, 640, n_obj=6, seed=4)]
    img, boxes = reid_boxes()
    eng = E.Engine(yolo_sd("yolov5s"), synth_reid(1702), precision="bf16", num_classes=NC, max_batch=2, max_frame_hw=(360, 640), max_crops=16, max_tracks=64,
                   nn_budget_cap=10)
    try:
        d0 = eng.detect(imgs)
        l0 = [eng.debug_layer(i, 2) for i in range(1, 24)]
        f0 = eng.embed(img, boxes[:7])
        eng.detect(other)
        eng.embed(img, boxes[7:14])
        eng.record_arm("yolo")
        d1 = eng.detect(imgs)
        n_det = len(eng.record_read()[0])
        l1 = [eng.debug_layer(i, 2) for i in range(1, 24)]
        eng.record_arm("reid")
        f1 = eng.embed(img, boxes[:7])
        n_reid = len(eng.record_read()[0])
        d2 = eng.detect(imgs)                                    # ... and the recorder disarms itself
        assert len(eng.record_read()[0]) == n_reid
    finally:
        eng.close()
    assert n_det > 40 and n_reid > 10 and sum(len(d) for d in d0) > 0
    for a, b, c in zip(d0, d1, d2):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert np.array_equal(a, b), "layer %d" % (i + 1)
    assert np.array_equal(f0, f1)
