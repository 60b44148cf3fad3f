"""GPU: YOLOv5x (yolo_variant 3: 80 .. 1280 channels, 4-8-12-4 bottlenecks, 126 convs) on the engine.

  * the graph in fp32 against the oracle and the bf16 ladder, restating tests/test_gpu_configs.py's YOLOv5m / full-size cases for x;
  * stem_direct_wide_kernel<5, U8> (stem_direct_wide.hip: 80 channels, two passes over the staged patch) bit for bit against the implicit GEMM it replaces, on one
    engine through the option "stem_direct": u8 fetch and letterboxed tensor, ragged right edge, several tiles per workgroup;
  * which kernel the stem runs on, from the profiler's op log;
  * the coded clip x640 end to end through the stream path against the committed fp32-oracle CSV (tests/golden/coded_x640.json)."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import coded_case as cc  # noqa: E402
import yolov5x_case as xc  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from oracle import yolov5 as oy  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource  # noqa: E402
from vehicle_counting_amd.synth import synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_yolo  # noqa: E402

X = xc.VARIANT
NC = 8
LAYERS = (0, 2, 4, 6, 9, 13, 17, 20, 23)


def nchw(x):
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def check_dets(dets, ref, atol_px=5e-2):          # tests/test_gpu_configs.py
    assert len(dets) == len(ref)
    for d, r in zip(dets, ref):
        assert len(d) == len(r), (len(d), len(r))
        if len(r):
            np.testing.assert_array_equal(d[:, 5], r[:, 5])
            np.testing.assert_allclose(d[:, :4], r[:, :4], rtol=0, atol=atol_px)
            np.testing.assert_allclose(d[:, 4], r[:, 4], rtol=0, atol=2e-4)


def iou_one(b, others):
    x1, y1 = np.maximum(b[0], others[:, 0]), np.maximum(b[1], others[:, 1])
    x2, y2 = np.minimum(b[2], others[:, 2]), np.minimum(b[3], others[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    return inter / ((b[2] - b[0]) * (b[3] - b[1]) + (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1]) - inter)


@pytest.fixture(scope="module")
def graph():
    """One 180 x 320 frame at AutoShape size 320 (192 x 320 tensor) under the fp32 oracle, computed once for the fp32 and the bf16 test.
    The head calibration of test_baseline_full_size_configs_fp32: the Detect inputs normalised by the oracle's own rms so that the
    seeded head emits tens of detections, not a saturated map."""
    sd = synth_yolo(X, nc=NC, seed=7, det_scale=3.0, obj_shift=0.0)
    frames = synth_frames(1, 180, 320, n_obj=4, seed=2)
    imgs = [frames[0][:, :, ::-1]]
    x, s0, s1 = oy.preprocess(imgs, 320)
    _, ys0, _ = oy.forward(sd, x, X, NC, return_layers=True)
    for i, layer in enumerate((17, 20, 23)):
        k = f"model.24.m.{i}.weight"
        sd[k] = (sd[k] / np.float32(np.sqrt((ys0[layer].numpy() ** 2).mean()))).astype(np.float32)
    pred, ys, _ = oy.forward(sd, x, X, NC, return_layers=True)
    ref = [np.concatenate((oy.scale_coords(s1, d[:, :4], s0[0]), d[:, 4:]), 1) if len(d) else d
           for d in oy.non_max_suppression(pred.numpy(), 0.25, 0.45, None, 300)]
    assert s1 == [192, 320] and 20 < len(ref[0]) < 300
    return types.SimpleNamespace(sd=sd, imgs=imgs, pred=pred.numpy(), ys=[y.numpy() for y in ys], ref=ref, out={})


def engine(sd, precision, img_size=320, max_batch=1, hw=(180, 320), variant=X):
    return E.Engine(sd, None, precision=precision, model_name=variant, num_classes=NC, img_size=img_size, max_batch=max_batch, max_frame_hw=hw)


def test_graph_fp32(graph):
    """yolov5x (1.33 / 1.25 multiples) at AutoShape size 320: test_yolov5m_graph_fp32 restated."""
    eng = engine(graph.sd, "f32")
    eng.debug_pred(arm=True)
    dets = eng.detect(graph.imgs)
    for layer in LAYERS:
        got, ref = nchw(eng.debug_layer(layer)), graph.ys[layer]
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        print(f"fp32 layer {layer}: max error {err:.3g} of max {np.abs(ref).max():.3g}")
        assert err <= 1e-4 * np.abs(ref).max() + 1e-6, layer
    np.testing.assert_allclose(eng.debug_pred()[:1][..., 4:], graph.pred[..., 4:], rtol=0, atol=2e-4)
    eng.close()
    graph.out["f32"] = dets[0]
    check_dets(dets, graph.ref)


def test_ladder_bf16(graph):
    """The bf16 kernels on this variant's shapes (80-wide and 160 / 320-wide pointwise layers on the implicit GEMM, 160-wide 3x3 on the
    v1 halo kernel, 320 / 640-wide on v2 and the stride-2 halo kernel, the 80-channel direct stem): layer outputs against the fp32
    oracle in relative max-norm, the 6e-2 test_baseline_full_size_configs_fp32 holds m and l to; detections cluster-match fp32's."""
    eng = engine(graph.sd, "bf16")
    d16 = eng.detect(graph.imgs)[0]
    for layer in LAYERS:
        got, ref = nchw(eng.debug_layer(layer)), graph.ys[layer]
        assert got.shape == ref.shape
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"bf16 layer {layer}: relative max-norm error {err:.3g}")
        assert err <= 6e-2, (layer, err)
    eng.close()
    d32 = graph.out["f32"] if "f32" in graph.out else graph.ref[0]       # the fp32 engine's detections (= the oracle's, test_graph_fp32)
    assert len(d32) > 0 and abs(len(d16) - len(d32)) <= max(2, len(d32) // 5)
    strong = d32[d32[:, 4] >= 0.5]
    hit = 0
    for b in strong:
        same = d16[d16[:, 5] == b[5]]
        hit += bool(len(same) and iou_one(b[:4], same[:, :4]).max() >= 0.6)
    assert len(strong) > 0 and hit >= 0.9 * len(strong), (hit, len(strong))


def stem_both_ways(eng, run, batch):
    out = []
    for v in (1, 0):
        eng.set_option("stem_direct", v)
        run()
        out.append(eng.debug_layer(0, batch=batch))
    eng.set_option("stem_direct", 1)
    assert out[0].any()
    np.testing.assert_array_equal(out[0], out[1])
    return out[0]


# (variant, img_size, frame h, w, batch, u8): u8 frames already at network size go through the stream path, where the stem fetches
# them itself (U8 = true); host frames through vc_detect are letterboxed first (U8 = false).  Output tiles are 8 x 32:
#   64 x 64    -> 32 x 32 outputs: one tile across, the bottom tile row whole
#   96 x 160   -> 48 x 80: two and a half tiles across, the ragged right edge
#   180 x 320  -> 192 x 320 tensor with 6 pad rows above and below: 96 x 160 outputs
#   320 x 320, batch 6 -> 600 tiles on the 448 workgroups the 80-channel kernel is launched with: a workgroup walks two tiles, the
#              second one in another frame, its patch prefetched while the first is multiplied
STEM_CASES = [(X, 64, 64, 64, 1, True), (X, 64, 64, 64, 3, True), (X, 160, 96, 160, 1, True), (X, 160, 96, 160, 3, True),
              (X, 320, 180, 320, 1, False), (X, 320, 180, 320, 3, False), (X, 320, 320, 320, 6, True),
              ("yolov5l", 160, 96, 160, 3, True), ("yolov5l", 320, 180, 320, 3, False)]       # stem_direct_kernel<4, U8>: the option behaves the same for a variant built before


@pytest.fixture(scope="module")
def stem_weights():
    return {v: synth_yolo(v, nc=NC, seed=11, det_scale=0.05, obj_shift=-8.0) for v in (X, "yolov5l")}      # a head that detects nothing: layer 0 is what is compared


@pytest.mark.parametrize("variant,img_size,h,w,batch,u8", STEM_CASES)
def test_stem_direct_equals_the_implicit_gemm_bit_for_bit(stem_weights, variant, img_size, h, w, batch, u8):
    import torch
    frames = synth_frames(batch, h, w, n_obj=3, seed=5)
    eng = engine(stem_weights[variant], "bf16", img_size=img_size, max_batch=batch, hw=(h, w), variant=variant)
    if u8:
        dev = torch.from_numpy(frames).cuda()

        def run():
            eng.stream_reset()
            eng.stream_submit(dev.data_ptr(), batch, h, w)
            eng.sync()
    else:
        def run():
            eng.detect([f[:, :, ::-1] for f in frames])
    y = stem_both_ways(eng, run, batch)
    eng.close()
    assert y.shape == (batch, (h + 31) // 32 * 16, w // 2, 80 if variant == X else 64)
    assert all(y[b].any() for b in range(batch))


def test_stem_dispatch(monkeypatch):
    """One 640 x 640 frame under the blocking profiler: the stem's op-log line (k=6x3) comes from stem_direct (cfg 100) by default and from
    a tile configuration of the implicit GEMM with "stem_direct" 0.  VC_CONV_STRICT unset: layers whose tuned family refuses a shape
    fall back to the implicit GEMM, and the pass completes."""
    monkeypatch.delenv("VC_CONV_STRICT", raising=False)
    sd = synth_yolo(X, nc=NC, seed=11, det_scale=0.05, obj_shift=-8.0)       # a head that detects nothing: the launches are what is looked at
    img = synth_frames(1, 640, 640, n_obj=4, seed=3)[0][:, :, ::-1]
    eng = engine(sd, "bf16", img_size=640, hw=(640, 640))
    cfgs = {}
    for v in (1, 0):
        eng.set_option("stem_direct", v)
        eng.detect([img])                                    # (tile autotuning of the new shapes happens here, outside the log)
        eng.profile(1); eng.profile_reset()
        eng.detect([img])
        log = eng.profile_ops()
        eng.profile(0)
        stem = [ln for ln in log.splitlines() if " k=6x3 " in ln]
        assert len(stem) == 1 and " N=80 " in stem[0], stem
        assert len([ln for ln in log.splitlines() if ln.startswith("conv ")]) >= 100, log
        cfgs[v] = int(stem[0].split("cfg=")[1].split()[0])
    eng.close()
    assert cfgs[1] == 100 and cfgs[0] != 100 and cfgs[0] < 100, cfgs        # ids >= 100 are the fused / direct kernels (engine_run.hip::conv_select)


def run_product(name, precision, tmp_path, batch):          # tests/test_gpu_coded.py
    c = cc.CASES[name]
    ysd, rsd, frames, _ = cc.build(name)
    cfg = types.SimpleNamespace(model_name=c["variant"], min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=str(tmp_path))
    eng = E.Engine(ysd, rsd, precision=precision, model_name=c["variant"], num_classes=cc.NC, img_size=c["size"], max_batch=batch,
                   max_frame_hw=(c["H"], c["W"]), max_crops=batch * 64, max_tracks=4096, nn_budget_cap=60, max_candidates=4096)
    pipe = CountingPipeline(args, cfg, {"cam": {"cam_04": {"tracking_config": cc.TRACK_CFG}}}, engine=eng,
                            class_names=[f"c{i}" for i in range(cc.NC)])
    rows, counts = pipe.run_stream(FrameSource(frames), "cam_04", cc.zone_file(name, tmp_path), batch=batch, asynchronous=True)
    eng.close()
    return rows, counts


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_csv_equals_the_fp32_oracle(precision, tmp_path):
    """The coded YOLOv5x clip (640 x 640, 16 frames, 12 objects) through the batched asynchronous stream path -- u8 frames fetched by the
    80-channel stem, ReID, DeepSORT, counting -- against the fp32 CPU oracle's CSV; tolerances of tests/test_gpu_coded.py (DESIGN.md
    section 5): row keys exact, boxes and first / last points within 2 px, counts exact."""
    name = "x640"
    g = cc.load_golden(name)
    rows, counts = run_product(name, precision, tmp_path, 8)
    assert len(g["rows"]) > 8 * cc.CASES[name]["T"], len(g["rows"])
    db, dp = cc.compare_rows(rows, g["rows"], box_px=2, point_px=2.0)
    print(f"{name} {precision}: {len(rows)} rows, max box difference {db} px, max first / last point difference {dp} px")
    assert counts == g["counts"]
