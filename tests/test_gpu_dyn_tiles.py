"""Claimed tiles (engine option "dyn_tiles"): front_fused_kernel takes the tiles after a workgroup's first from a per-launch counter.  Against
its own fixed-stride loop and against the launches it replaces, bit for bit.

Which workgroup computes a tile affects no value, so every comparison is exact.  What can go wrong is the book-keeping: a tile claimed twice or
never, a claimed index read by the other waves before it is there, a counter pair that does not return to zero (the next launch that gets the
pair would then skip tiles and leave stale values in its output).  Hence: grids of one workgroup (one claimer takes every tile), of five (claims
interleave) and the default (one tile per workgroup at these sizes: the first claim is already the last), tiles that hang over the right and the
bottom edge, and every pass three times in a row on ONE counter pair (option "dyn_tiles_ring" 1; the engine's ring has 1 024, so a short test would
never see a pair twice) with another input run in between, so that a skipped tile would show the other input's values.
The C3, Bottleneck (VC_BN_GRID), ReID-block and ReID-stem kernels keep their fixed stride (profiles/dyn_tiles.md); the Bottleneck grid is varied
along so that the layers compared behind the front see every combination.

Late-starting workgroups -- the reason the counter exists -- cannot be staged in a test; profiles/dyn_tiles.md measures them."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, tag, **extra_env):
    """Own process with VC_AUTOTUNE=0: the unfused 3x3 convs then run in their implicit-GEMM form, whose k order the fused kernels share
    (DESIGN.md section 5).  A value of None leaves the variable unset."""
    env = dict(os.environ, VC_AUTOTUNE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("VC_TUNE_CACHE", "VC_CONV_SLOTS", "VC_BN_GRID", "VC_DYN_TILES"):
        env.pop(k, None)
    env.update({k: v for k, v in extra_env.items() if v is not None})
    r = subprocess.run([sys.executable, "-c", script], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and tag in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


_FRONT_SCRIPT = r"""
import numpy as np
import torch
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import synth_yolo
H, W = 160, 224                     # layer 1 / 2 on 40 x 56 maps: 3 x 4 front tiles of 16 x 16 (8 rows and 8 columns over the edges), 5 x 4 C3
LAYERS = (1, 2, 4, 17)              # tiles of 8 x 16 (8 columns over); layers 4 and 17 on 20 x 28 maps: 3 x 2 Bottleneck tiles (4 rows, 4 columns over)
sd = synth_yolo("yolov5s", nc=8, seed=1702, det_scale=4.0, obj_shift=0.0)
fr = synth_frames(3, H, W, n_obj=6, seed=5)
other = np.ascontiguousarray(synth_frames(3, H, W, n_obj=4, seed=77)[:, ::-1])
eng = E.Engine(sd, None, precision="bf16", num_classes=8, max_batch=3, img_size=224, max_frame_hw=(H, W))
dev, dev_other = torch.from_numpy(fr).cuda(), torch.from_numpy(other).cuda()
def run(frames):                    # device BGR frames: the stream path's detector pass, front_fused_kernel on the u8 frames
    eng.stream_submit(frames.data_ptr(), 3, H, W)
    eng.sync()
    out = [eng.debug_layer(l, batch=3) for l in LAYERS]
    eng.stream_reset()              # the submission is never run through the tracker: drop it
    return out
eng.set_option("dyn_tiles", 0)
fixed = run(dev)
eng.set_option("dyn_tiles", 1)
eng.set_option("dyn_tiles_ring", 1)  # one counter pair: every launch gets the pair the launch before it left, not a fresh one of the engine's 1 024
dyn = []
for rep in range(3):
    dyn.append(run(dev))
    o = run(dev_other)              # every layer buffer now holds another input's values; the pair has been used once more
    assert not np.array_equal(o[0], dyn[-1][0])
for o in ("front_fused", "c3_fused", "bneck_fused"):
    eng.set_option(o, 0)
unfused = run(dev)
for i, l in enumerate(LAYERS):
    assert np.abs(unfused[i]).max() > 0.1, l
    assert np.array_equal(fixed[i], unfused[i]), ("dyn_tiles 0 vs unfused", l, float((fixed[i] == unfused[i]).mean()))
    for rep in range(3):
        assert np.array_equal(dyn[rep][i], fixed[i]), ("dyn_tiles 1 vs 0", l, rep, float((dyn[rep][i] == fixed[i]).mean()))
eng.close()
print("DYN_FRONT_OK")
"""


@pytest.mark.parametrize("bn_grid", [None, "5", "1"])
@pytest.mark.parametrize("slots", [None, "5", "1"])
def test_detector_front_claimed_tiles_bit_identical(slots, bn_grid):
    """YOLOv5s bf16, 3 frames of 160 x 224 at img_size 224: 36 front tiles on 1, 5 or (unset) 36 workgroups, 18 Bottleneck tiles on 1, 5 or 18.  Layers 1, 2, 4 and 17 with dyn_tiles 1 == dyn_tiles 0 == the unfused launches, three passes in a row with another input between them."""
    _run(_FRONT_SCRIPT, "DYN_FRONT_OK", VC_CONV_SLOTS=slots, VC_BN_GRID=bn_grid)


_STREAM_SCRIPT = r"""
import os, types
import numpy as np
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import synth_reid, synth_yolo
nc = 8
sd, rsd = synth_yolo("yolov5s", nc=nc, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
H, W = 273, 521                     # the front kernel's resize instance (640 / 521)
frames = synth_frames(16, H, W, n_obj=5, seed=3)
zone = os.environ["VC_ZONE"]
cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
args = types.SimpleNamespace(weight=None, mapping=None, output_path=None)
track = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
eng = E.Engine(sd, rsd, precision="bf16", num_classes=nc, max_batch=8, max_frame_hw=(H, W), max_crops=512, max_tracks=1024, nn_budget_cap=60)
pipe = CountingPipeline(args, cfg, {"cam": {"cam_04": {"tracking_config": track}}}, engine=eng, class_names=[f"c{i}" for i in range(nc)])
key = lambda rows: [(r["label"], r["track_id"], r["frame_id"], r["direction"], tuple(r["box"])) for r in rows]
out = {}
eng.set_option("dyn_tiles_ring", 2)  # the pairs come round again within the run
for dyn in (1, 0):
    eng.set_option("dyn_tiles", dyn)
    rows, counts = pipe.run_stream(FrameSource(frames), "cam_04", zone, batch=8, asynchronous=True)
    out[dyn] = (key(rows), counts)
eng.close()
assert len(out[1][0]) > 10, len(out[1][0])
assert out[1] == out[0]
print("DYN_STREAM_OK", len(out[1][0]))
"""


def test_stream_rows_equal_with_and_without_claimed_tiles(golden_dir):
    """One short run_stream (16 frames, batch 8, detector / ReID / tracker on their three streams) with dyn_tiles 1 and 0 on the same engine: same rows, same counts."""
    _run(_STREAM_SCRIPT, "DYN_STREAM_OK", VC_ZONE=os.path.join(golden_dir, "cam_04_halfres.json"))
