"""Claimed tiles in c3_fused_kernel and bneck_fused_kernel (engine options "dyn_tiles" / "dyn_tiles_mask": 1 front, 2 C3, 4 Bottleneck): the tiles
after a workgroup's first come in chunks from a per-launch counter (csrc/tile_sched.h) instead of by fixed stride.  Against the kernels' own
stride loops and against the launches they replace, bit for bit: which workgroup computes a tile changes no value.

What can go wrong is the book-keeping -- a tile computed twice or never, a chunk read by the other waves before it is there, the Bottleneck's
two wave groups disagreeing about the tile a b1 buffer holds or about the end, a counter pair that does not return to zero (the next launch on
that pair then skips tiles and leaves stale values).  Hence grids of one workgroup (one claimer takes every chunk), of five (claims interleave,
chunks of every length occur: tests/test_tile_sched_host.py pins that for 60 tiles) and the default (one tile per workgroup here: the first claim
is already the one past the end), tiles over the right and bottom edges, each mask alone and all together, and every pass three times in a row
on ONE counter pair (option "dyn_tiles_ring" 1) with another input run in between, so that a skipped tile shows the other input's values.

Late-starting workgroups -- the reason the counters exist -- cannot be staged in a test; profiles/dyn_tiles_blocks.md measures them."""
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
    for k in ("VC_TUNE_CACHE", "VC_CONV_SLOTS", "VC_BN_GRID", "VC_DYN_TILES", "VC_DYN_TILES_MASK", "VC_DYN_TILES_RING"):
        env.pop(k, None)
    env.update({k: v for k, v in extra_env.items() if v is not None})
    r = subprocess.run([sys.executable, "-c", script], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and tag in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


_BLOCK_SCRIPT = r"""
import os
import numpy as np
import torch
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import synth_yolo
N, H, W, S = (int(os.environ[k]) for k in ("T_N", "T_H", "T_W", "T_IMG"))
MASKS = [int(m) for m in os.environ["T_MASKS"].split(",")]
LAYERS = (1, 2, 4, 17)              # 2: c3_fused_kernel; 4: two Bottlenecks with the shortcut, the second with cv3; 17: one without, with cv3
sd = synth_yolo("yolov5s", nc=8, seed=1702, det_scale=4.0, obj_shift=0.0)
fr = synth_frames(N, H, W, n_obj=6, seed=5)
other = np.ascontiguousarray(synth_frames(N, H, W, n_obj=4, seed=77)[:, ::-1])
eng = E.Engine(sd, None, precision="bf16", num_classes=8, max_batch=N, img_size=S, max_frame_hw=(H, W))
dev, dev_other = torch.from_numpy(fr).cuda(), torch.from_numpy(other).cuda()
def run(frames):                    # device BGR frames: the stream path's detector pass
    eng.stream_submit(frames.data_ptr(), N, H, W)
    eng.sync()
    out = [eng.debug_layer(l, batch=N) for l in LAYERS]
    eng.stream_reset()              # the submission is never run through the tracker: drop it
    return out
eng.set_option("dyn_tiles", 0)
eng.set_option("dyn_tiles_mask", 7)  # honoured only while "dyn_tiles" is on: this pass walks by fixed stride
fixed = run(dev)
eng.set_option("dyn_tiles", 1)
eng.set_option("dyn_tiles_ring", 1)  # one counter pair: every launch gets the pair the launch before it left, not a fresh one of the engine's 1 024
dyn = {}
for m in MASKS:
    eng.set_option("dyn_tiles_mask", m)
    dyn[m] = []
    for rep in range(3):
        dyn[m].append(run(dev))
        o = run(dev_other)          # every layer buffer now holds another input's values; the pair has been used once more
        assert not np.array_equal(o[1], dyn[m][-1][1])
for o in ("front_fused", "c3_fused", "bneck_fused"):
    eng.set_option(o, 0)
unfused = run(dev)
for i, l in enumerate(LAYERS):
    assert np.abs(unfused[i]).max() > 0.1, l
    assert np.array_equal(fixed[i], unfused[i]), ("dyn_tiles 0 vs unfused", l, float((fixed[i] == unfused[i]).mean()))
    for m in MASKS:
        for rep in range(3):
            assert np.array_equal(dyn[m][rep][i], fixed[i]), ("dyn_tiles 1 vs 0", "mask", m, "layer", l, "pass", rep, float((dyn[m][rep][i] == fixed[i]).mean()))
eng.close()
print("DYN_BLOCKS_OK")
"""


@pytest.mark.parametrize("bn_grid", [None, "5", "1"])
@pytest.mark.parametrize("slots", [None, "5", "1"])
def test_c3_and_bottleneck_claimed_chunks_bit_identical(slots, bn_grid):
    """YOLOv5s bf16, 3 frames of 160 x 224 at img_size 224: 60 C3 tiles (40 x 56 maps, 8 columns over the edge) on 1, 5 or 60 workgroups, 18
    Bottleneck tiles (20 x 28 maps, 4 rows and 4 columns over) on 1, 5 or 18.  Layers 1, 2, 4 and 17 at masks 2, 4 and 7 == "dyn_tiles" 0 == the
    unfused launches, three passes in a row on one counter pair with another input between them."""
    _run(_BLOCK_SCRIPT, "DYN_BLOCKS_OK", VC_CONV_SLOTS=slots, VC_BN_GRID=bn_grid, T_N="3", T_H="160", T_W="224", T_IMG="224", T_MASKS="2,4,7")


def test_several_full_chunks_per_workgroup():
    """4 frames of 320 x 320: 200 C3 tiles and 60 Bottleneck tiles on five workgroups each, so a workgroup takes several chunks of the full length
    (C3: 20 of them, then fours, pairs and single tiles) and the claim for the next chunk is issued and read inside a run of consecutive tiles."""
    _run(_BLOCK_SCRIPT, "DYN_BLOCKS_OK", VC_CONV_SLOTS="5", VC_BN_GRID="5", T_N="4", T_H="320", T_W="320", T_IMG="320", T_MASKS="2,4,7")


_STREAM_SCRIPT = r"""
import os, types
import numpy as np
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import synth_reid, synth_yolo
nc = 8
sd, rsd = synth_yolo("yolov5s", nc=nc, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
H, W = 273, 521
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
eng.set_option("dyn_tiles_mask", 7)
for dyn in (1, 0):
    eng.set_option("dyn_tiles", dyn)
    rows, counts = pipe.run_stream(FrameSource(frames), "cam_04", zone, batch=8, asynchronous=True)
    out[dyn] = (key(rows), counts)
eng.close()
assert len(out[1][0]) > 10, len(out[1][0])
assert out[1] == out[0]
print("DYN_BLOCKS_STREAM_OK", len(out[1][0]))
"""


def test_stream_rows_equal_at_mask_7_and_with_fixed_strides(golden_dir):
    """One short run_stream (16 frames, batch 8, detector / ReID / tracker on their three streams) at mask 7 and with "dyn_tiles" 0 on the same engine: same rows, same counts."""
    _run(_STREAM_SCRIPT, "DYN_BLOCKS_STREAM_OK", VC_ZONE=os.path.join(golden_dir, "cam_04_halfres.json"))
