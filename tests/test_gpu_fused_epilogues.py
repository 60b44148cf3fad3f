"""The tile / crop loops of the fused Bottleneck and ReID-block kernels, bit for bit against the launches they replace.

The existing bit-identity tests (test_gpu_nets.py) give every Bottleneck workgroup a single tile (150 tiles on 224 workgroups), so the
persistent loop -- both b1 buffers reused, the producers' look-ahead running past the last tile, the consumers' loads of one tile issued
while the stores of the previous one are still in flight -- is never compared directly.  Here a forced small grid (VC_BN_GRID) makes
every workgroup walk several tiles, on maps whose tiles hang over the bottom and the right edge; and the ReID block runs crop counts at
which only SOME workgroups take a second or a third crop."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, tag, **extra_env):
    """Own process with VC_AUTOTUNE=0: the unfused 3x3 then runs in its implicit-GEMM form (tap-major k order, the fused kernels' order; the
    halo-staged variants the autotuner may pick sum slice-major and differ in the last bf16 bit)."""
    env = dict(os.environ, VC_AUTOTUNE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **extra_env)
    env.pop("VC_TUNE_CACHE", None)
    r = subprocess.run([sys.executable, "-c", script], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and tag in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


_BNECK_TILES_SCRIPT = r"""
import numpy as np
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import synth_yolo
H, W = 160, 224                                                  # layers 4 and 17 on 20 x 28 maps: 3 x 2 tiles of 8 x 16 per frame
sd = synth_yolo("yolov5s", nc=8, seed=1702, det_scale=4.0, obj_shift=0.0)
fr = synth_frames(3, H, W, n_obj=6, seed=5)
eng = E.Engine(sd, None, precision="bf16", num_classes=8, max_batch=3, img_size=224, max_frame_hw=(H, W))
eng.detect([f[:, :, ::-1] for f in fr])
a = [eng.debug_layer(l, batch=3) for l in (4, 17)]              # last Bottleneck + cv3 in one kernel (bneck_fused_kernel<true>)
eng.set_option("bneck_cv3", 0)
eng.detect([f[:, :, ::-1] for f in fr])
c = [eng.debug_layer(l, batch=3) for l in (4, 17)]              # Bottlenecks fused, cv3 a launch of its own
eng.set_option("bneck_fused", 0)
eng.detect([f[:, :, ::-1] for f in fr])
b = [eng.debug_layer(l, batch=3) for l in (4, 17)]              # every conv a launch of its own
for x, z, y in zip(a, c, b):
    assert x.shape == y.shape and 20 in x.shape and 28 in x.shape, x.shape
    assert np.abs(y).max() > 0.1
    assert np.array_equal(z, y), ("bneck_cv3=0", float((z == y).mean()))
    assert np.array_equal(x, y), ("default", float((x == y).mean()))
eng.close()
print("BNECK_TILES_OK")
"""


@pytest.mark.parametrize("grid", [5, 1])
def test_bneck_fused_several_tiles_per_workgroup(grid):
    """Three frames of 160 x 224 at img_size 224: 18 tiles of 8 x 16 on 20 x 28 maps (4 rows over the bottom, 4 columns over the right).
    On 5 workgroups each walks 3 - 4 tiles; on 1 a single workgroup walks all 18.  Layers 4 (both Bottlenecks with the shortcut, the
    second with cv3) and 17 (no shortcut, with cv3): default == bneck_cv3=0 == bneck_fused=0, bit for bit."""
    _run(_BNECK_TILES_SCRIPT, "BNECK_TILES_OK", VC_BN_GRID=str(grid))


_REID_CROPS_SCRIPT = r"""
import numpy as np
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.weights import synth_reid
eng = E.Engine(None, synth_reid(1702), precision="bf16", max_crops=1024)
rng = np.random.default_rng(11)
for k in (2, 257, 513):                                           # no second crop; a second / a third crop for one workgroup only (256 CUs)
    x = rng.standard_normal((k, 3, 50, 50)).astype(np.float32)
    eng.set_option("reid_block_fused", 1)
    a = eng.embed_tensor(x)
    eng.set_option("reid_block_fused", 0)
    b = eng.embed_tensor(x)
    assert a.shape == (k, 512) and np.isfinite(a).all()
    assert np.array_equal(a, b), (k, float((a == b).mean()), float(np.abs(a - b).max()))
eng.close()
print("REID_CROPS_OK")
"""


def test_reid_block_fused_second_crop_for_some_workgroups():
    """reid_block_fused_kernel against the two launches per block it replaces at 2, 257 and 513 crops of seeded noise: the crop loop's
    hand-over (the stores of one crop in flight while the next is fetched into the same LDS raster) is what differs between a workgroup's
    first and later crops, and at these counts one workgroup takes a second or a third crop while its neighbours have finished."""
    _run(_REID_CROPS_SCRIPT, "REID_CROPS_OK")
