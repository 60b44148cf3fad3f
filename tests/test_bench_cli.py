"""bench.py's command line.  CPU: the launcher contract -- `--gpus N` must become N ranks or fail loudly, never a silent single-rank
run -- and the --steps guard.  GPU: what a plain run prints and what --dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_enough_devices_fails_loudly():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = ""                      # also on a GPU box: no device visible to this child
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0
    assert "needs 2 visible GPUs" in r.stderr and "{" not in r.stdout       # no JSON line was printed


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr and "{" not in r.stdout


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run: exactly --steps timed steps, the headline keys, nothing of --full, and --dump-outputs' arrays of the last step."""
    import json

    import numpy as np
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert abs(d["value"] - d["config"]["frames_per_step"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "stage_ms_per_step", "extra_points", "cpu_baseline", "value_host_frames"):
        assert k not in d, k
    B = d["config"]["frames_per_step"]
    a = {n: np.load(out / f"{n}.npy") for n in ("rows", "rows_per_frame", "detections_per_frame", "counts")}
    assert all(v.dtype == np.float64 for v in a.values())
    # fixed shapes whatever the number of detections: rows per frame as the C ABI's buffer holds them, zero past each frame's rows
    assert a["rows"].shape == (B, 512, 6) and a["rows_per_frame"].shape == (B,) and a["detections_per_frame"].shape == (B,)
    assert a["rows_per_frame"].sum() > 0 and a["detections_per_frame"].sum() > 0
    filled = np.arange(512)[None, :] < a["rows_per_frame"][:, None]
    assert (a["rows"][filled][:, 4] > 0).all() and not a["rows"][~filled].any()
    assert list(a["counts"].shape) == d["config"]["counts_allgather_shape"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
