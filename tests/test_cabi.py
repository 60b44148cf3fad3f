"""CPU: the C-ABI library loads, exports every symbol include/vcount_hip.h declares, fails loudly without a GPU,
and its host-only logic (DeepSORT NMS) matches the reference's golden vectors.  The exact assignment runs on the device now
(vc_lap_host launches the tracker kernel's own solver): its SciPy comparison is the GPU test below; the same solver source
compiled for the host is compared with SciPy in tests/test_track_core_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from vehicle_counting_amd import _lib as L
import vehicle_counting_amd.engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "vcount_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vc_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = L.lib()
    names = declared_symbols()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vcount_hip.h but not exported"
        assert n in L.SIGNATURES, f"{n} has no ctypes prototype in _lib.py"
    assert set(L.SIGNATURES) == set(names)
    assert lib.vc_version() >= 100


def test_no_silent_cpu_fallback():
    """Without a GPU every compute entry point must return an error, never a result."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    n = C.c_int(-1)
    assert L.lib().vc_device_count(C.byref(n)) != 0 or n.value == 0
    with pytest.raises(L.VcError):
        E.conv2d(np.zeros((1, 4, 4, 8), np.float32), np.zeros((8, 8, 1, 1), np.float32), np.zeros(8, np.float32))
    with pytest.raises(L.VcError):
        E.Engine(None, None)
    with pytest.raises(L.VcError):
        E.kalman_initiate(np.ones((1, 4)))


    with pytest.raises(L.VcError):
        E.lap(np.ones((2, 2)))
    # one entry point of every host_*.hip: the staging harness returns at its first allocation
    with pytest.raises(L.VcError):
        E.iou_matrix(np.ones((1, 4)), np.ones((1, 4)))
    with pytest.raises(L.VcError):
        E.nms(np.ones((1, 4), np.float32), np.ones(1, np.float32), np.zeros(1, np.int32), max_cand=64)
    with pytest.raises(L.VcError):
        E.upsample2x(np.zeros((1, 2, 2, 8), np.float32), np.zeros((1, 4, 4, 8), np.float32), 0)
    with pytest.raises(L.VcError):
        w, b = np.zeros((64, 64, 3, 3), np.float32), np.zeros(64, np.float32)
        E.fused_block("reid", np.zeros((1, 8, 8, 64), np.float32), (w, b, w, b), view={}, y=np.zeros((1, 8, 8, 64), np.float32))


@pytest.mark.gpu
def test_lap_matches_scipy_including_ties():
    """vc_lap_host = track_core.h::lap_solve executed by one wavefront on the device (the tracker kernel's solver): row-sorted
    pairs identical to scipy.optimize.linear_sum_assignment, ties included, rows > columns (transposed solve) included."""
    rng = np.random.default_rng(0)
    for t in range(600):
        nr, nc = rng.integers(1, 14, 2)
        c = rng.uniform(0, 1, (nr, nc))
        if t % 3 == 1:
            c = np.round(c, 1)
        if t % 3 == 2:
            c[rng.random((nr, nc)) < 0.5] = 0.20001       # the clamp value min_cost_matching produces
        r, q = E.lap(c)
        r2, q2 = linear_sum_assignment(c)
        np.testing.assert_array_equal(r, r2)
        np.testing.assert_array_equal(q, q2)
    # 65 .. 128 columns: the two-columns-per-lane register solver (lsap_reg2; a dense class step of BASELINE.json configs[2] is about
    # 67 x 87 after the transpose); above 128 the LDS-list solver
    for t in range(60):
        nr, nc = (int(v) for v in rng.integers(40, 129, 2)) if t < 50 else (int(v) for v in rng.integers(120, 200, 2))
        c = rng.uniform(0, 1, (nr, nc))
        if t % 3 == 1:
            c = np.round(c, 1)                               # many exact ties
        if t % 3 == 2:
            c[rng.random((nr, nc)) < 0.6] = 0.20001          # mostly gated
        r, q = E.lap(c)
        r2, q2 = linear_sum_assignment(c)
        np.testing.assert_array_equal(r, r2, err_msg=f"{nr}x{nc} case {t}")
        np.testing.assert_array_equal(q, q2, err_msg=f"{nr}x{nc} case {t}")


def test_dsort_nms_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "dsort_nms.npz"))
    for ci in range(6):
        for ov in (0.5, 0.3, 1.0):
            keep = E.dsort_nms(g[f"c{ci}_boxes"], g[f"c{ci}_scores"], ov)
            ref = g[f"c{ci}_ov{ov}"]
            if ci == 4:
                # case 4 holds two equal scores: the reference's order is whatever np.argsort's unstable quicksort
                # yields (NumPy-version dependent); the product uses a stable sort.  Same survivors up to the tied pair.
                assert len(keep) == len(ref) and set(keep) - {5, 6} == set(ref.tolist()) - {5, 6}
                continue
            np.testing.assert_array_equal(np.asarray(keep, dtype=np.int64), ref)
    assert E.dsort_nms(np.zeros((0, 4)), np.zeros(0), 0.5) == []
