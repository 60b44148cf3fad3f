"""GPU: the tracker's single-function entry points (host_track.hip: vc_kalman_*_host, vc_iou_cost_host, vc_cosine_cost_host, vc_lap_host) at
the smallest shapes.  Every output of these entry points lies between guard blocks, so a store one element past a 1-track pool, a 1 x 1
matrix or a 1-pair assignment is reported as an error instead of landing in a neighbour's memory; the values are compared with the oracle
at the tolerances tests/test_gpu_kernels.py uses for the same kernels at larger shapes."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu

import vehicle_counting_amd.engine as E  # noqa: E402
from oracle import deepsort as od  # noqa: E402


def unit_rows(rng, n):
    f = rng.standard_normal((n, 512)).astype(np.float32)
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def test_kalman_one_track():
    kf = od.KalmanCV()
    z0, z1 = np.array([320.5, 241.25, 0.45, 96.0]), np.array([323.0, 240.0, 0.47, 98.5])
    m, c = E.kalman_initiate(z0[None])
    om, oc = kf.initiate(z0)
    assert m.shape == (1, 8) and c.shape == (1, 8, 8)
    np.testing.assert_array_equal(m[0], om)
    np.testing.assert_array_equal(c[0], oc)
    m1, c1 = E.kalman_predict(om[None], oc[None])
    pm, pc = kf.predict(om, oc)                         # exact: F is 0 / 1
    np.testing.assert_array_equal(m1[0], pm)
    np.testing.assert_array_equal(c1[0], pc)
    # update / gating: LAPACK's operation order is not reproducible bit for bit -> 1e-9
    um, uc = E.kalman_update(pm[None], pc[None], z1[None])
    rm, rc = kf.update(pm, pc, z1)
    np.testing.assert_allclose(um[0], rm, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(uc[0], rc, rtol=1e-9, atol=1e-9)
    gd = E.kalman_gating(pm, pc, z1[None])
    assert gd.shape == (1,)
    np.testing.assert_allclose(gd, kf.gating(pm, pc, z1[None]), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("t,d", [(1, 1), (1, 3), (3, 1)])
def test_iou_smallest(t, d):
    rng = np.random.default_rng(100 * t + d)
    a = np.concatenate([rng.uniform(0, 60, (t, 2)), rng.uniform(20, 80, (t, 2))], 1)
    b = np.concatenate([rng.uniform(0, 60, (d, 2)), rng.uniform(20, 80, (d, 2))], 1)
    b[0] = a[-1]                                        # identical boxes -> iou 1
    got = E.iou_matrix(a, b)
    assert got.shape == (t, d)
    np.testing.assert_array_equal(got, np.stack([od.iou_one_to_many(a[i], b) for i in range(t)]))


@pytest.mark.parametrize("counts,d", [((1,), 1), ((1, 3), 3)])
def test_cosine_smallest(counts, d):
    rng = np.random.default_rng(7 + d)
    galleries = [unit_rows(rng, s) for s in counts]
    feats = unit_rows(rng, d)
    feats[0] = galleries[-1][0]                         # a detection that is a gallery sample -> cost 0
    got = E.cosine_cost(galleries, feats)
    assert got.shape == (len(counts), d)
    ref = np.stack([od.cosine_nn_cost(g, feats) for g in galleries])
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6)     # f32 dot products, free summation order


@pytest.mark.parametrize("nr,nc", [(1, 1), (1, 2), (2, 1), (3, 2)])
def test_lap_smallest(nr, nc):
    rng = np.random.default_rng(10 * nr + nc)
    for c in (rng.uniform(0, 1, (nr, nc)), np.round(rng.uniform(0, 1, (nr, nc)), 1), np.full((nr, nc), 0.20001)):
        r, q = E.lap(c)
        r2, q2 = linear_sum_assignment(c)
        np.testing.assert_array_equal(r, r2)
        np.testing.assert_array_equal(q, q2)
