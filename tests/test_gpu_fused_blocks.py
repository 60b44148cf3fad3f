"""GPU: the four fused block kernels -- c3_fused_kernel, bneck_fused_kernel<false>, bneck_fused_kernel<true>, reid_block_fused_kernel -- one
launch at a time, without an engine (tests/fused_block_cases.py holds the cases, the buffers and the float64 references;
tests/test_fused_block_cases.py holds that module to its own conditions).

Every case goes through vc_c3_fused_host / vc_bneck_fused_host / vc_reid_block_fused_host, which build the ConvP chain the engine's plan
builds and call the block's launcher, and is checked four ways:
  (a) every element outside the written slice -- the rest of the output buffers, the whole input buffer, under cv3 the m slice of the
      concat buffer -- holds what it held before (the sentinel, the operands, NaN); the entry point itself reports a broken guard block
      and an intermediate (y1, b1, [m | y2], t) that did not stay on chip as errors;
  (b) the written slice is finite: every element of an input buffer that is not an operand is NaN, so one that reaches a sum shows;
  (c) the written slice is inside the project's bf16 gate (conv_view_cases.GATE, rtol 2^-7 / atol 2e-3: never more than one bf16 ulp
      away) of the float64 reference of the chain, each intermediate rounded to bf16 where the unfused graph stores it;
  (d) the written slice equals, bit for bit, the SAME chain run through launch_conv by the same entry point under VC_CONV_CFG = 3 and
      VC_CONV_STRICT: the implicit GEMM, tap-major k order.  The ReID view whose output offset is a multiple of 4 only has (a) to (c):
      there the unfused launches leave conv_epilogue_fast_bf16's 16-byte store for the general loop, another instruction sequence
      (tests/test_gpu_conv_views.py).
Grid caps of 1, 2 and 3 workgroups walk all tiles or crops of these tiny cases in one process.  Every refusal case must raise VcError
code 1 with the launcher's empty message and leave every array as it was passed."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fused_block_cases as FB  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from conv_view_cases import GATE  # noqa: E402
from aux_cases import rnd  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402

_twin = {}
_worst = collections.defaultdict(float)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def launch(case, unfused=False):
    x, y, z = case.buffers()
    return E.fused_block(case.kind, x, case.weights(), view=case.view_dict(unfused), y=y, z=z)


def twin(case, mp):
    """(npix, cout): the case's chain, one launch_conv per convolution, on the implicit GEMM"""
    key = case.twin_key()
    if key not in _twin:
        mp.setenv("VC_CONV_CFG", "3")
        mp.setenv("VC_CONV_STRICT", "1")
        out = launch(case, unfused=True)
        assert case.untouched_ok(*out, unfused=True), case.name + ": the unfused chain changed an element outside its outputs"
        _twin[key] = case.written(*out).copy()
    return _twin[key]


def check_runs(case, mp):
    mp.delenv("VC_CONV_CFG", raising=False)
    mp.delenv("VC_CONV_STRICT", raising=False)
    out = launch(case)
    assert case.untouched_ok(*out), case.name + ": an element outside the written slice changed"                               # (a)
    got = case.written(*out)
    assert np.isfinite(got).all(), case.name + ": a non-operand element reached the result"                                     # (b)
    ref = case.reference()
    ratio = FB.gate_ratio(got, ref)
    _worst[FB.kernel_of(case)] = max(_worst[FB.kernel_of(case)], ratio)
    np.testing.assert_allclose(got, rnd(ref.astype(np.float32), "bf16"), err_msg="%s (gate ratio %.3f)" % (case.name, ratio), **GATE["bf16"])   # (c)
    if case.twin_same_store_path:                                                                                               # (d)
        np.testing.assert_array_equal(bits(got), bits(twin(case, mp)), err_msg=case.name + ": differs from the unfused chain")
    return ratio


GROUPS = sorted({(FB.kernel_of(c), c.shape) for c in FB.CASES}, key=lambda g: (g[0], g[1]))


@pytest.mark.parametrize("kernel,shape", GROUPS, ids=["%s-%dx%dx%d" % ((k,) + s) for k, s in GROUPS])
def test_fused_block(kernel, shape, monkeypatch):
    cases = [c for c in FB.CASES if FB.kernel_of(c) == kernel and c.shape == shape]
    assert cases
    worst = max(check_runs(c, monkeypatch) for c in cases)
    print("%s %s: %d launches (views x switches x grid caps), worst gate ratio %.3f" % (kernel, shape, len(cases), worst))


def test_worst_gate_ratio_per_kernel():
    """the figures DESIGN.md section 5 quotes (runs after the cases above; alone it launches the largest shape of each kernel)"""
    if set(_worst) != set(FB.KERNELS.values()):
        mp = pytest.MonkeyPatch()
        try:
            for k in FB.KERNELS.values():
                for c in [c for c in FB.CASES if FB.kernel_of(c) == k and c.grid == 0 and c.shape == max(s for kk, s in GROUPS if kk == k)]:
                    check_runs(c, mp)
        finally:
            mp.undo()
    for k in sorted(_worst):
        print("%-28s worst gate ratio on the GPU %.3f" % (k, _worst[k]))
        assert _worst[k] <= 1.0


@pytest.mark.parametrize("case", FB.REFUSALS, ids=[c.name for c in FB.REFUSALS])
def test_refusals_leave_every_array_alone(case, monkeypatch):
    """one case per condition of c3_fused_applicable, bneck_fused_applicable, bneck_cv3_fused_applicable and reid_block_fused_applicable that
    a view or a shape can trip: the launcher's own quiet VC_ERR_ARG, nothing written"""
    monkeypatch.delenv("VC_CONV_CFG", raising=False)
    assert FB.refusal_reasons(case) == [case.reason]
    with pytest.raises(L.VcError) as ei:
        launch(case)
    assert ei.value.code == 1, case.name
    assert str(ei.value).endswith("status 1: "), case.name + ": not the launcher's own quiet refusal: " + str(ei.value)
    for before, after in zip(case.buffers(), ei.value.outputs):
        assert (before is None) == (after is None)
        assert before is None or np.array_equal(before, after, equal_nan=True), case.name + ": a refused launch wrote"
