"""GPU: the kernels that open a detector pass -- stem_direct_kernel<CT, U8> (CT = 1 .. 4), stem_direct_wide_kernel<5, U8> and
front_fused_kernel<false> / <true> / <true, false, true> -- one launch at a time, without an engine (tests/front_cases.py holds the cases, the
buffers and the float64 references; tests/test_front_cases.py holds that module to its own conditions).

Every case goes through vc_stem_host / vc_front_fused_host, which fill the ConvPs as the engine's plan fills them and call the launcher the engine
calls, and is checked these ways:
  (a) every element outside the written slice still holds the sentinel; the entry point itself reports as errors a broken guard block around an
      output or an input, a changed input, and -- direct launches -- a letterboxed tensor or a layer 0 that did not stay untouched;
  (b) the written slice is finite: the guard blocks around the tensor input are bf16 NaNs;
  (c) the written slice is inside the project's bf16 gate (conv_view_cases.GATE, rtol 2^-7 / atol 2e-3) of the float64 reference;
  (d) the written slice equals, bit for bit, the SAME ConvPs run through launch_conv by the same entry point (behind launch_letterbox for
      frames), under VC_CONV_CFG = 3 with VC_CONV_STRICT and on the heuristic's tile; one ragged stem case per width also under every
      implicit-GEMM id;
  (e) the e4m3 view equals, byte for byte, q8 (tests/test_gpu_fp8.py) of the kernel's own bf16 output times inv_scale, and
      vc_bf16_to_fp8_host on that output;
  (f) grid caps of 1, 2 and 3 workgroups give the bytes of the product's grid.
Every refusal case must raise VcError code 1 with the launcher's own message (most are quiet) and leave every array as it was passed."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import front_cases as FC  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from aux_cases import rnd  # noqa: E402
from conv_view_cases import GATE  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402

_twin = {}
_product = {}
_worst = collections.defaultdict(float)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def launch(case, mode=1):
    y, q = case.buffers()
    net = case.net[1:]
    try:
        if case.kind == "stem":
            return E.stem(case.input(), *case.weights(), y, view=case.view_dict(mode), net=net, q8=q)
        return E.front_fused(case.input(), *case.weights(), y, view=case.view_dict(mode), net=net), None
    except L.VcError as err:
        if err.code == 2:                # VC_ERR_HIP: a device error or a write outside a buffer -- nothing more is launched on that device
            pytest.exit("%s (mode %d): %s" % (case.name, mode, err), returncode=3)
        raise


def set_env(mp, cfg=None, strict=False):
    for name, val in (("VC_CONV_CFG", cfg), ("VC_CONV_STRICT", 1 if strict else None), ("VC_CONV_SLOTS", None)):
        if val is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(val))


def twin(case, mp, cfg):
    """(written slice, e4m3 slice or None): the case's ConvPs through launch_conv under tile id cfg (None: the heuristic's)"""
    key = case.twin_key() + (cfg,)
    if key not in _twin:
        set_env(mp, cfg, strict=cfg is not None)
        y, q = launch(case, mode=0)
        assert case.untouched_ok(y, q), case.name + ": the launch_conv chain changed an element outside its outputs"
        _twin[key] = (case.written(y).copy(), case.written_q(q).copy() if case.q else None)
        set_env(mp)
    return _twin[key]


def check_runs(case, mp):
    set_env(mp)
    y, q = launch(case)
    assert case.untouched_ok(y, q), case.name + ": an element outside the written slice changed"                                  # (a)
    got = case.written(y)
    assert np.isfinite(got).all(), case.name + ": a value from outside the input reached the result"                               # (b)
    ref = case.reference()
    ratio = FC.gate_ratio(got, ref)
    print("%-58s %-36s gate ratio %.3f" % (case.name, case.instance, ratio))
    _worst[FC.kernel_of(case)] = max(_worst[FC.kernel_of(case)], ratio)
    np.testing.assert_allclose(got, rnd(ref.astype(np.float32), "bf16"), err_msg="%s (gate ratio %.3f)" % (case.name, ratio), **GATE["bf16"])   # (c)
    for cfg in (3, None):                                                                                                          # (d)
        ty, tq = twin(case, mp, cfg)
        np.testing.assert_array_equal(bits(got), bits(ty), err_msg="%s: differs from launch_conv under tile %s" % (case.name, cfg))
        if case.q:
            np.testing.assert_array_equal(case.written_q(q), tq, err_msg="%s: e4m3 view differs from the bf16 -> fp8 launch behind tile %s" % (case.name, cfg))
    if case.q:                                                                                                                     # (e)
        gq = case.written_q(q)
        want = FC.q8_reference(got, case.q[2])
        assert np.array_equal(gq, want), "%s: %d bytes of the e4m3 view are not q8(y * inv_scale)" % (case.name, int((gq != want).sum()))
        cast = E.bf16_to_fp8(got, case.cout, 0, case.q[2], np.full((case.npix, case.cout), FC.Q_SENTINEL, np.uint8), 0)
        assert np.array_equal(gq, cast), case.name + ": e4m3 view differs from vc_bf16_to_fp8_host on the same y"
    key = case.twin_key()                                                                                                          # (f)
    if case.grid == 0:
        _product[key] = (got.copy(), case.written_q(q).copy() if case.q else None)
    else:
        assert key in _product, case.name
        np.testing.assert_array_equal(bits(got), bits(_product[key][0]), err_msg=case.name + ": the grid cap changed the result")
    return ratio


GROUPS = sorted({(c.kind, c.cout, c.net) for c in FC.CASES})


@pytest.mark.parametrize("kind,cout,net", GROUPS, ids=["%s%d-%dx%dx%d" % ((k, co) + n) for k, co, n in GROUPS])
def test_front_kernel(kind, cout, net, monkeypatch):
    cases = sorted([c for c in FC.CASES if (c.kind, c.cout, c.net) == (kind, cout, net)], key=lambda c: c.grid)                 # the product's grid first
    assert cases
    worst = max(check_runs(c, monkeypatch) for c in cases)
    print("%s %d %s: %d launches (inputs x views x grid caps), worst gate ratio %.3f" % (kind, cout, net, len(cases), worst))


@pytest.mark.parametrize("case", FC.IGEMM_SWEEP, ids=[c.name for c in FC.IGEMM_SWEEP])
def test_stem_equals_every_implicit_gemm_tile(case, monkeypatch):
    """"bit-identical to conv_igemm_kernel" -- held here for every tile id of that family, not only the tuned one"""
    assert len(FC.IGEMM_SWEEP) == len(FC.STEM_COUTS) and case.units == 2
    set_env(monkeypatch)
    y, _ = launch(case)
    got = bits(case.written(y))
    differ = [cfg for cfg in FC.IDS_IGEMM if not np.array_equal(got, bits(twin(case, monkeypatch, cfg)[0]))]
    assert not differ, "%s: differs from conv_igemm_kernel under tile ids %s" % (case.name, differ)


def test_worst_gate_ratio_per_kernel(monkeypatch):
    """the figures DESIGN.md section 5 quotes (runs after the cases above; alone it launches the multi-frame shape of each kernel)"""
    kernels = {"stem_direct_kernel", "stem_direct_wide_kernel", "front_fused_kernel"}
    if set(_worst) != kernels:
        for c in FC.CASES:
            if c.net[0] == 3 and c.grid == 0 and c.view == "dense" and c.cout in (64, 80):
                check_runs(c, monkeypatch)
    for k in sorted(_worst):
        print("%-26s worst gate ratio on the GPU %.3f" % (k, _worst[k]))
        assert _worst[k] <= 1.0
    assert set(_worst) == kernels


@pytest.mark.parametrize("case", FC.REFUSALS, ids=[c.name for c in FC.REFUSALS])
def test_refusals_leave_every_array_alone(case, monkeypatch):
    """one case per condition of launch_stem_direct, launch_stem_direct_u8 and launch_front_fused that a geometry, a view or a width can trip:
    VC_ERR_ARG with the launcher's own message (quiet but for the e4m3 view and the staging limit), nothing written"""
    set_env(monkeypatch)
    assert FC.refusal_reasons(case) == [case.reason]
    with pytest.raises(L.VcError) as ei:
        launch(case)
    assert ei.value.code == 1, case.name
    assert str(ei.value).endswith("status 1: " + case.message), case.name + ": not the launcher's own refusal: " + str(ei.value)
    for before, after in zip(case.buffers(), ei.value.outputs):
        assert (before is None) == (after is None)
        assert before is None or np.array_equal(before, after), case.name + ": a refused launch wrote"
