"""GPU: the fp8 convolution under EVERY tile id the tuner can pick (engine_run.hip::tuned_cfg), one dense launch at a time through
vc_conv2d_host under VC_CONV_CFG = id, VC_CONV_STRICT (the id's own kernel or an error) and VC_CONV_SLOTS in (0, 8): the 19 implicit-GEMM
ids conv_igemm.hip::launch_one takes for fp8 and the direct pointwise ids 69 - 72 on the problems they admit.  tests/fp8_tile_cases.py holds
the problems, the float64 references and the comparisons; tests/test_fp8_tile_cases.py holds that module to its own conditions and shows
that the comparisons reject a dropped K tile, a ring slot read one lap late, a misread padding ring, a missing clamp and a shifted image.

Per id:
  exact   operands whose sums are exact in fp32 in any order (multiples of 2^-2 below 2^12): the stored bytes equal the float64 reference's
          clamp + e4m3 rounding, np.array_equal, no allowance.  3 - 4 % of the outputs per side sit on the clamp, others in the subnormals.
          (This assumes the MX-scaled fp8 MFMA adds such products exactly.)
  silu    three of the shapes with SiLU and standard_normal operands at step 1 of the fp8 ladder: one e4m3 ulp,
          >= 97 % of the bytes identical, finite
  twin    the operand sets of the fp8 view cases' dense launches at the same gate: tests/test_gpu_conv_views.py check (c) compares a view
          with this launch bit for bit, and this holds the launch itself to float64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import conv_view_cases as V  # noqa: E402
import fp8_tile_cases as T  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402


def set_env(mp, cfg, slots):
    mp.setenv("VC_CONV_STRICT", "1")                              # a refusal is an error, not a quiet fall-back to the heuristic's tile
    mp.setenv("VC_CONV_CFG", str(cfg))
    if slots:
        mp.setenv("VC_CONV_SLOTS", str(slots))
    else:
        mp.delenv("VC_CONV_SLOTS", raising=False)


def launch(x, o, cout, stride, pad, act, res_mode):
    y = E.conv2d(x, o["w"], o["b"], stride=stride, pad=pad, act=act, res=o.get("res"), res_mode=res_mode, precision="fp8")
    return y.reshape(-1, cout)


@pytest.mark.parametrize("cfg", T.IDS)
def test_fp8_conv_under_every_tile_id_against_float64(cfg, monkeypatch):
    ran = {"exact": 0, "silu": 0, "twin": 0}
    failures = []
    for slots in T.SLOTS:
        set_env(monkeypatch, cfg, slots)
        for p in T.EXACT + T.SILU_PROBLEMS:
            if not p.admits(cfg):
                continue
            y = launch(p.operands()["x"], p.operands(), p.cout, p.stride, p.pad, p.act, p.res_mode)
            msg = (T.exact_mismatch if p.kind == "exact" else T.gate_mismatch)(y, p.expected())
            ran[p.kind] += 1
            if msg:
                failures.append("id %d, %s, slots %d: %s" % (cfg, p.name, slots, msg))
        for name, c in T.twins(cfg):
            y = launch(c.x_dense(), c.operands(), c.cout, c.stride, c.pad, c.act, c.res_mode)
            msg = T.gate_mismatch(y, T.twin_expected(c))
            ran["twin"] += 1
            if msg:
                failures.append("id %d, %s, slots %d: %s" % (cfg, name, slots, msg))
    print("id %d: %d (problem, slots) pairs ran: %d exact, %d silu, %d twin; %d failed" % (cfg, sum(ran.values()), ran["exact"], ran["silu"], ran["twin"], len(failures)))
    assert ran["exact"] > 0, "id %d ran no exact problem" % cfg
    assert not failures, "\n".join(failures)


def test_every_other_id_refuses_fp8_and_the_direct_ids_what_they_do_not_admit(monkeypatch):
    """VC_CONV_CFG / VC_CONV_STRICT decide the kernel of the launches above: an id outside the 19 + 4 refuses the smallest exact problem, a
    direct id every problem fp8_tile_cases.Problem.admits denies it (quietly: VC_ERR_ARG, nothing launched)"""
    refused = 0
    for cfg in range(V.NIDS):
        for p in T.EXACT:
            if p.admits(cfg) or (cfg not in T.DIRECT_IDS and p.tag != "pw64"):
                continue
            set_env(monkeypatch, cfg, 0)
            with pytest.raises(L.VcError) as ei:
                launch(p.operands()["x"], p.operands(), p.cout, p.stride, p.pad, p.act, p.res_mode)
            assert ei.value.code == 1, (cfg, p.name, str(ei.value))
            refused += 1
    print("%d (id, problem) pairs refused" % refused)
    assert refused == (V.NIDS - len(T.IDS)) + sum(not p.admits(cfg) for cfg in T.DIRECT_IDS for p in T.EXACT)
