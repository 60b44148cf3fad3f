"""GPU: the launch views of a convolution, one launch at a time, under every tile configuration (tests/conv_view_cases.py holds the cases, the
references and the acceptance table; tests/test_conv_view_cases.py holds that module to its own conditions).

Every (case, id) that EXPECT says runs is launched through vc_conv2d_view_host under VC_CONV_CFG = id and VC_CONV_STRICT (the id's own
kernel or an error), with a short persistent grid too where the family has one, and checked four ways:
  (a) every element outside the written slice, and every row >= min(M, m_valid), still holds the sentinel; the guard blocks around y
      and y2 are intact (the entry point reports a broken guard as an error);
  (b) the written slice is inside the project's own gate against float64 on the rounded operands: bf16 stores rtol 2^-7 / atol 2e-3,
      f32 stores (the f32 path and out_f32) rtol 1e-4 / atol 1e-4, fp8 arithmetic with the bf16 store the bf16 gate on the quantised
      operands; fp8 -> fp8 has no gate of its own and rests on (c) (tests/test_gpu_fp8_tiles.py holds the dense launch of every id, on
      these operands too, to float64);
  (c) the written slice equals, bit for bit, the DENSE launch of the same configuration through vc_conv2d_host wherever both take the
      same store path: every fp8 -> fp8 and f32 case, and the bf16 cases whose view keeps conv_epilogue_fast_bf16 as the dense launch has
      it.  m_dev rows are the first rows of the full launch; an `up` launch is compared with the dense launch on the concat that NumPy
      builds.  out_f32 results rounded to bf16 equal the dense bf16 result; out_bf16 results (another element type than the dense launch
      stores) equal the heuristic tile's launch of the same view.  The bf16 views with offsets that are multiples of 4 only take the
      general store loop where the dense launch takes the 16-byte lane-pair path: fp32 sums agree, but the two paths are different
      instruction sequences and nothing promises the same bits, so those cases have (a), (b) and (d) only;
  (d) the result is finite: every element of x, x_up and res that is not an operand is NaN, so an element that reaches a sum shows.
Every (case, id) that EXPECT says refuses must raise VcError code 1 under VC_CONV_STRICT and leave y / y2 at the sentinel, and without
VC_CONV_STRICT give what VC_CONV_CFG unset gives (launch_conv's fall-back), bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import conv_view_cases as V  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402

GROUPS = {"igemm0_13": tuple(range(0, 14)), "igemm14_27": tuple(range(14, 28)), "igemm40_68": (40, 41, 42, 43) + tuple(range(60, 69)),
          "splitk": V.IDS_SK, "halo": V.IDS_HALO + V.IDS_V2, "halo_s2": V.IDS_S2, "pointwise": V.IDS_DIRECT + V.IDS_STREAM, "direct8": V.IDS_D8}
assert sorted(i for g in GROUPS.values() for i in g) == list(range(V.NIDS))

_twin, _fallback = {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def launch(case):
    """the case through vc_conv2d_view_host under the environment as it stands: (y, y2) whole"""
    o = case.operands()
    x, xu, res, y, y2 = case.buffers()
    out = E.conv2d_view(x, o["w"], o["b"], y, view=case.v, x_up=xu, res=res, y2=y2, stride=case.stride, pad=case.pad, act=case.act,
                        res_mode=case.res_mode, precision=case.precision)
    return out if y2 is not None else (out, None)


def set_env(mp, cfg=None, strict=False, slots=0):
    for name, val in (("VC_CONV_CFG", cfg), ("VC_CONV_STRICT", 1 if strict else None), ("VC_CONV_SLOTS", slots or None)):
        if val is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(val))


def dense_twin(case, cfg, mp):
    """(M, cout): vc_conv2d_host on the same operands under the same configuration"""
    key = (case.problem_key(), cfg)
    if key not in _twin:
        set_env(mp, cfg, strict=True)
        o = case.operands()
        y = E.conv2d(case.x_dense(), o["w"], o["b"], stride=case.stride, pad=case.pad, act=case.act, res=o.get("res"), res_mode=case.res_mode,
                     precision=case.precision)
        _twin[key] = y.reshape(-1, case.cout)
    return _twin[key]


def fallback(case, mp):
    if case.name not in _fallback:
        set_env(mp)
        _fallback[case.name] = launch(case)
    return _fallback[case.name]


def check_runs(case, cfg, mp):
    for slots in ((0, 8) if cfg in V.PERSISTENT else (0,)):
        where = "%s id %d slots %d" % (case.name, cfg, slots)
        set_env(mp, cfg, strict=True, slots=slots)
        y, y2 = launch(case)
        assert (case.untouched(y, y2) == V.SENTINEL).all(), where + ": an element outside the written slice changed"             # (a)
        got = case.written(y, y2)[:case.rows]
        assert np.isfinite(got).all(), where + ": a non-operand element reached the result"                                      # (d)
        gate = V.gate_of(case)
        if gate is not None:                                                                                                      # (b)
            np.testing.assert_allclose(got, gate[0][:case.rows], err_msg=where, **gate[1])
        if case.twin_same_store_path:                                                                                             # (c)
            np.testing.assert_array_equal(bits(got), bits(dense_twin(case, cfg, mp)[:case.rows]), err_msg=where + ": differs from the dense launch")
        elif case.v["out_f32"]:
            np.testing.assert_array_equal(bits(V.rnd(got, "bf16")), bits(dense_twin(case, cfg, mp)[:case.rows]), err_msg=where + ": rounded to bf16, differs from the dense launch")
        elif case.v["out_bf16"]:
            fy, fy2 = fallback(case, mp)
            np.testing.assert_array_equal(bits(got), bits(case.written(fy, fy2)), err_msg=where + ": differs from the heuristic tile")


def check_refuses(case, cfg, mp):
    where = "%s id %d" % (case.name, cfg)
    set_env(mp, cfg, strict=True)
    with pytest.raises(L.VcError) as ei:
        launch(case)
    assert ei.value.code == 1, where
    assert str(ei.value).endswith("status 1: "), where + ": not the launcher's own quiet refusal: " + str(ei.value)
    for buf in ei.value.outputs:
        assert buf is None or (buf == V.SENTINEL).all(), where + ": a refused launch wrote"
    set_env(mp, cfg)
    y, y2 = launch(case)
    # (a) on the fall-back too: a family that took the launch and ignored a device-side count would have written the rows past it
    assert (case.untouched(y, y2) == V.SENTINEL).all(), where + ": the fall-back changed an element outside the written slice"
    assert np.isfinite(case.written(y, y2)[:case.rows]).all(), where
    fy, fy2 = fallback(case, mp)
    np.testing.assert_array_equal(bits(y), bits(fy), err_msg=where + ": the fall-back differs from the heuristic launch")
    if y2 is not None:
        np.testing.assert_array_equal(bits(y2), bits(fy2), err_msg=where)


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("row", V.ROWS)
def test_conv_views(row, group, monkeypatch):
    ran = refused = 0
    for cfg in GROUPS[group]:
        cases = V.cases_of(row, cfg)
        assert cases, (row, cfg)
        for case in cases:
            if V.EXPECT[row][cfg] == V.RUNS:
                check_runs(case, cfg, monkeypatch)
                ran += 1
            else:
                check_refuses(case, cfg, monkeypatch)
                refused += 1
    print("%s %s: %d (case, id) pairs ran, %d refused" % (row, group, ran, refused))


def test_conv_check_refusals_leave_the_outputs_alone(monkeypatch):
    """one case per VC_CHECK of conv_check that a view can trip (and the out_bf16 + split one this table added): VC_ERR_ARG with that check's
    message before any launch, y / y2 still the sentinel"""
    set_env(monkeypatch)
    for case in V.REFUSALS:
        assert not V.conv_check_admits(case), case.name
        with pytest.raises(L.VcError) as ei:
            launch(case)
        assert ei.value.code == 1, case.name
        assert (": " + case.message) in str(ei.value), (case.name, str(ei.value))      # conv_check's own line, not the entry point's checks
        for buf in ei.value.outputs:
            assert buf is None or (buf == V.SENTINEL).all(), case.name


@pytest.mark.parametrize("case", V.F2_CASES, ids=[c.name for c in V.F2_CASES])
def test_s2_conv_fused_with_its_pointwise_reader(case, monkeypatch):
    """conv3x3s2_halo_kernel<..., F2> (launch_s2halo_pw) as one launch: bit for bit configuration 49 followed by the pointwise conv on
    configuration 3, inside the bf16 gate against float64 (conv -> SiLU -> bf16 -> 1x1 -> SiLU), sentinels intact; the 3x3 reads a slice
    between NaN channels."""
    xs, w3, b3, w1, b1 = case.operands()
    B, H, W = case.shape
    x = np.full((B, H, W, case.v3["in_cs"]), np.nan, np.float32)
    x[..., case.v3["in_co"]:case.v3["in_co"] + case.cin] = xs
    _, _, _, y0, y20 = case.second.buffers()
    set_env(monkeypatch)
    out = E.conv_s2_pw(x, w3, b3, w1, b1, y0, view=dict(case.v3, **case.v1), y2=y20)
    y, y2 = out if y20 is not None else (out, None)
    assert (case.second.untouched(y, y2) == V.SENTINEL).all()
    got = case.second.written(y, y2)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, V.rnd(case.reference().astype(np.float32), "bf16"), **V.GATE["bf16"])
    set_env(monkeypatch, 49, strict=True)
    mid = E.conv2d_view(x, w3, b3, np.full((B, case.Ho, case.Wo, 128), V.SENTINEL, np.float32), view=case.v3, stride=2, pad=1, act=1)
    assert np.isfinite(mid).all()
    set_env(monkeypatch, 3, strict=True)
    un = E.conv2d_view(mid, w1, b1, y0, view=case.v1, y2=y20, act=1)
    uy, uy2 = un if y20 is not None else (un, None)
    np.testing.assert_array_equal(bits(y), bits(uy))
    if y2 is not None:
        np.testing.assert_array_equal(bits(y2), bits(uy2))
