"""CPU: the conditions under which the comparisons of tests/test_gpu_fp8_tiles.py mean something (tests/fp8_tile_cases.py), and the
comparisons themselves against the outputs of wrong kernels built from the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_view_cases as V
import fp8_tile_cases as T

EXACT = {p.tag: p for p in T.EXACT}
SILU = {p.tag: p for p in T.SILU_PROBLEMS}
ids_of = lambda ps: [p.name for p in ps]  # noqa: E731


# ---- 1. the ids ------------------------------------------------------------------------------------------------------------------------
def test_the_fp8_ids_are_the_nineteen_launch_one_takes_and_every_id_has_problems():
    assert T.FP8_IGEMM_IDS == (4, 5, 6, 8, 10, 12, 13, 15, 16, 18, 20, 22, 25, 27, 43, 60, 61, 62, 63)
    assert set(T.FP8_IGEMM_IDS) == {i for i, e in V.EXPECT["slices8/fp8"].items() if e == V.RUNS and i < 69}
    assert T.DIRECT_IDS == (69, 70, 71, 72) and len(T.IDS) == 19 + 4
    assert {T.RING[i] for i in T.FP8_IGEMM_IDS} == {2, 3, 4, 6, 8}
    for cfg in T.FP8_IGEMM_IDS:
        assert all(p.admits(cfg) for p in T.EXACT + T.SILU_PROBLEMS), cfg
    # the direct ids: pointwise problems only, by the acceptance table's own function; each has at least one
    took = {cfg: {p.tag for p in T.EXACT if p.admits(cfg)} for cfg in T.DIRECT_IDS}
    assert took == {69: {"pw64", "pw128"}, 70: {"pw256"}, 71: {"pw64", "pw128"}, 72: {"pw64", "pw128"}}
    assert not any(p.admits(cfg) for p in T.SILU_PROBLEMS for cfg in T.DIRECT_IDS)         # (all 3x3)
    assert not any(p.admits(cfg) for p in T.EXACT for cfg in range(V.NIDS) if cfg not in T.IDS)
    # the twins: the view cases' two dense problems under the heuristic's ids, id 43 and the direct ids that take them; pw64 elsewhere
    for cfg in T.IDS:
        tags = {name for name, _ in T.twins(cfg)}
        assert tags == (set() if cfg == 70 else {"twin-pw128", "twin-pw64"} if cfg in V.IDS_FP8 else {"twin-pw64_rest"}), cfg
        for _, c in T.twins(cfg):
            assert c.precision == "fp8" and V.accepts(c, cfg) and c.x_dense().shape == c.shape + (c.cin,)


def test_the_problems_are_the_ones_stated_and_reach_their_edges():
    want = {"taps": (2, 23, 19, 64, 72, 3, 1, 1, T.NONE, T.AFTER), "s2wrap": (3, 13, 11, 128, 136, 3, 2, 1, T.RELU, T.BEFORE),
            "thin": (1, 9, 9, 48, 40, 3, 1, 1, T.NONE, 0), "longk": (3, 5, 7, 1152, 64, 1, 1, 0, T.NONE, 0),
            "walk": (2, 25, 22, 24, 264, 3, 1, 1, T.RELU, 0), "pw64": (1, 17, 13, 64, 72, 1, 1, 0, T.NONE, 0),
            "pw128": (2, 12, 12, 128, 128, 1, 1, 0, T.RELU, T.AFTER), "pw256": (2, 11, 9, 256, 200, 1, 1, 0, T.RELU, T.BEFORE)}
    assert {t: (*p.shape, p.cin, p.cout, p.k, p.stride, p.pad, p.act, p.res_mode) for t, p in EXACT.items()} == want
    assert {t: (*p.shape, p.cin, p.cout, p.k, p.stride, p.pad, p.act, p.res_mode) for t, p in SILU.items()} == \
        {t: want[t][:8] + (T.SILU, want[t][9]) for t in ("taps", "s2wrap", "walk")}
    t, s, n, k, w = (EXACT[x] for x in ("taps", "s2wrap", "thin", "longk", "walk"))
    assert (t.K, t.nk, t.M) == (576, 5, 874) and t.K % T.BK == 64 and T.BK % t.cin_eff == 0 and t.cin_eff < T.BK          # a tile spans two taps, half-empty last tile
    assert t.M % 64 and any(m0 < t.Ho * t.Wo < m0 + 256 for m0 in range(0, t.M, 256)) and t.cout % 16 == 8
    assert (s.K, s.nk) == (1152, 9) and s.nk > max(T.RING.values()) and s.shape[1] % 2 and s.shape[2] % 2 and 128 < s.cout < 256
    assert (n.K, n.M) == (432, 81) and T.BK / n.cin_eff > 2.6 and 128 % n.cin_eff and n.M % 16         # 81 pixels: a ragged tile under every id, less than one of 128
    assert 64 < n.M < 128 and min(V.IGEMM[i][0] for i in T.FP8_IGEMM_IDS) == 64
    assert (k.nk, k.M, k.k) == (9, 105, 1)
    assert (w.cin, w.cin_eff, w.M) == (24, 32, 1100)
    for cfg in T.FP8_IGEMM_IDS:                                      # 8 workgroups walk more than one tile under every id
        BP, BC = V.IGEMM[cfg][:2]
        assert -(-w.M // BP) * -(-w.cout // BC) >= 10, cfg
    for p in T.EXACT + T.SILU_PROBLEMS:
        assert p.M * p.cout < 300000 and p.M * p.K * p.cout < 2 ** 28, p.name        # small


# ---- 2. the exact problems ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", T.EXACT, ids=ids_of(T.EXACT))
def test_exact_operands_follow_the_recipe(p):
    o = p.operands()
    x, w, b, res = o["x"], o["w"], o["b"], o["res"]
    assert p.act in (T.NONE, T.RELU) and (res is None) == (p.res_mode == 0)
    assert np.abs(x).max() == 2.0 and (x * 4 == np.round(x * 4)).all() and (T.q8(x) == x).all() and len(np.unique(x)) == 17
    amax = np.abs(w).reshape(p.cout, -1).max(1)
    sw = (amax / np.float32(448.0)).astype(np.float32)                # pack_and_upload: amax / 448.0f
    j = -np.log2(sw.astype(np.float64))
    assert (j == np.round(j)).all() and set(j) == set(range(9))       # the scale is exactly 2^-j, every j in 0 .. 8 occurs
    wq = (w / sw[:, None, None, None]).reshape(p.cout, -1)
    assert (wq == np.round(wq)).all() and (T.q8(wq) == wq).all()     # w / scale is an e4m3 integer
    assert ((np.abs(wq) == 448).sum(1) == 1).all() and (np.abs(wq)[np.abs(wq) != 448] <= 8).all()
    assert {-448.0, 448.0} <= set(np.unique(wq))
    np.testing.assert_array_equal(p.weights_used(), w)               # so quantising the weights changes nothing
    bq = b / sw
    assert (bq == np.round(bq)).all() and np.abs(bq).max() <= 64
    if res is not None:
        assert (T.q8(res) == res).all() and {448.0, -448.0, 2.0 ** -9, -2.0 ** -9} <= set(np.unique(res)) and len(np.unique(res)) > 200


@pytest.mark.parametrize("p", T.EXACT, ids=ids_of(T.EXACT))
def test_exact_reference_holds_in_fp32_whatever_the_order_and_reaches_the_value_edges(p):
    o = p.operands()
    A, Wm = p.im2col()
    acc = p.sums()
    assert acc.dtype == np.float64 and acc.shape == (p.M, p.cout)
    np.testing.assert_array_equal(A @ Wm.T, acc)                     # the K-ordered restatement is the float64 conv
    sw = np.abs(o["w"]).reshape(p.cout, -1).max(1).astype(np.float64) / 448.0
    # every product is a multiple of scale / 4 and the sum of their magnitudes is below 2^22 x scale / 4 ... so every partial sum, in any
    # order, is an integer below 2^24 in units of scale / 4: fp32 holds it
    units = np.abs(A) @ np.abs(Wm).T / sw * 4
    assert (units == np.round(units)).all() and units.max() < 2 ** 22
    assert np.abs(acc / sw).max() < 2 ** 12 and (acc / sw * 4 == np.round(acc / sw * 4)).all()       # the accumulators themselves: below 2^12
    A32, W32 = A.astype(np.float32), Wm.astype(np.float32)
    fwd = A32 @ W32.T
    rev = A32[:, ::-1] @ W32[:, ::-1].T
    tiles = np.zeros((p.M, p.cout), np.float32)
    for i in range(p.nk):                                            # as the MFMA adds: one K tile's sum on the running fp32 sum
        tiles = tiles + A32[:, i * T.BK:(i + 1) * T.BK] @ W32[:, i * T.BK:(i + 1) * T.BK].T
    for got in (fwd, rev, tiles):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.float64), acc)
    # acc (in units of the scale) x scale + bias in fp32, and the residual add behind it
    lin32 = (acc / sw).astype(np.float32) * sw.astype(np.float32) + o["b"]
    lin = acc + o["b"].astype(np.float64)
    assert lin32.dtype == np.float32
    np.testing.assert_array_equal(lin32.astype(np.float64), lin)
    pre = p.pre()
    np.testing.assert_array_equal(pre.astype(np.float32).astype(np.float64), pre)       # no double rounding on the way to e4m3
    if p.res_mode == T.BEFORE:
        lin = lin + o["res"].reshape(p.M, p.cout)
        np.testing.assert_array_equal(lin.astype(np.float32).astype(np.float64), lin)
    # the clamp decides at least 1 % of the bytes on each side.  Under ReLU no output is negative: there the low side is the value ReLU
    # takes (below -448 before the activation), and only the high side is an output
    e = p.expected()
    assert (pre > 448).mean() >= 0.01 and (e == 448).mean() >= 0.01, p.name
    if p.act == T.RELU:
        assert (lin < -448).mean() >= 0.01, p.name
    else:
        assert (pre < -448).mean() >= 0.01 and (e == -448).mean() >= 0.01, p.name
    # the subnormals of the store: 2^-9 .. 7 x 2^-9
    assert ((np.abs(e) > 0) & (np.abs(e) < 2.0 ** -6)).any(), p.name
    assert np.isfinite(e).all() and (T.q8(e) == e).all()


def test_exact_problems_also_store_exact_zeros_and_rounding_ties():
    zeros = sum(int((p.expected() == 0).sum()) for p in T.EXACT if p.act == T.NONE)
    assert zeros > 0
    # a value half way between two e4m3 neighbours: round to nearest EVEN decides the byte
    ties = 0
    for p in T.EXACT:
        pre, e = np.clip(p.pre(), -448, 448), p.expected().astype(np.float64)
        up = T.q8(np.nextafter(pre.astype(np.float32), np.float32(np.inf))).astype(np.float64)
        dn = T.q8(np.nextafter(pre.astype(np.float32), np.float32(-np.inf))).astype(np.float64)
        ties += int(((up != dn) & (pre != e)).sum())
    assert ties > 100


# ---- 3. the SiLU problems and the twins ----------------------------------------------------------------------------------------------------
def conv32(x, wq, b, res, stride, pad, act, res_mode):
    """the same launch in torch's float32"""
    t = F.conv2d(torch.tensor(x).permute(0, 3, 1, 2), torch.tensor(wq), torch.tensor(b), stride=stride, padding=pad)
    r = None if res is None else torch.tensor(res).permute(0, 3, 1, 2)
    if res_mode == T.BEFORE:
        t = t + r
    t = F.silu(t) if act == T.SILU else (F.relu(t) if act == T.RELU else t)
    if res_mode == T.AFTER:
        t = t + r
    return T.q8(t.permute(0, 2, 3, 1).reshape(-1, wq.shape[0]).numpy())


@pytest.mark.parametrize("p", T.SILU_PROBLEMS, ids=ids_of(T.SILU_PROBLEMS))
def test_silu_inputs_leave_the_reference_alone_well_inside_the_cap(p):
    o = p.operands()
    assert p.act == T.SILU and (T.q8(o["x"]) == o["x"]).all() and (o["res"] is None or (T.q8(o["res"]) == o["res"]).all())
    A, Wm = p.im2col()
    np.testing.assert_allclose(A @ Wm.T, p.sums(), rtol=0, atol=1e-12)
    y = conv32(o["x"], p.weights_used(), o["b"], o["res"], p.stride, p.pad, p.act, p.res_mode)
    same = float((y == p.expected()).mean())
    print(p.name, "float32 conv identical to the float64 reference: %.5f" % same)
    assert same >= 0.99, same
    assert T.gate_mismatch(y, p.expected()) is None
    assert np.abs(p.pre()).max() < 448                                # no saturation here: the exact problems own that


def test_twin_operands_leave_the_reference_alone_too():
    seen = set()
    for cfg in T.IDS:
        for name, c in T.twins(cfg):
            if name in seen:
                continue
            seen.add(name)
            o = c.operands()
            y = conv32(c.x_dense(), c.weights_used(), o["b"], o.get("res"), c.stride, c.pad, c.act, c.res_mode)
            ref = T.twin_expected(c)
            assert ref.shape == (c.M, c.cout) and float((y == ref).mean()) >= 0.99 and T.gate_mismatch(y, ref) is None, name
    assert seen == {"twin-pw128", "twin-pw64", "twin-pw64_rest"}


# ---- 4. the comparisons reject wrong kernels -----------------------------------------------------------------------------------------------
def stored(p, A, Wm):
    """what a kernel that multiplied A by Wm stores"""
    return T.q8(p.finish(A @ Wm.T))


def last_tile_dropped(p):
    A, Wm = p.im2col()
    A[:, (p.nk - 1) * T.BK:] = 0
    return stored(p, A, Wm)


def stale_ring_slot(p, ns):
    """K tile i multiplied out of a slot that still holds tile i - ns (both operands share a stage)"""
    A, Wm = p.im2col()
    A2, W2 = A.copy(), Wm.copy()
    for i in range(ns, p.nk):
        A2[:, i * T.BK:(i + 1) * T.BK] = A[:, (i - ns) * T.BK:(i - ns + 1) * T.BK]
        W2[:, i * T.BK:(i + 1) * T.BK] = Wm[:, (i - ns) * T.BK:(i - ns + 1) * T.BK]
    return stored(p, A2, W2)


def ring_read_as_neighbour(p):
    A, Wm = p.im2col("edge")
    return stored(p, A, Wm)


def clamp_left_out(p):
    y = p.expected().copy()
    y[np.abs(p.pre()) > 448] = np.nan                                # v_cvt_pk_fp8_f32 does not saturate
    return y


def second_image_shifted(p):
    y, hw = p.expected().copy(), p.Ho * p.Wo
    y[hw:2 * hw] = np.roll(y[hw:2 * hw], 1, axis=0)
    return y


def both_kinds(tags):
    return [EXACT[t] for t in tags] + [SILU[t] for t in tags if t in SILU]


def rejects(p, y, what):
    msg = (T.exact_mismatch if p.kind == "exact" else T.gate_mismatch)(y, p.expected())
    assert msg is not None, "%s: %s passes" % (p.name, what)
    return msg


def test_the_comparisons_accept_the_reference_and_name_the_first_difference():
    for p in T.EXACT + T.SILU_PROBLEMS:
        assert T.exact_mismatch(p.expected(), p.expected()) is None and T.gate_mismatch(p.expected(), p.expected()) is None
        A, Wm = p.im2col()
        assert (T.exact_mismatch if p.kind == "exact" else T.gate_mismatch)(stored(p, A, Wm), p.expected()) is None, p.name
    p = EXACT["thin"]
    y = p.expected().copy()
    y[37, 5] = y[37, 5] + 1 if y[37, 5] != 96 else 0
    y[60, 2] = np.nan
    assert "2 of 3240 outputs differ; first at pixel 37, channel 5" in T.exact_mismatch(y, p.expected())
    assert T.exact_mismatch(y[:-1], p.expected()).startswith("shape")
    # the gate: one ulp passes while few, more than 3 % of them or two ulps do not
    s = SILU["walk"]
    e = s.expected()
    ulp_up = T.q8(np.nextafter(T.q8(e * 1.07), np.float32(np.inf)))
    assert T.gate_mismatch(np.where(np.arange(e.size).reshape(e.shape) % 40 == 0, ulp_up, e), e) is None
    assert "identical" in T.gate_mismatch(np.where(np.arange(e.size).reshape(e.shape) % 25 == 0, ulp_up, e), e)
    y = e.copy()
    y[3, 3] = T.q8(e[3:4, 3] * 1.3 + 0.01)[0]
    assert "one e4m3 ulp" in T.gate_mismatch(y, e)
    y[3, 3] = np.inf
    assert "finite" in T.gate_mismatch(y, e)


@pytest.mark.parametrize("p", both_kinds(("taps", "s2wrap", "longk")), ids=ids_of(both_kinds(("taps", "s2wrap", "longk"))))
def test_a_dropped_last_k_tile_is_rejected(p):
    rejects(p, last_tile_dropped(p), "the last K tile dropped")


@pytest.mark.parametrize("ns", (3, 4, 6, 8))
@pytest.mark.parametrize("p", both_kinds(("s2wrap", "longk")), ids=ids_of(both_kinds(("s2wrap", "longk"))))
def test_a_ring_slot_read_one_lap_late_is_rejected(p, ns):
    assert p.nk > ns
    rejects(p, stale_ring_slot(p, ns), "K tile i replaced by tile i - %d" % ns)


@pytest.mark.parametrize("p", both_kinds(("taps", "s2wrap")), ids=ids_of(both_kinds(("taps", "s2wrap"))))
def test_a_padding_ring_read_as_the_neighbouring_pixel_is_rejected(p):
    rejects(p, ring_read_as_neighbour(p), "the padding ring read as the neighbouring pixel")


@pytest.mark.parametrize("p", T.EXACT, ids=ids_of(T.EXACT))
def test_a_missing_clamp_is_rejected(p):
    y = clamp_left_out(p)
    assert np.isnan(y).mean() >= 0.01
    assert "differ" in rejects(p, y, "the clamp left out")


@pytest.mark.parametrize("p", both_kinds(("taps",)), ids=ids_of(both_kinds(("taps",))))
def test_a_second_image_shifted_by_one_pixel_is_rejected(p):
    msg = rejects(p, second_image_shifted(p), "rows of the second image shifted by one pixel")
    if p.kind == "exact":
        assert "first at pixel %d," % (p.Ho * p.Wo) in msg or "first at pixel %d," % (p.Ho * p.Wo + 1) in msg
