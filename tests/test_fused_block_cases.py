"""CPU: tests/fused_block_cases.py held to its own conditions -- the table reaches every geometry class, view and grid cap it promises
(checked by predicate, not by name), the buffers carry the poison and the sentinel where the module says, the restated applicability
takes every case and refuses every refusal for exactly its reason, and an independent float32-accumulating emulation of every chain
stays inside the project's bf16 gate of the float64 reference."""
import collections

import numpy as np

import fused_block_cases as FB
from aux_cases import SENTINEL
from conv_view_cases import GATE


def _by(pred):
    return [c for c in FB.CASES if pred(c)]


def test_shapes_reach_every_geometry_class():
    for what, pred in FB.CLASSES.items():
        hit = [s for s in FB.SHAPES if pred(*s)]
        assert len(hit) == 1, (what, hit)
        print("%-66s %s, %d tiles" % (what, hit[0], FB.ntiles(*hit[0])))
    assert len({tuple(p(*s) for p in FB.CLASSES.values()) for s in FB.SHAPES}) == len(FB.SHAPES)       # no shape stands for two classes
    for kind, cv3 in (("c3", 0), ("bneck", 0), ("bneck", 1)):
        for res in ((1,) if kind == "c3" else (0, 1)):
            for s in FB.SHAPES:
                assert _by(lambda c: c.kind == kind and c.cv3 == cv3 and c.res == res and c.shape == s), (kind, cv3, res, s)
    assert sorted({c.shape[0] for c in _by(lambda c: c.kind == "reid")}) == [1, 2, 3, 7]
    assert {c.shape[0] for c in _by(lambda c: c.kind != "reid")} >= {1, 2, 3, 5}                          # B other than 3 too


def test_every_problem_runs_on_every_grid_cap():
    caps = collections.defaultdict(set)
    for c in FB.CASES:
        caps[c.twin_key()].add(c.grid)
    for key, got in caps.items():
        units = key[1][0] if key[0] == "reid" else FB.ntiles(*key[1])
        assert got == ({0, 1, 2, 3} if units >= 4 else {0, 1, 2}), (key, got)
    # a workgroup that takes a second and a third tile or crop, for every kernel
    for k in FB.KERNELS.values():
        assert _by(lambda c: FB.kernel_of(c) == k and 0 < c.grid and c.units >= 3 * c.grid), k
    print("%d cases, %d unfused twins" % (len(FB.CASES), len(caps)))


def test_views_cover_the_product_layouts_and_the_others():
    aligned = lambda c, n: all(c.v[f] % n == 0 for f in ("in_cs", "in_co", "out_cs", "out_co", "z_cs", "z_co"))
    off_product = lambda c: c.v["in_co"] > 0 and c.v["out_co"] > 0 and c.v["in_cs"] > c.v["in_co"] + 64 and not c.v["out_buf"] and aligned(c, 8)
    c3 = _by(lambda c: c.kind == "c3")
    assert [c for c in c3 if c.v["in_cs"] == 64 and c.v["out_cs"] == 64]                                   # dense 64 -> 64
    assert [c for c in c3 if off_product(c)]
    bn = _by(lambda c: c.kind == "bneck" and not c.cv3)
    assert [c for c in bn if c.v["in_cs"] == 64 and (c.v["out_cs"], c.v["out_co"]) == (128, 0)]           # x dense, m -> cat[0:64]
    assert [c for c in bn if off_product(c)]
    one = [c for c in bn if c.v["out_buf"] == 1]
    assert one and all(abs(c.v["out_co"] - c.v["in_co"]) >= 64 for c in one)                               # disjoint slices of ONE buffer
    cv = _by(lambda c: c.cv3)
    cat = [c for c in cv if c.v["in_cs"] == 64 and (c.v["out_cs"], c.v["out_co"]) == (128, 0)]            # y2 at 64 of the concat buffer
    assert [c for c in cat if (c.v["z_cs"], c.v["z_co"]) == (128, 0)] and [c for c in cat if (c.v["z_cs"], c.v["z_co"]) == (256, 128)]
    assert [c for c in cv if off_product(c) and c.v["z_co"] > 0 and c.v["out_cs"] != c.v["in_cs"]]        # y2's stride is not x's
    rd = _by(lambda c: c.kind == "reid")
    assert [c for c in rd if c.v["in_cs"] == 64 and c.v["out_cs"] == 64] and [c for c in rd if off_product(c)]
    four = [c for c in rd if c.v["out_co"] % 8 == 4]
    assert four and all(not c.twin_same_store_path for c in four)
    assert all(c.twin_same_store_path for c in FB.CASES if c not in four)
    for c in FB.CASES:                                                                                      # every slice inside its stride
        assert c.v["in_cs"] >= c.v["in_co"] + 64 and c.v["out_cs"] >= c.v["out_co"] + (128 if c.cv3 else 64), c.name
        assert not c.cv3 or c.v["z_cs"] >= c.v["z_co"] + 128, c.name
    assert len({c.name for c in FB.CASES + FB.REFUSALS}) == len(FB.CASES) + len(FB.REFUSALS)


def test_buffers_carry_poison_and_sentinel():
    for c in FB.CASES + FB.REFUSALS:
        x, y, z = c.buffers()
        o, v = c.operands(), c.v
        assert np.array_equal(x[..., v["in_co"]:v["in_co"] + 64], o["x"]), c.name
        assert c.untouched_ok(x, y, z) and c.untouched_ok(x, y, z, unfused=True), c.name
        if c.reason:
            continue
        got = c.written(x, y, z)
        assert got.shape == (c.npix, c.cout) and (got == SENTINEL).all(), c.name                            # the output starts as the sentinel
        n_op = x.shape[:3] + (64,)
        if c.cv3:
            cat = x if v["out_buf"] else y
            assert np.array_equal(cat[..., v["out_co"] + 64:v["out_co"] + 128], o["y2"]), c.name
            assert np.isnan(cat[..., v["out_co"]:v["out_co"] + 64]).all(), c.name                          # m: never read, never written
            assert np.isnan(cat).sum() == cat.size - np.prod(n_op), c.name
        elif y is not None:
            assert (y == SENTINEL).all(), c.name
        if not v["out_buf"] and v["z_buf"] != 1:
            assert np.isnan(x).sum() == x.size - np.prod(n_op), c.name                                      # every non-operand of x is NaN
        # a changed element anywhere outside the written slice shows
        for buf in (x, y, z):
            if buf is None or c.grid:                                                                       # (the cap does not change the buffers)
                continue
            idx = np.argwhere(np.ones(buf.shape, bool))
            keep = [tuple(i) for i in idx[:: max(1, len(idx) // 7)]]
            for i in keep:
                dest, co = c._dest(x, y, z)
                if buf is dest and co <= i[3] < co + c.cout:
                    continue
                old = buf[i]
                buf[i] = 1.5
                assert not c.untouched_ok(x, y, z), (c.name, i)
                buf[i] = old
    for a in FB._operands("bneck", (2, 9, 33)).values():
        assert (a != SENTINEL).all() and np.isfinite(a).all()
    xs = FB._operands("c3", (1, 20, 28))["x"]
    assert (xs < 0).mean() > 0.4 and (xs > 0).mean() > 0.4 and (xs[:, :, 1:] != xs[:, :, :-1]).mean() > 0.99   # both signs, no flat regions


def test_restated_applicability():
    for c in FB.CASES:
        assert FB.refusal_reasons(c) == [], c.name
    want = {"output over the input slice", "cv3 output over x", "cv3 output over [m | y2]", "input slice not 8-aligned", "output in the input buffer",
            "map is not 25 x 25", "chain broken: split"}
    assert {c.reason for c in FB.REFUSALS} == want
    for c in FB.REFUSALS:
        assert FB.refusal_reasons(c) == [c.reason], (c.name, FB.refusal_reasons(c))
    assert {c.kind for c in FB.REFUSALS if c.reason == "input slice not 8-aligned"} == {"c3", "bneck"}


def test_emulation_inside_the_gate():
    """float32 convolutions with the same roundings against the float64 reference: inside the bf16 gate for every problem, never two ulps"""
    worst = collections.defaultdict(float)
    ulp1 = collections.defaultdict(lambda: [0, 0])
    seen = set()
    for c in FB.CASES:
        if c.problem() in seen:
            continue
        seen.add(c.problem())
        ref, emu = c.reference(), c.emulation()
        assert ref.shape == emu.shape == (c.npix, c.cout) and np.isfinite(ref).all()
        assert np.abs(ref).max() > 0.5, c.name
        r = FB.gate_ratio(emu, ref)
        assert r < 1.0, (c.name, r)
        np.testing.assert_allclose(emu, FB.rnd(ref.astype(np.float32), "bf16"), err_msg=c.name, **GATE["bf16"])
        k = FB.kernel_of(c)
        worst[k] = max(worst[k], r)
        ulp1[k][0] += int((emu != FB.rnd(ref.astype(np.float32), "bf16")).sum())
        ulp1[k][1] += emu.size
    assert set(worst) == set(FB.KERNELS.values())
    for k in sorted(worst):
        print("%-28s emulation worst gate ratio %.3f, %.1e of %d elements off by one bf16 ulp" % (k, worst[k], ulp1[k][0] / ulp1[k][1], ulp1[k][1]))


def test_references_tell_the_planted_faults_apart():
    """the reference is sensitive to what the GPU test must catch: a halo filled with SiLU(bias) instead of 0 moves border pixels outside
    the gate (computed here by padding b1 with the activation of the bias on a one-tile map)"""
    import torch
    import torch.nn.functional as F
    o = {k: torch.as_tensor(np.array(v)).double() for k, v in FB._operands("bneck", (2, 8, 16)).items()}
    x = o["x"].permute(0, 3, 1, 2)
    b1 = FB.silu(F.conv2d(x, o["w1"], o["b1"])).float().bfloat16().double()
    pad = FB.silu(o["b1"]).float().bfloat16().double().view(1, 64, 1, 1).expand(2, 64, 10, 18).clone()
    pad[:, :, 1:-1, 1:-1] = b1
    wrong = FB.silu(F.conv2d(pad, o["w2"], o["b2"])).permute(0, 2, 3, 1).reshape(-1, 64).numpy()
    ref = FB._reference("bneck", (2, 8, 16), 0, 0)
    assert FB.gate_ratio(FB.rnd(wrong.astype(np.float32), "bf16"), ref) > 4.0
