"""CPU: tests/front_cases.py held to its own conditions -- the shape tables reach every geometry class they promise (by predicate, not by name),
every frame geometry selects the kernel instance it is there for (the launchers' predicates restated), the buffers carry the sentinel, the
references are sensitive to the faults the GPU test must catch, at least half of every reference output is well away from zero, and an
independent float32-accumulating emulation of every chain stays inside the project's bf16 gate of the float64 reference."""
import collections

import numpy as np
import torch

import front_cases as FC
from aux_cases import SENTINEL
from conv_view_cases import GATE


def _by(pred):
    return [c for c in FC.CASES if pred(c)]


def test_shapes_reach_every_geometry_class():
    for kind, shapes, out, (th, tw) in (("stem", FC.STEM_SHAPES, FC.stem_out, (FC.STEM_TH, FC.STEM_TW)), ("front", FC.FRONT_SHAPES, FC.front_out, (FC.FF_TH, FC.FF_TW))):
        for what, pred in FC.CLASSES.items():
            hit = [s for s in shapes if pred(s[0], *out(*s[1:]), th, tw)]
            assert len(hit) == 1, (kind, what, hit)
            print("%-5s %-58s %s -> %s, %d tiles" % (kind, what, hit[0], out(*hit[0][1:]), FC.ntiles(kind, hit[0])))
    assert FC.ntiles("stem", (3, 34, 130)) == 27 and FC.stem_out(34, 130) == (17, 65)
    assert FC.ntiles("front", (3, 68, 132)) == 18 and FC.front_out(68, 132) == (17, 33)
    assert [FC.ntiles("stem", s) for s in FC.STEM_SHAPES[:2]] == [1, 1] and [FC.ntiles("stem", s) for s in FC.STEM_SHAPES[2:4]] == [2, 2]
    assert [FC.ntiles("front", s) for s in FC.FRONT_SHAPES[:2]] == [1, 1] and [FC.ntiles("front", s) for s in FC.FRONT_SHAPES[2:4]] == [2, 2]
    # the engine's 8-pixel granularity, and the one tensor whose layer 0 has odd sides
    assert FC.front_out(32, 96) == (8, 24) and (1, 32, 96) in FC.FRONT_SHAPES
    assert FC.stem_out(34, 70) == (17, 35) and FC.front_out(34, 70) == (9, 18) and (1, 34, 70) in FC.FRONT_SHAPES
    odd = [s for s in FC.FRONT_SHAPES if FC.stem_out(*s[1:])[0] % 2 or FC.stem_out(*s[1:])[1] % 2]
    assert odd == [(1, 34, 70)]
    # every stem width on every shape, from the tensor and from frames
    for co in FC.STEM_COUTS:
        for s in FC.STEM_SHAPES:
            for u8 in (False, True):
                assert _by(lambda c: c.kind == "stem" and c.cout == co and c.net == s and (c.src is not None) == u8), (co, s, u8)
    for s in FC.FRONT_SHAPES:
        for u8 in (False, True):
            assert _by(lambda c: c.kind == "front" and c.net == s and (c.src is not None) == u8), (s, u8)


def test_every_problem_runs_on_every_grid_cap():
    caps = collections.defaultdict(set)                                                      # per kernel width, tensor and frame size
    for c in FC.CASES:
        caps[(c.kind, c.cout, c.net, c.src and c.src[:2])].add(c.grid)
    for key, got in caps.items():
        assert got == set(FC.caps_of(FC.ntiles(key[0], key[2]))), (key, got)
    # every kernel instance walks the tiles of three frames on 1, 2 and 3 workgroups: a workgroup's prefetched next tile lies in another frame
    # (9 and 6 tiles per frame: a stride of 2 does not divide the stem's, 1 walks through every frame boundary of both)
    for inst in sorted({c.instance for c in FC.CASES}):
        walk = _by(lambda c: c.instance == inst and c.grid in (1, 2, 3) and c.net[0] == 3 and c.units >= 6 * c.grid)
        assert {c.grid for c in walk} == {1, 2, 3}, inst
    assert len({c.name for c in FC.CASES + FC.REFUSALS}) == len(FC.CASES) + len(FC.REFUSALS)
    twins = {c.twin_key() for c in FC.CASES}
    print("%d stem cases, %d front cases, %d launch_conv twins, %d refusals" % (len(FC.STEM_CASES), len(FC.FRONT_CASES), len(twins), len(FC.REFUSALS)))


def test_views_and_e4m3_views():
    for kind, cs in (("stem", None), ("front", 96)):
        dense = _by(lambda c: c.kind == kind and c.out_cs == c.cout and c.out_co == 0)
        sl = _by(lambda c: c.kind == kind and c.out_co == 8 and c.out_cs == (cs or c.cout + 16))
        assert dense and sl
        assert {c.src is None for c in sl} == {True, False}
        assert any(c.units > 1 for c in sl)
    assert all(c.twin_same_store_path for c in FC.CASES)
    q = _by(lambda c: c.q is not None)
    assert {c.cout for c in q} == {32, 64} and all(c.kind == "stem" for c in q)
    assert {c.net for c in q} == {(1, 14, 66), (1, 18, 62)}                                  # the ragged shapes
    for co in (32, 64):
        assert [c for c in q if c.cout == co and c.q[:2] == (co, 0)]                         # dense
        assert {c.q[2] for c in q if c.cout == co and c.q[:2] == (co + 16, 8)} == {1.0, 0.5, 1.0 / 3.0}
        assert {c.src is None for c in q if c.cout == co} == {True, False}
    for c in FC.CASES:
        assert c.out_cs >= c.out_co + c.cout and (c.q is None or c.q[0] >= c.q[1] + c.cout), c.name


def test_every_frame_geometry_selects_its_instance():
    """launch_front_fused's `resize` predicate and front_rs_plan, stem_u8_applicable's geometry part, restated in front_cases"""
    want = {"stem_direct_kernel<%d,%s>" % (ct, u) for ct in (1, 2, 3, 4) for u in ("false", "true")}
    want |= {"stem_direct_wide_kernel<5,false>", "stem_direct_wide_kernel<5,true>", "front_fused_kernel<false>", "front_fused_kernel<true>",
             "front_fused_kernel<true,false,true>"}
    assert {c.instance for c in FC.CASES} == want
    for c in FC.CASES:
        g = c.geom
        if g is None:
            assert c.instance.endswith("false>"), c.name
            continue
        assert (g.unpad_h + g.top + g.bottom, g.unpad_w + g.left + g.right) == c.net[1:], c.name
        same = g.unpad_h == g.src_h and g.unpad_w == g.src_w and g.src_w % 2 == 0 and g.left % 2 == 0
        if c.kind == "stem":
            assert same and c.instance.endswith(",true>"), c.name
        else:
            assert c.instance == ("front_fused_kernel<true>" if same else "front_fused_kernel<true,false,true>"), c.name
            assert same or FC.rs_plan(g) is not None, c.name
    # the frames of the resize instance are what the table says they are
    G = lambda net, hw: FC.Geom(hw[0], hw[1], net[1], net[2])
    checks = {"same scale, odd left pad": lambda g: (g.unpad_h, g.unpad_w) == (g.src_h, g.src_w) and g.left % 2 == 1 and g.src_w % 2 == 0,
              "same scale, odd source width": lambda g: (g.unpad_h, g.unpad_w) == (g.src_h, g.src_w) and g.src_w % 2 == 1,
              "portrait: pads left and right": lambda g: g.src_h > g.src_w and g.left > 0 and g.right > 0 and g.top == 0 and g.unpad_w != g.src_w,
              "2 : 1 down-scale": lambda g: (g.src_h, g.src_w) == (2 * g.unpad_h, 2 * g.unpad_w),
              "4 / 3 up-scale": lambda g: (3 * g.unpad_h, 3 * g.unpad_w) == (4 * g.src_h, 4 * g.src_w) and (g.src_w * 3) % 4 != 0}
    seen = set()
    for net, frames in FC.RESIZE_FRAMES.items():
        for hw, why in frames.items():
            hit = [k for k in checks if why.startswith(k)]
            assert len(hit) == 1 and checks[hit[0]](G(net, hw)), (net, hw, why)
            seen.add(hit[0])
            for b in (1, 3):
                assert _by(lambda c: c.kind == "front" and c.net == (b,) + net[1:] and c.src == hw + (0,)), (net, hw, b)
    assert seen == set(checks)
    # a tile that covers the whole frame, in resize mode
    assert _by(lambda c: c.instance == "front_fused_kernel<true,false,true>" and FC.ntiles("front", (1,) + c.net[1:]) == 1 and c.net[0] == 3)
    # same-scale frames with pad rows above and below and with an even left pad, both channel orders, for every kernel that reads frames
    for kind in ("stem", "front"):
        u = _by(lambda c: c.kind == kind and c.geom is not None and c.geom.same_scale)
        assert [c for c in u if c.geom.top > 0 and c.geom.bottom > 0] and [c for c in u if c.geom.left > 0 and c.geom.left % 2 == 0]
        assert {c.src[2] for c in u if c.geom.top > 0} == {0, 1} and {c.src[2] for c in u if c.geom.left > 0} == {0, 1}
    for co in FC.STEM_COUTS:
        assert _by(lambda c: c.kind == "stem" and c.cout == co and c.src and c.src[2] == 1 and c.geom.top > 0)
    # plan figures of the geometry the tracker's reference runs on, by hand: 1280 x 720 -> 640 x 360 stages 140 rows x 28 chunks
    assert FC.rs_plan(FC.Geom(720, 1280, 384, 640)) == (140, 28)


def test_restated_applicability():
    for c in FC.CASES:
        assert FC.refusal_reasons(c) == [], c.name
    want = {"refused: not a same-scale geometry", "no e4m3 view at 80 channels", "e4m3 view not 8-aligned", "refused: the resize does not fit the staging area",
            "output slice not 8-aligned", "layer 1 is not 32 -> 64"}
    assert {c.reason for c in FC.REFUSALS} == want
    for c in FC.REFUSALS:
        assert FC.refusal_reasons(c) == [c.reason], (c.name, FC.refusal_reasons(c))
    odd = [c.geom for c in FC.REFUSALS if c.kind == "stem" and c.geom is not None]
    assert sorted((g.left % 2, g.src_w % 2) for g in odd) == [(0, 1), (1, 0)]                 # an odd left pad; an odd width
    big = [c for c in FC.REFUSALS if c.kind == "front" and c.geom is not None][0]
    assert FC.rs_plan(big.geom) is None and big.geom.net_h % 4 == 0 and big.geom.net_w % 4 == 0    # the staging limit, nothing else


def test_buffers_carry_the_sentinel():
    for c in FC.CASES + FC.REFUSALS:
        y, q = c.buffers()
        assert (y == SENTINEL).all() and y.shape == (c.net[0],) + c.out_hw + (c.out_cs,), c.name
        assert (q is None) == (c.q is None) and (q is None or (q == FC.Q_SENTINEL).all()), c.name
        assert c.untouched_ok(y, q), c.name
        if c.grid or c.reason:
            continue
        assert c.written(y).shape == (c.npix, c.cout), c.name
        for buf in (y, q):
            if buf is None or buf.shape[3] == c.cout:
                continue
            for ch in (0, buf.shape[3] - 1):
                old = buf[0, 0, 0, ch]
                buf[0, 0, 0, ch] = 1
                assert not c.untouched_ok(y, q), (c.name, ch)
                buf[0, 0, 0, ch] = old
        x = c.input()
        assert x.dtype == (np.float32 if c.src is None else np.uint8) and x.shape[0] == c.net[0]
    x = FC._input((1, 64, 64), None)
    assert (x != SENTINEL).all() and np.isfinite(x).all() and (x < 0).mean() > 0.4 and (x[:, :, 1:] != x[:, :, :-1]).mean() > 0.99
    f = FC._input((1, 64, 64), (64, 64, 0))
    assert len(np.unique(f)) == 256 and (f[..., 0] != f[..., 2]).mean() > 0.99                   # a channel swap moves every pixel


def _problems():
    seen = {}
    for c in FC.CASES:
        seen.setdefault(c.problem(), c)
    return list(seen.values())


def test_half_of_every_reference_is_away_from_zero():
    worst = 1.0
    for c in _problems():
        ref = c.reference()
        assert ref.shape == (c.npix, c.cout) and np.isfinite(ref).all(), c.name
        frac = float((np.abs(ref) > 0.1).mean())
        worst = min(worst, frac)
        assert frac >= 0.5, (c.name, frac)
    print("smallest share of |reference| > 0.1 over %d problems: %.2f" % (len(_problems()), worst))


def test_emulation_inside_the_gate():
    """float32 convolutions with the same roundings against the float64 reference: inside the bf16 gate for every problem"""
    worst = collections.defaultdict(float)
    for c in _problems():
        ref, emu = c.reference(), c.emulation()
        r = FC.gate_ratio(emu, ref)
        assert r < 1.0, (c.name, r)
        np.testing.assert_allclose(emu, FC.rnd(ref.astype(np.float32), "bf16"), err_msg=c.name, **GATE["bf16"])
        worst[FC.kernel_of(c)] = max(worst[FC.kernel_of(c)], r)
    assert set(worst) == {"stem_direct_kernel", "stem_direct_wide_kernel", "front_fused_kernel"}
    for k in sorted(worst):
        print("%-26s emulation worst gate ratio %.3f" % (k, worst[k]))


def test_the_odd_layer0_case_stores_outputs_that_read_the_zero_padding():
    """34 x 70: layer 0 is 17 x 35, so the last output row and column of layer 1 (9 x 18) read row 17 / column 35 of layer 0: the zero padding.
    With that padding replaced by SiLU(bias) -- a halo whose `inside` test is lost -- exactly those outputs (and the first row and column) leave
    the gate; an even-sided tensor has no such output on its bottom and right."""
    for src in (None, (34, 70, 0)):
        ref = FC._reference("front", 64, (1, 34, 70), src)
        wrong = FC.halo_of_bias(64, (1, 34, 70), src).reshape(9, 18, 64)
        refb = FC.rnd(ref.astype(np.float32), "bf16").reshape(9, 18, 64)
        out = np.abs(wrong.astype(np.float64) - refb) > GATE["bf16"]["atol"] + GATE["bf16"]["rtol"] * np.abs(refb)
        assert out[8, 1:17].any(axis=1).all() and out[1:8, 17].any(axis=1).all(), "the bottom row / right column do not feel the padding"
        assert not out[1:8, 1:17].any()
        assert FC.gate_ratio(wrong[8, 1:17], ref.reshape(9, 18, 64)[8, 1:17]) > 4.0 and FC.gate_ratio(wrong[1:8, 17], ref.reshape(9, 18, 64)[1:8, 17]) > 4.0
    ref = FC._reference("front", 64, (1, 32, 96), None)
    wrong = FC.halo_of_bias(64, (1, 32, 96), None).reshape(8, 24, 64)
    refb = FC.rnd(ref.astype(np.float32), "bf16").reshape(8, 24, 64)
    assert np.array_equal(wrong[1:, 1:], refb[1:, 1:]) and not np.array_equal(wrong[0], refb[0])


def test_references_tell_the_planted_value_faults_apart():
    # the e4m3 copy formed from the f32 value instead of the bf16-rounded one: other bytes somewhere, at every inv_scale
    for co in (32, 64):
        x = torch.as_tensor(np.array(FC.tensor_of((1, 14, 66), None))).permute(0, 3, 1, 2)
        w = FC._weights("stem", co)
        f32 = FC._flat(FC.silu(torch.nn.functional.conv2d(x, torch.as_tensor(np.array(w["w0"])), torch.as_tensor(np.array(w["b0"])), stride=2, padding=2)))
        for inv in (1.0, 0.5, 1.0 / 3.0):
            right = FC.q8_reference(FC.rnd(f32, "bf16"), inv)
            wrong = FC.e4m3_bytes(FC.q8(f32 * np.float32(inv)))
            assert (right != wrong).sum() >= 3, (co, inv)
    # swap_rb ignored: the tensor of a swap case without its swap differs in most pixels, same-scale and resized
    for net, src in (((1, 16, 64), (12, 64, 1)), ((1, 64, 64), (56, 64, 1)), ((1, 60, 68), (120, 136, 1))):
        assert _by(lambda c: c.net == net and c.src == src), (net, src)
        frames = np.array(FC._input(net, src))
        unswapped = FC.rnd(np.stack([FC.oi.letterbox(f, net[1], net[2]) for f in frames]).astype(np.float32) / np.float32(255), "bf16")
        g = FC.Geom(src[0], src[1], net[1], net[2])
        inside = (slice(None), slice(g.top, g.top + g.unpad_h), slice(g.left, g.left + g.unpad_w))
        assert (np.abs(unswapped - FC.tensor_of(net, src))[inside][..., (0, 2)] > 0.02).mean() > 0.8, (net, src)
        assert np.array_equal(unswapped[inside][..., 1], FC.tensor_of(net, src)[inside][..., 1])
    # the row alignment term of the resize staging: 153-byte rows put the first pixel of consecutive rows at different offsets in a chunk
    g = FC.Geom(45, 51, 60, 68)
    assert len({(r * g.src_w * 3) % 16 for r in range(g.src_h)}) == 16
