"""CPU: the conditions under which the comparisons of tests/test_gpu_conv_views.py mean something (tests/conv_view_cases.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_view_cases as V
from aux_cases import rnd

ALL = V.CASES + [c for f in V.F2_CASES for c in (f.first, f.second)]


def test_the_sentinel_round_trips_and_is_no_result():
    for precision in ("bf16", "fp8", "f32"):
        assert rnd(np.float32([V.SENTINEL]), precision)[0] == V.SENTINEL
    for c in V.CASES:
        assert not (V.gate_of(c) is not None and (V.gate_of(c)[0] == V.SENTINEL).any()), c.name
        assert not (c.store == "fp8" and (rnd(c.reference().astype(np.float32), "fp8") == V.SENTINEL).any()), c.name


def test_every_reference_is_the_float64_conv_of_the_extracted_slices_and_finite():
    seen = set()
    for c in ALL:
        if c.problem_key() in seen:
            continue
        seen.add(c.problem_key())
        x, xu, res, y, y2 = c.buffers()
        v = c.v
        xs = x[..., v["in_co"]:v["in_co"] + c.cin].copy()
        if v["up_c"]:
            assert np.isnan(xs[..., :v["up_c"]]).all()                 # the replaced channels are poison in the concat buffer
            u = xu[..., v["up_co"]:v["up_co"] + v["up_c"]]
            xs[..., :v["up_c"]] = np.repeat(np.repeat(u, 2, axis=1), 2, axis=2)
        assert np.isfinite(xs).all() and (rnd(xs, c.precision) == xs).all(), c.name
        t = F.conv2d(torch.as_tensor(xs).permute(0, 3, 1, 2).double(), torch.as_tensor(c.weights_used()).double(),
                     torch.tensor(c.operands()["b"]).double(), stride=c.stride, padding=c.pad)
        if c.res_mode:
            r = torch.as_tensor(res[..., v["res_co"]:v["res_co"] + c.cout]).permute(0, 3, 1, 2).double()
            assert torch.isfinite(r).all()
        if c.res_mode == 2:
            t = t + r
        t = F.silu(t) if c.act == 1 else (F.relu(t) if c.act == 2 else t)
        if c.res_mode == 1:
            t = t + r
        ref = c.reference()
        assert ref.dtype == np.float64 and ref.shape == (c.M, c.cout) and np.isfinite(ref).all(), c.name
        np.testing.assert_array_equal(t.permute(0, 2, 3, 1).reshape(-1, c.cout).numpy(), ref, err_msg=c.name)
    for f in V.F2_CASES:
        assert np.isfinite(f.reference()).all() and f.reference().shape == (f.M, 128)


def test_weights_are_what_the_packer_uploads():
    for c in V.CASES:
        w = c.weights_used()
        if c.precision == "bf16":
            assert (rnd(w, "bf16") == w).all()
        elif c.precision == "fp8":
            sw = np.abs(c.operands()["w"]).reshape(c.cout, -1).max(1) / np.float32(448.0)
            q = w / sw[:, None, None, None]
            np.testing.assert_allclose(rnd(q, "fp8"), q, rtol=1e-6)       # e4m3 values times the channel's scale
            assert np.abs(q).max() <= 448.0 * (1 + 1e-6)


def test_everything_outside_the_operands_is_poison_and_every_output_the_sentinel():
    for c in V.CASES + V.REFUSALS:
        x, xu, res, y, y2 = c.buffers()
        bufs, sl = {"x": x, "x_up": xu, "res": res}, c.slices()
        for name, buf in bufs.items():
            if buf is None:
                assert name not in sl
                continue
            operand = np.zeros(buf.shape[-1], bool)
            for lo, hi, what in sl[name]:
                if what != "replaced by the upsampled map":
                    operand[lo:hi] = True
            assert np.isfinite(buf[..., operand]).all() and np.isnan(buf[..., ~operand]).all(), (c.name, name)
            if c.view != "refuse":
                assert (~operand).any(), (c.name, name)                 # there IS a neighbour to leak
        assert (y == V.SENTINEL).all() and (y2 is None or (y2 == V.SENTINEL).all())
        assert (y2 is None) == (c.v["split"] == 0)


def test_slices_lie_inside_their_buffers_and_do_not_overlap():
    for c in ALL:
        strides = c.strides()
        for name, ranges in c.slices().items():
            ranges = sorted(ranges)
            for lo, hi, _ in ranges:
                assert 0 <= lo < hi <= strides[name], (c.name, name)
            for (_, hi, _), (lo, _, _) in zip(ranges, ranges[1:]):
                assert hi <= lo, (c.name, name)
        # the written slice leaves sentinel channels on at least one side, and rows past m_valid exist where the case says so
        _, _, _, y, y2 = c.buffers()
        n_untouched = c.untouched(y, y2).size
        assert n_untouched == y.size + (0 if y2 is None else y2.size) - c.rows * c.cout
        if c in V.CASES:
            assert n_untouched > 0, c.name


def test_written_and_untouched_partition_the_outputs():
    c = V.BY_NAME["split4/bf16-h1b_68"]
    _, _, _, y, y2 = c.buffers()
    y = np.arange(y.size, dtype=np.float32).reshape(y.shape)
    y2 = -np.arange(1, y2.size + 1, dtype=np.float32).reshape(y2.shape)
    w, u = c.written(y, y2), c.untouched(y, y2)
    assert w.shape == (c.M, 130) and len(set(w.ravel()) | set(u.ravel())) == y.size + y2.size and not set(w.ravel()) & set(u.ravel())
    assert (w[:, :68] >= 0).all() and (w[:, 68:] < 0).all()
    assert w[1, 0] == y.reshape(c.M, -1)[1, c.v["out_co"]] and w[1, 68] == y2.reshape(c.M, -1)[1, c.v["out2_co"]]
    m = V.BY_NAME["m_dev/bf16-m65"]
    _, _, _, y, _ = m.buffers()
    assert m.rows == 65 and m.untouched(y, None).size == y.size - 65 * 72
    assert V.BY_NAME["m_dev/bf16-m5000"].rows == 300 and V.BY_NAME["m_dev/f32-m0"].rows == 0


def test_the_dense_twin_has_the_same_operands():
    for c in V.CASES:
        x, xu, res, _, _ = c.buffers()
        v, d = c.v, c.x_dense()
        assert d.shape == c.shape + (c.cin,) and np.isfinite(d).all()
        np.testing.assert_array_equal(d[..., v["up_c"]:], x[..., v["in_co"] + v["up_c"]:v["in_co"] + c.cin])
        if v["up_c"]:
            np.testing.assert_array_equal(d[:, ::2, ::2, :v["up_c"]], xu[..., v["up_co"]:v["up_co"] + v["up_c"]])
            np.testing.assert_array_equal(d[:, 1::2, 1::2, :v["up_c"]], xu[..., v["up_co"]:v["up_co"] + v["up_c"]])
        if c.res_mode:
            np.testing.assert_array_equal(c.operands()["res"], res[..., v["res_co"]:v["res_co"] + c.cout])
    # cases of one problem share their operands whatever the view
    a, b = V.BY_NAME["slices8/bf16-gpw"], V.BY_NAME["split8/bf16-gpw_40"]
    assert a.problem_key() == b.problem_key() and a.operands() is b.operands()


def test_check_c_applies_where_the_store_paths_agree():
    for c in V.CASES:
        if c.precision in ("f32", "fp8"):
            assert c.twin_same_store_path == (not c.v["out_bf16"]), c.name
    assert V.BY_NAME["slices8/bf16-gpw"].twin_same_store_path and V.BY_NAME["split8/bf16-gpw_40"].twin_same_store_path
    assert not V.BY_NAME["slices4/bf16-gpw"].twin_same_store_path and not V.BY_NAME["split4/bf16-gpw_36"].twin_same_store_path
    assert V.BY_NAME["slices4/bf16-h1b"].twin_same_store_path            # 130 outputs: the dense launch takes the general loop too
    assert not V.BY_NAME["out_f32/bf16-pw72_0"].twin_same_store_path
    # the general loop with a second destination runs: split not a multiple of 8, a ragged tail in out2, and the f32 store
    assert not V.BY_NAME["split4/bf16-h1b_68"].fast_store() and (130 - 68) % 4 == 2
    assert not V.BY_NAME["out_f32/bf16-pw255_128"].fast_store() and V.BY_NAME["out_f32/bf16-pw255_128"].v["split"] == 128


def test_every_row_lists_every_id_once_and_is_what_the_launchers_take():
    assert set(V.EXPECT) == set(V.ROWS)
    for row in V.ROWS:
        assert sorted(V.EXPECT[row]) == list(range(V.NIDS)), row
        assert set(V.EXPECT[row].values()) <= {V.RUNS, V.REFUSES}
        got = V.derive_row(row)                                          # raises where two cases of one id disagree or an id has none
        assert got == "".join("r" if V.EXPECT[row][i] == V.RUNS else "x" for i in range(V.NIDS)), row
    for c in V.CASES:
        assert V.conv_check_admits(c), c.name
    for c in V.REFUSALS:
        assert not V.conv_check_admits(c), c.name
    assert len({c.tag for c in V.REFUSALS}) == 11 and all(c.message.startswith("conv") for c in V.REFUSALS)


def test_the_rows_the_issue_fixes_in_words():
    families = set(V.IGEMM) | set(V.SPLITK) | set(V.HALO) | V.HALO_V2 | set(V.HALO_S2) | set(V.DIRECT) | set(V.STREAM) | set(V.DIRECT8)
    assert families == set(range(V.NIDS))
    # up: exactly the UP_OK instantiations
    assert {i for i, e in V.EXPECT["up/bf16"].items() if e == V.RUNS} == set(V.UP_OK)
    for i, (BP, BC, WP, WC, KC, NS, OCC) in V.IGEMM.items():
        up_ok = OCC == 1 and ((BP == 256 and BC == 256 and KC == 4 and NS <= 4) or
                              (WP == 2 and WC == 2 and BC == 128 and BP in (128, 256) and (KC == 8 or (KC == 4 and NS == 2 and BP == 128))))
        assert up_ok == (i in V.UP_OK), i
    # m_dev: the implicit GEMM without split-K, nothing else
    for row in ("m_dev/bf16", "m_dev/f32"):
        runs = {i for i, e in V.EXPECT[row].items() if e == V.RUNS}
        assert runs <= set(V.IGEMM) and not runs & set(V.SPLITK)
    assert {i for i, e in V.EXPECT["m_dev/bf16"].items() if e == V.RUNS} == set(V.IGEMM)
    # the heuristic's tiles run every case conv_check admits: the tile conv_heuristic picks always, ids 0 - 3 every bf16 / f32 case but
    # the upsample fold-in (conv_heuristic sends that to 2, the one of the four that is instantiated for it), ids 4 - 6 every fp8 case
    for c in V.CASES:
        assert V.accepts(c, V.heuristic(c)), c.name
        for i in ((4, 5, 6) if c.precision == "fp8" else (0, 1, 2, 3)):
            if not (c.v["up_c"] and i != 2):
                assert V.accepts(c, i), (c.name, i)
    # every family runs under the 8-aligned slices, and every view has an id that runs and one that refuses
    assert all(V.EXPECT["slices8/bf16"][i] == V.RUNS for i in range(69))
    for row in V.ROWS:
        assert {V.RUNS, V.REFUSES} == set(V.EXPECT[row].values()), row


def test_the_device_side_count_alone_decides_the_refusals_of_the_other_families():
    """every family but the implicit GEMM has an m_dev case it would TAKE without the count (so a launcher that forgot to refuse it runs,
    writes the rows past the count and fails the GPU test), and 0 < m_valid < M there"""
    import copy
    took = set()
    for c in V.cases_of("m_dev/bf16") + V.cases_of("m_dev/fp8"):
        plain = copy.copy(c)
        plain.v = dict(c.v, m_valid=-1)
        for cfg in c.ids:
            if cfg not in V.IGEMM and V.accepts(plain, cfg):
                assert not V.accepts(c, cfg) and 0 < c.v["m_valid"] < c.M, (c.name, cfg)
                took.add(cfg)
    assert took == set(V.SPLITK) | set(V.HALO) | V.HALO_V2 | set(V.HALO_S2) | set(V.DIRECT) | set(V.STREAM) | {69, 71, 72}
    # the general loop with a second destination and the f32 store also run behind the split-K reduction
    for row in ("split4/bf16", "out_f32/bf16", "split8/bf16", "slices4/bf16"):
        assert all(V.EXPECT[row][i] == V.RUNS for i in V.SPLITK), row
    assert any(c.v["split"] for c in V.cases_of("out_f32/bf16", 56))


def test_split_k_cases_do_not_depend_on_the_chip():
    """launch_one_sk: ks = min(resident workgroups / tiles, K tiles / 4, 8); the first term is at least 256 / tiles on any chip this runs on"""
    for c in V.CASES:
        for cfg in c.ids:
            if cfg in V.SPLITK and V.accepts(c, cfg):
                BP, BC, WP, WC, KC, NS = V.SPLITK[cfg]
                tiles = ((c.M + BP - 1) // BP) * ((c.cout + BC - 1) // BC)
                nk = V.round_up(c.k * c.k * c.cin, KC * 8) // (KC * 8)
                assert V.SK_SLOTS_MIN // tiles >= min(nk // 4, 8), (c.name, cfg)


def test_the_cases_are_small_and_cover_the_shapes_the_issue_names():
    for c in V.CASES:
        assert c.M < 1200 and c.cout <= 256, c.name
    assert {c.v["m_valid"] for c in V.cases_of("m_dev/bf16") if c.shape == (1, 1, 300)} == {0, 1, 64, 65, 299, 300, 5000}
    ups = V.cases_of("up/bf16")
    assert {c.shape for c in ups} == {(3, 10, 14), (2, 6, 10)} and {(c.cin, c.v["up_c"]) for c in ups} == {(128, 64), (192, 128)}
    assert {c.cout for c in ups} == {72, 256} and {c.v["split"] for c in ups} == {0, 40}
    assert all(c.v["up_co"] == 8 and c.v["up_cs"] == c.v["up_c"] + 16 and c.v["in_co"] == 64 for c in ups)
    assert {(c.cout, c.v["split"]) for c in V.cases_of("split8/bf16") if c.cout == 72} == {(72, 40), (72, 64)}
    assert {(c.cout, c.v["split"]) for c in V.cases_of("split4/bf16")} == {(72, 36), (130, 68), (256, 132)}       # (256, 132): the split-K problem
    assert {(c.cout, c.v["split"]) for c in V.cases_of("out_f32/bf16")} == {(255, 0), (72, 0), (255, 128), (256, 0), (256, 128)}   # 256: the split-K problem
    for c in V.cases_of("slices8/bf16"):
        assert (c.v["in_co"], c.v["in_cs"], c.v["out_co"], c.v["out_cs"]) == (16, c.cin + 24, 8, V.round_up(c.cout, 8) + 24), c.name
        assert not c.res_mode or (c.v["res_co"], c.v["res_cs"]) == (8, V.round_up(c.cout, 8) + 16)
    assert {c.res_mode for c in V.cases_of("slices8/bf16")} == {0, 1, 2}
    for c in V.cases_of("slices4/bf16") + V.cases_of("slices4/f32"):
        assert (c.v["out_co"], c.v["out_cs"]) == (4, V.round_up(c.cout, 4) + 12) and (not c.res_mode or c.v["res_co"] == 4), c.name
    assert all(c.v["in_co"] == 4 for c in V.cases_of("slices4/f32"))
    assert all(c.v["in_co"] % 16 == 0 and c.v["in_co"] > 0 for c in V.cases_of("slices8/fp8"))
    assert len(V.F2_CASES) == 6


# (narrow and deep: every rectangle of full area has parity classes past the patch buffer -- 4 columns x 32 rows is 165 of 159, 5 columns fit)
@pytest.mark.parametrize("G,Wo,bp,ok", [(20, 3, 256, True), (20, 3, 128, True), (60, 12, 128, True), (1, 1, 128, True), (200, 4, 128, False),
                                        (200, 5, 128, True), (300, 4, 256, False), (300, 5, 256, True), (78, 1, 128, True), (79, 1, 128, False)])
def test_s2halo_geom_restated(G, Wo, bp, ok):
    assert V.s2halo_geom(G, Wo, bp) == ok
