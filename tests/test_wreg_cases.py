"""CPU: tests/wreg_cases.py against its own conditions -- the operands are bf16-representable, the float64 references agree with an
independent evaluation, the cases cover what they say they cover, and conv_pointwise.hip::wreg_applicable restated in Python accepts
every case that runs and refuses every refusal."""
import re
from pathlib import Path

import numpy as np

import conv_view_cases as V
import wreg_cases as W
from aux_cases import rnd

CSRC = Path(__file__).resolve().parents[1] / "vehicle-counting_amd" / "csrc"


def test_the_table_is_the_header_s():
    text = (CSRC / "conv_cfgs.h").read_text()
    line = next(l for l in text.splitlines() if l.startswith("#define VC_WREG_CFGS"))
    got = {int(a): (int(b), int(c), int(d), int(e)) for a, b, c, d, e in re.findall(r"W\((\d+), (\d+), (\d+), (\d+), (\d+)\)", line)}
    assert got == W.WREG
    assert W.IDS == tuple(range(V.NIDS, V.NIDS + len(W.WREG)))           # appended: no earlier id changed
    for cfg in W.IDS:
        cin, cout, bp, lds = W.shape_of(cfg)
        assert cin in (128, 256) and cout in (128, 256) and lds <= 64 * 1024 and bp % 32 == 0
    assert {W.shape_of(c)[:2] for c in W.IDS} == {(128, 128), (128, 256), (256, 128), (256, 256)}


def test_operands_are_bf16_and_references_agree():
    seen = set()
    for run in W.RUNS:
        c = run.case
        if c.problem_key() in seen:
            continue
        seen.add(c.problem_key())
        o = c.operands()
        np.testing.assert_array_equal(o["x"], rnd(o["x"], "bf16"))
        np.testing.assert_array_equal(c.weights_used(), rnd(c.weights_used(), "bf16"))
        np.testing.assert_allclose(c.reference(), W.reference64(c), rtol=1e-12, atol=1e-12)
        assert np.isfinite(c.reference()).all()


def test_buffers_poison_everything_but_the_operands():
    for run in W.RUNS:
        c = run.case
        x, xu, res, y, y2 = c.buffers()
        v = c.v
        assert xu is None and res is None
        assert v["in_co"] == 8 and np.isnan(x[..., :8]).all() and np.isnan(x[..., 8 + c.cin:]).all() and x.shape[-1] > 8 + c.cin
        np.testing.assert_array_equal(x[..., 8:8 + c.cin], c.operands()["x"])
        assert (y == V.SENTINEL).all() and (y2 is None) == (v["split"] == 0)
        if v["split"]:
            assert (y2 == V.SENTINEL).all() and v["out2_cs"] != v["out_cs"] and v["split"] == c.cout // 2


def test_every_id_walks_every_shape():
    for cfg in W.IDS:
        cin, cout, bp, _ = W.shape_of(cfg)
        runs = [r for r in W.RUNS if r.cfg == cfg]
        assert all((r.case.cin, r.case.cout) == (cin, cout) for r in runs)
        assert {(r.case.M, r.slots) for r in runs} >= {(1, 0), (bp - 1, 0), (bp, 0), (2 * bp + 17, 0), (5 * bp, 1), (5 * bp, 2), (7 * bp, 3)}
        assert {r.case.act for r in runs} == {0, 1, 2}
        assert any(r.case.v["split"] for r in runs) and any(r.case.v["split"] and r.slots for r in runs)


def test_applicability():
    for run in W.RUNS:
        assert V.conv_check_admits(run.case), run.name
        assert W.wreg_applicable(run.case, run.cfg), run.name
        for other in W.IDS:                                               # another width's id refuses it
            if W.shape_of(other)[:2] != W.shape_of(run.cfg)[:2]:
                assert not W.wreg_applicable(run.case, other), (run.name, other)
    assert {why for _, _, why in W.REFUSALS} == {"device-side pixel count", "upsample fold-in", "f32 store", "K = 512", "Cout = 64", "residual"}
    for cfg, case, why in W.REFUSALS:
        assert V.conv_check_admits(case), why                            # launch_conv gets as far as the family
        assert not W.wreg_applicable(case, cfg), why
