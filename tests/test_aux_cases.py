"""CPU: what tests/test_gpu_aux_kernels.py relies on (tests/aux_cases.py) -- the SPPF reference equals the model's chained form on every
case shape, the case tables contain the inputs that make a wrong kernel fail and reach every launcher branch, and the order-preserving
keys of the pool kernels (vehicle-counting_amd/csrc/sppf_keys.h compiled for the host, tests/native/sppf_keys_host.cpp) are checked
exhaustively: all 65536 bf16 halves and all 256 fp8 bytes, NaNs excluded; f32 on its edge values and a seeded million of bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aux_cases as A

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- references and tables ----------------------------------------------------------------------------------------------------
def test_sppf_reference_equals_the_chained_form_on_every_case_shape():
    shapes = sorted({(c.shape, c.precision) for c in A.sppf_cases().values()})
    assert len(shapes) == 15 * 3 + 1                                           # (1, 5, 6) is fp8 only
    for shape, precision in shapes:
        x = A.plane_values(np.random.default_rng(len(shapes)), (*shape, 4), precision)
        direct = np.concatenate([A.window_max(x, r) for r in (2, 4, 6)], axis=-1)
        np.testing.assert_array_equal(direct, A.sppf_chained(x), err_msg=str(shape))
    x = np.random.default_rng(1).standard_normal((1, 70, 70, 1)).astype(np.float32)
    for n in (1, 2, 3, 5, 6, 7, 12, 13, 14, 27, 70):
        np.testing.assert_array_equal(np.concatenate([A.window_max(x[:, :n, :n], r) for r in (2, 4, 6)], axis=-1), A.sppf_chained(x[:, :n, :n]))


def test_sppf_rule_anchors():
    """the restated steering rule against values read off launch_sppf_pool by hand"""
    for C, ws in ((64, 32), (32, 16), (16, 8), (8, 4), (128, 32)):
        assert A.sppf_rule(20, 20, C, "bf16", 1) == ("sep", ws)
    assert A.sppf_rule(40, 40, 256, "bf16", 1) == ("sep", 8)              # the detector's own: 20 x 20 -> 32, 40 x 40 -> 8
    assert A.sppf_rule(20, 20, 256, "f32", 1) == ("sep", 32) and A.sppf_rule(21, 9, 64, "bf16", 1) == ("sep", 8)
    assert A.sppf_rule(41, 17, 64, "bf16", 1) == A.sppf_rule(41, 17, 64, "bf16", 0) == ("wide", 8)      # 2 * 697 * 4 * 16 > 76 KB
    assert A.sppf_rule(20, 20, 256, "bf16", 0) == ("wide", 16) and A.sppf_rule(60, 70, 8, "bf16", 0) == ("wide", 4)
    assert A.sppf_rule(69, 69, 8, "f32", 1) == ("wide", 4) and A.sppf_rule(70, 70, 8, "f32", 1) == ("plain", 4)      # 4800 positions is the edge
    assert A.sppf_rule(5, 6, 8, "fp8", 1) == ("fp8", 1) and A.sppf_rule(70, 70, 16, "fp8", 0) == ("fp8", 1)
    assert A.sppf_rule(20, 20, 12, "bf16", 1) is None and A.sppf_rule(20, 20, 12, "bf16", 0) is None


def test_sppf_wide_slices_above_64_bytes_never_won():
    """launch_sppf_pool used to offer the LDS form 32 / 16 / 8 / 4 words under 150 KB after 16 / 8 / 4 under 76 KB; the second list could
    only ever yield 4, which is what the launcher (and sppf_rule) now says.  The two rules agree on every plane up to 80 x 80."""
    def two_lists(H, W, C, es):
        plane = 2 * H * W * 4
        for cap, cands in ((76 * 1024, (16, 8, 4)), (150 * 1024, (32, 16, 8, 4))):
            for cand in cands:
                if plane * cand <= cap and C % (cand * 4 // es) == 0:
                    return "wide", cand
        return None
    for p in A.PRECISIONS:
        for H in list(range(1, 81, 3)) + [69, 70, 80]:
            for W in (1, 7, 20, 40, 41, 60, 69, 70, 80):
                for C in range(4, 260, 4):
                    want, got = two_lists(H, W, C, A.ES[p]), A.sppf_rule(H, W, C, p, 0)
                    assert got == want or (want is None and got is not None and got[0] != "wide"), (p, H, W, C)


def test_sppf_table_reaches_every_branch_and_width():
    cases = A.sppf_cases().values()
    got = lambda **kw: {c.expect for c in cases if all(getattr(c, k) == v for k, v in kw.items())}
    assert all(c.expect is not None for c in cases)
    for p in A.PRECISIONS:
        table = [c for c in cases if c.precision == p and c.form == 1 and c.shape in A.SPPF_SHAPES]
        side20 = {c.expect for c in table if max(c.shape[1:]) <= 20}
        side40 = {c.expect for c in table if max(c.shape[1:]) > 20}
        assert side20 == {("sep", ws) for ws in (32, 16, 8, 4)} and side40 == {("sep", 8), ("sep", 4)}
        assert got(precision=p, form=0) == {("wide", ws) for ws in (16, 8, 4)}           # every instance of the LDS form
        assert got(precision=p, shape=(1, 41, 17)) <= {("wide", ws) for ws in (32, 16, 8, 4)}
        c = A.sppf_cases()["1x60x70-%s-c%d-form0" % (p, 16 // A.ES[p])]
        assert c.expect == ("wide", 4) and 2 * 60 * 70 * 4 * 4 > 64 * 1024
        # B > 1 with more than one channel group, for the blockIdx decomposition
        assert any(c.shape[0] > 1 and c.C // (c.expect[1] * 4 // A.ES[p]) > 1 for c in cases if c.precision == p and c.expect[0] == "sep")
        assert any(c.shape[0] > 1 and c.C // (c.expect[1] * 4 // A.ES[p]) > 1 for c in cases if c.precision == p and c.expect[0] == "wide")
    assert got(shape=(1, 70, 70), precision="f32") == got(shape=(1, 70, 70), precision="bf16") == {("plain", 4)}
    assert got(shape=(1, 70, 70), precision="fp8") == got(shape=(1, 5, 6), C=8) == {("fp8", 1)}
    assert {c.shape for c in cases if c.form == 1 and c.expect[0] == "sep"} == set(A.SPPF_SHAPES)
    assert {c.shape for c in cases if c.form == 0} >= set(A.SPPF_SHAPES)


@pytest.mark.parametrize("precision", A.PRECISIONS)
def test_sppf_inputs_hold_what_they_were_built_for(precision):
    sub, big = np.float32(A.SUB[precision]), np.float32(A.BIG[precision])
    assert sub > 0 and np.isfinite(big) and A.rnd([sub, big, A.SENTINEL], precision).tolist() == [sub, big, A.SENTINEL]
    assert A.rnd([sub / 2], precision)[0] == 0 and (precision == "fp8" or np.isinf(A.rnd([np.float64(big) * 1.01], precision)[0]))
    seen = set()
    for c in A.sppf_cases().values():
        if c.precision != precision:
            continue
        x, buf = c.x(), c.buffer()
        assert x.dtype == np.float32 and np.isfinite(x).all() and np.array_equal(A.rnd(x, precision), x)          # representable, finite
        assert not (x == A.SENTINEL).any()
        assert c.cs > c.co + 4 * c.C and c.co > 0 and c.cs % 16 == 0 and c.co % 16 == 0
        assert (buf[..., :c.co] == A.SENTINEL).all() and (buf[..., c.co + c.C:] == A.SENTINEL).all()
        assert (x[..., 0::4] < 0).all()                                    # all-negative planes: a zero pad would win
        ref = A.sppf_ref(c.name)
        assert (ref[..., 0::4] < 0).all() and ref.shape == (*c.shape, 3 * c.C)
        if x[..., 0].size >= 30:
            assert (x[..., 3::4] > 0).any() and (x[..., 3::4] < 0).any()  # mixed signs
            v = x[..., 1::4]
            for name, s in (("+0", (v == 0) & ~np.signbit(v)), ("-0", (v == 0) & np.signbit(v)), ("+sub", v == sub), ("-sub", v == -sub),
                            ("+big", v == big), ("-big", v == -big)):
                assert s.any(), (c.name, name)
                seen.add(name)
    assert len(seen) == 6


def test_other_tables():
    for p in A.PRECISIONS:
        for shape in A.UPSAMPLE_SHAPES:
            x = A.upsample_input(shape, p)
            assert np.array_equal(A.rnd(x, p), x) and A.upsample_ref(x).shape == (shape[0], 2 * shape[1], 2 * shape[2], A.UPSAMPLE_C)
    assert A.UPSAMPLE_CO > 0 and A.UPSAMPLE_CS > A.UPSAMPLE_CO + A.UPSAMPLE_C and A.MAXPOOL_CO > 0 and A.MAXPOOL_CS > A.MAXPOOL_CO + A.MAXPOOL_C
    r = A.upsample_ref(np.arange(6, dtype=np.float32).reshape(1, 2, 3, 1))[0, :, :, 0]
    assert r.tolist() == [[0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 2, 2], [3, 3, 4, 4, 5, 5], [3, 3, 4, 4, 5, 5]]
    assert {s[1:] for s in A.MAXPOOL_SHAPES} == {(50, 50), (25, 25), (6, 7), (2, 2), (1, 1)}
    for shape in A.MAXPOOL_SHAPES:
        for p in ("f32", "bf16"):
            x = A.maxpool_input(shape, p)
            assert (x[..., 0] < 0).all() and np.array_equal(A.rnd(x, p), x)
            assert A.maxpool_ref(x).shape == (shape[0], (shape[1] - 1) // 2 + 1, (shape[2] - 1) // 2 + 1, A.MAXPOOL_C)
    for shape in A.LAYOUT_SHAPES:
        x = A.layout_input(shape)
        assert not np.array_equal(A.rnd(x, "bf16"), x)
        b = A.layout_ref(x, "bf16")
        assert b.shape[-1] == 8 and (b[..., 3:] == 0).all() and (A.layout_ref(x, "f32")[..., 3:] == 0).all()
        assert b.reshape(-1, 8)[4, 0] == 1.0 and b.reshape(-1, 8)[5, 0] == np.float32(1 + 2.0 ** -6)      # ties go to the even neighbour
    assert sorted(k for k, _, _ in A.AVGPOOL_CASES) == [1, 2, 5] and A.REID_STEM_K == (1, 3, 60) and 60 * 13 > 704 >= 54 * 13


def test_fp8_cast_inputs_and_reference():
    v = A.all_bf16_values()
    assert v.shape[1] == A.FP8_C and v.size >= 65536 - 254 and not np.isnan(v).any()
    assert len(np.unique(v.view(np.uint32))) == 65536 - 254                  # every non-NaN pattern (the zero padding repeats +0)
    assert np.isinf(v).sum() == 2 and np.array_equal(A.rnd(v, "bf16").view(np.uint32), v.view(np.uint32))
    for s in (A.FP8_SRC_CS, A.FP8_SRC_CO, A.FP8_DST_CS, A.FP8_DST_CO, A.FP8_C):
        assert s % 8 == 0
    assert A.FP8_SRC_CS > A.FP8_SRC_CO + A.FP8_C and A.FP8_DST_CS > A.FP8_DST_CO + A.FP8_C
    # the reference on hand-computed points: saturation, infinities, ties to even, subnormals (steps of 2^-9), underflow to zero
    x = np.array([448, 1e30, np.inf, -np.inf, 464, 1.0625, 1.1875, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 2.0 ** -10, 1.01 * 2.0 ** -10, -0.0], np.float32)
    want = [448, 448, 448, -448, 448, 1.0, 1.25, 2.0 ** -9, 2.0 ** -8, 2.0 ** -8, 0.0, 2.0 ** -9, 0.0]
    assert A.fp8_cast_ref(x, 1.0).tolist() == want
    assert A.fp8_cast_ref(np.array([896, 3.0], np.float32), 0.5).tolist() == [448, 1.5]
    assert A.e4m3_values(np.array([0x7e, 0xfe, 0x01, 0x80, 0x38], np.uint8)).tolist() == [448, -448, 2.0 ** -9, 0.0, 1.0]


def test_avgpool_bound_is_tighter_than_the_network_gate():
    for case in A.AVGPOOL_CASES:
        for p in ("f32", "bf16"):
            x = A.avgpool_input(case, p)
            assert np.array_equal(A.rnd(x, p), x) and (np.abs(x).reshape(len(x), -1).max(1) > 0).all()
            b = A.avgpool_bound(x)
            assert b.shape == (case[0], 512) and 0 < b.max() < 2e-5, b.max()
            np.testing.assert_allclose(np.linalg.norm(A.avgpool_ref(x), axis=1), 1.0, rtol=1e-12)
    x = A.avgpool_input((5, 4, 4), "f32").astype(np.float64)
    ratio = np.abs(x).mean(axis=(1, 2)).mean(1) / np.abs(x.mean(axis=(1, 2))).mean(1)
    assert ratio[1] > 10 > ratio[0] and 500 < np.abs(x[2]).mean() < 1500 and 5e-4 < np.abs(x[3]).mean() < 1.5e-3


# ---- the keys -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("skh") / "libskh.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "native", "sppf_keys_host.cpp")], check=True)
    lib = C.CDLL(so)
    pu = C.POINTER(C.c_uint32)

    def call(fn, et, *arrays):
        arrays = [np.ascontiguousarray(a, dtype=np.uint32) for a in arrays]
        out = np.zeros_like(arrays[0])
        args = ([et] if et is not None else []) + [a.ctypes.data_as(pu) for a in arrays] + [out.ctypes.data_as(pu), C.c_long(out.size)]
        getattr(lib, fn)(*args)
        return out

    class K:
        key = staticmethod(lambda et, v: call("skh_key", et, v))
        unkey = staticmethod(lambda et, k: call("skh_unkey", et, k))
        max = staticmethod(lambda et, a, b: call("skh_max", et, a, b))
        umax4 = staticmethod(lambda a, b: call("skh_umax4", None, a, b))
    return K


def _ordered(values, bits, keys):
    """key order equals value order with -0 below +0; key 0 below every key; keys distinct"""
    order = np.lexsort((~np.signbit(values), values))                       # by value, -0 before +0
    k = keys[order].astype(np.int64)
    assert (np.diff(k) > 0).all() and k[0] > 0


def test_bf16_keys_exhaustive(skh):
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7fff) <= 0x7f80]                                   # NaNs excluded, infinities kept
    values = (bits << 16).view(np.float32)
    other = np.uint32(0x3f80)
    lo = skh.key(1, bits | (other << 16)) & 0xffff                           # the half under test in the low half ...
    hi = skh.key(1, (bits << 16) | other) >> 16                              # ... and in the high half
    assert np.array_equal(lo, hi)
    _ordered(values, bits, lo)
    # the halves are independent: the other half's key does not depend on this one, whatever its sign
    for o in (0x3f80, 0xbf80, 0x0000, 0x8000, 0x7f7f, 0xff7f):
        k = skh.key(1, bits | np.uint32(o << 16))
        assert len(np.unique(k >> 16)) == 1 and np.array_equal(k & 0xffff, lo)
        assert np.array_equal(skh.unkey(1, k), bits | np.uint32(o << 16))   # the round trip is the identity
        k2 = skh.key(1, (bits << 16) | np.uint32(o))
        assert len(np.unique(k2 & 0xffff)) == 1 and np.array_equal(k2 >> 16, lo)
        assert np.array_equal(skh.unkey(1, k2), (bits << 16) | np.uint32(o))
    # per-half max: each half against a shuffled partner, the two halves with different winners
    rng = np.random.default_rng(5)
    a, b, c, d = (rng.permutation(lo) for _ in range(4))
    m = skh.max(1, a | (b << 16), c | (d << 16))
    assert np.array_equal(m & 0xffff, np.maximum(a, c)) and np.array_equal(m >> 16, np.maximum(b, d))
    assert np.array_equal(skh.max(1, a | (b << 16), np.zeros_like(a)), a | (b << 16))       # key 0 never wins


def test_fp8_keys_exhaustive(skh):
    bits = np.arange(256, dtype=np.uint32)
    bits = bits[(bits & 0x7f) != 0x7f]                                        # e4m3fn NaNs excluded (no infinities in the format)
    values = A.e4m3_values(bits.astype(np.uint8))
    assert np.isfinite(values).all() and values.max() == 448
    base = None
    for lane in range(4):
        for o in (0x38, 0xb8, 0x00, 0x80, 0x7e, 0xfe):
            word = np.uint32(o * 0x01010101) & ~np.uint32(0xff << (8 * lane)) | (bits << (8 * lane))
            k = skh.key(2, word)
            mine = (k >> (8 * lane)) & 0xff
            base = mine if base is None else base
            assert np.array_equal(mine, base)                                 # the same key in every byte, whatever the neighbours hold
            rest = k & ~np.uint32(0xff << (8 * lane))
            assert len(np.unique(rest)) == 1                                  # the neighbours' keys do not depend on this byte
            assert np.array_equal(skh.unkey(2, k), word)
    _ordered(values, bits, base)
    rng = np.random.default_rng(6)
    q = [rng.permutation(np.resize(base, 1024)) for _ in range(8)]
    a = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24)
    b = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24)
    want = np.maximum(q[0], q[4]) | (np.maximum(q[1], q[5]) << 8) | (np.maximum(q[2], q[6]) << 16) | (np.maximum(q[3], q[7]) << 24)
    assert np.array_equal(skh.max(2, a, b), want) and np.array_equal(skh.umax4(a, b), want)
    assert np.array_equal(skh.max(2, a, np.zeros_like(a)), a) and np.array_equal(skh.umax4(np.zeros_like(a), a), a)


def test_f32_keys_on_edges_and_a_seeded_million(skh):
    edges = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)),
                      np.finfo(np.float32).max, -np.finfo(np.float32).max, np.inf, -np.inf], np.float32)
    rng = np.random.default_rng(7)
    bits = np.concatenate([edges.view(np.uint32), rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32)])
    bits = np.unique(bits[(bits & 0x7fffffff) <= 0x7f800000])
    values = bits.view(np.float32)
    k = skh.key(0, bits)
    _ordered(values, bits, k)
    assert np.array_equal(skh.unkey(0, k), bits)
    p = rng.permutation(k)
    assert np.array_equal(skh.max(0, k, p), np.maximum(k, p)) and np.array_equal(skh.max(0, k, np.zeros_like(k)), k)
