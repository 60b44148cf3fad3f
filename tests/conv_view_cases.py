"""Cases, buffers, float64 references and the acceptance table for the launch VIEWS of a convolution (ConvP, csrc/vc_common.h): channel slices
of wider buffers on the input, the output and the residual, the split store into two destinations, the f32 store of bf16 arithmetic,
the bf16 store of fp8 arithmetic, a pixel count that lives on the device, and Upsample + Concat folded into the pointwise conv that reads
them.  tests/test_gpu_conv_views.py launches every case under every tile configuration through vc_conv2d_view_host;
tests/test_conv_view_cases.py holds this module to its own conditions on the CPU.

Poison: every element of x, x_up and res that is not an operand is NaN (the channels around a slice and, under `up`, channels
[in_co, in_co + up_c) of the concat buffer, which the kernel replaces by the upsampled map).  A fetched neighbour multiplied by a
zero-padded weight gives NaN, not the right answer.  y and y2 start as SENTINEL everywhere.

A row of EXPECT is (view, precision); a case of that row belongs to the ids of ONE kernel family (its `ids`), so every (row, id) has
its cases and one expectation.  `accepts` restates the launchers' applicability functions (conv_igemm.hip::launch_one / launch_one_sk,
conv_device.h::halo_applicable, conv_halo_v2.hip::v2_applicable, conv_halo_s2.hip::s2halo_applicable, conv_pointwise.hip::*_applicable)
with every A/B switch at its default; EXPECT is that function written out, and the CPU test holds the two together."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from aux_cases import SENTINEL, rnd, upsample_ref

NIDS = 73
CH = {"bf16": 8, "f32": 4, "fp8": 16}          # input channels per 16-byte chunk

# ---- the tile table (conv_cfgs.h) -----------------------------------------------------------------------------------------------
# implicit GEMM: id -> (BP, BC, WP, WC, KC, NS, OCC)
IGEMM = {0: (256, 32, 4, 1, 4, 2), 1: (128, 64, 2, 2, 4, 2), 2: (128, 128, 2, 2, 4, 2), 3: (64, 64, 2, 2, 4, 2), 4: (128, 64, 2, 2, 8, 2),
         5: (128, 128, 2, 2, 8, 2), 6: (64, 64, 2, 2, 8, 2), 7: (256, 64, 4, 1, 4, 2), 8: (256, 64, 4, 1, 8, 2), 9: (256, 128, 2, 2, 4, 2),
         10: (256, 128, 2, 2, 8, 2), 11: (64, 128, 1, 4, 4, 2), 12: (64, 128, 1, 4, 8, 2), 13: (256, 32, 4, 1, 8, 2), 14: (64, 64, 2, 2, 4, 4),
         15: (64, 64, 2, 2, 8, 3), 16: (64, 64, 2, 2, 8, 4), 17: (128, 64, 2, 2, 4, 4), 18: (128, 64, 2, 2, 8, 3), 19: (128, 128, 2, 2, 4, 4),
         20: (128, 128, 2, 2, 8, 3), 21: (64, 128, 1, 4, 4, 4), 22: (64, 128, 1, 4, 8, 3), 23: (256, 32, 4, 1, 4, 4), 24: (256, 64, 4, 1, 4, 4),
         25: (256, 64, 4, 1, 8, 3), 26: (256, 128, 2, 2, 4, 4), 27: (256, 128, 2, 2, 8, 3),
         40: (256, 256, 4, 4, 4, 2), 41: (256, 256, 4, 4, 4, 3), 42: (256, 256, 4, 4, 4, 4), 43: (256, 256, 4, 4, 8, 2),
         60: (64, 64, 2, 2, 8, 6), 61: (64, 64, 2, 2, 8, 8), 62: (128, 64, 2, 2, 8, 6), 63: (64, 128, 1, 4, 8, 6)}
IGEMM = {i: t + (1,) for i, t in IGEMM.items()}
IGEMM.update({64: (256, 128, 4, 2, 4, 3, 2), 65: (128, 256, 2, 4, 4, 3, 2), 66: (256, 128, 4, 2, 4, 2, 2), 67: (256, 128, 2, 2, 4, 3, 2),
              68: (256, 128, 2, 2, 4, 2, 2)})
SPLITK = {56: (64, 64, 2, 2, 8, 3), 57: (64, 64, 2, 2, 8, 4), 58: (128, 64, 2, 2, 8, 3), 59: (64, 128, 1, 4, 8, 3)}
HALO = {28: 128, 29: 128, 30: 128, 31: 128, 36: 128, 37: 128, 38: 256, 39: 256}      # id -> BP
HALO_V2 = {55}
HALO_S2 = {44: 128, 45: 128, 46: 256, 47: 128, 48: 128, 49: 256}                     # id -> BP
DIRECT = {32: (2, 1), 33: (4, 2), 34: (4, 2), 35: (4, 4)}                            # id -> (CT, KS)
STREAM = {50: (8, 4), 51: (16, 8), 52: (8, 8), 53: (16, 4), 54: (8, 4)}
DIRECT8 = {69: (4, 1), 70: (4, 2), 71: (4, 1), 72: (8, 1)}

IDS_IGEMM = tuple(sorted(IGEMM))
IDS_SK = tuple(sorted(SPLITK))
IDS_HALO = tuple(sorted(HALO))
IDS_V2 = (55,)
IDS_S2 = tuple(sorted(HALO_S2))
IDS_DIRECT = tuple(sorted(DIRECT))
IDS_STREAM = tuple(sorted(STREAM))
IDS_D8 = tuple(sorted(DIRECT8))
IDS_FP8 = (4, 5, 6, 43) + IDS_D8                 # the ids of the fp8 cases pw128 / pw64 (what the fp8 path can take: fp8_tile_cases.IDS)
IDS_ALL = tuple(range(NIDS))
# persistent grids: VC_CONV_SLOTS = 8 makes a few workgroups walk all tiles
PERSISTENT = set(IDS_IGEMM) | set(IDS_DIRECT) | set(IDS_STREAM) | set(IDS_D8)
UP_OK = (2, 5, 10, 20, 27, 40, 41, 42)           # conv_igemm.hip::launch_one, `constexpr bool UP_OK`, read off the tile table by hand


def round_up(x, m):
    return (x + m - 1) // m * m


def q8(x):
    return rnd(x, "fp8")


class Case:
    """One launch: problem (precision, (B, H, W), cin -> cout, k, stride, pad, act, res_mode) + the view fields of vc_conv_view + the ids of
    the family it belongs to.  res_mode 0 = no residual."""

    def __init__(self, view, tag, precision, shape, cin, cout, k=1, stride=1, pad=0, act=1, res_mode=0, ids=IDS_ALL, **vf):
        self.view, self.tag, self.precision, self.shape = view, tag, precision, tuple(shape)
        self.cin, self.cout, self.k, self.stride, self.pad, self.act, self.res_mode = cin, cout, k, stride, pad, act, res_mode
        self.ids = tuple(ids)
        self.row = "%s/%s" % (view, precision)
        self.name = "%s-%s" % (self.row, tag)
        B, H, W = self.shape
        self.Ho, self.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        self.M = B * self.Ho * self.Wo
        self.v = dict(in_cs=cin, in_co=0, out_cs=round_up(cout, 8 if precision == "fp8" else 4), out_co=0, res_cs=0, res_co=0, split=0, out2_cs=0,
                      out2_co=0, out_f32=0, out_bf16=0, m_valid=-1, up_c=0, up_cs=0, up_co=0)
        if res_mode:
            self.v.update(res_cs=round_up(cout, 4), res_co=0)
        unknown = set(vf) - set(self.v)
        assert not unknown, unknown
        self.v.update(vf)

    # ---- derived --------------------------------------------------------------------------------------------------------------
    @property
    def store(self):
        """element type of y / y2"""
        if self.precision == "f32" or self.v["out_f32"]:
            return "f32"
        return "bf16" if self.precision == "bf16" or self.v["out_bf16"] else "fp8"

    @property
    def n1(self):
        """channels that go to y"""
        return self.v["split"] if self.v["split"] else self.cout

    @property
    def rows(self):
        """output pixels the launch may write"""
        return self.M if self.v["m_valid"] < 0 else min(self.M, self.v["m_valid"])

    def fast_store(self, v=None):
        """conv_device.h::conv_epilogue_fast_bf16: the 16-byte lane-pair store path (bf16 arithmetic only)"""
        v = self.v if v is None else v
        return (self.precision == "bf16" and not v["out_f32"] and self.cout % 8 == 0 and v["out_cs"] % 8 == 0 and v["out_co"] % 8 == 0 and
                (v["split"] == 0 or (v["split"] % 8 == 0 and v["out2_cs"] % 8 == 0 and v["out2_co"] % 8 == 0)))

    def dense_view(self):
        """the view vc_conv2d_host builds for the same problem"""
        cs = round_up(self.cout, 8 if self.precision == "fp8" else 4)
        return dict(self.v, in_cs=self.cin, in_co=0, out_cs=cs, out_co=0, res_cs=cs, res_co=0, split=0, out2_cs=0, out2_co=0, out_f32=0, out_bf16=0,
                    m_valid=-1, up_c=0, up_cs=0, up_co=0)

    @property
    def twin_same_store_path(self):
        """check (c) applies: the dense launch of the same configuration stores the same element type through the same epilogue path"""
        if self.v["out_f32"] or self.v["out_bf16"]:
            return False                         # (out_f32 has its own form of (c): rounded to bf16 it equals the dense result)
        return self.precision != "bf16" or self.fast_store() == self.fast_store(self.dense_view())

    # ---- operands: a function of the PROBLEM alone, so the dense twin of a case has the same ones ------------------------------------
    def problem_key(self):
        return (self.precision, self.shape, self.cin, self.cout, self.k, self.stride, self.pad, self.act, self.res_mode, self.v["up_c"])

    def operands(self):
        return _operands(self.problem_key())

    def x_dense(self):
        """(B, H, W, cin): the operand channels as the dense launch reads them (under `up`: the materialised concat)"""
        o = self.operands()
        if not self.v["up_c"]:
            return o["x"]
        return np.concatenate([upsample_ref(o["up"]), o["x"][..., self.v["up_c"]:]], axis=-1)

    def buffers(self):
        """x, x_up, res (whole buffers, NaN outside the operands), y, y2 (SENTINEL); None where the case has none"""
        o, v = self.operands(), self.v
        B, H, W = self.shape
        x = np.full((B, H, W, v["in_cs"]), np.nan, np.float32)
        lo = v["in_co"] + v["up_c"]                                  # under `up` the first up_c channels of the slice are not read
        x[..., lo:v["in_co"] + self.cin] = o["x"][..., v["up_c"]:]
        xu = None
        if v["up_c"]:
            xu = np.full((B, H // 2, W // 2, v["up_cs"]), np.nan, np.float32)
            xu[..., v["up_co"]:v["up_co"] + v["up_c"]] = o["up"]
        res = None
        if self.res_mode:
            res = np.full((B, self.Ho, self.Wo, v["res_cs"]), np.nan, np.float32)
            res[..., v["res_co"]:v["res_co"] + self.cout] = o["res"]
        y = np.full((B, self.Ho, self.Wo, v["out_cs"]), SENTINEL, np.float32)
        y2 = np.full((B, self.Ho, self.Wo, v["out2_cs"]), SENTINEL, np.float32) if v["split"] else None
        return x, xu, res, y, y2

    def slices(self):
        """{buffer: [(lo, hi, what)]}: the channel ranges of every buffer that hold operands or results"""
        v = self.v
        s = {"x": [(v["in_co"] + v["up_c"], v["in_co"] + self.cin, "input")], "y": [(v["out_co"], v["out_co"] + self.n1, "output")]}
        if v["up_c"]:
            s["x"].append((v["in_co"], v["in_co"] + v["up_c"], "replaced by the upsampled map"))
            s["x_up"] = [(v["up_co"], v["up_co"] + v["up_c"], "upsampled input")]
        if self.res_mode:
            s["res"] = [(v["res_co"], v["res_co"] + self.cout, "residual")]
        if v["split"]:
            s["y2"] = [(v["out2_co"], v["out2_co"] + self.cout - v["split"], "second output")]
        return s

    def strides(self):
        v = self.v
        return {"x": v["in_cs"], "x_up": v["up_cs"], "res": v["res_cs"], "y": v["out_cs"], "y2": v["out2_cs"]}

    def written(self, y, y2):
        """(M, cout): the launch's result out of the two destinations"""
        v = self.v
        a = y.reshape(self.M, -1)[:, v["out_co"]:v["out_co"] + self.n1]
        if not v["split"]:
            return a
        return np.concatenate([a, y2.reshape(self.M, -1)[:, v["out2_co"]:v["out2_co"] + self.cout - v["split"]]], axis=1)

    def untouched(self, y, y2):
        """the elements no launch may write, as one flat array (all SENTINEL after a correct launch)"""
        v = self.v
        parts = []
        for buf, co, n in ((y, v["out_co"], self.n1), (y2, v["out2_co"], self.cout - v["split"])):
            if buf is None:
                continue
            m = np.ones(buf.reshape(self.M, -1).shape, bool)
            m[:self.rows, co:co + n] = False
            parts.append(buf.reshape(self.M, -1)[m])
        return np.concatenate(parts)

    def reference(self):
        return _reference(self.problem_key())

    def weights_used(self):
        return _weights_used(self.problem_key())


def _rng(key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def _operands(key):
    precision, (B, H, W), cin, cout, k, stride, pad, act, res_mode, up_c = key
    rng = _rng(key)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    o = {"x": rnd(rng.standard_normal((B, H, W, cin)), precision),
         "w": (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32),
         "b": (rng.standard_normal(cout) * 0.1).astype(np.float32)}
    if res_mode:
        o["res"] = rnd(rng.standard_normal((B, Ho, Wo, cout)), precision)
    if up_c:
        o["up"] = rnd(rng.standard_normal((B, H // 2, W // 2, up_c)), precision)
    for a in o.values():
        a.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _weights_used(key):
    """the weights as the kernel multiplies them: bf16-rounded, f32 as given, fp8 = e4m3 x one scale per output channel (pack_and_upload)"""
    precision, cout = key[0], key[3]
    w = np.array(_operands(key)["w"])
    if precision == "bf16":
        return rnd(w, "bf16")
    if precision == "fp8":
        sw = (np.abs(w).reshape(cout, -1).max(1) / np.float32(448.0)).astype(np.float32)
        return q8(w / sw[:, None, None, None]) * sw[:, None, None, None]
    return w


@functools.lru_cache(maxsize=None)
def _reference(key):
    """float64 (M, cout): conv of the rounded operands, bias, residual / activation in the launch's order; no final rounding"""
    precision, (B, H, W), cin, cout, k, stride, pad, act, res_mode, up_c = key
    o = _operands(key)
    x = o["x"] if not up_c else np.concatenate([upsample_ref(o["up"]), o["x"][..., up_c:]], axis=-1)
    t = F.conv2d(torch.tensor(x).permute(0, 3, 1, 2).double(), torch.tensor(_weights_used(key)).double(), torch.tensor(o["b"]).double(),
                 stride=stride, padding=pad)
    r = torch.tensor(o["res"]).permute(0, 3, 1, 2).double() if res_mode else None
    if res_mode == 2:
        t = t + r
    t = F.silu(t) if act == 1 else (F.relu(t) if act == 2 else t)
    if res_mode == 1:
        t = t + r
    ref = t.permute(0, 2, 3, 1).reshape(-1, cout).numpy()
    ref.setflags(write=False)
    return ref


# ---- the gates: the project's own (tests/test_gpu_kernels.py::test_conv2d), nothing new --------------------------------------------------
GATE = {"bf16": dict(rtol=2 ** -7, atol=2e-3), "f32": dict(rtol=1e-4, atol=1e-4)}


def gate_of(case):
    """(reference as the store type holds it, tolerances), or None for fp8 -> fp8 (no gate: bit-equality with the dense twin carries it)"""
    ref = case.reference()
    if case.store == "f32":
        return ref.astype(np.float32), GATE["f32"]
    if case.store == "bf16":
        return rnd(ref.astype(np.float32), "bf16"), GATE["bf16"]
    return None


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _slice_views(cin, cout, align, res, in_shift, in_extra=24):
    """slices8 / slices4: input offset in_shift inside a buffer in_extra wider (fp8: 32, its stride is a multiple of 16), output offset
    `align` inside round(cout) + 3 * align, residual alike"""
    r = round_up(cout, align)
    v = dict(in_co=in_shift, in_cs=cin + in_extra, out_co=align, out_cs=r + 3 * align)
    if res:
        v.update(res_co=align, res_cs=r + 2 * align)
    return v


# (cfg, cin, couts) rows of tests/test_gpu_kernels.py::test_conv1x1_direct_configs / test_conv1x1_stream_configs
DIRECT_ROWS = [(32, 32, (32, 64, 128)), (33, 64, (64, 128, 256)), (34, 64, (64, 128, 256)), (35, 128, (64, 128, 256))]
STREAM_ROWS = [(50, 128, 128), (51, 256, 256), (52, 256, 128), (53, 128, 256), (54, 128, 128)]
SK_PROBLEM = ((2, 7, 7), 256, 256, 3, 1, 1)          # tests/test_gpu_round6.py::SK_CASES[1]: a tile spans both images


def _family_problems(precision, with_res):
    """[(tag, ids, shape, cin, cout, k, stride, pad, act, res_mode)]: the small problems of every family under the slice views"""
    r = (lambda m: m) if with_res else (lambda m: 0)
    if precision == "fp8":
        return [("pw128", IDS_FP8, (2, 12, 12), 128, 128, 1, 1, 0, 1, r(1)), ("pw64", IDS_FP8, (1, 17, 13), 64, 72, 1, 1, 0, 0, 0)]
    if precision == "f32":
        every = tuple(i for i in IDS_ALL)
        return [("g3x3", every, (2, 23, 19), 24, 72, 3, 1, 1, 1, r(1)), ("g1x1s2", every, (3, 20, 20), 136, 40, 1, 2, 0, 1, r(2)),
                ("gpw", every, (2, 20, 17), 64, 72, 1, 1, 0, 1, 0)]
    p = [("g3x3", IDS_IGEMM, (2, 23, 19), 24, 72, 3, 1, 1, 1, r(1)), ("g1x1s2", IDS_IGEMM, (3, 20, 20), 136, 40, 1, 2, 0, 1, r(2)),
         ("gpw", IDS_IGEMM, (2, 20, 17), 64, 72, 1, 1, 0, 1, 0),
         ("sk", IDS_SK, *SK_PROBLEM, 2, r(2)),
         ("h1a", IDS_HALO, (2, 23, 19), 64, 72, 3, 1, 1, 1, r(1)), ("h1b", IDS_HALO, (9, 4, 5), 128, 130, 3, 1, 1, 1, 0),
         ("h2a", IDS_V2, (2, 23, 19), 64, 72, 3, 1, 1, 1, r(1)), ("h2b", IDS_V2, (5, 7, 7), 64, 40, 3, 1, 1, 2, r(2)),
         ("s2a", IDS_S2, (5, 8, 6), 64, 40, 3, 2, 1, 2, 0), ("s2b", IDS_S2, (3, 20, 24), 128, 136, 3, 2, 1, 0, 0)]
    for cfg, ci, cos in DIRECT_ROWS:
        for co in cos:
            p.append(("d%d_%d" % (cfg, co), (cfg,), (3, 7, 9), ci, co, 1, 1, 0, 1 if co != 128 else 0, 0))
    for cfg, ci, co in STREAM_ROWS:
        p.append(("st%d" % cfg, (cfg,), (3, 7, 9), ci, co, 1, 1, 0, 1 if cfg % 2 else 0, 0))
    return p


def _build():
    cases = []

    def add(view, tag, precision, shape, cin, cout, k, stride, pad, act, res_mode, ids, **vf):
        cases.append(Case(view, tag, precision, shape, cin, cout, k, stride, pad, act, res_mode, ids, **vf))

    # slices8: every family's problems; fp8 with 16-aligned input offsets
    for precision in ("bf16", "fp8"):
        for tag, ids, shape, ci, co, k, s, p, act, rm in _family_problems(precision, True):
            add("slices8", tag, precision, shape, ci, co, k, s, p, act, rm, ids, **_slice_views(ci, co, 8, rm, 16, 32 if precision == "fp8" else 24))
    # slices4: the general store loop (bf16: offsets and strides that are multiples of 4 only; f32: the input slice 4-aligned too)
    for precision in ("bf16", "f32"):
        for tag, ids, shape, ci, co, k, s, p, act, rm in _family_problems(precision, True):
            add("slices4", tag, precision, shape, ci, co, k, s, p, act, rm, ids, **_slice_views(ci, co, 4, rm, 4 if precision == "f32" else 16))
    # split8 / split4 (no residual: conv_check).  Cout = 72 problems: a boundary inside a 16-channel MFMA tile (40) and on a tile edge (64);
    # 36 on 72 and 68 on 130 (ragged tail in the second destination) for the general loop.  The weight-stationary families and fp8 get the
    # C3 cv1 | cv2 form on their own problems: split = cout / 2.
    def split_view(co, split, align):
        return dict(split=split, out_co=align, out_cs=round_up(split, align) + 3 * align, out2_co=align, out2_cs=round_up(co - split, align) + 16)

    bf = _family_problems("bf16", False)
    for tag, ids, shape, ci, co, k, s, p, act, rm in bf:
        if co == 72:
            for split in (40, 64):
                add("split8", "%s_%d" % (tag, split), "bf16", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 24, **split_view(co, split, 8))
            add("split4", "%s_36" % tag, "bf16", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 24, **split_view(co, 36, 4))
        elif co == 130:
            add("split4", "%s_68" % tag, "bf16", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 24, **split_view(co, 68, 4))
        elif ids[0] in DIRECT or ids[0] in STREAM or tag == "sk":
            add("split8", "%s_half" % tag, "bf16", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 24, **split_view(co, co // 2, 8))
            if tag == "sk":                                        # the general loop's second destination behind the split-K reduction
                add("split4", "sk_132", "bf16", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 24, **split_view(co, 132, 4))
    for tag, ids, shape, ci, co, k, s, p, act, rm in _family_problems("f32", False):
        if co == 72:
            add("split4", "%s_36" % tag, "f32", shape, ci, co, k, s, p, act, 0, ids, in_co=4, in_cs=ci + 24, **split_view(co, 36, 4))
    for tag, ids, shape, ci, co, k, s, p, act, rm in _family_problems("fp8", False):
        split = 64 if co == 128 else 40
        add("split8", "%s_%d" % (tag, split), "fp8", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 32, **split_view(co, split, 8))
        add("out_bf16", tag, "fp8", shape, ci, co, k, s, p, act, 0, ids, in_co=16, in_cs=ci + 32, out_co=8, out_cs=co + 24, out_bf16=1)
    # out_f32 (the dense Detect heads): 255 and 72 outputs, no activation, once with a split
    # (the split-K ids on their own problem, 256 outputs: the pointwise problem's K is too short for them)
    not_sk = tuple(i for i in IDS_ALL if i not in SPLITK)
    for co, split in ((255, 0), (72, 0), (255, 128), (256, 0), (256, 128)):
        sk = co == 256
        ci = SK_PROBLEM[1] if sk else 64
        vf = dict(in_co=16, in_cs=ci + 24, out_co=4, out_cs=round_up(split or co, 4) + 12, out_f32=1)
        if split:
            vf.update(split=split, out2_co=4, out2_cs=round_up(co - split, 4) + 8)
        if sk:
            add("out_f32", "sk%d_%d" % (co, split), "bf16", *SK_PROBLEM, 0, 0, IDS_SK, **vf)
        else:
            add("out_f32", "pw%d_%d" % (co, split), "bf16", (2, 20, 17), 64, co, 1, 1, 0, 0, 0, not_sk, **vf)
    # m_dev (the sparse Detect head): one row of 300 pixels, the count on the device
    for precision, ci in (("bf16", 64), ("f32", 24)):
        for mv in (0, 1, 64, 65, 299, 300, 5000):
            add("m_dev", "m%d" % mv, precision, (1, 1, 300), ci, 72, 1, 1, 0, 1, 0, IDS_ALL, in_co=CH[precision], in_cs=ci + 24, out_co=8, out_cs=96, m_valid=mv)
    # ... and on a problem every OTHER family would take but for the count: a launcher that ignored m_dev would run these, write the rows
    # >= m_valid and differ from the heuristic launch; they must refuse
    md = dict(out_co=8, m_valid=0)
    for tag, ids, shape, ci, co, k, s, p, act, rm in _family_problems("bf16", False):
        if tag in ("h1a", "h2a", "sk", "s2a") or ids[0] in DIRECT or ids[0] in STREAM:
            M = shape[0] * ((shape[1] + 2 * p - k) // s + 1) * ((shape[2] + 2 * p - k) // s + 1)
            add("m_dev", "%s_m%d" % (tag, M // 2 + 1), "bf16", shape, ci, co, k, s, p, act, 0, ids, in_co=8, in_cs=ci + 24,
                **dict(md, out_cs=round_up(co, 8) + 24, m_valid=M // 2 + 1))
    add("m_dev", "pw128_m100", "fp8", (2, 12, 12), 128, 128, 1, 1, 0, 1, 0, IDS_ALL, in_co=16, in_cs=160, out_co=8, out_cs=152, m_valid=100)
    # up: odd half-size maps (5 x 7, 3 x 5) that span several images per tile
    for shape in ((3, 10, 14), (2, 6, 10)):
        for ci, uc in ((128, 64), (192, 128)):
            for co in (72, 256):
                for split in (0, 40):
                    vf = dict(in_co=64, in_cs=64 + ci + 8, up_c=uc, up_co=8, up_cs=uc + 16)
                    vf.update(split_view(co, split, 8) if split else dict(out_co=8, out_cs=co + 24))
                    add("up", "%dx%d_%d_%d_%d_%d" % (shape[1], shape[2], ci, uc, co, split), "bf16", shape, ci, co, 1, 1, 0, 1, 0, IDS_ALL, **vf)
    # every row is crossed with EVERY id: the ids whose family has no problem of its own in a row (another precision, no 72-channel
    # problem) get the row's pointwise case
    for row, tag in REST_OF_ROW.items():
        have = {i for c in cases if c.row == row for i in c.ids}
        t = next(c for c in cases if c.row == row and c.tag == tag)
        missing = tuple(i for i in IDS_ALL if i not in have)
        if missing:
            cases.append(Case(t.view, t.tag + "_rest", t.precision, t.shape, t.cin, t.cout, t.k, t.stride, t.pad, t.act, t.res_mode, missing, **t.v))
    return cases


REST_OF_ROW = {"slices8/bf16": "gpw", "slices8/fp8": "pw64", "slices4/bf16": "gpw", "split8/bf16": "gpw_40", "split8/fp8": "pw64_40",
               "split4/bf16": "gpw_36", "out_bf16/fp8": "pw64"}


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
ROWS = tuple(sorted({c.row for c in CASES}))


def cases_of(row, cfg=None):
    return [c for c in CASES if c.row == row and (cfg is None or cfg in c.ids)]


# ---- what the launchers take ------------------------------------------------------------------------------------------------------
def conv_check_admits(c):
    """conv_dispatch.hip::conv_check, the argument checks a test can reach"""
    v, ch = c.v, CH[c.precision]
    if c.precision == "fp8":
        if c.cout % 8 or v["out_cs"] % 8 or v["out_co"] % 8 or (v["split"] and (v["split"] % 8 or v["out2_cs"] % 8 or v["out2_co"] % 8)):
            return False
        if v["out_bf16"] and v["split"]:
            return False
    if c.cin % ch or v["in_cs"] % ch or v["in_co"] % ch or v["out_cs"] % 4 or v["out_co"] % 4:
        return False
    if v["split"] and (v["split"] % 4 or v["out2_cs"] % 4 or v["out2_co"] % 4 or c.res_mode):
        return False
    if c.res_mode and (v["res_cs"] % 4 or v["res_co"] % 4):
        return False
    if v["up_c"]:
        B, H, W = c.shape
        if not (c.precision == "bf16" and c.k == 1 and c.stride == 1 and c.pad == 0 and H % 2 == 0 and W % 2 == 0 and 0 < v["up_c"] < c.cin and
                v["up_c"] % 64 == 0 and c.cin % 64 == 0 and v["up_cs"] % 8 == 0 and v["up_co"] % 8 == 0 and v["m_valid"] < 0):
            return False
    return True


def heuristic(c):
    """conv_dispatch.hip::conv_heuristic"""
    t128 = ((c.M + 127) // 128) * ((c.cout + 127) // 128)
    if c.precision == "fp8":
        return 4 if c.cout <= 64 else (5 if t128 >= 512 else 6)
    if c.v["up_c"]:
        return 2
    if c.cout <= 32:
        return 0
    if c.cout <= 64:
        return 1
    return 2 if t128 >= 512 else 3


def s2halo_geom(G, Wo, bp):
    """conv_geom.h::s2halo_geom: does a tile rectangle exist"""
    for tw in range(1, min(Wo, 254) + 1):
        th = min(bp // tw, 254, G)
        if th >= 1 and (th + 1) * (tw + 1) <= bp // 128 * 5 * 32 - 1:
            return True
    return False


def _pointwise(c):
    return c.k == 1 and c.stride == 1 and c.pad == 0


def _direct_ok(c, ct, ks):
    v = c.v
    if c.precision != "bf16" or not _pointwise(c) or c.cin != ks * 32 or v["in_cs"] % 8 or v["in_co"] % 8 or v["up_c"] or v["m_valid"] >= 0:
        return False
    if v["out_f32"] or c.res_mode or c.act not in (0, 1) or v["out_cs"] % 8 or v["out_co"] % 8:
        return False
    if v["split"] and (v["split"] % 8 or v["out2_cs"] % 8 or v["out2_co"] % 8):
        return False
    return c.cout % (ct * 16) == 0 and c.cout // (ct * 16) in (1, 2, 4)


def accepts(c, cfg):
    """does launch_conv_cfg(p, cfg) launch (True) or refuse quietly with VC_ERR_ARG (False), for a case conv_check admits"""
    v, (B, H, W) = c.v, c.shape
    m_dev, up = v["m_valid"] >= 0, v["up_c"] > 0
    if cfg in IGEMM:
        BP, BC, WP, WC, KC, NS, OCC = IGEMM[cfg]
        if OCC != 1:
            return c.precision == "bf16" and not up
        if c.precision == "f32":
            return True
        if c.precision == "fp8":
            return KC == 8 and (BP // WP // 16) % 2 == 0
        return cfg in UP_OK if up else True
    if cfg in SPLITK:
        BP, BC, WP, WC, KC, NS = SPLITK[cfg]
        if c.precision != "bf16" or up or m_dev:
            return False
        tiles = ((c.M + BP - 1) // BP) * ((c.cout + BC - 1) // BC)
        nk = round_up(c.k * c.k * c.cin, KC * 8) // (KC * 8)
        return min(SK_SLOTS_MIN // tiles, nk // 4, 8) >= 2
    three = c.precision == "bf16" and c.k == 3 and c.pad == 1
    if cfg in HALO:
        if not (three and c.stride == 1 and c.cin % 32 == 0 and v["in_cs"] % 8 == 0 and v["in_co"] % 8 == 0 and not m_dev):
            return False
        bp = HALO[cfg]
        return ((bp - 1 + W - 1) // W + 1 + 2) * W <= 11 * 64 - 1
    if cfg in HALO_V2:
        if not (three and c.stride == 1 and c.cin % 64 == 0 and v["in_cs"] % 8 == 0 and v["in_co"] % 8 == 0 and not m_dev and 1 <= W <= 64):
            return False
        r = min(256 // W, 320 // W - 2, B * H)
        return r >= 1 and r * W >= 160
    if cfg in HALO_S2:
        if not (three and c.stride == 2 and c.cin % 64 == 0 and v["in_cs"] % 8 == 0 and v["in_co"] % 8 == 0 and H == 2 * c.Ho and W == 2 * c.Wo):
            return False
        if v["out_f32"] or c.res_mode or v["split"] or m_dev or c.cout % 8 or v["out_cs"] % 8 or v["out_co"] % 8:
            return False
        return s2halo_geom(B * c.Ho, c.Wo, HALO_S2[cfg])
    if cfg in DIRECT:
        return _direct_ok(c, *DIRECT[cfg])
    if cfg in STREAM:
        return _direct_ok(c, *STREAM[cfg]) and c.cout == STREAM[cfg][0] * 16
    if cfg in DIRECT8:
        ct, ks = DIRECT8[cfg]
        if c.precision != "fp8" or not _pointwise(c) or not ((ks - 1) * 128 < c.cin <= ks * 128) or c.cin % 64 or (c.cin % 128 and c.cin != 64):
            return False
        if v["in_cs"] % 16 or v["in_co"] % 16 or up or m_dev:
            return False
        return (round_up(c.cout, 8) + ct * 16 - 1) // (ct * 16) in (1, 2, 4)
    raise KeyError(cfg)


# launch_one_sk sizes its split by the resident workgroups of the kernel (occupancy x compute units).  One workgroup per unit of a 256-unit
# chip is the least it can be; the split-K cases are chosen so that this term never binds (tests/test_conv_view_cases.py).
SK_SLOTS_MIN = 256

RUNS, REFUSES = "runs", "refuses"
# One row per (view, precision), one character per id 0 .. 72: r = runs, x = refuses.  Written out from `accepts` over the cases of the
# row; tests/test_conv_view_cases.py holds the two together, and states the rows the issue fixes in words (up, m_dev, the heuristic's tiles).
_ROWS = {
    "m_dev/bf16": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxxxxxxxxxrrrrxxxxxxxxxxxxxxxxrrrrrrrrrxxxx",
    "m_dev/f32": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxxxxxxxxxrrrrxxxxxxxxxxxxxxxxrrrrxxxxxxxxx",
    "m_dev/fp8": "xxxxrrrxrxrxrrxrrxrxrxrxxrxrxxxxxxxxxxxxxxxrxxxxxxxxxxxxxxxxrrrrxxxxxxxxx",
    "out_bf16/fp8": "xxxxrrrxrxrxrrxrrxrxrxrxxrxrxxxxxxxxxxxxxxxrxxxxxxxxxxxxxxxxrrrrxxxxxrxrr",
    "out_f32/bf16": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxxxxxxxxxrrrrxxxxxxxxxxxxrrrrrrrrrrrrrxxxx",
    "slices4/bf16": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxrrrrrrrrxxxxxxxxxxxrrrrrrrrrrrrrrxxxx",
    "slices4/f32": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxxxxxxxxxrrrrxxxxxxxxxxxxxxxxrrrrxxxxxxxxx",
    "slices8/bf16": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxx",
    "slices8/fp8": "xxxxrrrxrxrxrrxrrxrxrxrxxrxrxxxxxxxxxxxxxxxrxxxxxxxxxxxxxxxxrrrrxxxxxrxrr",
    "split4/bf16": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxrrrrrrrrxxxxxxxxxxxrrrrrrrrrrrrrrxxxx",
    "split4/f32": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxxxxxxxxxrrrrxxxxxxxxxxxxxxxxrrrrxxxxxxxxx",
    "split8/bf16": "rrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrrxxxxxxrrrrrrrrrrrrrrrrrrrxxxx",
    "split8/fp8": "xxxxrrrxrxrxrrxrrxrxrxrxxrxrxxxxxxxxxxxxxxxrxxxxxxxxxxxxxxxxrrrrxxxxxrxrr",
    "up/bf16": "xxrxxrxxxxrxxxxxxxxxrxxxxxxrxxxxxxxxxxxxrrrxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx",
}
EXPECT = {row: {i: (RUNS if s[i] == "r" else REFUSES) for i in range(NIDS)} for row, s in _ROWS.items()}


def derive_row(row):
    """the row of EXPECT as `accepts` gives it; raises if two cases of one id disagree or an id has no case"""
    out = []
    for cfg in range(NIDS):
        got = {accepts(c, cfg) for c in cases_of(row, cfg)}
        if len(got) != 1:
            raise AssertionError("row %s, id %d: %s" % (row, cfg, sorted(got) or "no case"))
        out.append("r" if got.pop() else "x")
    return "".join(out)


# ---- conv_check refusals: one case per VC_CHECK, never launched -------------------------------------------------------------------------
def _refusals():
    pw = dict(shape=(2, 20, 18), cin=64, cout=72)
    up = dict(in_co=64, in_cs=200, up_c=64, up_co=8, up_cs=80, out_co=8, out_cs=96)
    r = [Case("refuse", "in_co4_bf16", "bf16", **pw, in_co=4, in_cs=88),
         Case("refuse", "out_co2", "bf16", **pw, out_co=2, out_cs=96),
         Case("refuse", "split6", "bf16", **pw, split=6, out_cs=16, out2_co=0, out2_cs=72),
         Case("refuse", "split_with_residual", "bf16", **pw, res_mode=1, split=40, out_cs=40, out2_co=0, out2_cs=32),
         Case("refuse", "up_odd_map", "bf16", (2, 20, 17), 128, 72, **up),
         Case("refuse", "up_c_is_cin", "bf16", (2, 20, 18), 64, 72, **dict(up, in_cs=136)),
         Case("refuse", "up_c32", "bf16", (2, 20, 18), 128, 72, **dict(up, up_c=32)),
         Case("refuse", "up_f32", "f32", (2, 20, 18), 128, 72, **up),
         Case("refuse", "up_with_m_valid", "bf16", (2, 20, 18), 128, 72, **dict(up, m_valid=100)),
         Case("refuse", "fp8_out_co4", "fp8", **pw, out_co=4, out_cs=96),
         # (not in conv_check before this table existed: conv_epilogue_fp8's bf16 store ignores the split and would store channels >= split
         # behind the first slice, so the combination is refused)
         Case("refuse", "fp8_out_bf16_split", "fp8", **pw, out_bf16=1, split=40, out_cs=40, out2_co=0, out2_cs=32)]
    msgs = ["conv: input channels", "conv: output stride", "conv: bad split", "conv: bad split", "conv: the upsample fold-in", "conv: the upsample fold-in",
            "conv: the upsample fold-in", "conv: the upsample fold-in", "conv: the upsample fold-in", "conv fp8: channel scales", "conv fp8: the bf16 store"]
    for c, m in zip(r, msgs):
        c.message = m                     # the start of conv_check's own message: a refusal by another check is not this refusal
    return r


REFUSALS = _refusals()


# ---- conv3x3s2_halo_kernel<..., F2>: the 3x3 / s2 with the pointwise conv that alone reads it ----------------------------------------------
F2_PROBLEMS = [((5, 8, 6), 64), ((2, 40, 32), 64), ((3, 20, 24), 128)]
F2_VIEWS = {"one": dict(out_co=8, out_cs=152), "split64": dict(split=64, out_co=8, out_cs=88, out2_co=8, out2_cs=80)}


class F2Case:
    def __init__(self, shape, cin, vname):
        self.shape, self.cin, self.vname = shape, cin, vname
        self.name = "f2-%dx%dx%d-%d-%s" % (*shape, cin, vname)
        B, H, W = shape
        self.Ho, self.Wo = H // 2, W // 2
        self.M = B * self.Ho * self.Wo
        self.v3 = dict(in_co=16, in_cs=cin + 24)                  # the 3x3 reads a slice
        self.v1 = dict(F2_VIEWS[vname])                           # the pointwise conv's store
        # the unfused pair through vc_conv2d_view_host: configuration 49, then the pointwise conv on configuration 3
        self.first = Case("f2a", self.name, "bf16", shape, cin, 128, 3, 2, 1, 1, 0, (49,), **self.v3)
        self.second = Case("f2b", self.name, "bf16", (B, self.Ho, self.Wo), 128, 128, 1, 1, 0, 1, 0, (3,), **self.v1)

    def operands(self):
        o1, o2 = self.first.operands(), self.second.operands()
        return o1["x"], o1["w"], o1["b"], o2["w"], o2["b"]

    def reference(self):
        """float64: conv -> SiLU -> bf16 -> 1x1 -> SiLU, (M, 128)"""
        x, w3, b3, w1, b1 = self.operands()
        mid = rnd(self.first.reference().astype(np.float32), "bf16").reshape(self.shape[0], self.Ho, self.Wo, 128)
        t = F.conv2d(torch.tensor(mid).permute(0, 3, 1, 2).double(), torch.tensor(rnd(np.array(w1), "bf16")).double(), torch.tensor(b1).double())
        return F.silu(t).permute(0, 2, 3, 1).reshape(-1, 128).numpy()


F2_CASES = [F2Case(shape, cin, vn) for shape, cin in F2_PROBLEMS for vn in F2_VIEWS]
