"""Problems, operands, float64 references and the two comparisons for the fp8 implicit GEMM under EVERY tile id the tuner can pick
(engine_run.hip::tuned_cfg times ids 0 .. 72; conv_igemm.hip::launch_one takes the fp8 ones listed in FP8_IGEMM_IDS), and for the direct
fp8 pointwise ids 69 - 72 where conv_view_cases.accepts admits them.  tests/test_gpu_fp8_tiles.py launches them through vc_conv2d_host under
VC_CONV_CFG / VC_CONV_STRICT / VC_CONV_SLOTS; tests/test_fp8_tile_cases.py holds this module to its own conditions on the CPU and shows
that both comparisons reject the outputs of wrong kernels.

EXACT problems: operands for which every product and every partial sum is a multiple of 2^-2 below 2^12, so the fp32 accumulator holds the
float64 sum whatever the order of the additions, `acc * scale + bias` is exact in fp32 and so is the residual add.  The only rounding
left is the store's: clamp to +-448, round to nearest even to e4m3fn.  The comparison is np.array_equal: any difference is a kernel error.
  x          multiples of 1/4 in [-2, 2] (e4m3 values)
  w[n]       integers in [-8, 8] times 2^-j[n], j[n] in 0 .. 8, one weight per channel +-448 * 2^-j[n]: pack_and_upload's amax / 448 is
             exactly 2^-j[n] and w / scale is an e4m3 integer
  bias[n]    an integer in [-64, 64] times 2^-j[n]
  residual   any finite e4m3 value, +-448 and +-2^-9 among them
  activation none or ReLU
Channels with small j saturate (the clamp decides the byte), channels with j = 7, 8 reach the subnormals of the store and exact zero.

SILU problems: the shapes of three exact problems with SiLU and standard_normal operands (tests/test_gpu_fp8.py::FP8_CASES), held to step 1
of the fp8 ladder: within one e4m3 ulp of the float64 reference's own rounding, >= 97 % of the bytes identical, finite.
TWINS: the operand sets of the fp8 view cases' dense launches (conv_view_cases.cases_of("slices8/fp8", id)), at the same gate: check (c)
of tests/test_gpu_conv_views.py compares a view with the dense launch of the same id, and this holds that launch to float64.

`im2col` restates the convolution as the kernel walks it -- K = (tap, channel of the 16-padded input), in tiles of 128 -- so that the CPU
test can drop, repeat or misread a K tile; it is held equal to the float64 conv."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import conv_view_cases as V
from aux_cases import rnd

NONE, SILU, RELU = 0, 1, 2                    # act
AFTER, BEFORE = 1, 2                          # res_mode (0: no residual)
BK = 128                                      # K elements of one fp8 K tile: KC = 8 chunks of 16 bytes
SLOTS = (0, 8)                                # VC_CONV_SLOTS: the chip's own persistent grid, and 8 workgroups that walk every tile

# conv_igemm.hip::launch_one: single occupancy, 128-byte LDS rows, an even number of 16-pixel tiles per wave (the fp8 epilogue pairs them)
FP8_IGEMM_IDS = tuple(sorted(i for i, (BP, BC, WP, WC, KC, NS, OCC) in V.IGEMM.items() if OCC == 1 and KC == 8 and (BP // WP // 16) % 2 == 0))
DIRECT_IDS = V.IDS_D8
IDS = FP8_IGEMM_IDS + DIRECT_IDS
RING = {i: V.IGEMM[i][5] for i in FP8_IGEMM_IDS}      # id -> NS, the stages of its K-tile ring


def q8(x):
    """round to OCP e4m3fn, saturating at +-448, back to float32 (tests/test_gpu_fp8.py::q8)"""
    with np.errstate(over="ignore"):
        return rnd(np.array(x, np.float32), "fp8")            # (a copy: operands are read-only)


E4M3 = np.unique(torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().numpy())
E4M3 = E4M3[np.isfinite(E4M3)]                # the 253 finite values (-0 folded into 0)


class Problem:
    def __init__(self, kind, tag, B, H, W, cin, cout, k, stride, pad, act, res_mode, seed=0):
        self.kind, self.tag, self.shape = kind, tag, (B, H, W)
        self.cin, self.cout, self.k, self.stride, self.pad, self.act, self.res_mode, self.seed = cin, cout, k, stride, pad, act, res_mode, seed
        self.name = "%s-%s" % (kind, tag)
        self.Ho, self.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        self.M = B * self.Ho * self.Wo
        self.cin_eff = V.round_up(cin, 16)    # vc_conv2d_host pads the input channels with zeros to the 16-byte chunk
        self.K = k * k * self.cin_eff
        self.nk = V.round_up(self.K, BK) // BK
        # the dense launch as the acceptance table sees it (the direct ids decide by it)
        self.case = V.Case(kind, tag, "fp8", (B, H, W), cin, cout, k, stride, pad, act, res_mode)

    def key(self):
        return (self.kind, self.tag, self.shape, self.cin, self.cout, self.k, self.stride, self.pad, self.act, self.res_mode, self.seed)

    def operands(self):
        """x (B, H, W, cin), w (cout, cin, k, k), b (cout), res (B, Ho, Wo, cout) or None: float32, read-only"""
        return _operands(self.key())

    def weights_used(self):
        """the weights as the kernel multiplies them: e4m3 x one fp32 scale per output channel (engine.hip::pack_and_upload)"""
        w = self.operands()["w"]
        sw = (np.abs(w).reshape(self.cout, -1).max(1) / np.float32(448.0)).astype(np.float32)
        return q8(w / sw[:, None, None, None]) * sw[:, None, None, None]

    def finish(self, acc):
        """(M, cout) float64 sums -> bias, residual / activation in the launch's order; no rounding"""
        o = self.operands()
        t = torch.tensor(np.asarray(acc, np.float64)) + torch.tensor(o["b"]).double()
        r = None if o["res"] is None else torch.tensor(o["res"]).double().reshape(self.M, self.cout)
        if self.res_mode == BEFORE:
            t = t + r
        t = F.silu(t) if self.act == SILU else (F.relu(t) if self.act == RELU else t)
        if self.res_mode == AFTER:
            t = t + r
        return t.numpy()

    def sums(self):
        """(M, cout) float64: the convolution without bias, by torch"""
        return _sums(self)

    def pre(self):
        """(M, cout) float64: the value the epilogue holds before the store rounds it"""
        return self.finish(self.sums())

    def expected(self):
        """(M, cout) float32: the e4m3 values a correct launch stores"""
        return _expected(self)

    def im2col(self, pad_mode="constant"):
        """A (M, nk * 128), Wm (cout, nk * 128), float64, K in the kernel's order: tap-major, the 16-padded channels inside a tap, zero
        columns up to the last K tile.  pad_mode "edge" reads the padding ring as the neighbouring pixel."""
        o, (B, H, W), p, k, s = self.operands(), self.shape, self.pad, self.k, self.stride
        x = np.pad(o["x"].astype(np.float64), ((0, 0), (p, p), (p, p), (0, 0)), mode=pad_mode)
        x = np.pad(x, ((0, 0), (0, 0), (0, 0), (0, self.cin_eff - self.cin)))
        taps = [x[:, r:r + s * (self.Ho - 1) + 1:s, c:c + s * (self.Wo - 1) + 1:s, :] for r in range(k) for c in range(k)]
        A = np.concatenate(taps, axis=-1).reshape(self.M, self.K)
        w = np.pad(self.weights_used().astype(np.float64).transpose(0, 2, 3, 1), ((0, 0), (0, 0), (0, 0), (0, self.cin_eff - self.cin)))
        tail = ((0, 0), (0, self.nk * BK - self.K))
        return np.pad(A, tail), np.pad(w.reshape(self.cout, self.K), tail)

    def admits(self, cfg):
        """does launch_conv_cfg take the dense launch of this problem under tile id `cfg`"""
        return cfg in FP8_IGEMM_IDS or (cfg in DIRECT_IDS and V.accepts(self.case, cfg))


def _rng(key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def _operands(key):
    kind, tag, (B, H, W), cin, cout, k, stride, pad, act, res_mode, seed = key
    rng = _rng(key)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if kind == "exact":
        x = rng.integers(-8, 9, (B, H, W, cin)) / 4.0
        j = rng.permutation(np.arange(cout) % 9)                       # every exponent 0 .. 8 on about cout / 9 channels
        s = 2.0 ** -j
        w = rng.integers(-8, 9, (cout, cin * k * k)).astype(np.float64)
        w[np.arange(cout), rng.integers(0, cin * k * k, cout)] = 448.0 * rng.choice([-1.0, 1.0], cout)
        w = (w * s[:, None]).reshape(cout, cin, k, k)
        b = rng.integers(-64, 65, cout) * s
        res = None
        if res_mode:
            res = rng.choice(E4M3, (B, Ho, Wo, cout))
            res.reshape(-1)[rng.choice(res.size, 8, replace=False)] = [448.0, -448.0, 2.0 ** -9, -2.0 ** -9] * 2
    else:                                                              # tests/test_gpu_fp8.py::FP8_CASES
        x = q8(rng.standard_normal((B, H, W, cin)))
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
        b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        res = q8(rng.standard_normal((B, Ho, Wo, cout))) if res_mode else None
    o = {"x": x, "w": w, "b": b, "res": res}
    for name, a in o.items():
        if a is not None:
            assert (a == a.astype(np.float32)).all(), name             # nothing is lost on the way to the C ABI
            o[name] = np.ascontiguousarray(a, np.float32)
            o[name].setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _sums(p):
    t = F.conv2d(torch.tensor(p.operands()["x"]).permute(0, 3, 1, 2).double(), torch.as_tensor(p.weights_used()).double(), None,
                 stride=p.stride, padding=p.pad)
    a = t.permute(0, 2, 3, 1).reshape(p.M, p.cout).numpy()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _expected(p):
    e = q8(p.pre())
    e.setflags(write=False)
    return e


# (B, H, W, Cin, Cout, k, stride, pad, act, res_mode): the smallest problems that still reach each edge
_SHAPES = {
    # K = 576 = 4.5 K tiles: a tile spans two taps, the last one is half empty; M = 874: ragged, a 256-pixel tile crosses the batch seam;
    # Cout = 72: a ragged 16-channel tile
    "taps": (2, 23, 19, 64, 72, 3, 1, 1, NONE, AFTER),
    # stride 2 on odd maps; K = 1152 = 9 K tiles, more than the deepest ring (8): every ring wraps; two channel tiles of 128, the second ragged
    "s2wrap": (3, 13, 11, 128, 136, 3, 2, 1, RELU, BEFORE),
    # Cin = 48: K = 432, a K tile spans 2.67 taps; M = 81: a ragged pixel tile under every id, less than one tile of 128 or 256
    "thin": (1, 9, 9, 48, 40, 3, 1, 1, NONE, 0),
    # pointwise, 9 K tiles, M = 105
    "longk": (3, 5, 7, 1152, 64, 1, 1, 0, NONE, 0),
    # Cin = 24: the host pads to 32, zero K columns inside every tap; M = 1100 x Cout = 264: 10 tiles even at 256 x 256, so 8 persistent
    # workgroups walk more than one tile under every id
    "walk": (2, 25, 22, 24, 264, 3, 1, 1, RELU, 0),
    # the shapes of the view cases' dense twins, also for the direct ids
    "pw64": (1, 17, 13, 64, 72, 1, 1, 0, NONE, 0),
    "pw128": (2, 12, 12, 128, 128, 1, 1, 0, RELU, AFTER),
    # the one pointwise shape id 70 (two K steps of 128 in registers) admits: 128 < Cin <= 256; 200 outputs: four channel groups, the last ragged
    "pw256": (2, 11, 9, 256, 200, 1, 1, 0, RELU, BEFORE),
}
EXACT = [Problem("exact", tag, *s) for tag, s in _SHAPES.items()]
SILU_TAGS = ("taps", "s2wrap", "walk")
SILU_PROBLEMS = [Problem("silu", tag, *_SHAPES[tag][:8], SILU, _SHAPES[tag][9]) for tag in SILU_TAGS]


def twins(cfg):
    """the fp8 view cases whose dense launch runs under `cfg`: (name, case); operands case.x_dense() / case.operands()"""
    if V.EXPECT["slices8/fp8"][cfg] != V.RUNS:
        return []
    return [("twin-" + c.tag, c) for c in V.cases_of("slices8/fp8", cfg)]


def twin_expected(case):
    return q8(case.reference())


# ---- the comparisons: a message, or None where the output passes ------------------------------------------------------------------------
def exact_mismatch(y, ref):
    """section "exact": np.array_equal, and where it fails the first differing (pixel, channel)"""
    y = np.asarray(y)
    if y.shape != ref.shape:
        return "shape %s, expected %s" % (y.shape, ref.shape)
    if np.array_equal(y, ref):
        return None
    bad = ~(y == ref)
    m, n = np.argwhere(bad)[0]
    return "%d of %d outputs differ; first at pixel %d, channel %d: got %r, expected %r" % (bad.sum(), bad.size, m, n, float(y[m, n]), float(ref[m, n]))


GATE = dict(rtol=0.126, atol=2.0 ** -9)       # one e4m3 ulp (tests/test_gpu_fp8.py)
SAME_MIN = 0.97


def gate_mismatch(y, ref):
    """step 1 of the fp8 ladder: finite, >= 97 % of the bytes identical, never more than one e4m3 ulp away"""
    y = np.asarray(y)
    if y.shape != ref.shape:
        return "shape %s, expected %s" % (y.shape, ref.shape)
    if not np.isfinite(y).all():
        m, n = np.argwhere(~np.isfinite(y))[0]
        return "%d outputs are not finite; first at pixel %d, channel %d" % ((~np.isfinite(y)).sum(), m, n)
    same = float((y == ref).mean())
    if same < SAME_MIN:
        return "%.4f of the outputs identical, %.2f wanted" % (same, SAME_MIN)
    far = ~np.isclose(y, ref, **GATE)
    if far.any():
        m, n = np.argwhere(far)[0]
        return "%d outputs more than one e4m3 ulp away; first at pixel %d, channel %d: got %r, expected %r" % (far.sum(), m, n, float(y[m, n]), float(ref[m, n]))
    return None
