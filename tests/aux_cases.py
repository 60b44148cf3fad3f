"""Inputs and CPU references for the kernels between the convolutions (aux_kernels.hip, reid_stem.hip): the SPPF pooling kernels, the
nearest upsample, MaxPool2d(3, 2, 1), AvgPool + L2 norm, the NCHW -> NHWC-pad layout kernel, the bf16 -> fp8 cast and the fused ReID stem.

All of them select, copy or round to nearest even, so every input here is a value the element type represents (f32, bf16, e4m3fn) and
every comparison but AvgPool + L2 is exact.  Inputs are finite: NaNs are outside the kernels' contract.

SPPF: the reference is three DIRECT window maxima of radius 2, 4 and 6 with -inf padding (not the chained 5 x 5 form the kernels
use).  Channel j of a plane is drawn by j % 4: 0 = strictly negative everywhere (a pad of 0 instead of -inf would win), 1 = mixed signs
with +-0, the smallest subnormal and the largest finite value planted, 2 = only +-0 and +-subnormal, 3 = plain mixed signs.  The buffer
has sentinel channels before and after the four slices and the sentinel in the three output slices.

`sppf_rule` restates the steering of launch_sppf_pool; tests/test_aux_cases.py pins it to the hand-derived anchors and asserts that the
table reaches every branch and every slice width, tests/test_gpu_aux_kernels.py asserts the launcher reports the same."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

ES = {"f32": 4, "bf16": 2, "fp8": 1}
PRECISIONS = ("f32", "bf16", "fp8")
SENTINEL = 96.0          # representable in all three types; no input value equals it
SUB = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "fp8": 2.0 ** -9}                    # smallest subnormal
BIG = {"f32": float(np.finfo(np.float32).max), "bf16": float(np.float32(2.0 ** 127 * (2 - 2.0 ** -7))), "fp8": 448.0}   # largest finite


def rnd(x, precision):
    """float32 array of the nearest values `precision` represents (fp8 saturates at +-448)"""
    with np.errstate(over="ignore"):
        t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    if precision == "bf16":
        t = t.bfloat16().float()
    elif precision == "fp8":
        t = t.clamp(-448, 448).to(torch.float8_e4m3fn).float()
    return t.numpy()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def plane_values(rng, shape, precision):
    """(B, H, W, C) of representable values, channel j drawn by j % 4 as the module docstring says"""
    sub, big = np.float32(SUB[precision]), np.float32(BIG[precision])
    x = rnd(rng.standard_normal(shape) * 2.0, precision)
    x[x == SENTINEL] = 1.0
    special = np.array([0.0, -0.0, sub, -sub, big, -big], np.float32)
    for j in range(shape[3]):
        v = x[..., j]
        if j % 4 == 0:
            v[...] = -np.abs(v)
            v[v == 0] = -1.0
        elif j % 4 == 1:
            flat = v.reshape(-1)
            pos = np.flatnonzero(rng.random(flat.size) < 0.3)
            flat[pos] = special[np.arange(len(pos)) % 6]
        elif j % 4 == 2:
            v[...] = special[rng.integers(0, 4, v.shape)]
    return x


# ---- SPPF ----------------------------------------------------------------------------------------------------------------------
def sppf_rule(H, W, C, precision, form):
    """(kernel, ws) launch_sppf_pool picks, or None where it refuses: its `for (int cand ...)` loops restated"""
    es, maxd = ES[precision], max(H, W)
    if C % 4:
        return None
    if form == 1 and maxd <= 40:
        for cand in (32, 16, 8, 4):
            rs = W * cand + ((cand - (W * cand) % 64) % 64 + 64) % 64
            if C % (cand * 4 // es) == 0 and maxd * cand <= (320 if maxd > 20 else 640) and H * rs * 4 <= 56 * 1024:
                return "sep", cand
    plane = 2 * H * W * 4
    for cand in (16, 8, 4):
        if plane * cand <= 76 * 1024 and C % (cand * 4 // es) == 0:
            return "wide", cand
    if plane * 4 <= 150 * 1024 and C % (16 // es) == 0:
        return "wide", 4
    if precision == "fp8":
        return "fp8", 1
    if C % (4 if precision == "f32" else 8):
        return None
    return "plain", 4


class SppfCase:
    """name, shape (B, H, W), precision, C, form, expect = (kernel, ws); cs / co of the buffer"""

    def __init__(self, shape, precision, C, form):
        self.shape, self.precision, self.C, self.form = shape, precision, C, form
        self.name = "%dx%dx%d-%s-c%d-form%d" % (*shape, precision, C, form)
        self.co, self.cs = 16, 4 * C + 32
        self.expect = sppf_rule(shape[1], shape[2], C, precision, form)

    def x(self):
        return plane_values(_rng(self.name), (*self.shape, self.C), self.precision)

    def buffer(self):
        buf = np.full((*self.shape, self.cs), SENTINEL, np.float32)
        buf[..., self.co:self.co + self.C] = self.x()
        return buf


SPPF_SHAPES = [(1, 1, 1), (1, 1, 20), (2, 20, 1), (1, 2, 3), (2, 5, 6), (1, 7, 13), (3, 12, 20), (2, 20, 12), (1, 20, 20), (1, 21, 9), (1, 24, 40),
               (2, 40, 40)]


def sppf_widths(shape):
    """channel counts of a shape in 32-bit words of a pixel: every slice width the register form can take at that side, and, where
    B > 1, a count that makes two channel groups of the widest"""
    if max(shape[1], shape[2]) <= 20:
        return (32, 16, 8, 4) + ((64,) if shape[0] > 1 else ())
    return (16, 4) if shape[0] > 1 else (8, 4)


@functools.lru_cache(maxsize=None)
def sppf_cases():
    cases = []
    for form in (1, 0):
        for shape in SPPF_SHAPES:
            for p in PRECISIONS:
                cases += [SppfCase(shape, p, words * 4 // ES[p], form) for words in sppf_widths(shape)]
    for p in PRECISIONS:
        cases += [SppfCase((1, 41, 17), p, words * 4 // ES[p], 1) for words in (16, 4)]       # a side above 40 falls through to the LDS form
        cases += [SppfCase((1, 60, 70), p, words * 4 // ES[p], 0) for words in (8, 4)]        # 131 KB of dynamic LDS
    cases += [SppfCase((1, 70, 70), p, 8, 1) for p in ("f32", "bf16")]                           # 4900 positions: no LDS form takes it
    cases += [SppfCase((1, 5, 6), "fp8", 8, 1), SppfCase((1, 70, 70), "fp8", 16, 1)]             # C % 16 != 0; a plane too large
    return {c.name: c for c in cases}


def window_max(x, r):
    """direct (2r + 1)^2 window maximum of (B, H, W, C) with -inf padding"""
    B, H, W, C = x.shape
    p = np.full((B, H + 2 * r, W + 2 * r, C), -np.inf, x.dtype)
    p[:, r:r + H, r:r + W] = x
    out = np.full(x.shape, -np.inf, x.dtype)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            np.maximum(out, p[:, dy:dy + H, dx:dx + W], out=out)
    return out


@functools.lru_cache(maxsize=None)
def sppf_ref(name):
    """the three output slices of a case, (B, H, W, 3C)"""
    x = sppf_cases()[name].x()
    return np.concatenate([window_max(x, r) for r in (2, 4, 6)], axis=-1)


def sppf_chained(x):
    """MaxPool2d(5, 1, 2) applied three times in float64 (the model's own formulation)"""
    t = torch.as_tensor(x).permute(0, 3, 1, 2).double()
    outs = []
    for _ in range(3):
        t = F.max_pool2d(t, 5, 1, 2)
        outs.append(t.permute(0, 2, 3, 1).numpy())
    return np.concatenate(outs, axis=-1)


# ---- upsample, max-pool, layout -------------------------------------------------------------------------------------------------
UPSAMPLE_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 20, 20)]
UPSAMPLE_C, UPSAMPLE_CS, UPSAMPLE_CO = 16, 48, 16          # 16 channels: one fp8 vector, two bf16, four f32


def upsample_input(shape, precision):
    return plane_values(_rng("up%s%s" % (shape, precision)), (*shape, UPSAMPLE_C), precision)


def upsample_ref(x):
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


MAXPOOL_SHAPES = [(2, 50, 50), (1, 25, 25), (2, 6, 7), (1, 2, 2), (3, 1, 1)]
MAXPOOL_C, MAXPOOL_CS, MAXPOOL_CO = 8, 24, 8


def maxpool_input(shape, precision):
    return plane_values(_rng("mp%s%s" % (shape, precision)), (*shape, MAXPOOL_C), precision)


def maxpool_ref(x):
    t = torch.as_tensor(x).permute(0, 3, 1, 2).double()
    return F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).numpy()


LAYOUT_SHAPES = [(1, 3, 50, 50), (3, 3, 50, 50), (3, 3, 5, 7)]


def layout_input(shape):
    """float32 values that bf16 does NOT represent (the kernel rounds), with +-0, f32 subnormals and bf16 rounding ties planted"""
    rng = _rng("layout%s" % (shape,))
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    tie_even, tie_odd = np.float32(1.0 + 2.0 ** -8), np.float32(1.0 + 3 * 2.0 ** -8)          # halfway between two bf16 values
    flat[:8] = [0.0, -0.0, 2.0 ** -149, -2.0 ** -140, tie_even, tie_odd, -tie_even, -tie_odd]
    return x


def layout_ref(x, precision):
    cpad = 4 if precision == "f32" else 8
    k, c, h, w = x.shape
    out = np.zeros((k, h, w, cpad), np.float32)
    out[..., :c] = x.transpose(0, 2, 3, 1)
    return out if precision == "f32" else torch.as_tensor(out).bfloat16().float().numpy()


# ---- bf16 -> fp8 ----------------------------------------------------------------------------------------------------------------
FP8_INV_SCALES = (1.0, 0.5, 16.0, 1.0 / 3.0)
FP8_C, FP8_SRC_CS, FP8_SRC_CO, FP8_DST_CS, FP8_DST_CO = 16, 32, 8, 48, 16


def all_bf16_values():
    """every bf16 bit pattern but the NaNs as float32, padded with zeros to a whole number of FP8_C-channel pixels: (npix, FP8_C)"""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7fff) <= 0x7f80]
    v = (bits << 16).view(np.float32)
    pad = -len(v) % FP8_C
    return np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, FP8_C)


def fp8_cast_ref(v, inv_scale):
    """the definition tests/test_gpu_fp8.py::q8 uses: the float32 product, clipped to +-448, rounded to nearest even; as float32"""
    with np.errstate(over="ignore"):
        p = np.clip(v.astype(np.float32) * np.float32(inv_scale), -448, 448)
    return torch.as_tensor(p).to(torch.float8_e4m3fn).float().numpy()


def e4m3_values(b):
    """uint8 array of e4m3fn bytes -> float32"""
    return torch.as_tensor(np.ascontiguousarray(b, dtype=np.uint8)).view(torch.float8_e4m3fn).float().numpy()


# ---- ReID stem ------------------------------------------------------------------------------------------------------------------
REID_STEM_K = (1, 3, 60)          # 60 x 13 = 780 items > the grid of 704: some workgroups take a second item


@functools.lru_cache(maxsize=None)
def reid_stem_input(k):
    rng = _rng("stem%d" % k)
    x = np.stack([rng.standard_normal((50, 50, 3)) * (0.5 + i % 4) for i in range(k)]).astype(np.float32)    # differs per crop
    w = (rng.standard_normal((64, 3, 3, 3)) / np.sqrt(27.0)).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    return x, w, b


def pool3s2_nhwc(y):
    return maxpool_ref(y).astype(np.float32)


def reid_stem_ref(k):
    """tests/test_gpu_kernels.py::torch_conv (float64 conv on bf16-rounded operands, ReLU, one rounding to bf16), then MaxPool2d(3, 2, 1)"""
    from test_gpu_kernels import torch_conv
    x, w, b = reid_stem_input(k)
    return pool3s2_nhwc(torch_conv(x, w, b, 1, 1, 2, None, 0, "bf16"))


# ---- AvgPool + L2 ---------------------------------------------------------------------------------------------------------------
AVGPOOL_CASES = [(1, 4, 4), (5, 4, 4), (2, 2, 3)]
U = 2.0 ** -24


def avgpool_input(case, precision):
    """crop 0: plain; crop 1: channel means of about 1 / 30 of the mean magnitude (cancellation); crop 2: x 1e3; crop 3: x 1e-3;
    crop 4: plain with an offset.  No all-zero crop."""
    k, h, w = case
    rng = _rng("avg%s" % (case,))
    x = rng.standard_normal((k, h, w, 512))
    if k > 1:
        x[1] = x[1] - x[1].mean(axis=(0, 1)) + rng.standard_normal(512) * 0.03
    if k > 2:
        x[2] *= 1e3
    if k > 3:
        x[3] *= 1e-3
    if k > 4:
        x[4] += 0.5
    return rnd(x, precision)


def avgpool_ref(x):
    a = x.astype(np.float64).mean(axis=(1, 2))
    return a / np.sqrt((a * a).sum(axis=1, keepdims=True))


def avgpool_bound(x):
    """per output the first-order bound of tests/test_gpu_aux_kernels.py::test_avgpool_l2norm (its docstring derives it)"""
    x = x.astype(np.float64)
    n = x.shape[1] * x.shape[2]
    a = x.mean(axis=(1, 2))
    A = np.abs(x).mean(axis=(1, 2))
    na = np.sqrt((a * a).sum(axis=1, keepdims=True))
    y = np.abs(a) / na
    e = n * U * A
    return 1.001 * ((e + y * np.sqrt((e * e).sum(axis=1, keepdims=True))) / na + 7.5 * U * y)
