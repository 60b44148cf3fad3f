"""Cases, buffers and float64 references for the kernels that open a detector pass, as single launches: stem_direct_kernel<CT, U8> (CT = 1 .. 4),
stem_direct_wide_kernel<5, U8> and front_fused_kernel<U8, false, RS> (layers 0 + 1).  tests/test_gpu_front_kernels.py launches every case through
vc_stem_host / vc_front_fused_host; tests/test_front_cases.py holds this module to its own conditions on the CPU.

Operands: the tensor input is seeded standard normal rounded to bf16, frames are uniform random bytes (every tap of every pixel matters), weights
N(0, 1 / fan-in) rounded to bf16 (the stem's times STEM_GAIN), biases 0.1 N(0, 1); every output element starts as SENTINEL (the e4m3 view: the
byte Q_SENTINEL).

Reference: oracle.imageops.letterbox (integer-exact) -> exact / 255 in float32 -> RNE to bf16; the stem in float64 -> SiLU -> bf16; for the front
zero padding -> 3 x 3 / s2 in float64 -> SiLU.  `emulation` is the same chain with float32 convolutions.  The e4m3 reference is the project's
definition tests/test_gpu_fp8.py::q8 applied to the kernel's own bf16 output times inv_scale.

Sizes are NETWORK tensors (b, net_h, net_w).  The stem's tiles are 8 x 32 outputs on a 20 x 34-pair patch, the front's 16 x 16 layer-1 outputs on a
33 x 33 layer-0 region and a 70 x 35-pair patch; STEM_SHAPES / FRONT_SHAPES hold the smallest tensors that reach each geometry class (the predicates
say which)."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from aux_cases import SENTINEL, rnd
from conv_view_cases import GATE, IDS_IGEMM
from oracle import imageops as oi
from test_gpu_fp8 import q8

SEED = 1                         # bump only if test_front_cases.py::test_emulation_inside_the_gate says a case sits on a rounding tie
Q_SENTINEL = 0xC3                # the e4m3 view before the launch
STEM_TH, STEM_TW = 8, 32
FF_TH, FF_TW = 16, 16
FF_PR, FF_PC = 70, 35            # input patch rows / pixel pairs of a front tile
FF_RS_CHUNKS = 8 * 8 * 64        # FF_RS_NRAW * FF_NW * 64: 16-byte chunks a tile may stage in resize mode
FF_L0_BYTES = 16 * 71 * 16 * 4   # sizeof(l0t): the staging area
STEM_COUTS = (16, 32, 48, 64, 80)
STEM_SHAPES = ((1, 2, 2), (1, 16, 64), (1, 14, 66), (1, 18, 62), (3, 34, 130))
FRONT_SHAPES = ((1, 4, 4), (1, 64, 64), (1, 60, 68), (1, 68, 60), (1, 32, 96), (1, 34, 70), (3, 68, 132))

# geometry classes by predicate on the OUTPUT map (Ho, Wo) of a kernel with th x tw tiles
CLASSES = {
    "one output pixel": lambda B, H, W, th, tw: H == 1 and W == 1,
    "exactly one tile": lambda B, H, W, th, tw: B == 1 and H == th and W == tw,
    "a row short, a column over": lambda B, H, W, th, tw: B == 1 and H == th - 1 and W == tw + 1,
    "a row over, a column short": lambda B, H, W, th, tw: B == 1 and H == th + 1 and W == tw - 1,
    "several frames of several tiles, one over on both sides": lambda B, H, W, th, tw: B == 3 and H % th == 1 and W % tw == 1 and H > th and W > tw,
}


def stem_out(nh, nw):
    return nh // 2, nw // 2


def front_out(nh, nw):
    h0, w0 = stem_out(nh, nw)
    return (h0 - 1) // 2 + 1, (w0 - 1) // 2 + 1


def ntiles(kind, net):
    B, nh, nw = net
    (H, W), (th, tw) = (stem_out(nh, nw), (STEM_TH, STEM_TW)) if kind == "stem" else (front_out(nh, nw), (FF_TH, FF_TW))
    return B * (-(-H // th)) * (-(-W // tw))


def caps_of(units):
    return (0, 1, 2, 3) if units >= 4 else (0,)


def silu(t):
    return t * torch.sigmoid(t)


def _rng(key):
    return np.random.default_rng(zlib.crc32(repr((SEED,) + tuple(key)).encode()))


# ---- the letterbox geometry and the launchers' predicates, restated (engine_run.hip::letterbox_geom, stem_direct.hip, front_fused.hip) --------------
class Geom:
    def __init__(self, h, w, nh, nw):
        self.src_h, self.src_w, self.net_h, self.net_w = h, w, nh, nw
        self.unpad_w, self.unpad_h, self.top, self.bottom, self.left, self.right = oi.letterbox_geometry(h, w, nh, nw)

    @property
    def same_scale(self):
        """the kernels read the frame's own pixels: no resize, whole pixel pairs, 2-byte aligned pair reads"""
        return self.unpad_h == self.src_h and self.unpad_w == self.src_w and self.src_w % 2 == 0 and self.left % 2 == 0


def rs_plan(g):
    """front_rs_plan: (source rows, 16-byte chunks per row) a tile stages in resize mode, or None when the launcher refuses the geometry"""
    if g.unpad_h < 1 or g.unpad_w < 1 or g.net_h % 4 or g.net_w % 4:
        return None
    y0, y1, _ = oi._v_tables(g.src_h, g.unpad_h)
    x0, x1, _ = oi._h_tables(g.src_w, g.unpad_w)
    H1, W1 = g.net_h // 4, g.net_w // 4
    rows, nbytes = 1, 16
    for ty in range(-(-H1 // FF_TH)):
        gy0 = 2 * ty * FF_TH - 1
        u0 = min(max(2 * gy0 - 2 - g.top, 0), g.unpad_h - 1)
        u1 = min(max(2 * gy0 - 2 + FF_PR - 1 - g.top, 0), g.unpad_h - 1)
        rows = max(rows, int(y1[u1] - y0[u0] + 1))
    for tx in range(-(-W1 // FF_TW)):
        gx0 = 2 * tx * FF_TW - 1
        u0 = min(max(2 * (gx0 - 1) - g.left, 0), g.unpad_w - 1)
        u1 = min(max(2 * (gx0 - 1) + 2 * FF_PC - 1 - g.left, 0), g.unpad_w - 1)
        nbytes = max(nbytes, int(x1[u1] - x0[u0] + 1) * 3 + 15)
    chunks = (nbytes + 15) // 16
    return (rows, chunks) if rows * chunks <= FF_RS_CHUNKS and rows * chunks * 16 <= FF_L0_BYTES else None


def instance_of(kind, cout, g):
    """the kernel instance launch_stem_direct[_u8] / launch_front_fused selects for a geometry (g None: the tensor input), or the reason it refuses"""
    if kind == "stem":
        name = "stem_direct_wide_kernel<5,%s>" if cout == 80 else "stem_direct_kernel<%d,%%s>" % (cout // 16)
        if g is None:
            return name % "false"
        return name % "true" if g.same_scale else "refused: not a same-scale geometry"
    if g is None:
        return "front_fused_kernel<false>"
    if g.same_scale:
        return "front_fused_kernel<true>"
    return "front_fused_kernel<true,false,true>" if rs_plan(g) else "refused: the resize does not fit the staging area"


# ---- operands and references -------------------------------------------------------------------------------------------------------------
def _w(rng, cout, cin, k):
    return rnd(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k), "bf16")


def _b(rng, n):
    return (rng.standard_normal(n) * 0.1).astype(np.float32)


# Gain of the stem's weights over N(0, 1 / fan-in), by input kind, so that at least half of every output map -- the 16 to 80 values of a
# one-pixel map included -- lies outside |SiLU| < 0.1: 2 for the normal tensor; 4 for frames, whose tensor of uniform bytes / 255 has a standard
# deviation of 0.29 (0.14 behind a 2 : 1 down-scale) against the normal tensor's 1.  Powers of two: the weights stay bf16 values.
STEM_GAIN = {False: 2.0, True: 4.0}


@functools.lru_cache(maxsize=None)
def _weights(kind, cout, u8=False):
    """a function of the kernel, its width and the input kind alone: every shape, view and grid cap sees the same weights"""
    rng = _rng(("w", kind, cout))
    o = {"w0": _w(rng, cout if kind == "stem" else 32, 3, 6) * np.float32(STEM_GAIN[u8]), "b0": _b(rng, cout if kind == "stem" else 32)}
    if kind == "front":
        o.update(w1=_w(rng, cout, 32, 3), b1=_b(rng, cout))
    for a in o.values():
        a.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _input(net, src):
    """src None: the tensor (b, nh, nw, 3), normals rounded to bf16; src (h, w, swap_rb): frames (b, h, w, 3) of random bytes"""
    rng = _rng(("x", net, src))
    B, nh, nw = net
    a = rnd(rng.standard_normal((B, nh, nw, 3)), "bf16") if src is None else rng.integers(0, 256, (B, src[0], src[1], 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tensor_of(net, src):
    """the letterboxed tensor (b, nh, nw, 3) the kernels compute on, bf16 values as float32"""
    a = _input(net, src)
    if src is None:
        return a
    B, nh, nw = net
    out = np.empty((B, nh, nw, 3), np.float32)
    for f in range(B):
        im = a[f][:, :, ::-1] if src[2] else a[f]                       # R and B exchange inside the image; the padding (114) is symmetric
        lb = oi.letterbox(np.ascontiguousarray(im), nh, nw)
        assert lb.shape == (nh, nw, 3), (lb.shape, net, src)
        out[f] = rnd(lb.astype(np.float32) / np.float32(255), "bf16")
    out.setflags(write=False)
    return out


def _chain(kind, cout, net, src, dt, l0_pad=None):
    """the kernel's function in dtype dt (float64: the reference, float32: the emulation), NCHW before the last rounding.  l0_pad (front): what
    surrounds layer 0 instead of zeros, per channel"""
    o = {k: torch.as_tensor(np.array(v)).to(dt) for k, v in _weights(kind, cout, src is not None).items()}
    bf = lambda t: t.float().bfloat16().to(dt)                          # where the unfused graph stores a tensor
    x = torch.as_tensor(np.array(tensor_of(net, src))).to(dt).permute(0, 3, 1, 2)
    l0 = silu(F.conv2d(x, o["w0"], o["b0"], stride=2, padding=2))
    if kind == "stem":
        return l0
    l0 = bf(l0)
    if l0_pad is None:
        return silu(F.conv2d(l0, o["w1"], o["b1"], stride=2, padding=1))
    B, C, H0, W0 = l0.shape
    p = l0_pad.to(dt).view(1, C, 1, 1).expand(B, C, H0 + 2, W0 + 2).clone()
    p[:, :, 1:-1, 1:-1] = l0
    return silu(F.conv2d(p, o["w1"], o["b1"], stride=2))


def _flat(t):
    r = t.permute(0, 2, 3, 1)
    return r.reshape(-1, r.shape[-1]).numpy()


@functools.lru_cache(maxsize=None)
def _reference(kind, cout, net, src):
    r = _flat(_chain(kind, cout, net, src, torch.float64))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _emulation(kind, cout, net, src):
    r = rnd(_flat(_chain(kind, cout, net, src, torch.float32)), "bf16")
    r.setflags(write=False)
    return r


def halo_of_bias(cout, net, src):
    """the front with layer 0's zero padding replaced by SiLU(bias) -- what a halo that skips the `inside` test holds -- as bf16, (npix, cout)"""
    b0 = torch.as_tensor(np.array(_weights("front", cout, src is not None)["b0"])).double()
    return rnd(_flat(_chain("front", cout, net, src, torch.float64, l0_pad=silu(b0).float().bfloat16())).astype(np.float32), "bf16")


def gate_ratio(got, ref64):
    """worst |got - ref| / (atol + rtol |ref|) against the reference as bf16 holds it: <= 1 is what assert_allclose(**GATE["bf16"]) accepts"""
    ref = rnd(ref64.astype(np.float32), "bf16").astype(np.float64)
    return float((np.abs(got.astype(np.float64) - ref) / (GATE["bf16"]["atol"] + GATE["bf16"]["rtol"] * np.abs(ref))).max())


def e4m3_bytes(values):
    """float values e4m3 represents -> their bytes"""
    return torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def q8_reference(y, inv_scale):
    """the e4m3 view of a bf16 output y: q8(y * inv_scale), the product formed in float32 as the kernel forms it; bytes"""
    return e4m3_bytes(q8(np.asarray(y, np.float32) * np.float32(inv_scale)))


class Case:
    """One launch: kernel ("stem" / "front"), its width (stem: cout, front: layer 1's), the network tensor (b, nh, nw), the input kind
    (src None = the tensor, (h, w, swap_rb) = u8 frames), the output view, the e4m3 view (stem; q = (q_cs, q_co, inv_scale)) and a grid cap."""

    def __init__(self, kind, cout, net, src=None, view="dense", out_cs=None, out_co=0, q=None, grid=0, reason=None, message=""):
        self.kind, self.cout, self.net, self.src, self.view, self.q, self.grid = kind, cout, tuple(net), src, view, q, grid
        self.reason, self.message = reason, message
        self.out_cs, self.out_co = (out_cs if out_cs is not None else cout), out_co
        self.geom = None if src is None else Geom(src[0], src[1], net[1], net[2])
        self.instance = instance_of(kind, cout, self.geom)
        s = "t" if src is None else "u%dx%d%s" % (src[0], src[1], "s" if src[2] else "")
        qn = "" if q is None else "-q%d.%d.%s" % (q[0], q[1], ("%.3g" % q[2]))
        self.name = "%s%d-%dx%dx%d-%s-%s%s-g%d" % ((kind, cout) + self.net + (s, view, qn, grid))

    @property
    def out_hw(self):
        return stem_out(*self.net[1:]) if self.kind == "stem" else front_out(*self.net[1:])

    @property
    def npix(self):
        return self.net[0] * self.out_hw[0] * self.out_hw[1]

    @property
    def units(self):
        return ntiles(self.kind, self.net)

    def problem(self):
        return (self.kind, self.cout, self.net, self.src)

    def twin_key(self):
        """the launch_conv chain does not depend on the grid cap"""
        return self.problem() + (self.out_cs, self.out_co, self.q)

    @property
    def twin_same_store_path(self):
        """launch_conv keeps conv_epilogue_fast_bf16's 16-byte store: every output offset is 8-aligned and whole 8-channel groups are stored"""
        return self.out_cs % 8 == 0 and self.out_co % 8 == 0 and self.cout % 8 == 0

    def weights(self):
        o = _weights(self.kind, self.cout, self.src is not None)
        return [np.array(o[n]) for n in (("w0", "b0") if self.kind == "stem" else ("w0", "b0", "w1", "b1"))]

    def input(self):
        return np.array(_input(self.net, self.src))

    def view_dict(self, mode=1):
        v = dict(out_co=self.out_co, mode=mode, grid_cap=self.grid if mode else 0, swap_rb=self.src[2] if self.src else 0)
        if self.q:
            v.update(q_co=self.q[1], inv_scale=self.q[2])
        return v

    def buffers(self):
        """y and the e4m3 view (or None) as the launch gets them: the sentinel everywhere"""
        H, W = self.out_hw
        y = np.full((self.net[0], H, W, self.out_cs), SENTINEL, np.float32)
        q = np.full((self.net[0], H, W, self.q[0]), Q_SENTINEL, np.uint8) if self.q else None
        return y, q

    def written(self, y):
        return y[..., self.out_co:self.out_co + self.cout].reshape(-1, self.cout)

    def written_q(self, q):
        return q[..., self.q[1]:self.q[1] + self.cout].reshape(-1, self.cout)

    def untouched_ok(self, y, q):
        """every element outside the written slices still holds the sentinel"""
        keep = np.ones(y.shape, bool)
        keep[..., self.out_co:self.out_co + self.cout] = False
        ok = bool((y[keep] == SENTINEL).all())
        if self.q:
            keep = np.ones(q.shape, bool)
            keep[..., self.q[1]:self.q[1] + self.cout] = False
            ok = ok and bool((q[keep] == Q_SENTINEL).all())
        return ok and (q is None) == (self.q is None)

    def reference(self):
        return _reference(*self.problem())

    def emulation(self):
        return _emulation(*self.problem())


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def _stem_cases():
    cases = []
    ragged = [s for s in STEM_SHAPES if s[0] == 1 and s[1] // 2 not in (1, STEM_TH)]
    for co in STEM_COUTS:
        for net in STEM_SHAPES:
            same = (net[1], net[2], 0)
            for src in (None, same):                                     # the tensor; frames of the tensor's own size
                for g in caps_of(ntiles("stem", net)):
                    cases.append(Case("stem", co, net, src, grid=g))
                if net in ragged or net[0] > 1:
                    cases.append(Case("stem", co, net, src, "slice8", out_cs=co + 16, out_co=8))
        one = (1, 16, 64)
        for swap in (0, 1):
            cases.append(Case("stem", co, one, (12, 64, swap)))         # pad rows above and below
            cases.append(Case("stem", co, one, (16, 60, swap)))         # an even left pad
        cases.append(Case("stem", co, one, (16, 64, 1)))
    for co in (32, 64):                                                  # the e4m3 view of the fp8 engine's stem
        for net in ragged:
            for src in (None, (net[1], net[2], 0)):
                cases.append(Case("stem", co, net, src, q=(co, 0, 1.0)))
                for inv in (1.0, 0.5, 1.0 / 3.0):
                    cases.append(Case("stem", co, net, src, "slice8", out_cs=co + 16, out_co=8, q=(co + 16, 8, inv)))
    return cases


# frames that take the front's resize instance, by network tensor: (h, w) -> why
RESIZE_FRAMES = {
    (1, 64, 64): {(64, 62): "same scale, odd left pad", (64, 63): "same scale, odd source width", (96, 50): "portrait: pads left and right"},
    (1, 60, 68): {(120, 136): "2 : 1 down-scale", (45, 51): "4 / 3 up-scale, row stride 153 bytes"},
    (1, 4, 4): {(8, 8): "2 : 1 down-scale of a frame one tile covers"},
    (1, 32, 96): {(64, 192): "2 : 1 down-scale"},
    (3, 68, 132): {(136, 264): "2 : 1 down-scale, several tiles per frame"},
}


def _front_cases():
    cases = []
    for net in FRONT_SHAPES:
        same = (net[1], net[2], 0)
        for src in (None, same):
            for g in caps_of(ntiles("front", net)):
                cases.append(Case("front", 64, net, src, grid=g))
            if net[1] % 32 or net[2] % 32:
                cases.append(Case("front", 64, net, src, "slice8", out_cs=96, out_co=8))
        for (h, w) in RESIZE_FRAMES.get(net, {}):
            for b in sorted({1, 3} | {net[0]}):
                n = (b,) + net[1:]
                for g in caps_of(ntiles("front", n)):
                    cases.append(Case("front", 64, n, (h, w, 0), grid=g))
            cases.append(Case("front", 64, net, (h, w, 1)))
    one = (1, 64, 64)
    for swap in (0, 1):
        cases.append(Case("front", 64, one, (56, 64, swap)))            # pad rows above and below
        cases.append(Case("front", 64, one, (64, 60, swap)))            # an even left pad
    cases.append(Case("front", 64, one, (64, 64, 1)))
    return cases


def _refusals():
    quiet = ""
    return [
        Case("stem", 32, (1, 16, 64), (16, 62, 0), reason="refused: not a same-scale geometry", message=quiet),     # an odd left pad
        Case("stem", 32, (1, 16, 64), (16, 63, 0), reason="refused: not a same-scale geometry", message=quiet),     # an odd source width
        Case("stem", 80, (1, 14, 66), None, q=(80, 0, 1.0), reason="no e4m3 view at 80 channels", message=quiet),
        Case("stem", 32, (1, 14, 66), None, "q_co4", q=(40, 4, 1.0), reason="e4m3 view not 8-aligned",
             message="stem_direct: the e4m3 view (stride 40, offset 4) must be 8-channel aligned"),
        Case("front", 64, (1, 64, 68), (192, 204, 0), reason="refused: the resize does not fit the staging area",
             message="front_fused: the resize geometry 192x204 -> 64x68 does not fit the staging area"),
        Case("front", 64, (1, 60, 68), None, "out_co4", out_cs=72, out_co=4, reason="output slice not 8-aligned", message=quiet),
        Case("front", 48, (1, 60, 68), None, reason="layer 1 is not 32 -> 64", message=quiet),
    ]


def refusal_reasons(c):
    """the conditions of the case's launcher that its geometry, view or width trips (empty: the launcher takes it)"""
    why = []
    if c.instance.startswith("refused"):
        why.append(c.instance)
    if c.kind == "stem":
        if c.cout % 16 or not 16 <= c.cout <= 80 or c.out_cs % 8 or c.out_co % 8:
            why.append("stem_direct_applicable")
        if c.q and c.cout == 80:
            why.append("no e4m3 view at 80 channels")
        elif c.q and (c.q[0] % 8 or c.q[1] % 8):
            why.append("e4m3 view not 8-aligned")
    else:
        if c.cout != 64:
            why.append("layer 1 is not 32 -> 64")
        if c.out_cs % 8 or c.out_co % 8:
            why.append("output slice not 8-aligned")
    return why


STEM_CASES = _stem_cases()
FRONT_CASES = _front_cases()
CASES = STEM_CASES + FRONT_CASES
REFUSALS = _refusals()
# one ragged case per stem width for the sweep over every implicit-GEMM id
IGEMM_SWEEP = [c for c in STEM_CASES if c.net == (1, 14, 66) and c.src is None and c.view == "dense" and c.q is None and c.grid == 0]


def kernel_of(c):
    return c.instance.split("<")[0] if c.kind == "front" else ("stem_direct_wide_kernel" if c.cout == 80 else "stem_direct_kernel")
