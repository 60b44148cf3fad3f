"""Cases, buffers and float64 references for the four fused block kernels as single launches: c3_fused_kernel (YOLOv5's first C3),
bneck_fused_kernel<false> / <true> (a 64-channel Bottleneck, and the one that also runs the block's cv3) and reid_block_fused_kernel (a
ReID BasicBlock).  tests/test_gpu_fused_blocks.py launches every case through vc_c3_fused_host / vc_bneck_fused_host /
vc_reid_block_fused_host; tests/test_fused_block_cases.py holds this module to its own conditions on the CPU.

Operands: seeded standard normal rounded to bf16 (both signs, no flat regions: two neighbouring pixels that swap differ), weights
N(0, 1 / K) rounded to bf16, biases 0.1 N(0, 1).  Poison: every element of a buffer a kernel reads that is not an operand is NaN -- the
channels around a slice and, under cv3, the m slice of the concat buffer, which the fused kernel neither reads nor writes -- and every
output element is SENTINEL.

Reference: float64 on the rounded operands, every intermediate rounded to bf16 where the unfused graph stores it; the 3x3 pads its own
input (b1, x, t) with zeros, not with the activation of a bias.  `emulation` is the same chain with float32 convolutions.

C3 / Bottleneck tiles are 8 x 16 output pixels on a 10 x 18 halo; SHAPES holds the smallest maps that reach each geometry class (the
predicates in CLASSES say which), every grid cap in caps_of makes 1, 2 or 3 workgroups walk all tiles or crops in one process."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from aux_cases import SENTINEL, rnd
from conv_view_cases import GATE

SEED = 1                         # bump only if test_fused_block_cases.py::test_emulation_inside_the_gate says a case sits on a rounding tie
TH, TW = 8, 16                   # C3_TH / BN_TH, C3_TW / BN_TW
REID_HW = 25                     # RB_HW
SHAPES = ((1, 1, 1), (5, 3, 5), (2, 8, 16), (3, 7, 17), (2, 9, 33), (1, 20, 28))
REID_K = (1, 2, 3, 7)

# geometry classes of a C3 / Bottleneck map, by predicate
CLASSES = {
    "a map of one pixel": lambda B, H, W: H == 1 and W == 1,
    "less than one tile per frame, more frames than tiles per frame": lambda B, H, W: 1 < H < TH and 1 < W < TW and B > 1,
    "exactly one tile per frame": lambda B, H, W: H == TH and W == TW,
    "one row short, one column over": lambda B, H, W: H % TH == TH - 1 and W % TW == 1 and W > TW,
    "one over on both sides": lambda B, H, W: H % TH == 1 and W % TW == 1 and H > TH and W > TW,
    "the product's own overhang (sides multiples of 4)": lambda B, H, W: H % 4 == 0 and W % 4 == 0 and H % TH != 0 and W % TW != 0 and H > TH and W > TW,
}


def ntiles(B, H, W):
    return B * (-(-H // TH)) * (-(-W // TW))


def caps_of(units):
    """grid caps of a case with `units` tiles or crops: 0 = the product's grid, then 1, 2 and 3 workgroups"""
    return (0, 1, 2, 3) if units >= 4 else (0, 1, 2)


def silu(t):
    return t * torch.sigmoid(t)


def _rng(key):
    return np.random.default_rng(zlib.crc32(repr((SEED,) + tuple(key)).encode()))


def _w(rng, cout, cin, k):
    return rnd(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k), "bf16")


def _b(rng, n):
    return (rng.standard_normal(n) * 0.1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _operands(kind, shape):
    """a function of (kernel family, shape) alone: every view, grid cap and the unfused twin of a problem see the same numbers"""
    rng = _rng((kind, shape))
    B, H, W = shape
    o = {"x": rnd(rng.standard_normal((B, H, W, 64)), "bf16")}
    if kind == "c3":
        o.update(w12=_w(rng, 64, 64, 1), b12=_b(rng, 64), wm1=_w(rng, 32, 32, 1), bm1=_b(rng, 32), wm2=_w(rng, 32, 32, 3), bm2=_b(rng, 32),
                 w3=_w(rng, 64, 64, 1), b3=_b(rng, 64))
    elif kind == "bneck":
        o.update(w1=_w(rng, 64, 64, 1), b1=_b(rng, 64), w2=_w(rng, 64, 64, 3), b2=_b(rng, 64), w3=_w(rng, 128, 128, 1), b3=_b(rng, 128),
                 y2=rnd(rng.standard_normal((B, H, W, 64)), "bf16"))
    else:
        o.update(w1=_w(rng, 64, 64, 3), b1=_b(rng, 64), w2=_w(rng, 64, 64, 3), b2=_b(rng, 64))
    for a in o.values():
        a.setflags(write=False)
    return o


def _chain(kind, shape, res, cv3, dt):
    """the block in dtype dt (float64: the reference, float32: the emulation), NCHW tensor before the last rounding"""
    o = {k: torch.as_tensor(np.array(v)).to(dt) for k, v in _operands(kind, shape).items()}
    nchw = lambda a: a.permute(0, 3, 1, 2)
    bf = lambda t: t.float().bfloat16().to(dt)                       # where the unfused graph stores a tensor
    x = nchw(o["x"])
    if kind == "c3":
        y12 = bf(silu(F.conv2d(x, o["w12"], o["b12"])))
        y1, y2 = y12[:, :32], y12[:, 32:]
        b1 = bf(silu(F.conv2d(y1, o["wm1"], o["bm1"])))
        m = bf(silu(F.conv2d(b1, o["wm2"], o["bm2"], padding=1)) + y1)
        return silu(F.conv2d(torch.cat([m, y2], 1), o["w3"], o["b3"]))
    if kind == "bneck":
        b1 = bf(silu(F.conv2d(x, o["w1"], o["b1"])))
        m = silu(F.conv2d(b1, o["w2"], o["b2"], padding=1))
        if res:
            m = m + x
        if not cv3:
            return m
        return silu(F.conv2d(torch.cat([bf(m), nchw(o["y2"])], 1), o["w3"], o["b3"]))
    t = bf(F.relu(F.conv2d(x, o["w1"], o["b1"], padding=1)))
    return F.relu(F.conv2d(t, o["w2"], o["b2"], padding=1) + x)


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, res, cv3):
    r = _chain(kind, shape, res, cv3, torch.float64).permute(0, 2, 3, 1)
    r = r.reshape(-1, r.shape[-1]).numpy()
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _emulation(kind, shape, res, cv3):
    r = _chain(kind, shape, res, cv3, torch.float32).permute(0, 2, 3, 1)
    r = rnd(r.reshape(-1, r.shape[-1]).numpy(), "bf16")
    r.setflags(write=False)
    return r


def gate_ratio(got, ref64):
    """worst |got - ref| / (atol + rtol |ref|) against the reference as bf16 holds it: <= 1 is what assert_allclose(**GATE["bf16"]) accepts"""
    ref = rnd(ref64.astype(np.float32), "bf16").astype(np.float64)
    return float((np.abs(got.astype(np.float64) - ref) / (GATE["bf16"]["atol"] + GATE["bf16"]["rtol"] * np.abs(ref))).max())


VIEW_FIELDS = ("in_cs", "in_co", "out_cs", "out_co", "z_cs", "z_co", "out_buf", "z_buf", "split")


class Case:
    """One launch: kernel family, (B, H, W), the block's switches (res, cv3), a named view (VIEW_FIELDS) and a grid cap."""

    def __init__(self, kind, shape, view, grid=0, res=0, cv3=0, reason=None, **vf):
        self.kind, self.shape, self.view, self.grid, self.res, self.cv3, self.reason = kind, tuple(shape), view, grid, int(res), int(cv3), reason
        if kind == "c3":
            self.res = 1                                             # the block has its shortcut
        self.v = dict(in_cs=64, in_co=0, out_cs=64, out_co=0, z_cs=128 if cv3 else 0, z_co=0, out_buf=0, z_buf=0, split=0)
        assert not set(vf) - set(self.v), vf
        self.v.update(vf)
        if self.v["out_buf"]:
            self.v["out_cs"] = self.v["in_cs"]
        if self.v["z_buf"]:
            self.v["z_cs"] = self.v["in_cs"] if self.v["z_buf"] == 1 else self.v["out_cs"]
        self.cout = 128 if cv3 else 64
        self.name = "%s%s%s-%dx%dx%d-%s-g%d" % ((kind, "+res" if res else "", "+cv3" if cv3 else "") + self.shape + (view, grid))

    @property
    def units(self):
        """tiles (C3, Bottleneck) or crops (ReID) the launch's workgroups share"""
        return self.shape[0] if self.kind == "reid" else ntiles(*self.shape)

    @property
    def npix(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    def problem(self):
        return (self.kind, self.shape, self.res, self.cv3)

    def twin_key(self):
        """the unfused chain does not depend on the grid cap"""
        return self.problem() + (self.view,)

    @property
    def twin_same_store_path(self):
        """check (d) applies: the unfused launches keep conv_epilogue_fast_bf16's 16-byte store, i.e. every output offset is 8-aligned"""
        v = self.v
        return v["out_cs"] % 8 == 0 and v["out_co"] % 8 == 0 and (not self.cv3 or (v["z_cs"] % 8 == 0 and v["z_co"] % 8 == 0))

    def operands(self):
        return _operands(self.kind, self.shape)

    def weights(self):
        o = self.operands()
        names = {"c3": ("w12", "b12", "wm1", "bm1", "wm2", "bm2", "w3", "b3"), "bneck": ("w1", "b1", "w2", "b2") + (("w3", "b3") if self.cv3 else ()),
                 "reid": ("w1", "b1", "w2", "b2")}[self.kind]
        ws = [np.array(o[n]) for n in names]
        return [w.reshape(w.shape[:2]) if w.ndim == 4 and w.shape[2] == 1 else w for w in ws]

    def view_dict(self, unfused=False):
        return dict(self.v, res=self.res if self.kind == "bneck" else 0, cv3=self.cv3, unfused=int(unfused), grid=0 if unfused else self.grid)

    def buffers(self):
        """x, y, z as the launch gets them (None where the view has none): operands in their slices, NaN in every other element a kernel could
        read, SENTINEL in every element of an output"""
        o, v = self.operands(), self.v
        B, H, W = self.shape
        x = np.full((B, H, W, v["in_cs"]), np.nan, np.float32)
        x[..., v["in_co"]:v["in_co"] + 64] = o["x"]
        y = z = None
        if not v["out_buf"]:
            y = np.full((B, H, W, v["out_cs"]), SENTINEL, np.float32)
        ybuf = x if v["out_buf"] else y
        if self.cv3:                                                 # y is the concat buffer, an INPUT: [m (never touched) | y2]
            if not v["out_buf"]:
                y[...] = np.nan
            ybuf[..., v["out_co"] + 64:v["out_co"] + 128] = o["y2"]
            if v["z_buf"] == 0:
                z = np.full((B, H, W, v["z_cs"]), SENTINEL, np.float32)
            else:
                zb = x if v["z_buf"] == 1 else ybuf
                free = np.isnan(zb[..., v["z_co"]:v["z_co"] + 128])
                zb[..., v["z_co"]:v["z_co"] + 128][free] = SENTINEL
        elif v["out_buf"]:
            free = np.isnan(x[..., v["out_co"]:v["out_co"] + 64])     # (an overlapping slice -- a refusal case -- keeps the operands)
            x[..., v["out_co"]:v["out_co"] + 64][free] = SENTINEL
        return x, y, z

    def _dest(self, x, y, z):
        """(buffer, first channel) of the block's output"""
        v = self.v
        if self.cv3:
            return (z if v["z_buf"] == 0 else x if v["z_buf"] == 1 else (x if v["out_buf"] else y)), v["z_co"]
        return (x if v["out_buf"] else y), v["out_co"]

    def written(self, x, y, z):
        """(npix, cout): the block's output out of the buffers a launch returned"""
        buf, co = self._dest(x, y, z)
        return buf[..., co:co + self.cout].reshape(-1, self.cout)

    def untouched_ok(self, x, y, z, unfused=False):
        """every element outside the written slice (unfused under cv3: and outside m, which those launches store) is what buffers() put
        there, NaN for NaN"""
        before, after = self.buffers(), (x, y, z)
        dest, co = self._dest(*after)
        for b0, b1 in zip(before, after):
            if (b0 is None) != (b1 is None):
                return False
            if b0 is None:
                continue
            keep = np.ones(b0.shape, bool)
            if b1 is dest:
                keep[..., co:co + self.cout] = False
            if unfused and self.cv3 and b1 is (x if self.v["out_buf"] else y):
                keep[..., self.v["out_co"]:self.v["out_co"] + 64] = False
            if not np.array_equal(b0[keep], b1[keep], equal_nan=True):
                return False
        return True

    def reference(self):
        return _reference(*self.problem())

    def emulation(self):
        return _emulation(*self.problem())


# ---- the launchers' applicability functions, restated (c3_fused.hip, bneck_fused.hip, reid_block_fused.hip) ------------------------------
def refusal_reasons(c):
    """the conditions of the case's *_applicable that its view or shape trips (empty: the launcher takes it)"""
    v, why = c.v, []
    over = lambda a, na, b, nb: a < b + nb and b < a + na
    if v["in_cs"] % 8 or v["in_co"] % 8:
        why.append("input slice not 8-aligned")
    if c.kind == "c3":
        if v["split"] not in (0, 32):
            why.append("chain broken: split")
        if v["out_cs"] % 8 or v["out_co"] % 8:
            why.append("output slice not 8-aligned")
    elif c.kind == "bneck":
        if v["out_buf"] and over(v["out_co"], 64, v["in_co"], 64):
            why.append("output over the input slice")
        if v["out_cs"] % 8 or v["out_co"] % 8:
            why.append("output slice not 8-aligned")
        if c.cv3:
            if v["out_cs"] < v["out_co"] + 128:
                why.append("[m | y2] outside the stride")
            zb = {0: "z", 1: "x", 2: "x" if v["out_buf"] else "y"}[v["z_buf"]]
            if zb == "x" and over(v["z_co"], 128, v["in_co"], 64):
                why.append("cv3 output over x")
            if zb == ("x" if v["out_buf"] else "y") and over(v["z_co"], 128, v["out_co"], 128):
                why.append("cv3 output over [m | y2]")
            if v["z_cs"] % 8 or v["z_co"] % 8:
                why.append("cv3 output slice not 8-aligned")
    else:
        if c.shape[1] != REID_HW or c.shape[2] != REID_HW:
            why.append("map is not 25 x 25")
        if v["out_buf"]:
            why.append("output in the input buffer")
        if v["out_cs"] % 4 or v["out_co"] % 4:
            why.append("output slice not 4-aligned")
    return why


# ---- the table ------------------------------------------------------------------------------------------------------------------------
# name -> view fields; the first of each family is the product's layout (engine_plan.hip::yolo_c3, reid_build_ops)
C3_VIEWS = {"dense": {}, "slice8": dict(in_cs=96, in_co=16, out_cs=88, out_co=24)}
BNECK_VIEWS = {"cat": dict(out_cs=128, out_co=0),                                       # x dense, m -> cat[0:64] of the 128-wide concat buffer
               "slice8": dict(in_cs=96, in_co=16, out_cs=88, out_co=24),
               "one_buffer": dict(in_cs=144, in_co=8, out_buf=1, out_co=72)}             # x and m: disjoint slices of ONE buffer
CV3_VIEWS = {"cat_dense": dict(out_cs=128, out_co=0, z_cs=128, z_co=0),                  # y2 at 64 of the concat buffer, z dense (layer 17)
             "cat_z128of256": dict(out_cs=128, out_co=0, z_cs=256, z_co=128),            # z -> the second half of cat16 (layer 4)
             "slice8": dict(in_cs=96, in_co=16, out_cs=152, out_co=16, z_cs=144, z_co=8)}
REID_VIEWS = {"dense": {}, "slice8": dict(in_cs=96, in_co=16, out_cs=88, out_co=24), "out4": dict(out_cs=72, out_co=4)}


def _build():
    cases = []
    for shape in SHAPES:
        for g in caps_of(ntiles(*shape)):
            for name, vf in C3_VIEWS.items():
                cases.append(Case("c3", shape, name, g, **vf))
            for res in (0, 1):
                for name, vf in BNECK_VIEWS.items():
                    cases.append(Case("bneck", shape, name, g, res=res, **vf))
                for name, vf in CV3_VIEWS.items():
                    cases.append(Case("bneck", shape, name, g, res=res, cv3=1, **vf))
    for k in REID_K:
        for g in caps_of(k):
            for name, vf in REID_VIEWS.items():
                cases.append(Case("reid", (k, REID_HW, REID_HW), name, g, **vf))
    return cases


def _refusals():
    s = (2, 9, 33)
    return [
        Case("bneck", s, "out_over_in", res=1, reason="output over the input slice", in_cs=144, in_co=8, out_buf=1, out_co=40),
        Case("bneck", s, "z_over_x", cv3=1, reason="cv3 output over x", in_cs=192, in_co=64, out_cs=128, out_co=0, z_buf=1, z_co=0),
        Case("bneck", s, "z_over_cat", cv3=1, reason="cv3 output over [m | y2]", out_cs=256, out_co=0, z_buf=2, z_co=64),
        Case("bneck", s, "in_co4", res=1, reason="input slice not 8-aligned", in_cs=96, in_co=4, out_cs=128, out_co=0),
        Case("c3", s, "in_co4", reason="input slice not 8-aligned", in_cs=96, in_co=4),
        Case("c3", s, "split16", reason="chain broken: split", split=16),
        Case("reid", (2, REID_HW, REID_HW), "one_buffer", reason="output in the input buffer", in_cs=136, in_co=0, out_buf=1, out_co=72),
        Case("reid", (1, 24, 24), "h24", reason="map is not 25 x 25"),
    ]


CASES = _build()
REFUSALS = _refusals()
KERNELS = {"c3": "c3_fused_kernel", "bneck": "bneck_fused_kernel<false>", "bneck+cv3": "bneck_fused_kernel<true>", "reid": "reid_block_fused_kernel"}


def kernel_of(c):
    return KERNELS["bneck+cv3" if c.cv3 else c.kind]
