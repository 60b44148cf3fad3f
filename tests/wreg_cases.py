"""Cases and float64 references for conv1x1_wreg_kernel (csrc/conv_pointwise.hip, tile configurations 73 - 78 of conv_cfgs.h): the
weight-stationary pointwise kernel that stages only the pixels through an LDS ring and runs a tile's epilogue under the next tile's
MFMAs.  tests/test_gpu_wreg.py launches them through vc_conv2d_view_host; tests/test_wreg_cases.py holds this module to its own
conditions on the CPU.

A case is conv_view_cases.Case (buffers with NaN around the operands, SENTINEL outputs, float64 reference of the rounded operands) plus
the id it runs under and the persistent grid (VC_CONV_SLOTS) it is launched with.  The shapes are the smallest at which the kernel can
still go wrong: M = 1, one tile minus one, one tile, two tiles + 17 (ragged last tile), five tiles on one and on two workgroups (one
workgroup walks a first, middle and last tile through the interleaved epilogue), seven tiles on three workgroups (uneven walk)."""
import numpy as np

from conv_view_cases import Case

# id -> (KS, NG, PT, NS): K = KS * 32 input channels, NG * 64 output channels, PT * 16 * 4 / NG pixels per tile, NS ring stages
WREG = {73: (8, 4, 2, 3), 74: (8, 4, 2, 4), 75: (8, 2, 2, 2), 76: (4, 4, 2, 4), 77: (4, 2, 2, 3), 78: (4, 2, 2, 4)}
IDS = tuple(sorted(WREG))
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2


def shape_of(cfg):
    """(cin, cout, pixels per tile, LDS bytes of the ring)"""
    ks, ng, pt, ns = WREG[cfg]
    bp = pt * 16 * (4 // ng)
    return ks * 32, ng * 64, bp, ns * bp * ks * 64


def wreg_applicable(case, cfg):
    """conv_pointwise.hip::wreg_applicable, restated on a Case"""
    ks, ng, _, _ = WREG[cfg]
    v = case.v
    if case.precision != "bf16" or case.k != 1 or case.stride != 1 or case.pad != 0:
        return False
    if case.cin != ks * 32 or case.cout != ng * 64 or v["up_c"] or v["m_valid"] >= 0:
        return False
    if v["in_cs"] % 8 or v["in_co"] % 8 or v["out_cs"] % 8 or v["out_co"] % 8:
        return False
    if v["out_f32"] or case.res_mode != 0 or case.act not in (ACT_NONE, ACT_SILU, ACT_RELU):
        return False
    return v["split"] == 0 or (v["split"] % 8 == 0 and v["out2_cs"] % 8 == 0 and v["out2_co"] % 8 == 0)


def _view(cin, cout, split):
    """the input at channel offset 8 of a buffer 24 channels wider; the output at offset 8 of a buffer 24 wider; under a split the second
    destination at offset 16 of a buffer with another stride"""
    v = dict(in_co=8, in_cs=cin + 24, out_co=8, out_cs=(split or cout) + 24)
    if split:
        v.update(split=split, out2_co=16, out2_cs=cout - split + 40)
    return v


class Run:
    def __init__(self, cfg, case, slots):
        self.cfg, self.case, self.slots = cfg, case, slots
        self.name = "id%d-%s-slots%d" % (cfg, case.tag, slots)


def _runs():
    out = []
    for cfg in IDS:
        cin, cout, bp, _ = shape_of(cfg)
        # (tag, M, slots, act, split)
        rows = [("m1", 1, 0, ACT_SILU, 0), ("tile-1", bp - 1, 0, ACT_RELU, 0), ("tile", bp, 0, ACT_NONE, 0),
                ("ragged", 2 * bp + 17, 0, ACT_SILU, 0), ("ragged-split", 2 * bp + 17, 0, ACT_SILU, cout // 2),
                ("walk5", 5 * bp, 1, ACT_SILU, 0), ("walk5", 5 * bp, 2, ACT_SILU, 0), ("walk5-split", 5 * bp, 1, ACT_RELU, cout // 2),
                ("walk7", 7 * bp, 3, ACT_NONE, cout // 2), ("walk7-silu", 7 * bp, 3, ACT_SILU, 0)]
        for tag, m, slots, act, split in rows:
            case = Case("wreg", "%s_%dx%d_a%d" % (tag, cin, cout, act), "bf16", (1, 1, m), cin, cout, act=act, ids=(cfg,), **_view(cin, cout, split))
            out.append(Run(cfg, case, slots))
    return out


def _refusals():
    """(cfg, case, why): what the family refuses quietly (VC_ERR_ARG without a message), each on the id whose widths it otherwise fits"""
    out = []
    v = _view(256, 256, 0)
    out.append((73, Case("wreg", "m_dev", "bf16", (1, 6, 12), 256, 256, ids=(73,), **dict(v, m_valid=50)), "device-side pixel count"))
    out.append((73, Case("wreg", "fold-in", "bf16", (1, 6, 12), 256, 256, ids=(73,), **dict(v, up_c=128, up_cs=136, up_co=8)), "upsample fold-in"))
    out.append((74, Case("wreg", "out_f32", "bf16", (1, 6, 12), 256, 256, ids=(74,), **dict(v, out_f32=1)), "f32 store"))
    out.append((73, Case("wreg", "k512", "bf16", (1, 6, 12), 512, 256, ids=(73,), **_view(512, 256, 0)), "K = 512"))
    out.append((77, Case("wreg", "cout64", "bf16", (1, 6, 12), 128, 64, ids=(77,), **_view(128, 64, 0)), "Cout = 64"))
    out.append((78, Case("wreg", "residual", "bf16", (1, 6, 12), 128, 128, res_mode=1, ids=(78,), **dict(_view(128, 128, 0), res_cs=144, res_co=8)),
                "residual"))
    return out


RUNS = _runs()
REFUSALS = _refusals()


def reference64(case):
    """float64 (M, cout) of the bf16-rounded operands, written out with einsum (independent of Case.reference's torch conv)"""
    o = case.operands()
    w = case.weights_used().reshape(case.cout, case.cin).astype(np.float64)
    t = np.einsum("mk,nk->mn", o["x"].reshape(case.M, case.cin).astype(np.float64), w) + o["b"].astype(np.float64)
    if case.act == ACT_SILU:
        t = t / (1.0 + np.exp(-t))
    elif case.act == ACT_RELU:
        t = np.maximum(t, 0.0)
    return t
