"""CPU: tests/graph_launch_cases.py held to itself, with no engine.  The records come from `emulate`: the engine's own launch lists
(tests/golden/graph_launches_*.json: yolov5s at 96 x 160 in bf16 and in fp8 and the ReID net in bf16; the bf16 detector also through the
u8 front, derived from its list) executed with float32 torch convolutions in the engine's rounding points.  A last test runs the
oracle's own bf16 layers on the emulated pass's inputs, so the emulation and the float64 reference do not only agree with each other.  Every record passes the float64 verdict and the
wiring check; every planted fault fails, with the launch it was planted in named and no other."""
import functools

import numpy as np
import pytest

import graph_launch_cases as G
from aux_cases import rnd
from oracle.imageops import letterbox
from vehicle_counting_amd.synth import synth_frames
from vehicle_counting_amd.weights import fold_reid, synth_reid, synth_yolo

NC = 8


@functools.lru_cache(maxsize=None)
def weights():
    return G.Weights(synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0), synth_reid(1702), nc=NC)


@functools.lru_cache(maxsize=None)
def frames():
    f = synth_frames(3, 83, 150, n_obj=6, seed=3)
    f.setflags(write=False)
    return f


def yolo_input():
    x = np.zeros((3, 96, 160, 4), np.float32)
    x[..., :3] = np.stack([letterbox(np.ascontiguousarray(f[:, :, ::-1]), 96, 160) for f in frames()]).astype(np.float32) / np.float32(255)
    return "in", G.bits_of(rnd(x, "bf16"), 2)


def reid_input():
    x = np.zeros((3, 50, 50, 8), np.float32)
    x[..., :3] = np.random.default_rng(5).standard_normal((3, 50, 50, 3))
    return "in", G.bits_of(rnd(x, "bf16"), 2)


PLANS = {"yolov5s_bf16": ("yolo", yolo_input, False), "yolov5s_bf16_u8": ("yolo", None, True), "yolov5s_fp8": ("yolo", yolo_input, False),
         "reid_bf16": ("reid", reid_input, False)}


@functools.lru_cache(maxsize=None)
def emulated(tag, fault=None):
    net, inp, u8 = PLANS[tag]
    launches, arena = G.emulate(G.load_plan(tag), weights(), inp() if inp else None, frames() if u8 else None, fault)
    return G.Pass(launches, arena, weights(), frames() if u8 else None), net


def find(tag, param):
    """index of the launch whose last op is `param`"""
    return next(i for i, L in enumerate(G.load_plan(tag)) if L["ops"][-1].get("param") == param)


def test_folded_reid_weights_are_the_engines():
    """the references use weights.fold_reid, whose output the engine uploads; oracle.reid._fold, the same expression in torch, agrees with it
    to the last float32 bit or the one before in every weight"""
    import torch
    from oracle import reid as oreid
    sd = {k: torch.as_tensor(v) for k, v in synth_reid(1702).items()}
    f = fold_reid(synth_reid(1702))
    assert set(f) == {n for n in weights().names if not n.startswith("model.")}
    for n, (w, b) in f.items():
        np.testing.assert_array_equal(w, weights().p[n][0])
        conv, bn = ("conv.0", "conv.1") if n == "conv" else ((n + ".0", n + ".1") if n.endswith("downsample") else (n, n.replace("conv", "bn")))
        wo, bo = oreid._fold(sd[conv + ".weight"], sd.get(conv + ".bias"), sd, bn)
        np.testing.assert_allclose(w, wo.numpy(), rtol=2.0 ** -22, atol=0)
        np.testing.assert_allclose(b, bo.numpy(), rtol=0, atol=1e-7)        # (b0 - mean) * scale + beta cancels


def test_plans_cover_what_the_module_models():
    ids = {tag: {L["cfg"] for L in G.load_plan(tag)} for tag in PLANS}
    assert {100, 103, 104, 105, 107} <= ids["yolov5s_bf16"] and {102, 103, 104, 105, 107} <= ids["yolov5s_bf16_u8"]
    assert 100 in ids["yolov5s_fp8"] and {101, 106} <= ids["reid_bf16"]
    kinds = {o["kind"] for tag in PLANS for L in G.load_plan(tag) for o in L["ops"]}
    assert kinds == {"conv", "sppf", "upsample", "maxpool", "to_fp8", "head_compact"}
    assert any("up" in o for L in G.load_plan("yolov5s_bf16") for o in L["ops"])          # a folded upsample
    assert any("m_dev" in o for L in G.load_plan("yolov5s_bf16") for o in L["ops"])       # the sparse head


@pytest.mark.parametrize("tag", sorted(PLANS))
def test_every_emulated_record_passes(tag):
    """... and on every launch of several convs the emulation uses at most HALF of what the chain conditions add to the one-conv gate, so
    the engine has the other half: the worst element at most half-way between 1 x and 2 x the bf16 gate (1.5; one summation order gives
    1.20 on the first C3 here and 1.21 on 5-conv chains at 384 x 640), and at most 0.5e-4 of the launch's elements above 1 x"""
    p, net = emulated(tag)
    fails, table = p.verdict()
    for i, name, worst, over, fp8, _ in table:
        print("%-100s worst %.3f  above the gate %d  e4m3 differing %.5f" % (name, worst, over, fp8))
    assert not fails, fails
    assert not p.wiring(net), p.wiring(net)
    for i, L in enumerate(p.launches):
        if sum(o["kind"] == "conv" for o in L["ops"]) > 1:
            f, figs = p.verdict_of(i)
            r = [x for x in figs if x[1] == "bf16"]
            worst, over, total = max(x[2] for x in r), sum(x[3] for x in r), sum(x[4] for x in r)
            print("chain %d (cfg %d): worst %.3f, %d of %d above the gate" % (i, L["cfg"], worst, over, total))
            assert worst <= 1 + (G.MULTI_WORST - 1) / 2, (i, r)
            assert over <= G.MULTI_SHARE / 2 * total, (i, r)


FAULTS = [("yolov5s_bf16", "model.1.conv", "ulp4", "worst error"),                      # one output column of one tile off by 4 bf16 ulps
          ("yolov5s_bf16", "model.6.cv3.conv", "swap_halves", "worst error"),           # the two halves of a concat input swapped
          ("yolov5s_bf16", "model.5.conv", "in_shift", "worst error"),                  # a slice offset moved by 8 channels
          ("yolov5s_bf16", "model.6.m.1.cv2.conv", "res_pingpong", "worst error"),      # the residual from the other ping-pong buffer
          ("yolov5s_bf16", "model.6.m.1.cv2.conv", "no_res", "worst error"),            # the residual dropped
          ("yolov5s_bf16", "model.10.conv", "byte_outside", "outside the output views"),    # one byte outside the output slice changed
          ("yolov5s_bf16", "model.4.cv3.conv", "byte_outside", "outside the output views"),  # ... behind a fused launch
          ("yolov5s_bf16", "model.4.cv3.conv", "no_res", "of the bf16 gate"),           # ... inside a fused launch (id 105)
          ("reid_bf16", "layer2.0.conv2", "no_res", "worst error"),
          ("reid_bf16", "layer1.1.conv2", "no_res", "of the bf16 gate"),                # id 106
          ("yolov5s_fp8", "model.5.conv", "scale", "e4m3 outputs")]                     # the fp8 scale of one channel halved


@pytest.mark.parametrize("tag,param,kind,what", FAULTS)
def test_planted_fault_fails_with_its_launch_named(tag, param, kind, what):
    i = find(tag, param)
    p, net = emulated(tag, (i, kind))
    fails, _ = p.verdict()
    assert fails, "the fault passed"
    assert all(f.startswith("launch %d " % i) for f in fails), fails
    assert any(what in f for f in fails), fails
    # the records stay consistent with each other: the fault is in one launch's arithmetic, not in the graph
    assert not p.wiring(net)


def test_wiring_names_a_rewired_input():
    """a record whose input bytes are not what its source left fails the wiring check at that launch"""
    p, net = emulated("yolov5s_bf16")
    i = find("yolov5s_bf16", "model.9.cv2.conv")
    L = p.launches[i]
    arena = p.arena.copy()
    b = L["bufs"][L["ops"][0]["in"]["buf"]]
    arena[b["before"] + 64] ^= 0x10
    fails = G.Pass(p.launches, arena, weights()).wiring(net)
    assert fails and all(f.startswith("launch %d " % i) for f in fails), fails
    # ... and a parameter recorded twice, or never
    fails = G.Pass(p.launches[:i + 1] + p.launches[i:], p.arena, weights()).wiring(net)
    assert any("recorded" in f for f in fails)


def _layer_out(p, tag, name):
    """(B, H, W, C) float32 the emulated pass left for conv `name`, or None where its launch kept it on chip"""
    for L in p.launches:
        for j, op in enumerate(L["ops"]):
            if op.get("param") == name:
                if j < L["n_ops"] - 1:
                    return None
                return G.Mem(L, p.arena, "after").read(op["out"]).reshape(op["B"], op["Ho"], op["Wo"], -1)
    raise KeyError(name)


def _close(got, ref, what):
    """two float32 implementations of at most one module (five convs): mostly the same bf16 values, none further than the chain conditions"""
    g = G.GATE["bf16"]
    ratio = np.abs(got.astype(np.float64) - ref) / (g["atol"] + g["rtol"] * np.abs(ref))
    print("%-22s identical %.4f  worst %.3f of the gate" % (what, (got == ref).mean(), ratio.max()))
    assert (got == ref).mean() >= 0.98 and ratio.max() <= G.MULTI_WORST and (ratio > 1).mean() <= G.MULTI_SHARE, what


def test_emulation_agrees_with_the_oracles_own_bf16_forward():
    """Independence: `emulate` runs the module's own conv_op, so a mistake there would be shared with the float64 reference.  Here every
    layer of oracle.yolov5's bf16 restatement (its _cba / _c3 / SPPF code, not this module's) is run on the emulated pass's own layer
    inputs and must give the layer the emulated pass left: the stem's pair layout, the split store of cv1 | cv2, the shortcut after the
    activation, the folded upsample + concat and the pooled concat all sit between the two.  The ReID net alike, block by block
    (shortcut before the activation, the downsample branch), against oracle.reid's arithmetic."""
    import torch
    import torch.nn.functional as F
    from oracle import reid as orr
    from oracle import yolov5 as oy
    p, _ = emulated("yolov5s_bf16")
    sd = {k: torch.as_tensor(v) for k, v in synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0).items()}
    sd = {k: (oy._r16(v) if k.endswith(".weight") else v) for k, v in sd.items()}
    nchw = lambda a: torch.as_tensor(np.ascontiguousarray(a)).permute(0, 3, 1, 2)
    x = oy._r16(torch.as_tensor(oy.preprocess([f[:, :, ::-1] for f in frames()], 160)[0]))
    ys, checked = [], 0
    with torch.no_grad():
        for idx, kind, frm, a in oy.build_graph("yolov5s"):
            name = "model.%d" % idx
            if kind == "conv":
                y, out = oy._cba(x, sd, name + ".conv", a[3], a[4], bf16=True), name + ".conv"
            elif kind == "c3":
                y, out = oy._c3(x, sd, name, a[2], a[3], bf16=True), name + ".cv3.conv"
            elif kind == "sppf":
                t = oy._cba(x, sd, name + ".cv1.conv", 1, 0, bf16=True)
                y1 = F.max_pool2d(t, 5, 1, 2)
                y2 = F.max_pool2d(y1, 5, 1, 2)
                y, out = oy._cba(torch.cat((t, y1, y2, F.max_pool2d(y2, 5, 1, 2)), 1), sd, name + ".cv2.conv", 1, 0, bf16=True), name + ".cv2.conv"
            elif kind == "up":
                y, out = F.interpolate(x, scale_factor=2.0, mode="nearest"), None
            elif kind == "cat":
                y, out = torch.cat((x, ys[frm[1]]), 1), None
            else:
                break
            got = _layer_out(p, "yolov5s_bf16", out) if out else None
            if got is not None:
                _close(got, y.permute(0, 2, 3, 1).numpy(), name)
                checked += 1
                y = nchw(got)                                    # the next layer starts from what the emulated pass holds
            ys.append(y)
            x = y
    assert checked >= 17                                             # every conv, C3 and SPPF layer but model.3, which id 107 keeps on chip
    # ReID
    p, _ = emulated("reid_bf16")
    sd = {k: torch.as_tensor(v) for k, v in synth_reid(1702).items()}
    r = lambda t: t.bfloat16().float()
    with torch.no_grad():
        y = nchw(_layer_out(p, "reid_bf16", "layer1.1.conv2"))
        for name, cin, cout, down in orr.BLOCKS[2:]:
            s = 2 if down else 1
            w, b = orr._fold(sd[name + ".conv1.weight"], None, sd, name + ".bn1")
            z = r(F.relu(F.conv2d(y, r(w), b, stride=s, padding=1)))
            if down or cin != cout:
                w, b = orr._fold(sd[name + ".downsample.0.weight"], None, sd, name + ".downsample.1")
                y = r(F.conv2d(y, r(w), b, stride=s))
            w, b = orr._fold(sd[name + ".conv2.weight"], None, sd, name + ".bn2")
            y = r(F.relu(F.conv2d(z, r(w), b, stride=1, padding=1) + y))
            got = _layer_out(p, "reid_bf16", name + ".conv2")
            _close(got, y.permute(0, 2, 3, 1).numpy(), name)
            y = nchw(got)
        x = nchw(G.values(reid_input()[1], 2).reshape(3, 50, 50, 8)[..., :3])
        feat = orr.reid_forward_bf16(sd, x)
        last = _layer_out(p, "reid_bf16", "layer4.1.conv2").astype(np.float64).mean(axis=(1, 2))
        cos = (feat * last).sum(1) / np.sqrt((feat * feat).sum(1) * (last * last).sum(1))
        print("whole ReID net, emulated against oracle.reid.reid_forward_bf16: 1 - cos %.3g" % (1 - cos.min()))
        assert 1 - cos.min() <= 1e-5
