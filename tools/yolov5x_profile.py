"""The numbers of profiles/yolov5x.md: YOLOv5x at 640 x 640, bf16, batch 64, detector only (stream path, device-resident u8 frames).

    python tools/yolov5x_profile.py --sections regs          # where the library was built (reads csrc/build/stem_direct*.o)
    python tools/yolov5x_profile.py --sections stem,layers,xl # on the GPU

Sections: `regs` registers / LDS / scratch of stem_direct_wide_kernel<5, U8> (tools/kernel_regs.sh); `stem` the 80-channel stem with option
"stem_direct" 1 against 0 in one process (median of the timed launches, blocking per-launch events); `layers` every conv launch of one
pass with the kernel family that ran, its time and share; `xl` detector-only frames/s and conv TFLOP/s of YOLOv5x beside YOLOv5l.
A section that is not asked for is carried over from the existing --out file, so the two runs above fill one document."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDER = ["regs", "stem", "layers", "xl"]
TITLE = {"regs": "## Registers of the 80-channel stem kernel", "stem": "## Stem: stem_direct 1 against 0",
         "layers": "## Conv launches of one pass", "xl": "## YOLOv5x beside YOLOv5l"}
S, NC = 640, 80


def family(cfg):
    """Kernel family of an op-log cfg id (csrc/conv_cfgs.h: the ids are persistent; engine_run.hip::conv_select for >= 100)."""
    if cfg >= 100:
        return {100: "stem_direct", 102: "front_fused", 103: "c3_fused", 104: "bneck_fused", 105: "bneck_cv3_fused", 107: "s2halo + pointwise"}.get(cfg, f"fused {cfg}")
    if 28 <= cfg <= 31 or 36 <= cfg <= 39:
        return "halo v1"
    if cfg == 55:
        return "halo v2"
    if 44 <= cfg <= 49:
        return "halo s2"
    if 32 <= cfg <= 35:
        return "direct 1x1"
    if 50 <= cfg <= 54:
        return "stream 1x1"
    return "implicit GEMM"


def conv_gflop(variant):
    from vehicle_counting_amd.weights import yolo_conv_table
    stride = {0: 2, 1: 4, 2: 4, 3: 8, 4: 8, 5: 16, 6: 16, 7: 32, 8: 32, 9: 32, 10: 32, 13: 16, 14: 16, 17: 8, 18: 16, 20: 16, 21: 32, 23: 32}
    fl = 0.0
    for n, ci, co, k in yolo_conv_table(variant, NC):
        i = int(n.split(".")[1])
        st = (8, 16, 32)[int(n.rsplit(".", 1)[1])] if i == 24 else stride[i]
        fl += 2.0 * (S // st) ** 2 * co * ci * k * k
    return fl / 1e9


def parse_ops(log):
    rows = []
    for ln in log.splitlines():
        m = re.match(r"conv M=(\d+) N=(\d+) K=(\d+) k=(\d)x(\d) s=(\d) cfg=(-?\d+) ms=([\d.]+) tflops=([\d.]+)", ln)
        if m:
            rows.append(tuple(int(v) for v in m.groups()[:7]) + (float(m.group(8)), float(m.group(9))))
    return rows


class Detector:
    def __init__(self, variant, B):
        import torch
        import vehicle_counting_amd.engine as E
        from vehicle_counting_amd.synth import synth_frames
        from vehicle_counting_amd.weights import synth_yolo
        self.B = B
        # obj_shift -8: the seeded head passes almost nothing, the sparse Detect head and the NMS stay small (the convs are what is timed)
        self.eng = E.Engine(synth_yolo(variant, nc=NC, det_scale=4.0, obj_shift=-8.0), None, precision="bf16", model_name=variant, num_classes=NC,
                            max_batch=B, img_size=S, max_frame_hw=(S, S), max_candidates=8192)
        self.frames = torch.from_numpy(synth_frames(B, S, S, 12, 1702)).cuda()

    def run(self):
        self.eng.stream_reset()
        self.eng.stream_submit(self.frames.data_ptr(), self.B, S, S)
        self.eng.sync()

    def ops(self):
        self.eng.profile(1); self.eng.profile_reset()
        self.run()
        rows = parse_ops(self.eng.profile_ops())
        self.eng.profile(0)
        return rows

    def pass_ms(self, n):
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            self.run()
            t.append((time.perf_counter() - t0) * 1e3)
        return t


def sec_regs():
    out = ""
    for name, filt in (("stem_direct.o", "stem_direct_kernel<4,"), ("stem_direct_wide.o", "stem_direct_wide_kernel<5,")):
        obj = os.path.join(ROOT, "vehicle-counting_amd", "csrc", "build", name)
        out += subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), obj, filt], capture_output=True, text=True, check=True).stdout
    lines = ["`tools/kernel_regs.sh csrc/build/stem_direct_wide.o` and `... stem_direct.o` (vgpr = the unified count, AGPRs included; a SIMD holds 512 per lane, so 256 is the",
             "most a kernel may use with two waves resident).  CT = 4 (YOLOv5l) for comparison.", "",
             "| kernel | VGPRs | of them AGPRs | SGPRs | spilled | LDS bytes | scratch bytes |", "|---|---|---|---|---|---|---|"]
    for ln in out.splitlines():
        m = re.search(r"stem_direct(?:_wide)?_kernel<(\d), (true|false)>.* vgpr (\d+) agpr (\d+) sgpr (\d+) spill (\d+) lds (\d+) scratch (\d+)", ln)
        if m:
            ct, u8, v, a, s, sp, lds, scr = m.groups()
            lines.append(f"| `stem_direct{'_wide' if ct == '5' else ''}_kernel<{ct}, {u8}>` | {v} | {a} | {s} | {sp} | {lds} | {scr} |")
            assert ct != "5" or (scr == "0" and sp == "0" and int(v) <= 256), ln
    return "\n".join(lines)


def sec_stem(x, reps):
    med = {}
    for v in (1, 0):
        x.eng.set_option("stem_direct", v)
        for _ in range(3):
            x.run()
        ms, cfg = [], None
        for _ in range(reps):
            stem = [r for r in x.ops() if (r[3], r[4]) == (6, 3)]
            assert len(stem) == 1
            ms.append(stem[0][7]); cfg = stem[0][6]
        med[v] = (statistics.median(ms), min(ms), max(ms), cfg)
    x.eng.set_option("stem_direct", 1)
    by = x.B * (S * S * 3 + (S // 2) ** 2 * 80 * 2) / 1e9
    lines = [f"Batch {x.B} of {S} x {S} u8 frames, median of {reps} timed launches (3 warm-up passes first), same engine, same process.  With the option at 0",
             "the letterbox kernel runs first and writes the 8-byte-per-pixel tensor the implicit GEMM reads; its time is NOT in the figure below.", "",
             "| stem_direct | kernel | median ms | min | max | GB/s of the layer's algorithmic bytes |", "|---|---|---|---|---|---|"]
    for v in (1, 0):
        m, lo, hi, cfg = med[v]
        lines.append(f"| {v} | {family(cfg)} (cfg {cfg}) | {m:.4f} | {lo:.4f} | {hi:.4f} | {by / (m * 1e-3):.0f} |")
    lines += ["", f"direct / implicit GEMM = {med[1][0] / med[0][0]:.2f}"]
    return "\n".join(lines)


def sec_layers(x):
    for _ in range(2):
        x.run()
    rows = x.ops()
    tot = sum(r[7] for r in rows)
    lines = [f"Batch {x.B}, blocking per-launch events (vc_profile_enable 1).  {len(rows)} launches, {tot:.2f} ms of conv time per pass.", "",
             "| launch (M x N x K, kernel, stride) | family (cfg) | ms | share | TFLOP/s |", "|---|---|---|---|---|"]
    fam = {}
    for M, N, K, kh, kw, s, cfg, ms, tf in rows:
        lines.append(f"| {M} x {N} x {K}, {kh}x{kw}, s{s} | {family(cfg)} ({cfg}) | {ms:.4f} | {100 * ms / tot:.1f} % | {tf:.0f} |")
        key = family(cfg) + (" 3x3" if kh == 3 else " 1x1" if kh == 1 else "")
        f = fam.setdefault(key, [0, 0.0, 0.0])
        f[0] += 1; f[1] += ms; f[2] += 2.0 * M * N * K
    lines += ["", "| family | launches | ms | share | TFLOP/s |", "|---|---|---|---|---|"]
    for k, (n, ms, fl) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"| {k} | {n} | {ms:.3f} | {100 * ms / tot:.1f} % | {fl / (ms * 1e-3) / 1e12:.0f} |")
    narrow = sum(r[7] for r in rows if r[1] == 80 or (r[3] == 1 and r[1] in (160, 320)))
    lines += ["", f"80-wide layers and 160 / 320-wide pointwise layers together: {narrow:.2f} ms, {100 * narrow / tot:.1f} % of the conv time."]
    return "\n".join(lines)


def sec_xl(dets, reps):
    lines = [f"Detector only (letterbox fold-in, convs, Detect head, NMS), batch 64 of {S} x {S}, bf16; median wall time of {reps} passes, each submitted and",
             "waited for on its own (3 warm-up passes), both engines alive in one process and timed alternately.", "",
             "| model | GFLOP / frame | ms / pass | frames/s | conv TFLOP/s |", "|---|---|---|---|---|"]
    t = {v: [] for v in dets}
    for d in dets.values():
        d.pass_ms(3)
    for _ in range(reps):
        for v, d in dets.items():
            t[v] += d.pass_ms(1)
    fps = {}
    for v, d in dets.items():
        ms = statistics.median(t[v])
        fps[v] = d.B / (ms * 1e-3)
        lines.append(f"| {v} | {conv_gflop(v):.1f} | {ms:.2f} | {fps[v]:.0f} | {conv_gflop(v) * fps[v] / 1e3:.0f} |")
    lines += ["", f"frames/s x / l = {fps['yolov5x'] / fps['yolov5l']:.2f}; FLOPs per frame x / l = {conv_gflop('yolov5x') / conv_gflop('yolov5l'):.2f}"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="regs,stem,layers,xl")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolov5x.md"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    want = a.sections.split(",")
    have = {}
    if os.path.exists(a.out):
        text = open(a.out).read()
        for k in ORDER:
            m = re.search(re.escape(TITLE[k]) + r"\n\n(.*?)(?=\n## |\Z)", text, re.S)
            if m:
                have[k] = m.group(1).strip()
    if "regs" in want:
        have["regs"] = sec_regs()
    if set(want) & {"stem", "layers", "xl"}:
        x = Detector("yolov5x", a.batch)
        if "stem" in want:
            have["stem"] = sec_stem(x, a.reps)
        if "layers" in want:
            have["layers"] = sec_layers(x)
        if "xl" in want:
            have["xl"] = sec_xl({"yolov5l": Detector("yolov5l", a.batch), "yolov5x": x}, a.reps)
    doc = ["# YOLOv5x on the engine: registers, stem, layers", "",
           "Written by `tools/yolov5x_profile.py` (tools/README.md).  YOLOv5x: depth 1.33, width 1.25 -- 80 / 160 / 320 / 640 / 1280 channels, 4-8-12-4",
           f"bottlenecks, 126 convs, {conv_gflop('yolov5x'):.1f} GFLOP per {S} x {S} frame.", ""]
    for k in ORDER:
        if k in have:
            doc += [TITLE[k], "", have[k], ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(doc))
    print("\n".join(doc))


if __name__ == "__main__":
    main()
