"""YUV egress measurement (profiles/yuv_egress.md):
 (a) bgr_to_yuv_kernel alone on device buffers -- 256 frames of 640 x 640 and of 1280 x 720, NV12 and I420, tight and pitched -- next to a
     device-to-device copy that moves the same total bytes (read + written), timed in the same process with the same events;
 (b) end-to-end frames/s of CountingPipeline.render on one annotated clip: pinned host NV12 -> pinned host NV12 and device surface ->
     device surface, 640 x 640 and 1280 x 720, 16 frames per batch, on a render-only engine (no detector, no ReID net).
usage (GPU box): python tools/yuv_egress_time.py [--out profiles/yuv_egress.md] [--frames 512] [--skip-e2e]"""
import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, YuvFrameSink, YuvFrameSource  # noqa: E402
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames  # noqa: E402

B = 256
GEOMETRIES = [(640, 640, "cam_04_halfres.json"), (720, 1280, "cam_04.json")]     # h, w, zone file


def event_ms(fn, warm=3, reps=20):
    """Mean time of one call of fn: `reps` calls enqueued back to back on the null stream between two events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / reps)
    return best


def kernel_table(out):
    out.append("## (a) bgr_to_yuv_kernel alone, 256 frames per launch\n")
    out.append("Bytes = read + written (3 + 1.5 B per pixel).  The copy is `hipMemcpyAsync` device to device (torch `copy_`) of half that many bytes,")
    out.append("so it reads + writes the same total; same process, same event pair, best of 3 x 20 back-to-back launches.\n")
    out.append("| frames | format | layout | kernel ms | kernel TB/s | copy ms | copy TB/s | kernel / copy |")
    out.append("|---|---|---|---|---|---|---|---|")
    worst = 0.0
    for h, w, _ in GEOMETRIES:
        px = B * h * w
        total = px * 9 // 2
        src_c = torch.randint(0, 256, (total // 2,), dtype=torch.uint8, device="cuda")
        dst_c = torch.empty_like(src_c)
        copy_ms = event_ms(lambda: dst_c.copy_(src_c))
        del src_c, dst_c
        bgr = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device="cuda")
        for fmt in ("nv12", "i420"):
            py = (w + 255) // 256 * 256 + (0 if w % 256 else 256)   # an encoder surface: padded pitch (768 / 1536), chroma below a 16-row aligned height
            layouts = [("tight", {}), (f"pitch {py}", dict(pitch_y=py, pitch_c=py if fmt == "nv12" else py // 2, offset_c=py * ((h + 15) // 16 * 16)))]
            for name, geo in layouts:
                desc = E.yuv_desc(fmt, **geo)
                yuv = torch.zeros((E.yuv_batch_bytes(desc, B, h, w),), dtype=torch.uint8, device="cuda")
                ms = event_ms(lambda: E.bgr_to_yuv_dev(bgr.data_ptr(), B, h, w, yuv.data_ptr(), desc))
                worst = max(worst, ms / copy_ms)
                out.append(f"| {B} x {w}x{h} | {fmt} | {name} | {ms:.4f} | {total / ms / 1e9:.2f} | {copy_ms:.4f} | {total / copy_ms / 1e9:.2f} | {ms / copy_ms:.2f} |")
                del yuv
        del bgr
    out.append("")
    return worst


def synthetic_rows(t, h, w, n_tracks=12):
    """CSV rows of n_tracks boxes that cross the frame during the clip: what run* would hand to render, without a detector."""
    rows = []
    for k in range(n_tracks):
        y = int(h * (k + 1) / (n_tracks + 2))
        bw, bh = w // 12, h // 10
        xs = [int((w - bw) * f / max(t - 1, 1)) for f in range(t)]
        for f in range(t):
            x = xs[f] if k % 2 == 0 else xs[t - 1 - f]
            rows.append({"track_id": k + 1, "frame_id": f + 1, "box": [x, y, x + bw, y + bh], "color": "", "label": k % 4, "direction": "01",
                         "fpoint": (xs[0] + bw / 2, y + bh / 2), "lpoint": (xs[-1] + bw / 2, y + bh / 2), "fframe": 1, "lframe": t})
    return rows


def e2e_table(out, t, batch):
    out.append(f"## (b) CountingPipeline.render, {t} frames, {batch} frames per batch, depth 2, render-only engine\n")
    out.append("A synthetic clip as tight NV12 with 12 tracked boxes per frame to annotate (zone polygon, direction arrows, boxes with labels, count text,")
    out.append("frame counter).  Wall time of the whole `render` call: building every batch's primitive lists in Python, submit, collect; one warm-up")
    out.append("call, then the best of 3.  `lists only` is the Python share alone (the same lists built with no GPU call in the loop); `path only` is the")
    out.append("same submit / collect loop through `Renderer` with the lists built beforehand, i.e. what the device path sustains.  PCIe = 1.5 B per")
    out.append("pixel x frames/s in EACH direction for the host rows; the device rows move nothing over PCIe but the lists.\n")
    out.append("| frames | source -> sink | render frames/s | ms per batch | PCIe GB/s each way | lists only frames/s | path only frames/s | path only PCIe GB/s each way |")
    out.append("|---|---|---|---|---|---|---|---|")
    for h, w, zone_name in GEOMETRIES:
        zone = os.path.join(ROOT, "tests", "golden", zone_name)
        base = synth_frames(32, h, w, n_obj=12, seed=1702)
        yuv = np.tile(bgr_to_yuv420(base, "nv12"), ((t + 31) // 32, 1))[:t]
        rows = synthetic_rows(t, h, w)
        eng = E.Engine(None, None, max_batch=batch, max_frame_hw=(h, w), max_crops=8, max_tracks=16, nn_budget_cap=4)
        cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
        args = types.SimpleNamespace(weight=None, mapping=None, output_path=None)
        pipe = CountingPipeline(args, cfg, {"cam": {"cam_04": {}}}, engine=eng, class_names=[str(i) for i in range(4)])
        src = YuvFrameSource(yuv, h, w)
        # the Python share of the call: the same primitive lists built without a GPU in the loop
        t0 = time.perf_counter()
        viz = pipe.visualizer(rows, zone)
        for f0 in range(0, t, batch):
            viz.batch_prims(list(range(f0 + 1, min(f0 + batch, t) + 1)), (h, w))
        lists_fps = t / (time.perf_counter() - t0)
        viz = pipe.visualizer(rows, zone)
        prebuilt = [viz.batch_prims(list(range(f0 + 1, min(f0 + batch, t) + 1)), (h, w)) for f0 in range(0, t, batch)]
        host_src, dev_src = torch.from_numpy(yuv).pin_memory(), torch.from_numpy(yuv).cuda()
        surf = torch.zeros((t * h * w * 3 // 2,), dtype=torch.uint8, device="cuda")
        sinks = {"pinned host NV12 -> pinned host NV12": YuvFrameSink(h, w, n_frames=t),
                 "device NV12 -> device NV12": YuvFrameSink(h, w, n_frames=t, device_ptr=surf.data_ptr())}
        for name, sink in sinks.items():
            best = float("inf")
            for rep in range(4):
                t0 = time.perf_counter()
                pipe.render(src, rows, "cam_04", zone, sink, batch=batch)
                dt = time.perf_counter() - t0
                if rep:
                    best = min(best, dt)
            fps = t / best
            path = float("inf")
            keep = dev_src if sink.is_device else host_src
            with E.Renderer(eng, max_batch=batch, max_hw=(h, w), depth=2) as rnd:
                for rep in range(4):
                    t0 = time.perf_counter()
                    for n, f0 in enumerate(range(0, t, batch)):
                        b = min(batch, t - f0)
                        if rnd.outstanding >= 2:
                            rnd.collect()
                        rnd.submit(keep[f0:f0 + b].data_ptr(), b, h, w, sink.address(f0), kind="yuv_dev" if sink.is_device else "yuv_host", src_desc=src.desc,
                                   prims=prebuilt[n][0], first=prebuilt[n][1], out_desc=sink.desc, out_is_dev=sink.is_device)
                    while rnd.outstanding:
                        rnd.collect()
                    if rep:
                        path = min(path, time.perf_counter() - t0)
            pfps = t / path
            gbs = (lambda r: r * h * w * 1.5 / 1e9 if not sink.is_device else 0.0)
            out.append(f"| {t} x {w}x{h} | {name} | {fps:.0f} | {best / ((t + batch - 1) // batch) * 1e3:.2f} | {gbs(fps):.1f} | {lists_fps:.0f} | {pfps:.0f} | {gbs(pfps):.1f} |")
            print(out[-1], flush=True)
        eng.close()
        del surf, host_src, dev_src
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    out = ["# YUV egress: conversion kernel and end-to-end render rate\n",
           f"`python tools/yuv_egress_time.py --frames {a.frames} --batch {a.batch}` on {torch.cuda.get_device_name(0)}.\n"]
    worst = kernel_table(out)
    print("\n".join(out), flush=True)
    out.append(f"Worst kernel / copy ratio: {worst:.2f}.\n")
    if not a.skip_e2e:
        e2e_table(out, a.frames, a.batch)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
