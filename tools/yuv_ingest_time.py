"""YUV ingest measurement (profiles/yuv_ingest.md):
 (a) yuv_to_bgr_kernel alone on device buffers -- 256 frames of 640 x 640 and of 1280 x 720, NV12 and I420 -- next to a device-to-device
     copy that moves the same total bytes (read + written), timed in the same process with the same events;
 (b) end-to-end frames/s of CountingPipeline.run_stream(host_frames=True, asynchronous=True) on one clip given as NV12 and as the BGR it converts to:
     640 x 640 and 1280 x 720, bf16 YOLOv5s, 256 frames per batch, both forms on one engine per geometry.
 (c) the kernel alone as in (a) for all six source formats -- nv12, i420 and the wider p016, i010, i422, i444 -- each next to the copy of
     ITS OWN read + written bytes (4.5, 5 or 6 B per pixel), all in one run.
usage (GPU box): python tools/yuv_ingest_time.py [--out profiles/yuv_ingest.md] [--batches 6] [--skip-e2e] [--only-wide]"""
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
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource, YuvFrameSource  # noqa: E402
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC, B = 80, 256
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
GEOMETRIES = [(640, 640, 1.0, "cam_04_halfres.json"), (720, 1280, 7.8, "cam_04.json")]     # h, w, bench.py's obj_shift and zone file for it


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
    out.append("## (a) yuv_to_bgr_kernel alone, 256 frames per launch\n")
    out.append("Bytes = read + written (1.5 + 3 B per pixel).  The copy is `hipMemcpyAsync` device to device (torch `copy_`) of half that many bytes,")
    out.append("so it reads + writes the same total; same process, same event pair, best of 3 x 20 back-to-back launches.\n")
    out.append("| frames | format | layout | kernel ms | kernel TB/s | copy ms | copy TB/s | kernel / copy |")
    out.append("|---|---|---|---|---|---|---|---|")
    worst = 0.0
    for h, w, _, _ in GEOMETRIES:
        px = B * h * w
        total = px * 9 // 2
        src_c = torch.randint(0, 256, (total // 2,), dtype=torch.uint8, device="cuda")
        dst_c = torch.empty_like(src_c)
        copy_ms = event_ms(lambda: dst_c.copy_(src_c))
        del src_c, dst_c
        bgr = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
        for fmt in ("nv12", "i420"):
            layouts = [("tight", {})]
            py = (w + 255) // 256 * 256 + (0 if w % 256 else 256)   # a decoder surface: padded pitch (768 / 1536), chroma below a 16-row aligned height
            if py:
                layouts.append((f"pitch {py}", dict(pitch_y=py, pitch_c=py if fmt == "nv12" else py // 2, offset_c=py * ((h + 15) // 16 * 16))))
            for name, geo in layouts:
                desc = E.yuv_desc(fmt, **geo)
                nbytes = E.yuv_batch_bytes(desc, B, h, w)
                yuv = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
                ms = event_ms(lambda: E.yuv_to_bgr_dev(yuv.data_ptr(), B, h, w, bgr.data_ptr(), desc))
                worst = max(worst, ms / copy_ms)
                out.append(f"| {B} x {w}x{h} | {fmt} | {name} | {ms:.4f} | {total / ms / 1e9:.2f} | {copy_ms:.4f} | {total / copy_ms / 1e9:.2f} | {ms / copy_ms:.2f} |")
                del yuv
        del bgr
    out.append("")
    return worst


FORMATS = ("nv12", "i420", "p016", "i010", "i422", "i444")
FORMAT_ID = {**E.L.PIX_ID, **E.L.PIX_WIDE_ID}


def wide_table(out):
    out.append("## (c) all six source formats, kernel alone, 256 frames per launch\n")
    out.append("As (a), one run for all rows.  Bytes = read + written: 3 B written per pixel, read 1.5 B (nv12, i420), 2 B (i422) or 3 B (p016, i010,")
    out.append("i444).  Every format is held against the device-to-device copy of half ITS OWN total; `pitch` = the luma pitch in bytes of a padded")
    out.append("decoder surface (the chroma pitch follows it, the chroma planes start below a 16-row aligned height).\n")
    out.append("| frames | format | B / px read | layout | kernel ms | kernel TB/s | copy ms | copy TB/s | kernel / copy |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    worst = {}
    for h, w, _, _ in GEOMETRIES:
        bgr = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
        copy_ms = {}
        for fmt in FORMATS:
            rowb, crow, hc, semi, _ = E.yuv_format_rows(FORMAT_ID[fmt], h, w)
            read = h * rowb + (1 if semi else 2) * hc * crow                                  # plane bytes of one frame
            total = B * (read + 3 * h * w)
            if total not in copy_ms:
                src_c = torch.randint(0, 256, (total // 2,), dtype=torch.uint8, device="cuda")
                dst_c = torch.empty_like(src_c)
                copy_ms[total] = event_ms(lambda: dst_c.copy_(src_c))
                del src_c, dst_c
            py = (rowb + 255) // 256 * 256 + (0 if rowb % 256 else 256)
            layouts = [("tight", {}), (f"pitch {py}", dict(pitch_y=py, pitch_c=py if crow == rowb else py // 2, offset_c=py * ((h + 15) // 16 * 16)))]
            for name, geo in layouts:
                desc = E.yuv_desc(fmt, **geo)
                yuv = torch.randint(0, 256, (E.yuv_batch_bytes(desc, B, h, w),), dtype=torch.uint8, device="cuda")
                ms = event_ms(lambda: E.yuv_to_bgr_dev(yuv.data_ptr(), B, h, w, bgr.data_ptr(), desc))
                c = copy_ms[total]
                worst[fmt] = max(worst.get(fmt, 0.0), ms / c)
                out.append(f"| {B} x {w}x{h} | {fmt} | {read / (h * w):.1f} | {name} | {ms:.4f} | {total / ms / 1e9:.2f} | {c:.4f} | {total / c / 1e9:.2f} | {ms / c:.2f} |")
                print(out[-1], flush=True)
                del yuv
        del bgr
    out.append("")
    out.append("Worst kernel / copy ratio per format: " + ", ".join(f"{f} {worst[f]:.2f}" for f in FORMATS) + ".\n")


def pinned(a):
    """The array in pinned host memory, as a numpy view (run_stream's own pin_memory() is then free: the frames are pinned already)."""
    t = torch.from_numpy(a).pin_memory()
    return t.numpy(), t


def e2e_table(out, batches):
    out.append(f"## (b) run_stream(host_frames=True, asynchronous=True), bf16 YOLOv5s, {B} frames per batch, {batches} batches per run\n")
    out.append("One engine per geometry; a 256-frame synthetic clip, repeated, as NV12 and as the BGR frames that NV12 converts to (the same pixels")
    out.append("reach the detector, so the CSV rows agree), both in pinned host memory before the clock starts.  Wall time of the whole `run_stream` call: staging, detector, ReID, tracker, row collection in Python")
    out.append("and the counting post-pass; one warm-up run per form (conv autotune, buffers), then the best of 3.  PCIe = frame bytes x frames/s.\n")
    out.append("| frames | source | frames/s | ms per 256-frame batch | PCIe GB/s | CSV rows |")
    out.append("|---|---|---|---|---|---|")
    for h, w, obj_shift, zone_name in GEOMETRIES:
        zone = os.path.join(ROOT, "tests", "golden", zone_name)
        clip = synth_frames(B, h, w, n_obj=12, seed=1702, bounce=True)
        yuv = np.concatenate([bgr_to_yuv420(clip[i:i + 32], "nv12") for i in range(0, B, 32)])          # 32 frames at a time: float64 temporaries
        clip = np.concatenate([E.yuv_to_bgr(yuv[i:i + 32], 32, h, w) for i in range(0, B, 32)])             # the BGR form shows the detector the same pixels
        bgr_np, keep_b = pinned(np.tile(clip, (batches, 1, 1, 1)))
        yuv_np, keep_y = pinned(np.tile(yuv, (batches, 1)))
        ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=obj_shift), synth_reid(1702)
        eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, max_batch=B, max_frame_hw=(h, w), max_crops=B * 64,
                       max_tracks=8192, nn_budget_cap=60, max_candidates=4096, max_trackers=256)
        cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
        args = types.SimpleNamespace(weight=None, mapping=None, output_path=None)
        pipe = CountingPipeline(args, cfg, {"cam": {"cam_04": {"tracking_config": TRACK_CFG}}}, engine=eng, class_names=[str(i) for i in range(NC)])
        sources = {"BGR (3 B/px)": (FrameSource(bgr_np), 3 * h * w), "NV12 (1.5 B/px)": (YuvFrameSource(yuv_np, h, w), 3 * h * w // 2)}
        for name, (src, frame_bytes) in sources.items():
            best, rows = float("inf"), None
            try:
                for rep in range(4):
                    t0 = time.perf_counter()
                    rows, _ = pipe.run_stream(src, "cam_04", zone, batch=B, asynchronous=True, host_frames=True)
                    dt = time.perf_counter() - t0
                    if rep:
                        best = min(best, dt)
            except E.L.VcError as ex:                          # e.g. more candidates than max_candidates on this clip: reported, not hidden
                out.append(f"| {len(src)} x {w}x{h} | {name} | failed: {ex} | | | |")
                print(out[-1], flush=True)
                continue
            fps = len(src) / best
            out.append(f"| {len(src)} x {w}x{h} | {name} | {fps:.0f} | {best / batches * 1e3:.2f} | {fps * frame_bytes / 1e9:.1f} | {len(rows)} |")
            print(out[-1], flush=True)
        eng.close()
        del keep_b, keep_y
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--only-wide", action="store_true", help="section (c) alone")
    a = ap.parse_args()
    out = ["# YUV ingest: conversion kernel and end-to-end rate\n",
           f"`python tools/yuv_ingest_time.py --batches {a.batches}` on {torch.cuda.get_device_name(0)}.\n"]
    if a.only_wide:
        out = [f"`python tools/yuv_ingest_time.py --only-wide` on {torch.cuda.get_device_name(0)}.\n"]
    else:
        worst = kernel_table(out)
        print("\n".join(out), flush=True)
        out.append(f"Worst kernel / copy ratio: {worst:.2f}.\n")
        if not a.skip_e2e:
            e2e_table(out, a.batches)
    wide_table(out)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
