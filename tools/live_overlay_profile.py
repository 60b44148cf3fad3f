"""Live annotated video on the bench workload's configuration (profiles/live_overlay.md): YOLOv5s 640 x 640 bf16, 80 classes, 256 frames per
step of the stream path (submit of batch i + 1, run_async of batch i, collect of batch i - 1, as bench.py runs them), with a live counter
attached, in ONE process on ONE engine, alternated run by run:
  (a) counter only      the rows are dropped: what the parent commit can run (`--only a` uses nothing newer, so the same file measures
                        a checkout of the parent);
  (b) overlay, rendered the overlay enabled: every batch's lists are built on the device behind its tracker launch and the batch is
                        rendered through Renderer.submit_live into a device NV12 surface, two batches in flight -- what
                        CountingPipeline.run_stream(annotate=) does per batch;
  (c) host lists        the only alternative the parent has: collect the rows, build the LiveVisualizer lists in Python, Renderer.submit
                        (`--alt-steps` steps: a step takes seconds).
Per run: ms per step and frames per second.  `--rounds` rounds of a, b; the table gives every figure, the median and the spread
(max - min).  The build launches by themselves: the tracker launch timed with blocking events (`Engine.profile(True)`, category
PROF_TRACK) without and with the overlay -- the difference is live_count_read_kernel + live_overlay_count_kernel +
live_overlay_build_kernel and the two small copies.
usage (GPU box): python tools/live_overlay_profile.py [--steps 20] [--warmup 3] [--rounds 3] [--alt-steps 2] [--out profiles/live_overlay.md]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402
from vehicle_counting_amd.counting import load_zone_anno  # noqa: E402
from vehicle_counting_amd.synth import synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC, B, SIZE, CLIP = 80, 256, 640, 512
TRACK = dict(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
ROWS_PER_FRAME = 64


def whole_frame_zone(out_dir):
    """tests/test_gpu_bench_config.py's zone: cam_04's directions, the polygon widened to the frame (every row is drawn)"""
    with open(os.path.join(ROOT, "tests", "golden", "cam_04_halfres.json")) as f:
        z = json.load(f)
    for sh in z["shapes"]:
        if sh["label"] == "zone":
            sh["points"] = [[0.0, 0.0], [float(SIZE), 0.0], [float(SIZE), float(SIZE)], [0.0, float(SIZE)]]
    path = os.path.join(out_dir, "zone.json")
    with open(path, "w") as f:
        json.dump(z, f)
    return path


def run(eng, dev, zone, variant, steps, warmup):
    """one run on new trackers; returns (ms per step, primitives of the last batch or 0)"""
    ptr = lambda i: dev[(i * B) % CLIP:(i * B) % CLIP + B].data_ptr()
    trackers = [eng.tracker_create(**TRACK) for _ in range(NC)]
    polygon, directions = load_zone_anno(zone)
    live = E.LiveCounter(eng, [trackers], [polygon], [[sum(directions[k], []) for k in directions]])
    rnd = lv = surf = None
    last_prims = 0
    if variant in "bc":
        rnd = E.Renderer(eng, max_batch=B, max_hw=(SIZE, SIZE), depth=2)
        surf = torch.zeros((2, B * SIZE * SIZE * 3 // 2), dtype=torch.uint8, device="cuda")         # two encoder surfaces, used in turn
    if variant == "b":
        live.enable_overlay([list(directions)], max_batch=B, max_rows_per_frame=ROWS_PER_FRAME, depth=2)
    if variant == "c":
        from vehicle_counting_amd.overlay import LiveVisualizer
        lv = LiveVisualizer([polygon], [directions], NC)

    def collected(i):
        nonlocal last_prims
        rows, fidx, _ = eng.stream_collect()
        if lv is not None:                                  # the parent's only way to the same picture: lists built in Python from the collected rows
            prims, first = lv.batch_prims([0] * B, range(i * B + 1, (i + 1) * B + 1), [rows[fidx == f] for f in range(B)], (SIZE, SIZE))
            last_prims = int(first[-1])
            while rnd.outstanding >= 2:
                rnd.collect()
            rnd.submit(ptr(i), B, SIZE, SIZE, surf[i % 2].data_ptr(), kind="bgr_dev", prims=prims, first=first, out_is_dev=True)

    n = warmup + steps
    t0 = None
    try:
        eng.stream_submit(ptr(0), B, SIZE, SIZE)
        for i in range(n):
            if variant == "b":
                while rnd.outstanding >= 2:                 # a list buffer is free for the run below
                    rnd.collect()
            if i + 1 < n:
                eng.stream_submit(ptr(i + 1), B, SIZE, SIZE)
            eng.stream_run_async(trackers, ptr(i), B, SIZE, SIZE)
            if variant == "b":
                rnd.submit_live(live, ptr(i), B, SIZE, SIZE, surf[i % 2].data_ptr(), kind="bgr_dev", out_is_dev=True)
            if i > 0:
                collected(i - 1)
                if i == warmup:
                    t0 = time.perf_counter()
        collected(n - 1)
        while rnd is not None and rnd.outstanding:
            rnd.collect()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
    finally:
        eng.stream_reset()
        if rnd is not None:
            rnd.close()
        live.close()
        for t in trackers:
            eng.tracker_destroy(t)
    return ms, last_prims


def launches_alone(eng, dev, zone, steps):
    """tracker launch ms per batch under blocking events without / with the overlay, and the primitives of the last batch"""
    out, n_prims = [], 0
    for overlay in (False, True):
        trackers = [eng.tracker_create(**TRACK) for _ in range(NC)]
        polygon, directions = load_zone_anno(zone)
        live = E.LiveCounter(eng, [trackers], [polygon], [[sum(directions[k], []) for k in directions]])
        if overlay:
            live.enable_overlay([list(directions)], max_batch=B, max_rows_per_frame=ROWS_PER_FRAME, depth=1)
        try:
            for i in range(steps + 1):
                if i == 1:
                    eng.profile(True)
                    eng.profile_reset()
                p = dev[(i * B) % CLIP:(i * B) % CLIP + B].data_ptr()
                eng.stream_submit(p, B, SIZE, SIZE)
                eng.stream_run_packed(trackers, p, B, SIZE, SIZE)
                if overlay:
                    n_prims = len(live.overlay_lists(cap_prims=1 << 22)[0])
            out.append(eng.profile_read(L.PROF_TRACK)["ms"] / steps)
        finally:
            eng.profile(False)
            eng.stream_reset()
            live.close()
            for t in trackers:
                eng.tracker_destroy(t)
    return out[0], out[1], n_prims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--alt-steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None, help="`--rounds` runs of one variant and nothing else")
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1 and a.rounds >= 1
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=1.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, img_size=SIZE, max_batch=B, max_frame_hw=(SIZE, SIZE), max_crops=B * 64,
                   max_tracks=8192, nn_budget_cap=60, max_candidates=4096, max_trackers=256)
    dev = torch.from_numpy(synth_frames(CLIP, SIZE, SIZE, n_obj=12, seed=1702, bounce=True)).cuda()
    names = {"a": "(a) live counter only", "b": "(b) overlay built on the device, rendered by submit_live", "c": "(c) lists built in Python from collected rows, Renderer.submit"}
    with tempfile.TemporaryDirectory() as tmp:
        zone = whole_frame_zone(tmp)
        run(eng, dev, zone, "a", 4, 1)                      # autotune and first-use allocations, untimed
        if a.only:
            for r in range(a.rounds):
                print(f"round {r} {names[a.only]}: {run(eng, dev, zone, a.only, a.steps, a.warmup)[0]:.2f} ms per step", flush=True)
            eng.close()
            return
        run(eng, dev, zone, "b", 4, 1)
        ms = {"a": [], "b": []}
        for r in range(a.rounds):
            for v in ms:
                ms[v].append(run(eng, dev, zone, v, a.steps, a.warmup)[0])
                print(f"round {r} {names[v]}: {ms[v][-1]:.2f} ms per step", flush=True)
        alt, alt_prims = run(eng, dev, zone, "c", a.alt_steps, 1)
        print(f"{names['c']}: {alt:.1f} ms per step", flush=True)
        trk0, trk1, n_prims = launches_alone(eng, dev, zone, 8)
    eng.close()
    out = [f"| variant | ms per step of {B} frames, {a.rounds} rounds ({a.steps} steps behind {a.warmup}) | median | spread (max - min) | frames/s at the median |", "|---|---|---|---|---|"]
    for v in ms:
        med = statistics.median(ms[v])
        out.append(f"| {names[v]} | {' '.join(f'{x:.2f}' for x in ms[v])} | {med:.2f} | {max(ms[v]) - min(ms[v]):.2f} | {B * 1e3 / med:.0f} |")
    out.append(f"| {names['c']} | {alt:.1f} ({a.alt_steps} steps behind 1, one run) | {alt:.1f} | - | {B * 1e3 / alt:.0f} |")
    out.append("")
    out.append(f"Tracker launch per batch under blocking events: {trk0:.3f} ms with the counter alone, {trk1:.3f} ms with the overlay "
               f"(live_count_read_kernel + live_overlay_count_kernel + live_overlay_build_kernel + two small copies: the difference, {trk1 - trk0:+.3f} ms); "
               f"the last batch's lists hold {n_prims} primitives ({n_prims * 48 / 1e6:.1f} MB), the Python lists of (c) {alt_prims}.")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
