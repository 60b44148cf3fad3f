"""Live counting on the bench workload's configuration (profiles/live_count.md): YOLOv5s 640 x 640 bf16, 80 classes, 256 frames per step of
the stream path (detector of batch i + 1, ReID of batch i, tracker kernel of batch i overlapped, as bench.py runs them), four ways of
counting in ONE process on ONE engine, alternated run by run:
  (a) none          submit / run_async / collect, the rows are dropped;
  (b) host          what CountingPipeline.run_stream does per batch without a live counter: collect, fan the rows out into the per-video
                    lists (`record()`), and NativeCounter.add of the batch's rows; vc_counts once at the end of the run;
  (c) live, every   a LiveCounter attached; the rows are dropped; counts() after every collect;
  (d) live, 16th    the same, counts() after every 16th collect.
Per run: ms per step (`--steps` timed steps behind `--warmup` untimed ones).  `--rounds` rounds of a, b, c, d in that order; the table
gives every figure, the median per variant and the spread (max - min) of each variant over its rounds.
The two new kernels by themselves: the tracker launch (plan, norm, dots, track_batch_kernel, live_count_apply_kernel, merge_free_kernel)
timed with blocking events (`Engine.profile(True)`, category PROF_TRACK) with and without a counter attached -- the difference is
live_count_apply_kernel -- and counts() on an idle engine (live_count_read_kernel, the copy of the tensor and the wait).
The kernels' own times come from a trace, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o live -- python tools/live_count_profile.py --only c --steps 16
usage (GPU box): python tools/live_count_profile.py [--steps 24] [--warmup 3] [--rounds 3] [--out profiles/live_count.md]"""
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
from vehicle_counting_amd.counting import NativeCounter, load_zone_anno  # noqa: E402
from vehicle_counting_amd.synth import synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC, B, SIZE, CLIP = 80, 256, 640, 512
TRACK = dict(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)


def whole_frame_zone(out_dir):
    """tests/test_gpu_bench_config.py's zone: cam_04's directions, the polygon widened to the frame (every row is counted)"""
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
    """one run on new trackers; returns (ms per step, the final counts or None)"""
    ptr = lambda i: dev[(i * B) % CLIP:(i * B) % CLIP + B].data_ptr()
    trackers = [eng.tracker_create(**TRACK) for _ in range(NC)]
    live = native = None
    obj = {"frames": [], "tracks": [], "labels": [], "boxes": []}
    if variant in "cd":
        polygon, directions = load_zone_anno(zone)
        live = E.LiveCounter(eng, [trackers], [polygon], [[sum(directions[k], []) for k in directions]])
    if variant == "b":
        native = NativeCounter(zone, NC)
    every = {"c": 1, "d": 16}.get(variant, 0)

    def collected(i):
        rows, fidx, _ = eng.stream_collect()
        if native is not None:                              # CountingPipeline.run_stream's record() + the counter, per batch
            frames = i * B + 1 + fidx
            obj["frames"].extend(frames.tolist())
            obj["tracks"].extend(rows[:, 4].tolist())
            obj["labels"].extend(rows[:, 5].tolist())
            obj["boxes"].extend(list(rows[:, :4].copy()))
            native.add(frames, rows[:, 4], rows[:, 5], rows[:, :4])
        if every and (i + 1) % every == 0:
            live.counts()

    n = warmup + steps
    t0 = None
    try:
        eng.stream_submit(ptr(0), B, SIZE, SIZE)
        for i in range(n):
            if i + 1 < n:
                eng.stream_submit(ptr(i + 1), B, SIZE, SIZE)
            eng.stream_run_async(trackers, ptr(i), B, SIZE, SIZE)
            if i > 0:
                collected(i - 1)
                if i == warmup:
                    t0 = time.perf_counter()
        collected(n - 1)
        final = native.counts() if native is not None else live.counts()[0] if live is not None else None
        ms = (time.perf_counter() - t0) * 1e3 / steps
    finally:
        eng.stream_reset()
        if live is not None:
            live.close()
        if native is not None:
            native.close()
        for t in trackers:
            eng.tracker_destroy(t)
    return ms, final


def kernels_alone(eng, dev, zone, steps):
    """(tracker launch ms per batch without / with a counter under blocking events, counts() ms on an idle engine)"""
    out = []
    read_ms = 0.0
    for attach in (False, True):
        trackers = [eng.tracker_create(**TRACK) for _ in range(NC)]
        live = None
        if attach:
            polygon, directions = load_zone_anno(zone)
            live = E.LiveCounter(eng, [trackers], [polygon], [[sum(directions[k], []) for k in directions]])
        try:
            for i in range(steps + 1):
                if i == 1:
                    eng.profile(True)
                    eng.profile_reset()
                p = dev[(i * B) % CLIP:(i * B) % CLIP + B].data_ptr()
                eng.stream_submit(p, B, SIZE, SIZE)
                eng.stream_run_packed(trackers, p, B, SIZE, SIZE)
            ms = eng.profile_read(L.PROF_TRACK)["ms"]
            eng.profile(False)
            out.append(ms / steps)
            if live is not None:
                eng.sync()
                live.counts()
                t0 = time.perf_counter()
                for _ in range(50):
                    live.counts()
                read_ms = (time.perf_counter() - t0) * 1e3 / 50
        finally:
            eng.profile(False)
            eng.stream_reset()
            if live is not None:
                live.close()
            for t in trackers:
                eng.tracker_destroy(t)
    return out[0], out[1], read_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["a", "b", "c", "d"], default=None, help="one run of one variant and nothing else: the program of a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1 and a.rounds >= 1
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=1.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, img_size=SIZE, max_batch=B, max_frame_hw=(SIZE, SIZE), max_crops=B * 64,
                   max_tracks=8192, nn_budget_cap=60, max_candidates=4096, max_trackers=256)
    dev = torch.from_numpy(synth_frames(CLIP, SIZE, SIZE, n_obj=12, seed=1702, bounce=True)).cuda()
    names = {"a": "(a) no counting", "b": "(b) host: record() + NativeCounter.add per batch", "c": "(c) live, counts() every batch", "d": "(d) live, counts() every 16th batch"}
    with tempfile.TemporaryDirectory() as tmp:
        zone = whole_frame_zone(tmp)
        if a.only:
            print(f"{names[a.only]}: {run(eng, dev, zone, a.only, a.steps, a.warmup)[0]:.2f} ms per step")
            eng.close()
            return
        run(eng, dev, zone, "a", 4, 1)                      # autotune and first-use allocations, untimed
        run(eng, dev, zone, "c", 4, 1)
        ms = {v: [] for v in names}
        finals = {}
        for r in range(a.rounds):
            for v in names:
                t, final = run(eng, dev, zone, v, a.steps, a.warmup)
                ms[v].append(t)
                finals[v] = final
                print(f"round {r} {names[v]}: {t:.2f} ms per step", flush=True)
        same = bool(np.array_equal(finals["b"], finals["c"][:len(finals["b"])]) and np.array_equal(finals["b"], finals["d"][:len(finals["b"])]))
        trk0, trk1, read_ms = kernels_alone(eng, dev, zone, 8)
    eng.close()
    out = [f"| variant | ms per step of {B} frames, {a.rounds} rounds ({a.steps} steps behind {a.warmup}) | median | spread (max - min) |", "|---|---|---|---|"]
    for v in names:
        out.append(f"| {names[v]} | {' '.join(f'{x:.2f}' for x in ms[v])} | {statistics.median(ms[v]):.2f} | {max(ms[v]) - min(ms[v]):.2f} |")
    out.append("")
    out.append(f"Final counts of (b), (c) and (d) equal: {same} (total {int(finals['b'].sum())}).")
    out.append(f"Tracker launch per batch under blocking events: {trk0:.3f} ms without a counter, {trk1:.3f} ms with one "
               f"(live_count_apply_kernel: the difference, {trk1 - trk0:+.3f} ms).  counts() on an idle engine "
               f"(live_count_read_kernel + the copy of the tensor + the wait): {read_ms:.3f} ms.")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
