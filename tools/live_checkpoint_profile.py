"""Live checkpoint on the bench's eight-camera operating point (profiles/live_checkpoint.md): YOLOv5s 640 x 640 bf16, 80 classes, eight
cameras interleaved in batches of 256 frames on ONE engine (bench.py's s640_8cam_one_gpu: submit of batch i + 1, run_async_multi of batch i,
collect of batch i - 1), a live counter over all 8 x 80 trackers, and a dense point: eight distinct scenes (bench.py's s640_8cam_distinct_clips).  Per point:
  * the blob's size and its tracks;
  * host time of `checkpoint_begin` inside the running stream (the call enqueues and returns);
  * `begin` -> `end` returned inside the running stream (`end` behind the collect of the checkpointed batch's own rows, as run_streams
    does it), the host time of `end` alone, and both on a drained engine (plan + pack + the copy to pinned memory and nothing else);
  * the stream's frames/s with checkpoint_every in {none, 64, 8} batches, alternated run by run, `--rounds` rounds: every figure, the
    median and the spread;
  * the parent commit's only route to the tracker part of the same data, three times: with one batch in flight stop submitting, drain
    (collect it), `tracker_snapshot` of every tracker -- its wall time is the stream's stall.  (It has no way to the counter's state at all.)
Kernel times (live_ckpt_plan_kernel, live_ckpt_pack_kernel beside track_batch_kernel) come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/live_checkpoint_profile.py --trace
usage (GPU box): python tools/live_checkpoint_profile.py [--steps 128] [--warmup 4] [--rounds 3] [--out profiles/live_checkpoint.md]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd.counting import load_zone_anno  # noqa: E402
from vehicle_counting_amd.synth import synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402
from live_overlay_profile import whole_frame_zone  # noqa: E402

NC, B, SIZE, CLIP, S = 80, 256, 640, 512, 8
TRACK = dict(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
CKPT_BYTES = 1 << 30


class Point:
    def __init__(self, distinct):
        n_obj = 12
        ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=1.0), synth_reid(1702)
        self.eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, img_size=SIZE, max_batch=B, max_frame_hw=(SIZE, SIZE),
                            max_crops=B * (160 if distinct else 64), max_tracks=32768 if distinct else 8192, nn_budget_cap=60, max_candidates=4096, max_trackers=S * NC)
        one = synth_frames(CLIP // S, SIZE, SIZE, n_obj=n_obj, seed=1702, bounce=True)
        per_cam = [one] * S                                       # bench.py: every camera shows one clip; distinct: eight scenes, several times the boxes
        if distinct:
            per_cam = [one] + [synth_frames(CLIP // S, SIZE, SIZE, n_obj=n_obj, seed=1702 + 101 * c, bounce=True) for c in range(1, S)]
        self.dev = torch.from_numpy(np.stack(per_cam, 1).reshape((CLIP,) + one.shape[1:])).cuda()          # frame j: camera j % S, time j // S
        self.cams = np.tile(np.arange(S, dtype=np.int32), B // S)

    def ptr(self, i):
        return self.dev[(i * B) % CLIP:(i * B) % CLIP + B].data_ptr()

    def run(self, zone, steps, warmup, every=None, probe=False):
        """one run on new trackers.  Returns ms per step; with probe also (blob bytes, tracks, begin ms list, begin->end ms list in the
        stream, begin->end ms drained, snapshot route ms, snapshot bytes)"""
        eng = self.eng
        tids = np.array([[eng.tracker_create(**TRACK) for _ in range(NC)] for _ in range(S)], np.int32)
        polygon, directions = load_zone_anno(zone)
        dirs = [sum(directions[k], []) for k in directions]
        live = E.LiveCounter(eng, tids, [polygon] * S, [dirs] * S)
        if every or probe:
            live.enable_checkpoint(CKPT_BYTES)
        t_begin, t_ready, t_end, pending, blob = [], [], [], None, b""
        n = warmup + steps
        try:
            eng.stream_submit(self.ptr(0), B, SIZE, SIZE)
            for i in range(n):
                if i + 1 < n:
                    eng.stream_submit(self.ptr(i + 1), B, SIZE, SIZE)
                eng.stream_run_async_multi(tids, self.cams, self.ptr(i), B, SIZE, SIZE)
                if every and i >= warmup and (i + 1) % every == 0:
                    t0 = time.perf_counter()
                    live.checkpoint_begin()
                    pending = (i, time.perf_counter())
                    t_begin.append((pending[1] - t0) * 1e3)
                if i > 0:
                    eng.stream_collect()
                    if pending is not None and pending[0] <= i - 1:      # the checkpointed batch's own rows are in: as run_streams does it
                        t0 = time.perf_counter()
                        blob = live.checkpoint_end()
                        t_end.append((time.perf_counter() - t0) * 1e3)
                        t_ready.append((time.perf_counter() - pending[1]) * 1e3)
                        pending = None
                    if i == warmup:
                        t0_run = time.perf_counter()
            eng.stream_collect()
            if pending is not None:
                live.checkpoint_end()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0_run) * 1e3 / steps
            if not probe:
                return ms
            # drained engine: plan + pack + copy and nothing else
            drained = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                live.checkpoint_begin()
                blob = live.checkpoint_end()
                drained.append((time.perf_counter() - t0) * 1e3)
            # the parent's route, three times: one batch in flight, then stop submitting, drain (its collect), snapshot every tracker
            snap_ms = []
            for j in range(n, n + 3):
                eng.stream_submit(self.ptr(j), B, SIZE, SIZE)
                eng.stream_run_async_multi(tids, self.cams, self.ptr(j), B, SIZE, SIZE)
                t0 = time.perf_counter()
                eng.stream_collect()
                snaps = [eng.tracker_snapshot(int(t)) for t in tids.reshape(-1)]
                snap_ms.append((time.perf_counter() - t0) * 1e3)
            n_tracks = int(np.frombuffer(blob, "<i4", 1, 28)[0])
            return ms, len(blob), n_tracks, t_begin, (t_ready, t_end), drained, snap_ms, sum(len(s) for s in snaps)
        finally:
            eng.stream_reset()
            live.close()
            for t in tids.reshape(-1):
                eng.tracker_destroy(int(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="one short run with a checkpoint every 4 batches and nothing else (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1 and a.rounds >= 1
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        zone = whole_frame_zone(tmp)
        for name, distinct in (("s640_8cam_one_gpu (eight cameras, one clip)", False), ("dense: s640_8cam_distinct_clips (eight scenes, several times the tracks)", True)):
            p = Point(distinct)
            p.run(zone, 4, 1)                                   # autotune and first-use allocations, untimed
            if a.trace:
                p.run(zone, 24, 4, every=4)
                p.eng.close()
                continue
            fps = {None: [], 64: [], 8: []}
            for r in range(a.rounds):
                for every in fps:
                    fps[every].append(B * 1e3 / p.run(zone, a.steps, a.warmup, every=every))
                    print(f"{name} round {r} checkpoint_every={every}: {fps[every][-1]:.0f} frames/s", flush=True)
            _, size, n_tracks, t_begin, (t_ready, t_end), drained, snap_ms, snap_bytes = p.run(zone, 32, a.warmup, every=4, probe=True)
            p.eng.close()
            med = {k: statistics.median(v) for k, v in fps.items()}
            out += [f"### {name}", "",
                    f"Blob: {size} bytes ({size / 1e6:.2f} MB), {n_tracks} tracks of {S * NC} trackers.", "",
                    f"| | every figure | median | spread (max - min) |", "|---|---|---|---|",
                    f"| host time of checkpoint_begin in the stream, ms | {' '.join(f'{x:.3f}' for x in t_begin)} | {statistics.median(t_begin):.3f} | {max(t_begin) - min(t_begin):.3f} |",
                    f"| begin -> end returned in the stream (the next batch's run and the batch's own collect in between), ms | {' '.join(f'{x:.2f}' for x in t_ready)} | {statistics.median(t_ready):.2f} | {max(t_ready) - min(t_ready):.2f} |",
                    f"| of that, host time of checkpoint_end (wait + the copy out of pinned memory into a bytes object), ms | {' '.join(f'{x:.2f}' for x in t_end)} | {statistics.median(t_end):.2f} | {max(t_end) - min(t_end):.2f} |",
                    f"| begin -> end ready on a drained engine (plan + pack + copy), ms | {' '.join(f'{x:.2f}' for x in drained)} | {statistics.median(drained):.2f} | {max(drained) - min(drained):.2f} |"]
            for every, v in fps.items():
                out.append(f"| frames/s, checkpoint_every = {every} ({a.steps} steps of {B} frames behind {a.warmup}) | {' '.join(f'{x:.0f}' for x in v)} | {med[every]:.0f} | {max(v) - min(v):.0f} |")
            step_ms = B * 1e3 / med[None]
            out += ["", f"Cost per checkpoint from the medians: every 64: {(B * 64e3 / med[64] - B * 64e3 / med[None]):+.2f} ms, every 8: {(B * 8e3 / med[8] - B * 8e3 / med[None]):+.2f} ms "
                        f"(a step is {step_ms:.2f} ms; differences below the spread above are noise).",
                    f"Parent's route (one batch in flight: stop submitting, collect it, tracker_snapshot of all {S * NC} trackers), ms of wall time with nothing submitted = the stream's stall: "
                    f"{' '.join(f'{x:.1f}' for x in snap_ms)}, median {statistics.median(snap_ms):.1f}, spread {max(snap_ms) - min(snap_ms):.1f} = "
                    f"{statistics.median(snap_ms) / step_ms:.1f} steps; {snap_bytes} bytes, trackers only -- it cannot capture the counter's state.  "
                    f"Ratio to begin -> end on the drained engine: {statistics.median(snap_ms) / statistics.median(drained):.0f}x.", ""]
            text = "\n".join(out) + "\n"
            if a.out:                                           # after every point: a later point's failure keeps the earlier table
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write(text)
    print("\n".join(out))


if __name__ == "__main__":
    main()
