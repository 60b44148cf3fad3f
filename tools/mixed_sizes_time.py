"""Sized-batch measurement (profiles/mixed_sizes.md):
 (a) letterbox_frames_kernel against letterbox_kernel / letterbox_copy_kernel on the same uniform bytes in device memory, bf16, BGR -> RGB:
     256 x 720x1280 -> 384x640 (resize) and 256 x 360x640 -> 384x640 (copy); same process, same event pair, the two alternated, best of
     3 x 20 launches each and the spread; outputs compared;
 (b) end to end, bf16 YOLOv5s, batch 256, eight cameras of pinned-host NV12, 4 x 1080p + 4 x 720p, max_frame_hw = (1080, 1920):
       new       one run_streams(mixed_sizes=True) call over the eight cameras (this tree);
       baseline  today's alternative, two run_streams calls, one per size, on the tree given by --baseline-root (a checkout of the parent
                 commit with its library built);
       uniform   one run_streams call over 8 x 720p (this tree): what the sized path costs over a uniform batch of the same count.
     Every run is a child process of its own (one engine per process), the three alternated `--reps` times inside one invocation.
The tool needs a GPU: without one it fails at the first device call.
usage (GPU box): python tools/mixed_sizes_time.py --baseline-root DIR [--out profiles/mixed_sizes.md] [--batches 3] [--reps 2] [--skip-e2e]"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, B, S = 80, 256, 8
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
SIZES = {"1080p": (1080, 1920), "720p": (720, 1280)}


def window_ms(torch, fn, reps=20):
    """`reps` calls enqueued back to back on the null stream between two events: ms per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_table(out):
    import torch

    import vehicle_counting_amd.engine as E
    out.append("## (a) letterbox_frames_kernel against the uniform letterbox kernels, 256 frames per launch, bf16, BGR -> RGB\n")
    out.append("The same packed uniform frames in device memory, the same 256 x 384 x 640 x 4 bf16 destination.  Sized kernel: one table entry per")
    out.append("frame (the table stays in device memory between launches).  Same process, same event pair, the two alternated; 3 windows of 20")
    out.append("back-to-back launches each after 3 warm-up launches; best window, and the spread (max - min over the 3 windows) of each.\n")
    out.append("| frames | case | sized ms (best) | spread | uniform ms (best) | spread | sized / uniform | GB/s written (sized) |")
    out.append("|---|---|---|---|---|---|---|---|")
    nh, nw = 384, 640
    for h, w, case in ((720, 1280, "resize x1/2"), (360, 640, "copy, top 12")):
        src = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device="cuda")
        table = torch.zeros(B * 64, dtype=torch.uint8, device="cuda")
        got, ref = (torch.zeros((B, nh, nw, 4), dtype=torch.bfloat16, device="cuda") for _ in range(2))
        E.letterbox_dev(src.data_ptr(), B, h, w, nh, nw, got.data_ptr(), table_dev_ptr=table.data_ptr(), mode=1)     # builds and uploads the table
        new = lambda: E.letterbox_dev(src.data_ptr(), B, h, w, nh, nw, got.data_ptr(), table_dev_ptr=table.data_ptr(), mode=2)
        old = lambda: E.letterbox_dev(src.data_ptr(), B, h, w, nh, nw, ref.data_ptr())
        for _ in range(3):
            new(); old()
        torch.cuda.synchronize()
        same = torch.equal(got.view(torch.int16), ref.view(torch.int16))
        t_new, t_old = [], []
        for _ in range(3):
            t_new.append(window_ms(torch, new))
            t_old.append(window_ms(torch, old))
        out.append(f"| {B} x {w}x{h} | {case} | {min(t_new):.4f} | {max(t_new) - min(t_new):.4f} | {min(t_old):.4f} | {max(t_old) - min(t_old):.4f} | "
                   f"{min(t_new) / min(t_old):.3f} | {B * nh * nw * 8 / min(t_new) / 1e6:.0f} |" + ("" if same else " OUTPUTS DIFFER"))
        print(out[-1], flush=True)
        del src, got, ref, table
    out.append("")


# ---- (b): one child process per run -------------------------------------------------------------------------------------------------
def child(mode, root, batches):
    """Runs in a process of its own with `root` as the tree the package is imported from; prints one JSON line."""
    sys.path.insert(0, root)
    import torch

    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd.pipeline import CountingPipeline, YuvFrameSource
    from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames
    from vehicle_counting_amd.weights import synth_reid, synth_yolo
    torch.cuda.get_device_name(0)
    per_cam = B * batches // S
    zone = os.path.join(root, "tests", "golden", "cam_04_halfres.json")

    def clip(h, w):
        """a 16-frame scene through 4:2:0, played round and round: (per_cam, h * w * 3 / 2) NV12 in pinned host memory"""
        base = synth_frames(16, h, w, n_obj=12, seed=1702, bounce=True)
        yuv = np.concatenate([bgr_to_yuv420(base[i:i + 4], "nv12") for i in range(0, 16, 4)])
        t = torch.from_numpy(yuv[np.arange(per_cam) % 16]).pin_memory()
        return t

    pools = {k: clip(*hw) for k, hw in SIZES.items() if not (mode == "uniform" and k == "1080p")}
    kinds = ["720p"] * S if mode == "uniform" else ["1080p"] * 4 + ["720p"] * 4
    keep = [torch.roll(pools[k], -c * 3, 0).pin_memory() for c, k in enumerate(kinds)]
    sources = [YuvFrameSource(t.numpy(), *SIZES[k]) for t, k in zip(keep, kinds)]
    names = [f"cam_{c:02d}" for c in range(S)]
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=1.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, max_batch=B, max_frame_hw=(1080, 1920), max_crops=B * 64,
                   max_tracks=8192, nn_budget_cap=60, max_candidates=4096, max_trackers=S * NC)
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=None)
    pipe = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": TRACK_CFG} for n in names}}, engine=eng, class_names=[str(i) for i in range(NC)])

    def run():
        if mode == "baseline":                                  # one call per frame size
            res = []
            for k in ("1080p", "720p"):
                idx = [c for c in range(S) if kinds[c] == k]
                res += pipe.run_streams([sources[c] for c in idx], [names[c] for c in idx], [zone] * len(idx), batch=B, host_frames=True)
            return res
        if mode == "new":
            return pipe.run_streams(sources, names, [zone] * S, batch=B, host_frames=True, mixed_sizes=True)
        return pipe.run_streams(sources, names, [zone] * S, batch=B, host_frames=True)

    times = []
    for rep in range(3):                                        # the first run tunes the convs and allocates
        t0 = time.perf_counter()
        res = run()
        if rep:
            times.append(time.perf_counter() - t0)
    eng.close()
    print("RESULT " + json.dumps({"mode": mode, "frames": S * per_cam, "s": times, "rows": sum(len(r[0]) for r in res),
                                  "rows_720p": sum(len(r[0]) for r, k in zip(res, kinds) if k == "720p")}), flush=True)


def e2e_table(out, baseline_root, batches, reps):
    per_cam = B * batches // S
    out.append(f"## (b) eight cameras, 4 x 1080p + 4 x 720p, pinned-host NV12, bf16 YOLOv5s, batch {B}, {batches} batches ({per_cam} frames per camera)\n")
    out.append("`new`: one `run_streams(mixed_sizes=True)` call.  `baseline`: two `run_streams` calls, one per size (batches of 256 frames from four")
    out.append(f"cameras each), on the parent commit's tree.  `uniform`: one `run_streams` call over 8 x 720p on this tree.  All with `max_frame_hw=(1080, 1920)`,")
    out.append(f"`host_frames=True`, every run a process of its own, the three alternated {reps} times in one invocation; per process one warm-up run, then 2 timed.\n")
    out.append("| run | frames/s (best) | frames/s (all timed runs) | CSV rows (all cameras) | CSV rows (720p cameras) |")
    out.append("|---|---|---|---|---|")
    got = {"new": [], "baseline": [], "uniform": []}
    for _ in range(reps):
        for mode, root in (("new", ROOT), ("baseline", baseline_root), ("uniform", ROOT)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--batches", str(batches)], capture_output=True, text=True,
                               timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise RuntimeError(f"child {mode} failed ({p.returncode}): {p.stderr[-2000:]}")
            got[mode].append(json.loads(line[0][7:]))
            print(got[mode][-1], flush=True)
    for mode, rs in got.items():
        fps = sorted(r["frames"] / s for r in rs for s in r["s"])
        out.append(f"| {mode} | {fps[-1]:.0f} | {' '.join(f'{v:.0f}' for v in fps)} | {rs[0]['rows']} | {rs[0]['rows_720p']} |")
    best = {m: max(r["frames"] / s for r in rs for s in r["s"]) for m, rs in got.items()}
    out.append("")
    out.append(f"new / baseline = {best['new'] / best['baseline']:.3f}; sized path over the uniform 8 x 720p run: {best['uniform'] / best['new']:.3f} x the time per frame.")
    out.append("CSV rows, new against baseline: " + ("equal counts." if got["new"][0]["rows"] == got["baseline"][0]["rows"] else
                                                    f"{got['new'][0]['rows']} against {got['baseline'][0]['rows']} (bf16: the conv tile configuration depends on the batch composition)."))
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.batches)
    sys.path.insert(0, ROOT)
    import torch
    out = ["# Sized batches: cameras of different frame sizes in one detector batch\n",
           f"`python tools/mixed_sizes_time.py --batches {a.batches} --reps {a.reps}` on {torch.cuda.get_device_name(0)}.\n"]
    kernel_table(out)
    if not a.skip_e2e:
        if not a.baseline_root:
            raise SystemExit("--baseline-root is needed for (b): a checkout of the parent commit with its library built (or --skip-e2e)")
        e2e_table(out, os.path.abspath(a.baseline_root), a.batches, a.reps)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
