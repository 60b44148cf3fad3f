"""Multi-camera ingest measurement (profiles/frame_table.md):
 (a) frames_to_bgr_kernel alone -- 256 NV12 frames per launch, 640 x 640 (pitch 768) and 1280 x 720 (pitch 1536), read from eight cameras'
     separate device allocations of 32 surfaces each, interleaved round-robin in the frame table -- against yuv_to_bgr_kernel on the same
     bytes in one contiguous allocation: same process, same event pair, the two alternated, best of 3 x 20 launches each and the spread;
 (b) end to end, bf16 YOLOv5s, eight 640 x 640 cameras, 256 frames per batch: run_streams on eight pinned-host NV12 YuvFrameSources
     (host_frames=True: every batch gathered by stream_stage_frames) against run_streams on the eight BGR FrameSources of the same pixels
     (the interleaved clip built on the host and uploaded whole), with the host time of the staging call per batch.
usage (GPU box): python tools/frame_table_time.py [--out profiles/frame_table.md] [--batches 6] [--skip-e2e]"""
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
from vehicle_counting_amd import _lib as L  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource, YuvFrameSource  # noqa: E402
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC, B, S = 80, 256, 8
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)


def window_ms(fn, reps=20):
    """`reps` calls enqueued back to back on the null stream between two events: ms per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_table(out):
    out.append("## (a) frames_to_bgr_kernel alone, 256 NV12 frames per launch\n")
    out.append(f"Table kernel: the frames are {S} cameras' separate device allocations of {B // S} pitched surfaces each, interleaved round-robin in the")
    out.append("frame table (the table stays in device memory between launches).  Contiguous kernel: `yuv_to_bgr_kernel` on the same bytes in one")
    out.append("allocation, one base and one stride.  Same process, same event pair, the two alternated; 3 windows of 20 back-to-back launches")
    out.append("each after 3 warm-up launches; best window, and the spread (max - min over the 3 windows) of each.  Outputs compared: equal.\n")
    out.append("| frames | pitch | table ms (best) | spread | contiguous ms (best) | spread | table / contiguous |")
    out.append("|---|---|---|---|---|---|---|")
    for h, w, py in ((640, 640, 768), (720, 1280, 1536)):
        off_c = py * ((h + 15) // 16 * 16)
        stride = off_c + py * (h // 2)                                  # whole rows of both planes
        desc = E.yuv_desc("nv12", pitch_y=py, pitch_c=py, offset_c=off_c, frame_stride=stride)
        one = E.yuv_desc("nv12", pitch_y=py, pitch_c=py, offset_c=off_c)
        whole = torch.randint(0, 256, (B, stride), dtype=torch.uint8, device="cuda")
        cams = [whole[c::S].clone() for c in range(S)]                  # camera c's surface t = frame t * S + c of the batch
        frames = [E.frame_src("yuv_dev", cams[f % S][f // S].data_ptr(), one) for f in range(B)]
        table = torch.zeros(B * L.FRAME_ENTRY_BYTES, dtype=torch.uint8, device="cuda")
        got, ref = (torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        E.frames_to_bgr_dev(frames, B, h, w, got.data_ptr(), table.data_ptr())          # builds and uploads the table
        new = lambda: E.frames_to_bgr_dev(None, B, h, w, got.data_ptr(), table.data_ptr())
        old = lambda: E.yuv_to_bgr_dev(whole.data_ptr(), B, h, w, ref.data_ptr(), desc)
        for _ in range(3):
            new(); old()
        torch.cuda.synchronize()
        same = torch.equal(got, ref)
        t_new, t_old = [], []
        for _ in range(3):
            t_new.append(window_ms(new))
            t_old.append(window_ms(old))
        out.append(f"| {B} x {w}x{h} | {py} | {min(t_new):.4f} | {max(t_new) - min(t_new):.4f} | {min(t_old):.4f} | {max(t_old) - min(t_old):.4f} | "
                   f"{min(t_new) / min(t_old):.3f} |" + ("" if same else " OUTPUTS DIFFER"))
        print(out[-1], flush=True)
        del whole, cams, got, ref, table
    out.append("")


def pinned(a):
    """The array in pinned host memory, as a numpy view (pin_memory() inside run_streams is then free: the frames are pinned already)."""
    t = torch.from_numpy(a).pin_memory()
    return t.numpy(), t


def e2e_table(out, batches):
    h = w = 640
    per_cam = B * batches // S
    out.append(f"## (b) run_streams, bf16 YOLOv5s, {S} cameras of {w}x{h}, {B} frames per batch, {batches} batches ({per_cam} frames per camera)\n")
    out.append("One engine.  A synthetic clip through 4:2:0; camera c plays it from another starting frame.  New path: eight NV12 `YuvFrameSource`s in")
    out.append("pinned host memory, `host_frames=True`: every batch is 256 host-to-device copies, one table copy and one `frames_to_bgr_kernel` launch")
    out.append("(`stream_stage_frames`), PCIe inside the clock.  Parent's path: eight BGR `FrameSource`s of the same pixels; `run_streams` stacks the")
    out.append("interleaved clip on the host and uploads it whole, which the first column leaves out (clock from the first `stream_submit`) and the")
    out.append("second includes (the whole call).  One warm-up run per form, then the best of 3.  The two runs do different work; no threshold.\n")
    out.append("| source | frames/s from the first submit | frames/s whole call | CSV rows (all cameras) | host ms in stream_stage_frames per batch (mean / max) |")
    out.append("|---|---|---|---|---|")
    zone = os.path.join(ROOT, "tests", "golden", "cam_04_halfres.json")
    clip = synth_frames(per_cam, h, w, n_obj=12, seed=1702, bounce=True)
    yuv = np.concatenate([bgr_to_yuv420(clip[i:i + 32], "nv12") for i in range(0, per_cam, 32)])
    clip = np.concatenate([E.yuv_to_bgr(yuv[i:i + 32], len(yuv[i:i + 32]), h, w) for i in range(0, per_cam, 32)])   # the BGR form shows the detector the same pixels
    keep = [pinned(np.roll(yuv, -c * (per_cam // S), axis=0)) for c in range(S)]
    yuv_sources = [YuvFrameSource(k[0], h, w) for k in keep]
    bgr_sources = [FrameSource(np.roll(clip, -c * (per_cam // S), axis=0)) for c in range(S)]
    names = [f"cam_{c:02d}" for c in range(S)]
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=1.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, max_batch=B, max_frame_hw=(h, w), max_crops=B * 64,
                   max_tracks=8192, nn_budget_cap=60, max_candidates=4096, max_trackers=S * NC)
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=None)
    pipe = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": TRACK_CFG} for n in names}}, engine=eng, class_names=[str(i) for i in range(NC)])
    # clocks: the first stream_submit of a run, and the host time inside every stream_stage_frames call
    first, stage_s = [], []
    submit, stage = eng.stream_submit, eng.stream_stage_frames

    def timed_submit(*a):
        if not first:
            first.append(time.perf_counter())
        return submit(*a)

    def timed_stage(*a):
        t0 = time.perf_counter()
        r = stage(*a)
        stage_s.append(time.perf_counter() - t0)
        return r

    eng.stream_submit, eng.stream_stage_frames = timed_submit, timed_stage
    n_rows = {}
    for name, srcs, host in (("8 x NV12, pinned host (new)", yuv_sources, True), ("8 x BGR, uploaded whole (parent)", bgr_sources, False)):
        best_sub = best_all = float("inf")
        best_stage = []
        for rep in range(4):
            first.clear(); stage_s.clear()
            t0 = time.perf_counter()
            res = pipe.run_streams(srcs, names, [zone] * S, batch=B, host_frames=host)
            t1 = time.perf_counter()
            if rep:
                best_all = min(best_all, t1 - t0)
                if t1 - first[0] < best_sub:
                    best_sub, best_stage = t1 - first[0], list(stage_s)
        n_rows[name] = sum(len(r[0]) for r in res)
        st = f"{np.mean(best_stage) * 1e3:.3f} / {np.max(best_stage) * 1e3:.3f}" if best_stage else "-"
        out.append(f"| {name} | {S * per_cam / best_sub:.0f} | {S * per_cam / best_all:.0f} | {n_rows[name]} | {st} |")
        print(out[-1], flush=True)
    out.append("")
    out.append("CSV row counts " + ("match." if len(set(n_rows.values())) == 1 else f"DIFFER: {n_rows}."))
    out.append("")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    out = ["# Multi-camera ingest: the frame-table kernel and run_streams from per-camera clips\n",
           f"`python tools/frame_table_time.py --batches {a.batches}` on {torch.cuda.get_device_name(0)}.\n"]
    kernel_table(out)
    if not a.skip_e2e:
        try:
            e2e_table(out, a.batches)
        except L.VcError as ex:                                # reported, not hidden; the kernel table above stands
            out.append(f"(b) failed: {ex}\n")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
