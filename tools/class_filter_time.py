"""Class filter and label map on the bench workload's configuration (profiles/class_filter.md): YOLOv5s 640 x 640 bf16, 80 classes, 256
frames per step of the stream path (detector of batch i + 1, ReID of batch i, tracker kernel of batch i overlapped, as bench.py runs
them), three maps in ONE process on ONE engine:
  no map            what the engine did before: no launch is added;
  identity map      every class kept under its own label: the cost of the two added launches (cand_class_filter_kernel, det_relabel_kernel);
  {2, 3, 5, 7}      cars, motorcycles, buses and trucks of a COCO head as labels 0..3: what a vehicle counter asks for.
Per run: ms per step (three repeats of `--steps` timed steps behind `--warmup` untimed ones), boxes that reached the ReID stage and crops
embedded per step (vc_stream_crop_stats over one untimed pass of the clip), and the trackers the run steps per camera.  The last row
repeats the first: the spread between them is the noise of the box.
usage (GPU box): python tools/class_filter_time.py [--steps 40] [--warmup 3] [--out profiles/class_filter_rows.md]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd.synth import synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC, B, SIZE, CLIP = 80, 256, 640, 512
TRACK = dict(max_dist=0.2, min_confidence=0.25, nms_max_overlap=0.5, max_iou_distance=0.6, max_age=30, n_init=3, nn_budget=60)
VEHICLES = [2, 3, 5, 7]


def reset(eng, trackers):
    eng.stream_reset()
    for t in trackers:
        eng.tracker_reset(t)


def counts(eng, dev, trackers):
    """the clip once, batch by batch with nothing overlapped: (boxes that reached ReID, crops embedded) per step.  Also what warms the
    run up: the ReID crop counts of the timed steps are the ones autotuned here."""
    reset(eng, trackers)
    nb = CLIP // B
    for i in range(nb):
        p = dev[i * B:(i + 1) * B].data_ptr()
        eng.stream_submit(p, B, SIZE, SIZE)
        eng.stream_run_packed(trackers, p, B, SIZE, SIZE)
    boxes, crops = eng.stream_crop_stats()
    return boxes / nb, crops / nb


def timed(eng, dev, trackers, steps, warmup):
    """`warmup` + `steps` steps of the three overlapped stages; ms per step from the moment the last warm-up step's rows are on the host
    to the moment the last step's are (the host clock around work that ends in a wait for the device)"""
    ptr = lambda i: dev[(i * B) % CLIP:(i * B) % CLIP + B].data_ptr()
    reset(eng, trackers)
    n = warmup + steps
    t0 = None
    eng.stream_submit(ptr(0), B, SIZE, SIZE)
    for i in range(n):
        if i + 1 < n:
            eng.stream_submit(ptr(i + 1), B, SIZE, SIZE)
        eng.stream_run_async(trackers, ptr(i), B, SIZE, SIZE)
        if i > 0:
            eng.stream_collect()
            if i == warmup:
                t0 = time.perf_counter()
    eng.stream_collect()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1, "the clock starts when the last warm-up step comes back"
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=1.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="bf16", model_name="yolov5s", num_classes=NC, img_size=SIZE, max_batch=B, max_frame_hw=(SIZE, SIZE), max_crops=B * 64,
                   max_tracks=8192, nn_budget_cap=60, max_candidates=4096, max_trackers=256)
    frames = synth_frames(CLIP, SIZE, SIZE, n_obj=12, seed=1702, bounce=True)
    dev = torch.from_numpy(frames).cuda()
    trackers = [eng.tracker_create(**TRACK) for _ in range(NC)]
    out = ["| run | trackers per camera | ms per step, 3 repeats | boxes to ReID per step | crops embedded per step |", "|---|---|---|---|---|"]
    for name, classes in (("no map", None), ("identity map", list(range(NC))), ("{2, 3, 5, 7} -> 0..3", VEHICLES), ("no map (again)", None)):
        eng.set_class_map(classes)
        n_labels = eng.num_labels
        boxes, crops = counts(eng, dev, trackers[:n_labels])
        t = [timed(eng, dev, trackers[:n_labels], a.steps, a.warmup) for _ in range(3)]
        out.append(f"| {name} | {n_labels} | {' '.join(f'{x:.2f}' for x in t)} | {boxes:.0f} | {crops:.0f} |")
        print(out[-1], flush=True)
    eng.close()
    text = "\n".join(out) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
