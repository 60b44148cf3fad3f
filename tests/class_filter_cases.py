"""Inputs and CPU references for the class filter and label map (class_filter.hip): cand_class_filter_kernel in front of the NMS kernels,
det_relabel_kernel behind them.

Candidate-level cases are built from tests/detect_post_cases.py (quarter-pixel boxes, 8 classes): the reference of a case is its frames
with the dropped candidates REMOVED, put through the same float32 oracle (nms_keep32 / nms_rows), and the class column replaced by the
label.  `kept_idx` is the positions of the kept candidates in ascending order (the filter is stable).

`run_video_classes` is oracle/pipeline.py::run_video restated with `classes` handed to autoshape_detect (where upstream applies it: in
front of the NMS and the max_det cut) and the relabel in front of tracker.run; trackers and counters are per label.

tests/test_class_filter_cases.py asserts the builders' conditions on the CPU; tests/test_gpu_class_filter.py runs the kernels on them."""
import functools

import numpy as np

from detect_post_cases import _frame, nms_keep32, nms_rows, rand_frame

NC = 8
SWAP = {3: 1, 7: 0}
MERGE = {3: 0, 7: 0}
SPARSE = {0: 2, 1: 2, 3: 0, 5: 1, 6: 1}
EDGE_KEPT = (0, 1, 63, 64, 65, 255, 256, 257)
EDGE_N = 600
PLACEMENTS = ("first", "last", "interleaved")
MIXED_COUNTS = (0, 1, 64, 600, 4096)


def table_of(mapping, nc=NC):
    t = np.full(nc, -1, np.int32)
    for c, l in mapping.items():
        t[c] = l
    return t


class FilterCase:
    """frames: list of (boxes [n][4] f32, conf [n] f32, cls [n] i32); table: label_of_class [NC]"""

    def __init__(self, name, frames, table, iou=0.45, max_det=300, max_cand=1024, geoms=None, notes=None):
        self.name, self.frames, self.table, self.iou, self.max_det, self.max_cand, self.notes = name, frames, np.asarray(table, np.int32), iou, max_det, max_cand, notes or {}
        self.geoms = geoms                                # per frame (net_h, net_w, src_h, src_w) for scale_coords, or None: network pixels

    @property
    def counts(self):
        return [len(f[1]) for f in self.frames]


def _reclass(frame, kept_pos, table, seed):
    """the frame with kept classes at `kept_pos` and dropped classes everywhere else (a copy; rand_frame's arrays are shared)"""
    boxes, conf, _ = frame
    rng = np.random.default_rng(seed)
    keep_cls, drop_cls = np.flatnonzero(table >= 0), np.flatnonzero(table < 0)
    cls = rng.choice(drop_cls, len(conf)).astype(np.int32)
    cls[kept_pos] = rng.choice(keep_cls, len(kept_pos))
    return boxes.copy(), conf.copy(), cls


def kept_positions(k, n, placement):
    if placement == "first":
        return np.arange(k)
    if placement == "last":
        return np.arange(n - k, n)
    return np.round(np.linspace(0, n - 1, k)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def filter_cases():
    """name -> FilterCase.  Built once; the tests must not write into the frames."""
    cases = []
    swap, merge = table_of(SWAP), table_of(MERGE)
    # kept-count edges of the 256-candidate chunk and the 64-lane ballot: 600 candidates (three chunks, the last one partial), one frame
    # per kept count, the kept candidates first / last / spread over the frame
    for p, placement in enumerate(PLACEMENTS):
        frames = [_reclass(rand_frame(400 + i, EDGE_N, NC), kept_positions(k, EDGE_N, placement), swap, 500 + 10 * p + i) for i, k in enumerate(EDGE_KEPT)]
        cases.append(FilterCase(f"edges_{placement}", frames, swap, notes={"kept": EDGE_KEPT, "placement": placement}))

    cases.append(FilterCase("identity", [rand_frame(420, EDGE_N, NC), rand_frame(421, 257, NC)], np.arange(NC)))
    cases.append(FilterCase("all_dropped", [_reclass(rand_frame(422, 300, NC), np.zeros(0, np.int64), swap, 522)], swap))

    # two boxes with IoU 0.6 (> 0.45): classes 3 and 7 share label 0 and both survive (the NMS separates ORIGINAL classes); the same boxes
    # with one class lose the weaker one
    pair = [[100, 100, 200, 200], [125, 100, 225, 200]]
    cases.append(FilterCase("merged", [_frame(pair, [0.9, 0.8], [3, 7])], merge, notes={"iou": 0.6, "rows": 2}))
    cases.append(FilterCase("same_class", [_frame(pair, [0.9, 0.8], [3, 3])], merge, notes={"iou": 0.6, "rows": 1}))

    # max_det = 10 binds: a 8 x 5 lattice of disjoint 20 px boxes; 24 of classes 3 / 7, 16 dropped ones that hold the HIGHEST scores, so
    # a filter behind the cut would return fewer than 10 rows
    gx, gy = np.meshgrid(np.arange(8) * 40.0, np.arange(5) * 40.0)
    xy = np.stack([gx.reshape(-1), gy.reshape(-1)], 1) + 0.25
    rng = np.random.default_rng(430)
    cls = np.array([3, 7] * 12 + [0, 1, 2, 4, 5, 6, 0, 1, 2, 4, 5, 6, 0, 1, 2, 4], np.int32)
    score = np.concatenate([0.3 + rng.permutation(24) / 256.0, 0.6 + rng.permutation(16) / 256.0])
    perm = rng.permutation(40)
    cases.append(FilterCase("maxdet10", [_frame(np.concatenate([xy, xy + 20.0], 1)[perm], score[perm], cls[perm])], swap, max_det=10, max_cand=64,
                            notes={"kept": 24}))

    # one batch of frames of very different sizes: empty, one candidate, one wave, three chunks, a full 4096-candidate buffer
    mixed = []
    for i, n in enumerate(MIXED_COUNTS):
        b, s, c = rand_frame(440 + i, n, NC, 160, 60) if n == 4096 else rand_frame(440 + i, n, NC)
        mixed.append((b, s, np.full(n, 3, np.int32)) if n == 1 else (b, s, c))
    # scale_coords behind the filter: a geometry per frame, boxes past every edge of the network frame (the "geometry" case of detect_post_cases)
    geoms = [(384, 640, 720, 1280), (448, 640, 333, 500)]
    gframes = []
    for i, g in enumerate(geoms):
        b, s, c = rand_frame(450 + i, 200, NC, extent=g[1] + 150)
        gframes.append(_frame(b - np.float32(120.0), s, c))
    cases.append(FilterCase("geometry", gframes, table_of(SPARSE), max_cand=256, geoms=geoms))
    cases.append(FilterCase("mixed", mixed, table_of(SPARSE), max_cand=4096, notes={"counts": MIXED_COUNTS}))
    return {c.name: c for c in cases}


def filtered_frame(frame, table):
    """(the frame without its dropped candidates, positions of the kept ones)"""
    boxes, conf, cls = frame
    pos = np.flatnonzero(table[cls] >= 0)
    return (boxes[pos], conf[pos], cls[pos]), pos


@functools.lru_cache(maxsize=None)
def filter_ref(name):
    """per frame: (expected rows [m][6] with the label in the class column, positions of the kept candidates)"""
    case = filter_cases()[name]
    out = []
    for f, frame in enumerate(case.frames):
        sub, pos = filtered_frame(frame, case.table)
        rows = nms_rows(sub, nms_keep32(sub, case.iou), case.max_det, case.geoms[f] if case.geoms else None)
        rows[:, 5] = case.table[rows[:, 5].astype(np.int64)].astype(np.float32)
        out.append((rows, pos))
    return out


def relabel_dets(det, table, drop=True):
    """host restatement on detector rows: rows of dropped classes removed, class column -> label"""
    if not len(det):
        return det
    lab = np.asarray(table)[det[:, 5].astype(np.int64)]
    out = det[lab >= 0].copy() if drop else det.copy()
    out[:, 5] = lab[lab >= 0] if drop else lab
    return out


CLIP = dict(T=18, H=360, W=640, n_obj=6, seed=3)                     # the clip of tests/test_gpu_pipeline.py::test_csv_parity
CLIP_YOLO = dict(nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0)


@functools.lru_cache(maxsize=None)
def clip():
    """(frames [18][360][640][3] BGR, detector weights, ReID weights) of test_csv_parity"""
    from vehicle_counting_amd.synth import synth_frames
    from vehicle_counting_amd.weights import synth_reid, synth_yolo
    frames = synth_frames(CLIP["T"], CLIP["H"], CLIP["W"], n_obj=CLIP["n_obj"], seed=CLIP["seed"])
    return frames, synth_yolo("yolov5s", **CLIP_YOLO), synth_reid(1702)


@functools.lru_cache(maxsize=None)
def _clip_pred(i):
    """frame i of the clip through the oracle's preprocess + forward (the part of autoshape_detect no `classes` / `max_det` reaches)"""
    from oracle import yolov5 as oy
    frames, ysd, _ = clip()
    x, shape0, shape1 = oy.preprocess([frames[i][:, :, ::-1]], 640)
    return oy.forward(ysd, x, "yolov5s", NC).numpy(), shape0, shape1


def clip_detect(i, classes=None, max_det=300, conf=0.25, iou=0.45):
    """oracle.yolov5.autoshape_detect on frame i of the clip (its own body, the forward pass shared between calls)"""
    from oracle import yolov5 as oy
    pred, shape0, shape1 = _clip_pred(i)
    d = oy.non_max_suppression(pred, conf, iou, classes, max_det)[0]
    return np.concatenate((oy.scale_coords(shape1, d[:, :4], shape0[0]), d[:, 4:]), 1) if len(d) else d


def run_video_classes(reid_sd, tracking_config, zone_path, mapping, nc=NC, max_det=300):
    """oracle/pipeline.py::run_video on the clip with the class filter in the detector (autoshape_detect(..., classes, ...)) and the
    relabel in front of tracker.run: (rows, counts, detections per frame).  mapping: {class: label}."""
    from oracle import counting as oc
    from oracle import deepsort as od
    from oracle import reid as orr
    from oracle import yolov5 as oy
    frames_bgr = clip()[0]
    table = table_of(mapping, nc)
    n_labels = int(table.max()) + 1
    tracker = od.VideoTrackerOracle(n_labels, tracking_config, orr.make_embedder(reid_sd))
    polygon, dirs = oc.load_zone(zone_path)
    obj = {"frames": [], "tracks": [], "labels": [], "boxes": []}
    n_det = []
    for i, f in enumerate(frames_bgr):
        det = relabel_dets(clip_detect(i, sorted(mapping), max_det), table)
        m = oy.marshal_like_reference(det)
        n_det.append(len(m["bboxes"]))
        if len(m["bboxes"]) == 0:
            continue
        res = tracker.run(f, m["bboxes"], m["classes"], m["scores"])
        for j in range(len(res["boxes"])):
            obj["frames"].append(i + 1)
            obj["tracks"].append(int(res["tracks"][j]))
            obj["labels"].append(int(res["labels"][j]))
            obj["boxes"].append(np.asarray(res["boxes"][j]))
    td = oc.build_track_dict(n_labels, polygon, dirs, obj["frames"], obj["tracks"], obj["labels"], obj["boxes"])
    rows = oc.csv_rows(td)
    return rows, oc.direction_counts(rows, list(dirs.keys()), n_labels), n_det
