"""Cases and NumPy restatement of the live counter (vehicle-counting_amd/csrc/live_count.hip), shared by tests/test_live_count_cases.py
(CPU: the restatement against NativeCounter over every row prefix) and tests/test_gpu_live_count.py (the kernels against the restatement).

A case is a short multi-camera clip described by its TRACKS -- which tracker owns a track, its id, the frames at which it emits a
row and the box of each, the frame at which the tracker deletes it -- and the cameras' zones.  `build(case, batch)` cuts the clip
into batches of `batch` frames and lays every batch out as the tracker kernel hands it to the counter: rows in an arena with the
pool slot of each, tasks (tracker, frame, label, first row, rows) grouped by tracker, the frame numbers, the freed list.  Slots
come from a pool that behaves like the engine's: taken from a stack inside a batch, freed slots only returned to it BETWEEN batches
(a slot never changes owner inside a batch), most recently freed first.

`Model` is the state machine of DESIGN.md 5 written with the pure-Python counting functions of vehicle_counting_amd/counting.py:
per slot {open, cam, label, first box, last box, last frame, at_last}, per counter base[cam][dir][label]; per batch the rows in task
order, then every freed open slot folded into base; counts = base + the open slots."""
import numpy as np

from vehicle_counting_amd import counting as pc

SLOT = np.dtype([("open", np.int32), ("cam", np.int32), ("label", np.int32), ("at_last", np.int32), ("last_frame", np.int64),
                 ("first", np.int64, 4), ("last", np.int64, 4)])
assert SLOT.itemsize == 88

SQUARE = [[10.0, 10.0], [50.0, 10.0], [50.0, 50.0], [10.0, 50.0]]
TRIANGLE = [[0.0, 0.0], [40.0, 0.0], [0.0, 40.0]]                      # its long edge x + y = 40 is not axis-parallel
RIGHT, UP, LEFT = [10.0, 30.0, 50.0, 30.0], [30.0, 50.0, 30.0, 10.0], [50.0, 20.0, 10.0, 20.0]


def box(cx, cy, r=3):
    return [cx - r, cy - r, cx + r, cy + r]


class Case:
    """cams: per camera (polygon, [direction lines]).  class_map: label of each detector class (one tracker per camera and LABEL).
    frames: the clip as (camera, ...) in arrival order -- `order` lists the camera of every global frame.
    tracks: dicts {cam, cls, id, rows: {global frame: box}, dies: global frame or None}; the track takes its slot at its first row."""

    def __init__(self, name, cams, class_map, order, tracks, max_tracks=6):
        self.name, self.cams, self.class_map, self.order, self.tracks, self.max_tracks = name, cams, list(class_map), list(order), tracks, max_tracks
        self.n_cam, self.n_labels = len(cams), max(class_map) + 1
        self.tracker_cam = [c for c in range(self.n_cam) for _ in range(self.n_labels)]     # tracker index = cam * n_labels + label
        self.frame_no, seen = [], [0] * self.n_cam                                            # 1-based number of a global frame in its camera
        for c in self.order:
            seen[c] += 1
            self.frame_no.append(seen[c])
        for t in tracks:
            t["label"] = self.class_map[t["cls"]]
            t["tracker"] = t["cam"] * self.n_labels + t["label"]
            assert all(self.order[f] == t["cam"] for f in t["rows"]), (name, t)
            assert t["dies"] is None or (t["dies"] > max(t["rows"]) and self.order[t["dies"]] == t["cam"]), (name, t)

    @property
    def n_dir(self):
        return [len(d) for _, d in self.cams]

    @property
    def max_dir(self):
        return max(self.n_dir)

    def polygons(self):
        return [p for p, _ in self.cams]

    def dir_lines(self):
        return [d for _, d in self.cams]

    def zone_json(self, cam):
        """The camera's zone as the labelme file VideoCounting / NativeCounter read."""
        poly, dirs = self.cams[cam]
        shapes = [{"label": "zone", "points": poly}]
        shapes += [{"label": "direction%02d" % (i + 1), "points": [[d[0], d[1]], [d[2], d[3]]]} for i, d in enumerate(dirs)]
        return {"shapes": shapes}

    def rows_of_frame(self, f):
        """(tracker, id, label, box) of every row of global frame f, trackers ascending, a tracker's tracks in birth order."""
        out = [(t["tracker"], t["id"], t["label"], t["rows"][f], k) for k, t in enumerate(self.tracks) if f in t["rows"]]
        return sorted(out, key=lambda r: (r[0], r[4]))


class Batch:
    def __init__(self):
        self.rows6, self.row_slot, self.tasks5, self.frame_no, self.freed = [], [], [], [], []
        self.frames = []                    # the global frames of the batch
        self.notes = set()                  # classes of tests/test_live_count_cases.py this batch realises by construction


def build(case, batch):
    """The clip as batches of `batch` frames (0: the whole clip)."""
    n = len(case.order)
    batch = batch or n
    stack = list(range(case.max_tracks - 1, -1, -1))
    slot_of, out, last_freed = {}, [], set()
    for f0 in range(0, n, batch):
        b = Batch()
        b.frames = list(range(f0, min(n, f0 + batch)))
        b.frame_no = [case.frame_no[f] for f in b.frames]
        per_tracker = {}
        for k, f in enumerate(b.frames):
            for trk, tid, label, bx, key in case.rows_of_frame(f):
                if key not in slot_of:
                    slot_of[key] = stack.pop()
                    if slot_of[key] in last_freed:
                        b.notes.add("a freed slot taken again by a new track in the next batch")
                per_tracker.setdefault(trk, {}).setdefault(k, []).append((list(bx) + [tid, label], slot_of[key]))
            dead = [key for key, t in enumerate(case.tracks) if t["dies"] == f]
            ids = [(case.tracks[key]["id"], case.tracks[key]["tracker"]) for key in dead]
            if len({i for i, _ in ids}) < len(ids) and len(set(ids)) == len(ids):
                b.notes.add("two trackers freeing equal track ids in one batch")
            for key in dead:
                b.freed.append(slot_of.pop(key))
        for trk in sorted(per_tracker):                                 # device order: grouped by tracker, frames ascending
            for k in sorted(per_tracker[trk]):
                rows = per_tracker[trk][k]
                b.tasks5.append([trk, k, rows[0][0][5], len(b.rows6), len(rows)])
                for r, s in rows:
                    b.rows6.append(r)
                    b.row_slot.append(s)
        stack.extend(b.freed)                                           # merge_free_kernel: between batches
        last_freed = set(b.freed)
        out.append(b)
    return out


def arrays(b):
    """A batch as the arrays of vehicle_counting_amd.engine.live_count."""
    return dict(rows6=np.array(b.rows6, np.int64).reshape(-1, 6), row_slot=np.array(b.row_slot, np.int32), tasks5=np.array(b.tasks5, np.int32).reshape(-1, 5),
                frame_no=np.array(b.frame_no, np.int64), freed=np.array(b.freed, np.int32))


def _score(vec, line):
    return pc.cosin_similarity(vec, [[line[0], line[1]], [line[2], line[3]]])


class Model:
    def __init__(self, case):
        self.case = case
        self.slots = np.zeros(case.max_tracks, SLOT)
        self.base = np.zeros((case.n_cam, case.max_dir, case.n_labels), np.int32)
        self.stats = np.zeros(2, np.int32)                              # open at the last read, retired so far
        self.seen = set()                                               # classes met while running

    def _direction(self, s):
        poly, dirs = self.case.cams[int(s["cam"])]
        f, l = s["first"].tolist(), s["last"].tolist()
        vec = (((f[2] + f[0]) / 2, (f[3] + f[1]) / 2), ((l[2] + l[0]) / 2, (l[3] + l[1]) / 2))
        paths = {i: [[d[0], d[1]], [d[2], d[3]]] for i, d in enumerate(dirs)}
        if vec[0] == vec[1]:
            self.seen.add("a zero-length first->last vector")
        elif all(not (_score(vec, d) > 0) for d in dirs):
            self.seen.add("all cosines <= 0")
        return pc.find_best_match_direction(vec, paths)

    def apply(self, b, last_batch=False):
        opened = set()
        for trk, k, label, off, n in b.tasks5:
            cam = self.case.tracker_cam[trk]
            if cam < 0:
                continue
            poly = self.case.cams[cam][0]
            for i in range(off, off + n):
                r, slot = b.rows6[i], b.row_slot[i]
                if not pc.check_bbox_intersect_polygon(poly, r[:4]):
                    continue
                s = self.slots[slot]
                if not s["open"]:
                    s["open"], s["cam"], s["label"], s["at_last"] = 1, cam, r[5], 1
                    s["first"] = r[:4]
                    opened.add(slot)
                else:
                    s["at_last"] = s["at_last"] + 1 if s["last_frame"] == b.frame_no[k] else 1
                s["last_frame"] = b.frame_no[k]
                s["last"] = r[:4]
        for slot in b.freed:
            s = self.slots[slot]
            if not s["open"]:
                self.seen.add("a track never in the zone (freed while closed)")
                continue
            self.base[s["cam"], self._direction(s), s["label"]] += s["at_last"]
            self.stats[1] += 1
            s["open"] = 0
            if not last_batch:
                self.seen.add("a track retired mid-stream")
            if slot in opened:
                self.seen.add("a track confirmed and deleted inside one batch")

    def counts(self):
        out = self.base.copy()
        self.stats[0] = 0
        for s in self.slots:
            if s["open"]:
                out[s["cam"], self._direction(s), s["label"]] += s["at_last"]
                self.stats[0] += 1
        return out


def geometry_classes(case):
    """Classes a case realises by its geometry alone."""
    got = set()
    for t in case.tracks:
        poly = case.cams[t["cam"]][0]
        inside = [pc.check_bbox_intersect_polygon(poly, t["rows"][f]) for f in sorted(t["rows"])]
        if not inside[0] and any(inside):
            got.add("a track whose first in-zone row is not its first row")
        for bx in t["rows"].values():
            x1, y1, x2, y2 = bx
            for pt in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
                if list(map(float, pt)) in poly:
                    got.add("a corner exactly on a polygon vertex")
                    continue
                for i in range(len(poly)):
                    a, c = poly[i], poly[(i + 1) % len(poly)]
                    if pc._orient(a, pt, c) == 0 and pc._on_segment(a, pt, c):
                        got.add("a corner exactly on a polygon edge")
    if len(set(case.n_dir)) > 1:
        got.add("two cameras with different n_dir")
    for label in range(case.n_labels):
        classes = {t["cls"] for t in case.tracks if t["label"] == label}
        if len(classes) > 1:
            got.add("a label map with shared labels")
    return got


CLASSES = ["a track retired mid-stream", "a track confirmed and deleted inside one batch", "two trackers freeing equal track ids in one batch",
           "a freed slot taken again by a new track in the next batch", "a track whose first in-zone row is not its first row",
           "a track never in the zone (freed while closed)", "a zero-length first->last vector", "all cosines <= 0",
           "a corner exactly on a polygon edge", "a corner exactly on a polygon vertex", "two cameras with different n_dir",
           "a label map with shared labels"]
BATCHES = (1, 3, 0)                                                      # frames per batch; 0 = the whole clip

ONE = [(SQUARE, [RIGHT, UP])]
CASES = [
    # one camera, one label: tracks are born, leave the zone, die, and a slot comes back
    Case("lifecycle", ONE, [0], [0] * 9, [
        dict(cam=0, cls=0, id=1, rows={0: box(15, 30), 1: box(25, 30), 2: box(35, 30)}, dies=4),
        dict(cam=0, cls=0, id=2, rows={0: box(80, 80), 1: box(82, 80)}, dies=2),                            # never in the zone
        dict(cam=0, cls=0, id=3, rows={3: box(30, 45), 4: box(30, 30)}, dies=5),                            # lives inside frames 3..5
        dict(cam=0, cls=0, id=4, rows={5: box(70, 30), 6: box(60, 30), 7: box(45, 30), 8: box(40, 31)}, dies=None),   # enters the zone late, still open
    ], max_tracks=4),
    # one camera, classes 0 / 1 / 2 on labels 0 / 1 / 1: the two trackers count their own ids from 1
    Case("equal-ids", ONE, [0, 1, 1], [0] * 6, [
        dict(cam=0, cls=0, id=1, rows={0: box(20, 20), 1: box(30, 20)}, dies=3),
        dict(cam=0, cls=1, id=1, rows={0: box(20, 40), 1: box(20, 30)}, dies=3),
        dict(cam=0, cls=2, id=2, rows={1: box(40, 40), 2: box(40, 25), 4: box(40, 15)}, dies=None),
        dict(cam=0, cls=1, id=3, rows={4: box(25, 25), 5: box(26, 25)}, dies=None),
    ]),
    # directions: a track that ends where it began, one that stands still for a single row, one that runs against every direction
    Case("directions", [(SQUARE, [RIGHT, UP, [10.0, 10.0, 50.0, 10.0]])], [0], [0] * 6, [
        dict(cam=0, cls=0, id=1, rows={0: box(30, 30), 1: box(40, 30), 2: box(30, 30)}, dies=4),            # back at its first box
        dict(cam=0, cls=0, id=2, rows={1: box(20, 20)}, dies=None),                                         # one row
        dict(cam=0, cls=0, id=3, rows={0: box(45, 15), 1: box(35, 25), 3: box(25, 35)}, dies=5),            # left and down: every cosine < 0
        dict(cam=0, cls=0, id=4, rows={2: box(30, 30), 3: box(20, 30), 5: box(15, 30)}, dies=None),         # cosines -1, 0, -1
    ]),
    # boxes that touch the zone with exactly one corner: on a vertex, on an axis-parallel edge, on the slanted edge
    Case("edges", [(SQUARE, [RIGHT]), (TRIANGLE, [RIGHT, LEFT])], [0], [0, 1] * 3, [
        dict(cam=0, cls=0, id=1, rows={0: [0, 0, 10, 10], 2: [2, 2, 9, 9]}, dies=4),                        # corner = vertex (10, 10), then outside
        dict(cam=0, cls=0, id=2, rows={0: [52, 20, 60, 30], 2: [50, 52, 60, 60], 4: [51, 20, 60, 30]}, dies=None),   # never inside: one pixel off, and on the edge's line beyond its end
        dict(cam=0, cls=0, id=3, rows={2: [50, 20, 60, 70], 4: [60, 20, 70, 70]}, dies=None),               # corner (50, 20) on the edge x = 50
        dict(cam=1, cls=0, id=1, rows={1: [20, 20, 60, 60], 3: [21, 20, 60, 60]}, dies=5),                  # corner (20, 20) on x + y = 40, then just outside
        dict(cam=1, cls=0, id=2, rows={3: [40, 0, 50, 9], 5: [41, 0, 50, 9]}, dies=None),                   # corner = vertex (40, 0)
    ]),
    # two cameras, two and three directions, two labels, interleaved two frames of camera 0 to one of camera 1
    Case("two-cameras", [(SQUARE, [RIGHT, UP]), (TRIANGLE, [RIGHT, LEFT, [0.0, 0.0, 0.0, 40.0]])], [0, 1], [0, 1, 0, 0, 1, 0, 0, 1, 0, 0], [
        dict(cam=0, cls=0, id=1, rows={0: box(15, 30), 2: box(30, 30), 3: box(45, 30)}, dies=6),
        dict(cam=0, cls=1, id=1, rows={2: box(30, 45), 3: box(30, 35), 5: box(30, 20)}, dies=None),
        dict(cam=1, cls=0, id=1, rows={1: box(30, 5), 4: box(15, 5)}, dies=7),
        dict(cam=1, cls=1, id=1, rows={1: box(5, 5), 4: box(5, 20), 7: box(5, 30)}, dies=None),
        dict(cam=0, cls=0, id=2, rows={6: box(20, 20), 8: box(30, 22), 9: box(40, 24)}, dies=None),
        dict(cam=1, cls=0, id=2, rows={7: box(10, 10)}, dies=None),
    ]),
]


def prefix_rows(case, upto_frame):
    """Per camera: (frames, ids, labels, boxes) of every row of the global frames [0, upto_frame), in arrival order -- what a
    NativeCounter of that camera is fed."""
    out = [([], [], [], []) for _ in range(case.n_cam)]
    for f in range(upto_frame):
        for trk, tid, label, bx, _ in case.rows_of_frame(f):
            o = out[case.order[f]]
            o[0].append(case.frame_no[f]); o[1].append(tid); o[2].append(label); o[3].append(list(bx))
    return out
