"""Cases of the live overlay (vehicle-counting_amd/csrc/live_overlay.hip, csrc/overlay_build.h), shared by tests/test_live_overlay_ref.py
(CPU: the header's host build against overlay.live_frame) and tests/test_gpu_live_overlay.py (the build kernels against the same).

A case is ONE batch written by hand: the cameras' zones, the frames (camera, the camera's frame number, rows as (label, track id, box)),
the tracks that were in their zone before the batch (`pre`: their first in-zone box), the counts before the batch, the arena size.
`build(case)` lays it out as the tracker launch leaves it in device memory -- rows in an arena grouped by tracker with the pool slot of
each, tasks (tracker, frame, label, first row, rows), the per-slot records AFTER the batch's apply launch -- and `expected(case)` is the
definition: overlay.live_frame per frame, fed the rows in emit order (labels ascending, a label's rows in the order given) and each
row's first in-zone box.  Frame size 64 x 96 unless a case says otherwise."""
import numpy as np

from vehicle_counting_amd import counting as pc
from vehicle_counting_amd import overlay as ov

SLOT = np.dtype([("open", np.int32), ("cam", np.int32), ("label", np.int32), ("at_last", np.int32), ("last_frame", np.int64),
                 ("first", np.int64, 4), ("last", np.int64, 4)])
HW = (64, 96)
SQUARE = [[10.0, 10.0], [50.0, 10.0], [50.0, 50.0], [10.0, 50.0]]
PENTAGON = [[5.5, 2.0], [60.0, 4.0], [90.9, 30.0], [60.0, 60.0], [5.0, 58.0]]             # non-integer corners: int() truncates them
RIGHT, UP, LEFT = [[10.0, 30.0], [50.0, 30.0]], [[30.0, 50.0], [30.0, 10.0]], [[80.5, 20.0], [12.0, 20.9]]
ONE = [(SQUARE, {"01": RIGHT, "02": UP})]
TWO = [(SQUARE, {"01": RIGHT, "02": UP}), (PENTAGON, {"01": RIGHT, "02": UP, "10": LEFT})]


def box(cx, cy, r=4):
    return [cx - r, cy - r, cx + r, cy + r]


class Case:
    def __init__(self, name, cams, n_labels, frames, hw=HW, pre=None, closed=(), counts_before=None, cap=None):
        self.name, self.cams, self.n_labels, self.frames, self.hw = name, cams, n_labels, frames, hw
        self.pre = dict(pre or {})                     # (cam, label, track id) -> first in-zone box, before the batch
        self.closed = set(closed)                      # tracks the batch's apply launch closed (their slot was freed inside the batch)
        self.counts_before = counts_before             # None, or per camera [[n per label] per direction]
        self.cap = cap                                 # arena primitives (a number or a function giving it); None = what the batch needs + 7
        self.n_cam = len(cams)
        self.n_dir = [len(d) for _, d in cams]
        self.max_dir = max(self.n_dir)

    def polygons(self):
        return [p for p, _ in self.cams]

    def dir_lines(self):
        return [[l[0] + l[1] for l in d.values()] for _, d in self.cams]

    def dir_keys(self):
        return [list(d.keys()) for _, d in self.cams]

    def counts_array(self):
        if self.counts_before is None:
            return None
        out = np.zeros((self.n_cam, self.max_dir, self.n_labels), np.int32)
        for c, per_dir in enumerate(self.counts_before):
            for d, per_label in enumerate(per_dir):
                out[c, d, :len(per_label)] = per_label
        return out

    def text_before(self, cam):
        if self.counts_before is None:
            return None
        arr = self.counts_array()
        return ov.count_text({int(k): {label: int(arr[cam, d, label]) for label in range(self.n_labels)} for d, k in enumerate(self.cams[cam][1])})


def build(case):
    """The batch as the arrays of vehicle_counting_amd.engine.live_overlay, and per frame what the definition is fed."""
    slot_of, first_of = {}, dict(case.pre)
    for key in case.pre:
        slot_of[key] = len(slot_of)
    per_frame = []                                      # (rows6 in emit order, firsts, slots)
    for cam, _, rows in case.frames:
        ordered = sorted(rows, key=lambda r: r[0])      # stable: labels ascending, the given order inside a label
        r6, firsts, slots = [], [], []
        for label, tid, bx in ordered:
            key = (cam, label, tid)
            slot_of.setdefault(key, len(slot_of))
            if pc.check_bbox_intersect_polygon(case.cams[cam][0], bx):
                first_of.setdefault(key, list(bx))
            r6.append(list(bx) + [tid, label]); firsts.append(first_of.get(key, [0, 0, 0, 0])); slots.append(slot_of[key])
        per_frame.append((r6, firsts, slots))
    n_slots = max(len(slot_of), 1) + 2                  # two slots no track ever took
    slots = np.zeros(n_slots, SLOT)
    for key, s in slot_of.items():
        if key in first_of:                             # in its zone at some point: the apply launch opened the record ...
            slots[s]["open"], slots[s]["cam"], slots[s]["label"], slots[s]["at_last"] = (0 if key in case.closed else 1), key[0], key[1], 1
            slots[s]["first"] = first_of[key]           # ... and closing it leaves `first` alone
            slots[s]["last"] = first_of[key]
    rows6, row_slot, tasks5 = [], [], []
    trackers = sorted({cam * case.n_labels + r[0] for cam, _, rows in case.frames for r in rows})
    for trk in trackers:                                # device order: grouped by tracker, frames ascending
        for f, (cam, _, _) in enumerate(case.frames):
            r6, _, sl = per_frame[f]
            mine = [(r, s) for r, s in zip(r6, sl) if cam * case.n_labels + r[5] == trk]
            if mine:
                tasks5.append([trk, f, trk % case.n_labels, len(rows6), len(mine)])
                rows6 += [r for r, _ in mine]; row_slot += [s for _, s in mine]
    return dict(rows6=np.array(rows6, np.int64).reshape(-1, 6), row_slot=np.array(row_slot, np.int32), tasks5=np.array(tasks5, np.int32).reshape(-1, 5),
                frame_no=np.array([n for _, n, _ in case.frames], np.int64), cam_of_frame=np.array([c for c, _, _ in case.frames], np.int32),
                slots=slots, tracker_cam=[c for c in range(case.n_cam) for _ in range(case.n_labels)], per_frame=per_frame)


def expected(case, built=None):
    """(prims12 of the frames that fit, frame_first, overflow) by the definition, under the case's arena size; and that size."""
    built = built or build(case)
    lists = [ov.live_frame(case.hw, case.cams[cam][0], case.cams[cam][1], built["per_frame"][f][0], built["per_frame"][f][1], case.text_before(cam), no)
             for f, (cam, no, _) in enumerate(case.frames)]
    need = sum(len(pl.rows) for pl in lists)
    cap = need + 7 if case.cap is None else (case.cap if isinstance(case.cap, int) else case.cap())
    kept, acc, fits = [], 0, True
    first = [0]
    for pl in lists:
        fits = fits and acc + len(pl.rows) <= cap
        if fits:
            kept.append(pl); acc += len(pl.rows)
        first.append(acc)
    prims, _ = ov.pack_prims(kept)
    return prims, np.array(first, np.int32), not fits, cap


def live_args(case, built=None):
    """keyword arguments of engine.live_overlay for this case (without cap_prims)"""
    b = built or build(case)
    return dict(polygons=case.polygons(), dir_lines=case.dir_lines(), dir_keys=case.dir_keys(), n_labels=case.n_labels, tracker_cam=b["tracker_cam"], slots=b["slots"],
                counts_before=case.counts_array(), rows6=b["rows6"], row_slot=b["row_slot"], tasks5=b["tasks5"], frame_no=b["frame_no"], cam_of_frame=b["cam_of_frame"],
                hw=case.hw)


def check(case, host):
    """engine.live_overlay on one case -- host=True: vc_overlay_build_host on the CPU, else one launch of the build kernels -- against the
    definition: frame_first, the overflow flag and every primitive equal; what no frame owns is not written; an overflow is
    VC_ERR_CAPACITY."""
    import vehicle_counting_amd.engine as E
    from vehicle_counting_amd._lib import VcError
    built = build(case)
    prims, first, overflow, cap = expected(case, built)
    arena, got_first, got_overflow = E.live_overlay(cap_prims=cap, host=host, allow_overflow=True, **live_args(case, built))
    print(f"{case.name}: {len(case.frames)} frames, {len(built['rows6'])} rows, {first[-1]} primitives of {cap}, overflow {overflow}")
    np.testing.assert_array_equal(got_first, first)
    assert got_overflow == overflow
    np.testing.assert_array_equal(arena[:first[-1]], prims)
    assert (arena[first[-1]:] == E.OVERLAY_UNWRITTEN).all()
    if overflow:
        try:
            E.live_overlay(cap_prims=cap, host=host, **live_args(case, built))
        except VcError as err:
            assert err.code == 4, err                   # VC_ERR_CAPACITY
        else:
            raise AssertionError("an arena that is too small was not reported")


# ---- the table ------------------------------------------------------------------------------------------------------------------------
_ROW = (0, 1, box(30, 30))
_FILL_FRAMES = [(0, 1, [_ROW, (0, 2, box(20, 40))]), (0, 2, [(0, 1, box(33, 30))]), (0, 3, [(0, 1, box(36, 30)), (0, 2, box(24, 40))])]
_FILL = Case("arena filled exactly", ONE, 1, _FILL_FRAMES, counts_before=[[[1], [0]]])
_FILL.cap = lambda: sum(len(pl) for pl in _need(_FILL))


def _need(case):
    b = build(case)
    return [ov.live_frame(case.hw, case.cams[cam][0], case.cams[cam][1], b["per_frame"][f][0], b["per_frame"][f][1], case.text_before(cam), no).rows
            for f, (cam, no, _) in enumerate(case.frames)]


_OVER = Case("one row more than the arena holds", ONE, 1, _FILL_FRAMES[:1] + [(0, 2, [(0, 1, box(33, 30)), (0, 3, box(40, 20))])] + _FILL_FRAMES[2:],
             counts_before=[[[1], [0]]], cap=_FILL.cap)
# beyond the issue's list: the arena ends one primitive short of frame 1 -- frames 1, 2 and 3 own nothing, although frame 3 alone would fit
_MID = Case("overflow in the middle of the batch", ONE, 1, _FILL_FRAMES + [(0, 4, [])], counts_before=[[[1], [0]]])
_MID.cap = lambda: sum(len(pl) for pl in _need(_MID)[:2]) - 1

CASES = [
    Case("a frame without rows", ONE, 2, [(0, 1, []), (0, 2, [(1, 1, box(30, 30))]), (0, 3, [])], counts_before=[[[0, 0], [0, 0]]]),
    Case("a row outside the zone beside one inside", ONE, 1, [(0, 5, [(0, 1, box(80, 30)), (0, 2, box(30, 30)), (0, 3, [51, 20, 60, 30]), (0, 4, [50, 20, 60, 30])])],
         counts_before=[[[2], [1]]]),
    Case("confirmed and freed inside the batch", ONE, 1, [(0, 7, [(0, 3, box(15, 30)), (0, 4, box(40, 40))]), (0, 8, [(0, 3, box(25, 30))]), (0, 9, [(0, 4, box(40, 30))])],
         pre={(0, 0, 4): box(40, 48)}, closed=[(0, 0, 3)], counts_before=[[[0], [1]]]),
    Case("digit counts of ids and labels", ONE, 12,
         [(0, 9, [(0, 1, box(20, 20)), (11, 10, box(30, 30)), (0, 12345, box(40, 40)), (11, 2 ** 31, box(25, 45)), (11, 1, box(45, 25))]),
          (0, 10, [(11, 2 ** 31, box(27, 45)), (0, 12345, box(42, 40))])],
         counts_before=[[[0] * 12, [3] + [0] * 10 + [12]]]),
    Case("two cameras interleaved", TWO, 2,
         [(0, 3, [(0, 1, box(20, 30)), (1, 1, box(30, 40))]), (1, 11, [(0, 1, box(70, 30)), (1, 7, box(20, 10))]), (0, 4, [(1, 1, box(30, 36))]),
          (1, 12, [(1, 7, box(24, 12)), (0, 2, [91, 29, 95, 33]), (0, 1, box(64, 30))])],
         pre={(0, 0, 1): box(12, 30), (1, 1, 7): box(10, 6)}, counts_before=[[[1, 0], [0, 1]], [[0, 0], [2, 0], [0, 5]]]),
    Case("no count text", ONE, 2, [(0, 1, [(0, 1, box(30, 30))]), (0, 2, [(1, 1, box(20, 20))])], counts_before=None),
    Case("count text all zero", ONE, 2, [(0, 2, [(0, 1, box(30, 30))])], counts_before=[[[0, 0], [0, 0]]]),
    Case("count text 0 9 10 100000", ONE, 2, [(0, 2, [(0, 1, box(30, 30))]), (0, 3, [])], counts_before=[[[0, 9], [10, 100000]]]),
    Case("1080 x 1920", [([[100.0, 100.0], [1800.0, 120.0], [1700.0, 1000.0], [150.0, 900.0]], {"01": [[200.0, 500.0], [1600.0, 520.0]], "02": [[900.0, 950.0], [880.0, 150.0]]})], 3,
         [(0, 100, [(0, 17, [400, 300, 520, 380]), (2, 230, [1000, 600, 1190, 745]), (1, 5, [1850, 40, 1900, 90])])], hw=(1080, 1920),
         pre={(0, 0, 17): [300, 310, 420, 390]}, counts_before=[[[4, 0, 1], [0, 12, 0]]]),
    _FILL,
    _OVER,
    _MID,
    Case("70 rows in one frame", ONE, 1, [(0, 2, [(0, 100 + i, box(12 + (i % 10) * 5, 12 + (i // 10) * 6, 2)) for i in range(70)])], counts_before=[[[7], [0]]]),
    # beyond the issue's list: more parts than the workgroup has lanes (the chunk loop of the build kernel takes a second and third turn)
    Case("600 rows over two labels", ONE, 2,
         [(0, 1, [(i % 2, 1 + i, box(8 + (i % 30) * 2, 8 + (i // 30) * 2, 2)) for i in range(600)]), (0, 2, [(1, 2, box(30, 30))])], counts_before=[[[0, 1], [2, 3]]]),
]
assert len({c.name for c in CASES}) == len(CASES)
