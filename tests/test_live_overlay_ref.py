"""CPU: the live overlay's definition (overlay.live_frame / overlay.LiveVisualizer) and its restatement csrc/overlay_build.h.

* vc_overlay_build_host -- the header compiled into the library, no HIP call -- equals the definition on every case of
  tests/live_overlay_cases.py, int32 for int32, arena limits included;
* the header compiled for the host on its own (tests/native/overlay_build_host.cpp): every part's count equals what it emits, and
  what it emits equals the PrimList helper it restates; the same file as a stand-alone program;
* vc_glyph_bits_host equals overlay.glyph_bits;
* the definition is tied to the pinned one (VideoCounting -> csv_records -> MergedVisualizer) on a clip's rows: the scenario of
  tests/test_gpu_live_count.py restated here, tracked by oracle/deepsort.py, cut into batches of 1, 4 and the whole clip."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import live_overlay_cases as OC
from vehicle_counting_amd import overlay as ov

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "overlay_build_host.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
_pd, _pl, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)


@pytest.mark.parametrize("case", OC.CASES, ids=[c.name for c in OC.CASES])
def test_host_build_equals_the_definition(case):
    OC.check(case, host=True)


def test_the_case_table_holds_what_it_names():
    by = {c.name: c for c in OC.CASES}
    over = [c for c in OC.CASES if OC.expected(c)[2]]
    assert {c.name for c in over} == {"one row more than the arena holds", "overflow in the middle of the batch"}
    p, f, o, cap = OC.expected(by["arena filled exactly"])
    assert f[-1] == cap and not o
    p, f, o, cap = OC.expected(by["overflow in the middle of the batch"])
    assert f.tolist() == [0, f[1], f[1], f[1], f[1]] and f[1] > 0
    b = OC.build(by["a row outside the zone beside one inside"])
    zone = by["a row outside the zone beside one inside"].cams[0][0]
    from vehicle_counting_amd import counting as pc
    assert [pc.check_bbox_intersect_polygon(zone, r[:4]) for r in b["rows6"].tolist()] == [False, True, False, True]
    freed = OC.build(by["confirmed and freed inside the batch"])
    assert 0 in freed["slots"]["open"][freed["row_slot"]].tolist()     # a drawn row whose record the batch closed


def test_glyph_bits_equal_the_python_table():
    from vehicle_counting_amd import _lib as L
    bits = C.c_uint64()
    for ch in list(ov._F) + [c.lower() for c in ov._F if c.isalpha()] + ["#", "~", "\x7f"]:
        L.check(L.lib().vc_glyph_bits_host(ord(ch), C.byref(bits)))
        assert bits.value == ov.glyph_bits(ch), ch
    assert ov.glyph_bits("#") == ov.glyph_bits("?")


# ---- the header on its own ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def obh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("obh") / "libobh.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.obh_glyph_bits.restype = C.c_uint64
    lib.obh_text_scale.argtypes = [C.c_double]
    lib.obh_fmt_i64.argtypes = [C.c_longlong, C.c_char_p]
    lib.obh_track_color.argtypes = [C.c_longlong, C.c_longlong]
    lib.obh_count_anno.argtypes = [_pd, C.c_int, _pd, C.c_int, _pi]
    lib.obh_emit_anno.argtypes = [_pd, C.c_int, _pd, C.c_int, _pi, _pi, C.c_int]
    lib.obh_count_row.argtypes = [C.c_longlong, C.c_longlong]
    lib.obh_emit_row.argtypes = [C.c_int, C.c_int, _pl, _pl, C.c_longlong, C.c_longlong, _pi, C.c_int]
    lib.obh_count_text.argtypes = [C.c_int, _pi, C.c_int, _pi]
    lib.obh_emit_text.argtypes = [C.c_int, C.c_int, _pi, C.c_int, _pi, _pi, C.c_int]
    lib.obh_count_frame_no.argtypes = [C.c_longlong]
    lib.obh_emit_frame_no.argtypes = [C.c_longlong, _pi, C.c_int]
    return lib


def prims_of(pl):
    return ov.pack_prims([pl])[0]


def test_header_scalars(obh):
    for ch in list(ov._F) + ["a", "z", "#"]:
        assert obh.obh_glyph_bits(ord(ch)) == ov.glyph_bits(ch), ch
    for fs in (0.0, 0.2, 0.25, 1 / 3, 0.5, 2 / 3, 0.75, 1.0, 1.25, 1.5, 4 / 3, 2.0):
        assert obh.obh_text_scale(fs) == ov.text_scale(fs), fs
    for n in (0, 1, 7, 30):
        for s in (1, 2, 3):
            assert (obh.obh_text_width(n, s), obh.obh_text_height(s)) == ov.text_size("x" * n, s)
    for m in (1, 64, 96, 499, 500, 501, 1499, 1500, 1501, 1920, 2500, 3840):                  # .5 ties round to even, as Python's round
        assert obh.obh_box_tl(m, 3) == (int(round(0.001 * max(m, 3))) or 1), m
    buf = C.create_string_buffer(24)
    for v in (0, 9, 10, 99, 100, 12345, 2 ** 31 - 1, 2 ** 31, 10 ** 18, 2 ** 63 - 1, -1, -2 ** 63):
        n = obh.obh_fmt_i64(v, buf)
        assert buf.raw[:n].decode() == str(v)
    for label, tid in ((0, 1), (11, 10), (3, 12345), (0, 2 ** 31), (7, 2 ** 40 + 5), (255, 2 ** 63 - 1)):
        b, g, r = ov.track_color(label, tid)
        assert obh.obh_track_color(label, tid) == b | g << 8 | r << 16


def test_header_parts_equal_the_primlist_helpers(obh):
    out = np.zeros((8192, 12), np.int32)
    po = out.ctypes.data_as(_pi)
    for polygon, directions in OC.TWO:
        poly = np.array(polygon, np.float64)
        lines = np.array([l[0] + l[1] for l in directions.values()], np.float64)
        keys = np.array([int(k) for k in directions], np.int32)
        pl = ov.PrimList()
        pl.draw_anno(polygon, directions)
        n = obh.obh_emit_anno(poly.ctypes.data_as(_pd), len(poly), lines.ctypes.data_as(_pd), len(lines), keys.ctypes.data_as(_pi), po, len(out))
        assert n == len(pl.rows) == obh.obh_count_anno(poly.ctypes.data_as(_pd), len(poly), lines.ctypes.data_as(_pd), len(lines), keys.ctypes.data_as(_pi))
        np.testing.assert_array_equal(out[:n], prims_of(pl))
    for hw in ((64, 96), (1080, 1920), (1500, 1000), (2160, 3840)):
        for label, tid, bx, first in ((0, 1, [20, 20, 30, 31], [5, 7, 14, 18]), (11, 2 ** 31, [0, 0, 95, 63], [1, 1, 2, 2]), (3, 12345, [-4, -9, 10, 10], [-7, -3, 0, 0])):
            pl = ov.PrimList()
            color = ov.track_color(label, tid)
            pl.draw_arrow((int((first[0] + first[2]) / 2), int((first[1] + first[3]) / 2)), (int((bx[0] + bx[2]) / 2), int((bx[1] + bx[3]) / 2)), color)
            pl.draw_one_box(hw, bx, f"id: {tid}", f"cls: {label}", color)
            b4, f4 = np.array(bx, np.int64), np.array(first, np.int64)
            n = obh.obh_emit_row(hw[0], hw[1], b4.ctypes.data_as(_pl), f4.ctypes.data_as(_pl), tid, label, po, len(out))
            assert n == len(pl.rows) == obh.obh_count_row(tid, label)
            np.testing.assert_array_equal(out[:n], prims_of(pl))
    for h, keys, counts in ((64, [1, 2], [[0, 9], [10, 100000]]), (1080, [1, 2, 10], [[0] * 12, [5] * 12, list(range(12))]), (64, [7], [[2 ** 31 - 1]])):
        cnt = np.array(counts, np.int32)
        k = np.array(keys, np.int32)
        pl = ov.PrimList()
        pl.draw_text(h, ov.count_text({key: {label: int(n) for label, n in enumerate(row)} for key, row in zip(keys, counts)}))
        n = obh.obh_emit_text(h, len(keys), k.ctypes.data_as(_pi), cnt.shape[1], cnt.ctypes.data_as(_pi), po, len(out))
        assert n == len(pl.rows) == obh.obh_count_text(len(keys), k.ctypes.data_as(_pi), cnt.shape[1], cnt.ctypes.data_as(_pi))
        np.testing.assert_array_equal(out[:n], prims_of(pl))
    for h in (64, 1080):
        for no in (1, 9, 10, 24, 99999, 2 ** 40):
            pl = ov.PrimList()
            pl.draw_frame_count(h, no)
            n = obh.obh_emit_frame_no(no, po, len(out))
            assert n == len(pl.rows) == obh.obh_count_frame_no(no)
            np.testing.assert_array_equal(out[:n], prims_of(pl))


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "overlay_build_host")
    subprocess.run(FLAGS + ["-DOBH_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


# ---- the definition against the pinned one, on a clip's rows --------------------------------------------------------------------------------
H, W, T, NL = 64, 96, 24, 2                      # the scenario of tests/test_gpu_live_count.py, restated
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=1.0, MAX_IOU_DISTANCE=0.7, MAX_AGE=2, N_INIT=1, NN_BUDGET=8)
ZONE = [[0.0, 0.0], [60.0, 0.0], [60.0, 64.0], [0.0, 64.0]]
RIGHT, DOWN, LEFT = [[10.0, 32.0], [80.0, 32.0]], [[48.0, 5.0], [48.0, 60.0]], [[80.0, 50.0], [10.0, 50.0]]
CAM_DIRS = [{"01": RIGHT, "02": DOWN}, {"01": RIGHT, "02": DOWN, "03": LEFT}]
OBJECTS = [
    [(0, 0, 23, 5, 8, 2.0, 0.0, 14, 12), (0, 0, 7, 72, 40, -3.0, 0.0, 14, 12), (1, 0, 23, 20, 4, 0.0, 1.5, 12, 14),
     (1, 5, 12, 75, 30, 0.0, 0.0, 14, 12), (0, 12, 18, 28, 42, 2.0, 0.0, 14, 12)],
    [(0, 0, 23, 8, 46, 1.0, 0.0, 14, 12), (1, 0, 23, 38, 18, 0.0, 0.0, 12, 14), (0, 2, 9, 56, 6, -2.0, 0.0, 14, 12),
     (1, 14, 23, 22, 26, 0.0, 1.0, 12, 14)],
]


def clip(cam):
    rng = np.random.default_rng(100 + cam)
    bg = rng.integers(60, 120, (H, W, 3), dtype=np.uint8)
    tex = [rng.integers(0, 256, (o[8], o[7], 3), dtype=np.uint8) for o in OBJECTS[cam]]
    frames = np.repeat(bg[None], T, 0).copy()
    boxes = []
    for t in range(T):
        bl = []
        for k, (label, t0, t1, x, y, vx, vy, w, h) in enumerate(OBJECTS[cam]):
            if t0 <= t <= t1:
                x1, y1 = int(round(x + vx * (t - t0))), int(round(y + vy * (t - t0)))
                frames[t, y1:y1 + h, x1:x1 + w] = tex[k]
                bl.append((x1, y1, w, h, label))
        boxes.append(bl)
    return frames, boxes


def embed(crops):
    """a stand-in for the ReID net: the crop's own pixels, centred (every object is a patch of its own fixed texture)"""
    return np.stack([np.resize(np.asarray(c, np.float32).ravel(), 512) - 127.5 for c in crops]).astype(np.float32)


@pytest.fixture(scope="module")
def clip_rows():
    """per camera, per frame: the rows [x1, y1, x2, y2, track id, label] in the order VideoTracker.run emits them (classes ascending)"""
    from oracle.deepsort import VideoTrackerOracle
    out = []
    for cam in range(2):
        frames, boxes = clip(cam)
        vt = VideoTrackerOracle(NL, TRACK_CFG, embed)
        per_frame = []
        for t in range(T):
            b = np.array(boxes[t], np.float64)
            res = vt.run(frames[t], b[:, :4], b[:, 4].astype(np.int64), np.full(len(b), 0.9))
            per_frame.append([[int(v) for v in bx] + [int(tid), int(label)] for bx, tid, label in zip(res["boxes"], res["tracks"], res["labels"])])
        assert sum(len(r) for r in per_frame) > 40
        out.append(per_frame)
    return out


def zone_file(tmp, cam):
    import json
    path = os.path.join(str(tmp), f"overlay_zone_{cam}.json")
    shapes = [{"label": "zone", "points": ZONE}] + [{"label": "direction" + k, "points": l} for k, l in CAM_DIRS[cam].items()]
    with open(path, "w") as f:
        json.dump({"shapes": shapes}, f)
    return path


def merged_of_cut(zone_path, rows_per_frame, upto):
    """the pinned visualiser of the video cut after frame `upto` (1-based): VideoCounting -> csv_records -> MergedVisualizer, read back as
    CountingPipeline.visualizer reads it (direction as an integer, colour = track_color)"""
    from vehicle_counting_amd.counting import csv_records, load_zone_anno
    from vehicle_counting_amd.track import VideoCounting
    vc = VideoCounting([f"c{i}" for i in range(NL)], zone_path)
    flat = [(f + 1, r) for f in range(upto) for r in rows_per_frame[f]]
    td = vc.run(frames=[f for f, _ in flat], tracks=[r[4] for _, r in flat], labels=[r[5] for _, r in flat], boxes=[np.array(r[:4], np.int64) for _, r in flat])
    rows = []
    for r in csv_records(td):
        r = dict(r)
        r["direction"] = int(r["direction"])
        r["color"] = ov.track_color(r["label"], r["track_id"])
        rows.append(r)
    polygon, directions = load_zone_anno(zone_path)
    return ov.MergedVisualizer(rows, directions, polygon, NL)


@pytest.fixture(scope="module")
def merged_cuts(clip_rows, tmp_path_factory):
    """per camera, for every cut f = 1..T: (the rows' primitive groups of frame f, anno primitives, frame-number primitives, the text held
    after frame f) of the pinned visualiser built on the video cut at f -- computed once, shared by the three batch sizes"""
    d = tmp_path_factory.mktemp("overlay_zones")
    out = []
    for cam in range(2):
        zp = zone_file(d, cam)
        per_cut = []
        for f in range(1, T + 1):
            mv = merged_of_cut(zp, clip_rows[cam], f)
            for g in range(1, f):
                mv.frame_prims(g, (H, W))
            rows_f = list(mv.by_frame.get(f, []))
            pl = mv.frame_prims(f, (H, W))
            groups = []
            for r in rows_f:
                one = ov.PrimList()
                one.visualize_one_frame((H, W), [r])
                groups.append(tuple(one.rows))
            anno, fno = ov.PrimList(), ov.PrimList()
            anno.draw_anno(mv.zones, mv.directions)
            fno.draw_frame_count(H, f)
            assert pl.rows[:len(anno.rows)] == anno.rows and pl.rows[-len(fno.rows):] == fno.rows
            per_cut.append((groups, anno.rows, fno.rows, mv.prev_text))
        out.append(per_cut)
    return out


@pytest.mark.parametrize("batch", [1, 4, 2 * T], ids=["b1", "b4", "whole"])
def test_definition_against_the_pinned_visualiser_on_a_clip(clip_rows, merged_cuts, batch):
    from vehicle_counting_amd import counting as pc
    lv = ov.LiveVisualizer([ZONE, ZONE], CAM_DIRS, NL)
    order = [(c, t) for t in range(T) for c in range(2)]                   # two cameras interleaved frame by frame
    frames_seen = drawn = 0
    for f0 in range(0, len(order), batch):
        part = order[f0:f0 + batch]
        done = [sum(1 for c, _ in order[:f0] if c == cam) for cam in range(2)]     # frames of each camera before this batch
        texts = [lv.text(cam) for cam in range(2)]
        for cam in range(2):
            # the text of batch k = the text the pinned visualiser holds after the last frame of the video cut at the end of batch k - 1
            assert texts[cam] == (merged_cuts[cam][done[cam] - 1][3] if done[cam] else None), (batch, f0, cam)
        lists = lv.batch_lists([c for c, _ in part], [t + 1 for _, t in part], [clip_rows[c][t] for c, t in part], (H, W))
        for (cam, t), pl in zip(part, lists):
            groups, anno, fno, _ = merged_cuts[cam][t]
            rows = list(pl.rows)
            assert rows[:len(anno)] == anno                                 # anno: equal, in order
            assert rows[-len(fno):] == fno                                  # frame number: equal, in order
            body = rows[len(anno):len(rows) - len(fno)]
            mine = []
            for r in clip_rows[cam][t]:                                     # emit order
                if pc.check_bbox_intersect_polygon(ZONE, r[:4]):
                    n = 13 + len(str(r[4])) + len(str(r[5]))
                    mine.append(tuple(body[:n]))
                    body = body[n:]
            assert len(mine) == len(groups) and set(mine) == set(groups), (batch, cam, t)       # every row's group, as sets
            text = ov.PrimList()
            if texts[cam] is not None:
                text.draw_text(H, texts[cam])
            assert body == text.rows                                        # what is left is the count text before the batch
            frames_seen += 1
            drawn += len(mine)
    assert frames_seen == 2 * T and drawn > 40                               # all frames, no row left out
