"""CPU: vehicle-counting_amd/csrc/count_core.h -- the zone test and find_best_match_direction that counting.hip runs on the host and the
live-count kernels run on the device -- compiled for the host (tests/native/count_core_host.cpp) and held to the reference's golden
vectors (tests/golden/counting.json), exactly; the per-slot record against vc_counter's own bookkeeping; and the same file as a
stand-alone program."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "count_core_host.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
_pd, _pl = C.POINTER(C.c_double), C.POINTER(C.c_int64)


def dptr(a):
    return a.ctypes.data_as(_pd)


@pytest.fixture(scope="module")
def cch(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cch") / "libcch.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.cch_point_in_polygon.argtypes = [_pd, C.c_int, C.c_double, C.c_double]
    lib.cch_box_in_polygon.argtypes = [_pd, C.c_int, _pl]
    lib.cch_best_direction_vec.argtypes = [C.c_double] * 4 + [_pd, C.c_int]
    lib.cch_best_direction.argtypes = [_pd, C.c_int, _pl, _pl, _pd, _pd]
    lib.cch_slot_add.argtypes = [C.c_void_p, C.c_int, C.c_int, _pl, _pl, C.c_int]
    return lib


def test_polygon_and_direction_against_the_reference_golden(cch, golden_dir):
    g = json.load(open(os.path.join(golden_dir, "counting.json")))
    zone = np.array(g["zone"], np.float64)
    sq = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float64)
    assert len(g["boxes"]) > 100 and {r["inside"] for r in g["boxes"]} == {True, False}
    for r in g["boxes"]:
        b = np.array(r["box"], np.int64)
        assert bool(cch.cch_box_in_polygon(dptr(zone), len(zone), b.ctypes.data_as(_pl))) == r["inside"], r
    assert {r["poly"] for r in g["points"]} == {"zone", "square"}
    for r in g["points"]:
        poly = zone if r["poly"] == "zone" else sq
        assert bool(cch.cch_point_in_polygon(dptr(poly), len(poly), *r["pt"])) == r["inside"], r
    keys = list(g["two_dirs"])
    two = np.array([g["two_dirs"][k] for k in keys], np.float64).reshape(-1, 4)
    assert len(g["vectors"]) > 10
    for r in g["vectors"][:-1]:
        (x0, y0), (x1, y1) = r["vec"]
        assert keys[cch.cch_best_direction_vec(x0, y0, x1, y1, dptr(two), len(two))] == r["best"], r
    one = np.array(g["directions"]["01"], np.float64).reshape(-1, 4)                 # every cosine <= 0: the first key
    (x0, y0), (x1, y1) = g["vectors"][-1]["vec"]
    assert cch.cch_best_direction_vec(x0, y0, x1, y1, dptr(one), 1) == 0 and g["vectors"][-1]["best"] == "01"
    # the tracks of the golden CSV: direction and first / last points from the first and last box
    import re
    want = {}
    for line in g["csv_text"].splitlines()[1:]:
        m = re.match(r'(\d+),\d+,"\[.*?\]",\w*,(\d+),(\d+),', line)
        want[int(m.group(2)), int(m.group(1))] = m.group(3)
    for t in g["csv_tracks"]:
        f, l = np.array(t["boxes"][0], np.int64), np.array(t["boxes"][-1], np.int64)
        fp, lp = np.zeros(2), np.zeros(2)
        d = cch.cch_best_direction(dptr(two), len(two), f.ctypes.data_as(_pl), l.ctypes.data_as(_pl), dptr(fp), dptr(lp))
        assert keys[d] == want[t["label"], t["track"]], t
        assert fp.tolist() == [(f[2] + f[0]) / 2, (f[3] + f[1]) / 2] and lp.tolist() == [(l[2] + l[0]) / 2, (l[3] + l[1]) / 2]


def test_slot_record_follows_vc_counter_add(cch):
    """first box, last box and the rows at the last frame, as vc_counter_add keeps them (counting.hip), over rows that repeat a frame"""
    import live_count_cases as LC
    assert cch.cch_slot_bytes() == LC.SLOT.itemsize
    s = np.zeros(1, LC.SLOT)
    frames = np.array([3, 4, 4, 4, 7, 9, 9], np.int64)
    boxes = np.arange(28, dtype=np.int64).reshape(7, 4)
    for n, at_last in zip(range(1, 8), [1, 1, 2, 3, 1, 1, 2]):
        s[:] = np.zeros(1, LC.SLOT)
        cch.cch_slot_add(s.ctypes.data, 2, 5, frames.ctypes.data_as(_pl), boxes.ctypes.data_as(_pl), n)
        assert (s["open"][0], s["cam"][0], s["label"][0], s["at_last"][0], s["last_frame"][0]) == (1, 2, 5, at_last, frames[n - 1])
        assert s["first"][0].tolist() == boxes[0].tolist() and s["last"][0].tolist() == boxes[n - 1].tolist()


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "count_core_host")
    subprocess.run(FLAGS + ["-DCCH_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
