"""CPU: the class filter and label map without a GPU -- the conditions the cases of tests/class_filter_cases.py are built to satisfy, the
rules of a class map (vc_class_map_check_host, engine.class_table), the new symbols, validation in front of every device call, and the
reason the filter sits in front of the NMS: on the clip of test_csv_parity with max_det = 10, filter-then-NMS differs from NMS-then-filter."""
import ctypes as C

import numpy as np
import pytest

import class_filter_cases as F
import detect_post_cases as D
import vehicle_counting_amd.engine as E
from vehicle_counting_amd import _lib as L

VC_ERR_ARG = 1
NEW_SYMBOLS = ("vc_engine_set_class_map", "vc_engine_class_map", "vc_class_map_check_host", "vc_class_filter_nms_host")


def _iou(a, b):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    return w * h / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - w * h)


def test_cases_hold_what_they_were_built_for():
    cases = F.filter_cases()
    for name, case in cases.items():
        assert case.table.shape == (F.NC,) and case.max_cand % 64 == 0
        for boxes, conf, cls in case.frames:
            assert boxes.dtype == np.float32 and conf.dtype == np.float32 and cls.dtype == np.int32
            assert len(conf) <= case.max_cand and (len(conf) == 0 or (cls.min() >= 0 and cls.max() < F.NC)), name
            assert np.array_equal(boxes * 4, np.round(boxes * 4))                           # quarter-pixel corners: exact float32 areas
    for placement in F.PLACEMENTS:
        case, ref = cases[f"edges_{placement}"], F.filter_ref(f"edges_{placement}")
        assert case.counts == [F.EDGE_N] * len(F.EDGE_KEPT)
        for k, (rows, pos) in zip(F.EDGE_KEPT, ref):
            assert len(pos) == k and (np.diff(pos) > 0).all()
            if k:
                want = {"first": (0, k - 1), "last": (F.EDGE_N - k, F.EDGE_N - 1), "interleaved": (0, F.EDGE_N - 1)}[placement]
                assert (pos[0], pos[-1]) == want if k > 1 else pos[0] == want[0]
            assert len(rows) <= k and (k == 0 or len(rows) > 0)
            assert set(rows[:, 5].tolist()) <= {0.0, 1.0}
    inter = F.filter_ref("edges_interleaved")[5][1]
    assert (np.diff(inter) >= 2).all()                                                      # really interleaved: a dropped one between any two
    assert [len(pos) for _, pos in F.filter_ref("identity")] == cases["identity"].counts
    assert [len(pos) for _, pos in F.filter_ref("all_dropped")] == [0] and cases["all_dropped"].counts == [300]
    # the merged pair overlaps above the threshold: two classes with one label keep both, one class keeps one
    for name in ("merged", "same_class"):
        b = cases[name].frames[0][0]
        assert abs(_iou(b[0], b[1]) - cases[name].notes["iou"]) < 1e-6 and _iou(b[0], b[1]) > cases[name].iou
        rows = F.filter_ref(name)[0][0]
        assert len(rows) == cases[name].notes["rows"] and (rows[:, 5] == 0).all()
    # max_det binds on the kept candidates: at least 2 * max_det of them, none overlapping, and the cut removes some
    case = cases["maxdet10"]
    sub, pos = F.filtered_frame(case.frames[0], case.table)
    assert len(pos) == case.notes["kept"] >= 2 * case.max_det
    assert len(D.nms_keep32(sub, case.iou)) == len(pos) and len(D.nms_keep32(case.frames[0], case.iou)) == 40
    rows = F.filter_ref("maxdet10")[0][0]
    assert len(rows) == case.max_det
    late = D.nms_rows(case.frames[0], D.nms_keep32(case.frames[0], case.iou), case.max_det)   # the cut first, the filter behind it
    assert (case.table[late[:, 5].astype(int)] >= 0).sum() < case.max_det
    assert cases["mixed"].counts == list(F.MIXED_COUNTS) and cases["mixed"].max_cand == 4096
    kept = [len(pos) for _, pos in F.filter_ref("mixed")]
    assert kept[0] == 0 and kept[1] == 1 and 0 < kept[2] < 64 and 256 < kept[3] < 600 and 1024 < kept[4] < 4096
    assert len(set(F.filter_ref("mixed")[4][0][:, 5].tolist())) == 3                         # labels 0, 1, 2 of the sparse map all occur


def test_new_symbols_are_exported_and_bound():
    lib = L.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in L.SIGNATURES, n


def test_class_map_check_rules():
    assert E.class_map_check(np.arange(8)) == (8, 8)
    assert E.class_map_check(F.table_of(F.SWAP)) == (2, 2)
    assert E.class_map_check(F.table_of(F.MERGE)) == (1, 2)
    assert E.class_map_check(F.table_of(F.SPARSE)) == (3, 5)
    assert E.class_map_check([-1, -1, 2]) == (3, 1)                                         # labels need not be dense
    assert E.class_map_check([0]) == (1, 1)
    for bad in ([-1, -1, -1], [0, 3, -1], [0, -2, 1], [8] + [-1] * 7):
        with pytest.raises(L.VcError) as ei:
            E.class_map_check(bad)
        assert ei.value.code == VC_ERR_ARG, bad
    nl, nk = C.c_int(), C.c_int()
    assert L.lib().vc_class_map_check_host(None, 8, C.byref(nl), C.byref(nk)) == VC_ERR_ARG
    t = np.zeros(4, np.int32)
    assert L.lib().vc_class_map_check_host(L.ptr(t, C.c_int), 0, C.byref(nl), C.byref(nk)) == VC_ERR_ARG
    assert L.lib().vc_class_map_check_host(L.ptr(t, C.c_int), 4, None, None) == 0          # the outputs are optional


def test_class_table_forms_and_errors():
    np.testing.assert_array_equal(E.class_table(8, [2, 3, 5, 7]), [-1, -1, 0, 1, -1, 2, -1, 3])
    np.testing.assert_array_equal(E.class_table(8, [7, 3]), F.table_of(F.SWAP))              # list order gives the labels
    np.testing.assert_array_equal(E.class_table(8, F.SWAP), F.table_of(F.SWAP))
    np.testing.assert_array_equal(E.class_table(8, F.MERGE), F.table_of(F.MERGE))
    np.testing.assert_array_equal(E.class_table(8, F.SPARSE), F.table_of(F.SPARSE))
    np.testing.assert_array_equal(E.class_table(3, {np.int64(1): np.int32(2)}), [-1, 2, -1])
    assert E.class_table(8, [1]).dtype == np.int32
    for bad in ([8], [-1], [3, 3], {3: 8}, {3: -1}, {9: 0}, [], {}, [1.5], {2: 0.5}):
        with pytest.raises(ValueError):
            E.class_table(8, bad)


def test_bad_tables_are_refused_before_any_device_call():
    """VC_ERR_ARG (not VC_ERR_HIP) on a machine without a GPU as well: the table is judged before the engine or the device is touched."""
    lib = L.lib()
    case = F.filter_cases()["merged"]
    boxes, conf, cls = case.frames[0]
    mc, md = 64, 10
    bx, cf, cl = np.zeros((1, mc, 4), np.float32), np.zeros((1, mc), np.float32), np.zeros((1, mc), np.int32)
    bx[0, :2], cf[0, :2], cl[0, :2] = boxes, conf, cls
    cnt = np.array([2], np.int32)
    out, n_out, kept = np.zeros((1, md, 6), np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(table, counts=cnt, classes=cl, max_cand=mc):
        t = np.ascontiguousarray(table, dtype=np.int32)
        return lib.vc_class_filter_nms_host(L.ptr(bx, C.c_float), L.ptr(cf, C.c_float), L.ptr(classes, C.c_int), L.ptr(counts, C.c_int), 1, L.ptr(t, C.c_int), len(t),
                                            0.45, md, max_cand, None, L.ptr(out, C.c_float), L.ptr(n_out, C.c_int), L.ptr(kept, C.c_int), None)

    assert call([-1] * 8) == VC_ERR_ARG                                                     # nothing kept
    assert call([0, 9, -1, -1, -1, -1, -1, -1]) == VC_ERR_ARG                               # label outside [-1, n)
    assert call([0, -2, -1, -1, -1, -1, -1, -1]) == VC_ERR_ARG
    assert call(case.table, counts=np.array([65], np.int32)) == VC_ERR_ARG                 # more candidates than max_cand
    assert call(case.table, max_cand=100) == VC_ERR_ARG                                     # not a multiple of 64
    assert call(case.table[:4]) == VC_ERR_ARG                                               # candidate classes 3 / 7 outside a 4-class table
    bad_cls = cl.copy()
    bad_cls[0, 1] = -1
    assert call(case.table, classes=bad_cls) == VC_ERR_ARG
    # vc_engine_set_class_map judges the table before it looks at the engine
    for bad in ([-1] * 8, [0, 9] + [-1] * 6, [-3] + [0] * 7):
        t = np.asarray(bad, np.int32)
        assert lib.vc_engine_set_class_map(None, L.ptr(t, C.c_int), len(t)) == VC_ERR_ARG
        assert b"class map" in lib.vc_last_error()
    assert lib.vc_engine_set_class_map(None, None, 0) == VC_ERR_ARG and b"null engine" in lib.vc_last_error()


def test_filter_in_front_of_the_nms_is_not_the_filter_behind_it():
    """max_det = 10, classes [3, 7], frames 11 and 17 of the clip: upstream's order (filter, NMS, cut) returns 10 rows, filtering the
    unfiltered result returns fewer -- the reason the filter runs on the device in front of the NMS."""
    for i in (11, 17):
        early = F.clip_detect(i, classes=[3, 7], max_det=10)
        full = F.clip_detect(i, classes=None, max_det=10)
        late = full[np.isin(full[:, 5], [3, 7])]
        assert len(early) == 10 and len(full) == 10 and len(late) < 10, (i, len(early), len(late))
        assert set(early[:, 5].tolist()) <= {3.0, 7.0}
        np.testing.assert_array_equal(early[:len(late)], late)                              # the late rows are a prefix of the early ones
