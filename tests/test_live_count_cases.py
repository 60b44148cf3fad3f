"""CPU: tests/live_count_cases.py held to its own conditions, and the rule of the live counter checked on it: the NumPy
restatement of the per-slot / base state machine equals `NativeCounter.counts()` over the row prefix at EVERY batch boundary, for
batches of 1 frame, 3 frames and the whole clip.  The case table reaches every class it promises (checked while the cases run, not
by name)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import live_count_cases as LC
from vehicle_counting_amd import _lib as L
from vehicle_counting_amd.counting import NativeCounter

PAIRS = [(c, b) for c in LC.CASES for b in LC.BATCHES]


@pytest.fixture(scope="module")
def zone_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("zones")
    out = {}
    for c in LC.CASES:
        for cam in range(c.n_cam):
            out[c.name, cam] = str(d / f"{c.name}_{cam}.json")
            with open(out[c.name, cam], "w") as f:
                json.dump(c.zone_json(cam), f)
    return out


def native_counts(case, zone_files, upto):
    """Per camera the counts of a NativeCounter fed the rows of global frames [0, upto), padded to max_dir; and the tracks it holds."""
    out = np.zeros((case.n_cam, case.max_dir, case.n_labels), np.int32)
    tracks = 0
    for cam, (fr, ids, labels, boxes) in enumerate(LC.prefix_rows(case, upto)):
        nc = NativeCounter(zone_files[case.name, cam], case.n_labels)
        nc.add(fr, ids, labels, np.array(boxes, np.int64).reshape(-1, 4))
        out[cam, :case.n_dir[cam]] = nc.counts()
        n = C.c_int()
        L.check(L.lib().vc_counter_tracks(nc._h, C.byref(n)))
        tracks += n.value
        nc.close()
    return out, tracks


@pytest.mark.parametrize("case,batch", PAIRS, ids=[f"{c.name}-b{b}" for c, b in PAIRS])
def test_restatement_equals_native_counter_at_every_boundary(case, batch, zone_files):
    m = LC.Model(case)
    batches = LC.build(case, batch)
    for k, b in enumerate(batches):
        m.apply(b, last_batch=k == len(batches) - 1)
        got = m.counts()
        want, tracks = native_counts(case, zone_files, b.frames[-1] + 1)
        np.testing.assert_array_equal(got, want, err_msg=f"{case.name} after batch {k} of {batch or 'all'} frames")
        assert m.stats[0] + m.stats[1] == tracks                      # every track the counter holds is open or retired, once
        for cam in range(case.n_cam):
            assert not got[cam, case.n_dir[cam]:].any()
    assert sum(len(b.frames) for b in batches) == len(case.order)


def test_the_table_reaches_every_class():
    where = {k: [] for k in LC.CLASSES}
    for case, batch in PAIRS:
        m = LC.Model(case)
        batches = LC.build(case, batch)
        got = set(LC.geometry_classes(case))
        for k, b in enumerate(batches):
            m.apply(b, last_batch=k == len(batches) - 1)
            m.counts()
            got |= b.notes
        got |= m.seen
        assert got <= set(LC.CLASSES), got - set(LC.CLASSES)
        for k in got:
            where[k].append(f"{case.name}/b{batch}")
    for k in LC.CLASSES:
        print("%-62s %s" % (k, ", ".join(where[k])))
        assert where[k], k
    # the classes that depend on where a batch ends are met at more than one batch size
    assert len({w.split("/")[1] for w in where["a track retired mid-stream"]}) >= 2
    assert any(w.endswith("/b0") for w in where["a track confirmed and deleted inside one batch"])
    assert any(w.endswith("/b1") for w in where["two trackers freeing equal track ids in one batch"])


@pytest.mark.parametrize("case,batch", PAIRS, ids=[f"{c.name}-b{b}" for c, b in PAIRS])
def test_batches_are_what_the_tracker_kernel_hands_over(case, batch):
    """tasks grouped by tracker with frames ascending, rows inside the arena, and no slot with two owners inside one batch"""
    owner = {}
    for b in LC.build(case, batch):
        a = LC.arrays(b)
        t = a["tasks5"]
        assert list(t[:, 0]) == sorted(t[:, 0])
        for trk in set(t[:, 0]):
            fr = t[t[:, 0] == trk, 1]
            assert list(fr) == sorted(set(fr))
        assert (t[:, 3] + t[:, 4] <= len(a["rows6"])).all() and t[:, 4].sum() == len(a["rows6"])
        in_batch = {}
        for trk, k, label, off, n in t:
            for i in range(off, off + n):
                key = (trk, int(a["rows6"][i, 4]))
                slot = int(a["row_slot"][i])
                assert in_batch.setdefault(slot, key) == key, (case.name, slot)
                assert 0 <= slot < case.max_tracks
                owner[slot] = key
        assert len(set(a["freed"])) == len(a["freed"])
    assert LC.SLOT.itemsize == 88
