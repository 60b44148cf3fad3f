"""CPU: vehicle-counting_amd/csrc/live_ckpt.h -- the live-checkpoint format, its size and offset functions, the per-item pack / unpack
functions the kernels call and ckpt_validate -- compiled for the host (tests/native/live_ckpt_host.cpp) and held to the Python
restatement of the format (tests/live_ckpt_cases.py) byte for byte on a small hand-written state; pack -> unpack under a permuted slot
table -> pack; every truncation and corruption refused; and the same file as a stand-alone program, also under
-fsanitize=address,undefined (a host program run directly: nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import live_ckpt_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "live_ckpt_host.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
_pi, _pu = C.POINTER(C.c_int), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def lch(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lch") / "liblch.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.lch_sizes.argtypes = [_pi]
    lib.lch_offsets.argtypes = [C.c_int] * 5 + [_pu]
    lib.lch_track_offsets.argtypes = [_pi, C.c_int, C.c_int, C.c_int, C.c_int, _pu]
    lib.lch_track_offsets.restype = C.c_uint64
    lib.lch_track_rows.argtypes = [C.c_int, C.c_int]
    lib.lch_pack.argtypes = [C.POINTER(K.View), C.c_char_p, C.c_uint64, _pi]
    lib.lch_pack.restype = C.c_uint64
    lib.lch_validate.argtypes = [C.c_char_p, C.c_uint64]
    lib.lch_unpack.argtypes = [C.c_char_p, C.c_uint64, _pi, C.POINTER(K.View)]
    return lib


def c_pack(lch, st, cap=1 << 20, fill=0x5a):
    buf = C.create_string_buffer(bytes([fill]) * cap, cap)
    ovf = C.c_int(-1)
    v = K.view_of(st)
    n = lch.lch_pack(C.byref(v), buf, cap, C.byref(ovf))
    return n, ovf.value, buf.raw


@pytest.fixture(scope="module")
def hand(lch):
    st = K.hand_state()
    n, ovf, raw = c_pack(lch, st)
    assert ovf == 0
    return st, raw[:n]


def test_sizes_and_offsets(lch):
    s = (C.c_int * 10)()
    lch.lch_sizes(s)
    assert list(s)[:8] == [K.HEADER.itemsize, K.CAMERA.itemsize, K.STATS.itemsize, K.TRACKER.itemsize, K.TRACK.itemsize, K.REC.itemsize, K.HDR.itemsize, 88]
    assert s[9] == C.sizeof(K.View)
    for n_cam, max_dir, n_labels in [(1, 1, 1), (2, 3, 2), (8, 16, 4), (3, 5, 7)]:
        o = (C.c_uint64 * 5)()
        for cam, t in [(0, 0), (n_cam - 1, n_cam * n_labels - 1)]:
            lch.lch_offsets(n_cam, max_dir, n_labels, cam, t, o)
            assert list(o) == [K.camera_bytes(max_dir, n_labels), K.camera_off(cam, max_dir, n_labels), K.stats_off(n_cam, max_dir, n_labels),
                               K.tracker_off(t, n_cam, max_dir, n_labels), K.tracks_off(n_cam, max_dir, n_labels)]
            assert all(v % 16 == 0 for v in o)
        rows = np.array([0, 3, 100, 1, 0, 0, 7], np.int32)
        off = np.zeros(len(rows), np.uint64)
        total = lch.lch_track_offsets(rows.ctypes.data_as(_pi), len(rows), n_cam, max_dir, n_labels, off.ctypes.data_as(_pu))
        want, want_total = K.track_offsets(rows.tolist(), n_cam, max_dir, n_labels)
        assert off.tolist() == want and total == want_total
    assert [lch.lch_track_rows(g, 3) for g in (-1, 0, 2, 3, 9)] == [0, 0, 2, 3, 3]


def test_hand_state_packs_to_the_python_blob(lch, hand):
    st, blob = hand
    want = K.pack(st)
    assert len(blob) == len(want) == K.tracks_off(2, 3, 2) + 4 * 704 + sum(K.HAND_ROWS) * 2048
    assert blob == want
    assert lch.lch_validate(blob, len(blob)) == 0
    p = K.parse(blob)
    # the cases the state is written for
    n = [int(t["params"]["n_tracks"]) for t in p["trackers"]]
    assert n == [2, 0, 1, 1]
    t0 = p["trackers"][0]["tracks"]
    assert t0[0]["rec"]["state"] == K.TENTATIVE and t0[0]["rec"]["gal_count"] == 0 and t0[0]["slot"].tobytes() == bytes(88)   # closed: zeros, not the stale fields
    assert t0[1]["rec"]["state"] == K.CONFIRMED and t0[1]["rec"]["gal_count"] == 3 == p["trackers"][0]["params"]["nn_budget"] and t0[1]["rec"]["gal_head"] != 0
    assert t0[1]["slot"]["open"] == 1 and p["trackers"][2]["tracks"][0]["slot"]["open"] == 0 and p["trackers"][3]["tracks"][0]["slot"]["open"] == 1
    assert [int(c["frames_done"]) for c, _ in p["cameras"]] == [24, 19] and p["retired"] == 18
    assert [int(t["params"]["err"]) for t in p["trackers"]] == [0, 2, 0, 0]                               # a stopped tracker stays stopped
    np.testing.assert_array_equal(p["trackers"][0]["gallery"][1], st["gallery"][2, :3])                  # physical rows [0, 3), list order
    np.testing.assert_array_equal(p["cameras"][1][1], st["base"][1])
    # a staging buffer that is too small: the flag, the size, and nothing behind the header
    n2, ovf, raw = c_pack(lch, st, cap=len(blob) - 16, fill=0x33)
    assert (n2, ovf) == (len(blob), 1) and raw[:64] == blob[:64] and set(raw[64:]) == {0x33}


def test_pack_unpack_under_permuted_slots_pack(lch, hand):
    st, blob = hand
    other = K.empty_state(2, 2, 3, n_trackers=6, list_cap=4, max_tracks=9, budget_cap=7)                 # another budget cap: other row strides
    for k in ("trackers", "params", "frames_done", "poly_n", "n_dir", "polygons", "dir_lines"):
        other[k][:] = st[k]
    other["slots"][:] = np.frombuffer(bytes([0x11]) * (9 * 88), K.SLOT)                                  # every slot a track takes is rewritten
    slot_of = np.array([8, 0, 3, 5], np.int32)
    v = K.view_of(other)
    assert lch.lch_unpack(blob, len(blob), slot_of.ctypes.data_as(_pi), C.byref(v)) == 0
    assert other["lists"][3, :2].tolist() == [8, 0] and other["lists"][5, 0] == 3 and other["lists"][2, 0] == 5
    np.testing.assert_array_equal(other["mean"][[8, 0, 3, 5]], st["mean"][K.HAND_SLOTS])
    np.testing.assert_array_equal(other["base"], st["base"])
    assert other["hdrs"]["err"][[3, 0, 5, 2]].tolist() == [0, 2, 0, 0]
    n, ovf, raw = c_pack(lch, other)
    assert ovf == 0 and raw[:n] == blob


def test_validate_refuses_truncations_trailing_bytes_and_every_field_out_of_range(lch, hand):
    _, blob = hand
    for n in range(len(blob)):                                               # every proper prefix, from an exact-size buffer
        assert lch.lch_validate(blob[:n], n) != 0, n
    assert lch.lch_validate(blob + b"\0", len(blob) + 1) != 0 and lch.lch_validate(blob + bytes(16), len(blob) + 16) != 0
    table = K.corruption_table(blob)
    assert len(table) > 100 and len({name for name, _, _ in table}) == len(table)
    for name, off, data in table:
        bad = K.apply_patch(blob, off, data)
        assert bad != blob, name
        assert lch.lch_validate(bad, len(bad)) != 0, name


def test_python_reader_of_frames_done(lch, hand):
    """engine.checkpoint_frames_done restates two sizes of the header: held to the C structs and to the hand blob"""
    import vehicle_counting_amd.engine as E
    s = (C.c_int * 10)()
    lch.lch_sizes(s)
    assert (E.CKPT_HEADER_BYTES, E.CKPT_CAMERA_BYTES) == (s[0], s[1])
    _, blob = hand
    assert E.checkpoint_frames_done(blob).tolist() == [24, 19] and E.checkpoint_dims(blob) == (2, 2, 3)
    with pytest.raises(ValueError):
        E.checkpoint_frames_done(b"VCTRK01\0" + blob[8:])


@pytest.mark.parametrize("sanitize", [False, True])
def test_stand_alone_program(tmp_path, hand, sanitize):
    _, blob = hand
    exe = str(tmp_path / "live_ckpt_host")
    flags = FLAGS + (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    subprocess.run(flags + ["-DLCH_MAIN", "-o", exe, SRC], check=True)
    path = str(tmp_path / "table.bin")
    with open(path, "wb") as f:
        f.write(K.table_file(blob, K.corruption_table(blob)))
    for args in ([exe], [exe, path]):
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and "0 failures" in r.stdout and r.stderr == "", r.stdout + r.stderr
