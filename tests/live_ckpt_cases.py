"""The live-checkpoint blob (vehicle-counting_amd/csrc/live_ckpt.h) restated with NumPy structured types: sizes, offsets, an independent
`pack` of a state held in arrays, a `parse` of a blob into fields, a small hand-written state, and the table of corruptions a validator
must refuse.  CPU tests hold the header's host build to it byte for byte (tests/test_live_ckpt_host.py); the GPU tests parse the blobs
the kernels pack with it (tests/test_gpu_live_checkpoint.py)."""
import ctypes as C
import struct

import numpy as np

from live_count_cases import SLOT

MAX_POINTS, MAX_DIRS, FEAT, ROW_BYTES = 64, 16, 512, 2048
MAGIC = b"VCLIVE01"
TENTATIVE, CONFIRMED = 1, 2

HEADER = np.dtype([("magic", "S8"), ("version", "<i4"), ("feat_dim", "<i4"), ("n_cam", "<i4"), ("n_labels", "<i4"), ("max_dir", "<i4"),
                   ("n_tracks", "<i4"), ("total_size", "<u8"), ("pad", "<u8", 3)])
CAMERA = np.dtype([("frames_done", "<i8"), ("poly_n", "<i4"), ("n_dir", "<i4"), ("polygon", "<f8", MAX_POINTS * 2), ("dir_lines", "<f8", MAX_DIRS * 4)])
STATS = np.dtype([("retired", "<i4"), ("pad", "<i4", 3)])
TRACKER = np.dtype([("next_id", "<i8"), ("max_dist", "<f8"), ("min_confidence", "<f8"), ("nms_max_overlap", "<f8"), ("max_iou_distance", "<f8"),
                    ("max_age", "<i4"), ("n_init", "<i4"), ("nn_budget", "<i4"), ("n_tracks", "<i4"), ("err", "<i4"), ("pad", "<i4")])
REC = np.dtype([("id", "<i8"), ("state", "<i4"), ("hits", "<i4"), ("age", "<i4"), ("tsu", "<i4"), ("gal_count", "<i4"), ("gal_head", "<i4")])
TRACK = np.dtype([("rec", REC), ("mean", "<f8", 8), ("cov", "<f8", 64), ("slot", SLOT), ("pad", "<i8")])
HDR = np.dtype([("max_dist", "<f8"), ("max_iou_distance", "<f8"), ("next_id", "<i8"), ("max_age", "<i4"), ("n_init", "<i4"), ("nn_budget", "<i4"),
                ("n_tracks", "<i4"), ("err", "<i4"), ("pad", "<i4")])
assert (HEADER.itemsize, CAMERA.itemsize, STATS.itemsize, TRACKER.itemsize, REC.itemsize, TRACK.itemsize, HDR.itemsize) == (64, 1552, 16, 64, 32, 704, 48)


def align(x):
    return (x + 15) // 16 * 16


def camera_bytes(max_dir, n_labels):
    return align(CAMERA.itemsize + 4 * max_dir * n_labels)


def camera_off(cam, max_dir, n_labels):
    return HEADER.itemsize + cam * camera_bytes(max_dir, n_labels)


def stats_off(n_cam, max_dir, n_labels):
    return camera_off(n_cam, max_dir, n_labels)


def tracker_off(t, n_cam, max_dir, n_labels):
    return stats_off(n_cam, max_dir, n_labels) + STATS.itemsize + t * TRACKER.itemsize


def tracks_off(n_cam, max_dir, n_labels):
    return tracker_off(n_cam * n_labels, n_cam, max_dir, n_labels)


def track_bytes(rows):
    return TRACK.itemsize + rows * ROW_BYTES


def track_offsets(rows, n_cam, max_dir, n_labels):
    """per-track offsets and the total size"""
    o, off = tracks_off(n_cam, max_dir, n_labels), []
    for r in rows:
        off.append(o)
        o += track_bytes(r)
    return off, o


# ---- a state in arrays, as the engine holds it: the tracker pool and one counter -----------------------------------------------
def empty_state(n_cam, n_labels, max_dir, n_trackers, list_cap, max_tracks, budget_cap):
    return {
        "n_cam": n_cam, "n_labels": n_labels, "max_dir": max_dir, "list_cap": list_cap, "max_tracks": max_tracks, "budget_cap": budget_cap,
        "hdrs": np.zeros(n_trackers, HDR), "lists": np.zeros((n_trackers, list_cap), np.int32), "recs": np.zeros(max_tracks, REC),
        "mean": np.zeros((max_tracks, 8)), "cov": np.zeros((max_tracks, 64)), "gallery": np.zeros((max_tracks, budget_cap, FEAT), np.float32),
        "slots": np.zeros(max_tracks, SLOT), "base": np.zeros((n_cam, max_dir, n_labels), np.int32), "stats": np.zeros(2, np.int32),
        "polygons": np.zeros((n_cam, MAX_POINTS * 2)), "poly_n": np.zeros(n_cam, np.int32), "dir_lines": np.zeros((n_cam, MAX_DIRS * 4)),
        "n_dir": np.zeros(n_cam, np.int32), "trackers": np.zeros(n_cam * n_labels, np.int32), "params": np.zeros((n_cam * n_labels, 2)),
        "frames_done": np.zeros(n_cam, np.int64),
    }


def pack(st) -> bytes:
    """The blob of a state, written from the format's description alone."""
    n_cam, n_labels, max_dir = st["n_cam"], st["n_labels"], st["max_dir"]
    tracks = []                                                    # (tracker section index, slot, rows) in blob order
    for t in range(n_cam * n_labels):
        h = st["hdrs"][st["trackers"][t]]
        for i in range(h["n_tracks"]):
            slot = int(st["lists"][st["trackers"][t], i])
            tracks.append((t, slot, min(max(int(st["recs"][slot]["gal_count"]), 0), int(h["nn_budget"]))))
    off, total = track_offsets([r for _, _, r in tracks], n_cam, max_dir, n_labels)
    out = bytearray(total)
    hd = np.zeros(1, HEADER)
    hd["magic"], hd["version"], hd["feat_dim"], hd["n_cam"], hd["n_labels"], hd["max_dir"] = MAGIC, 1, FEAT, n_cam, n_labels, max_dir
    hd["n_tracks"], hd["total_size"] = len(tracks), total
    out[:64] = hd.tobytes()
    for c in range(n_cam):
        cam = np.zeros(1, CAMERA)
        cam["frames_done"], cam["poly_n"], cam["n_dir"] = st["frames_done"][c], st["poly_n"][c], st["n_dir"][c]
        cam["polygon"], cam["dir_lines"] = st["polygons"][c], st["dir_lines"][c]
        o = camera_off(c, max_dir, n_labels)
        out[o:o + CAMERA.itemsize] = cam.tobytes()
        b = st["base"][c].astype("<i4").tobytes()
        out[o + CAMERA.itemsize:o + CAMERA.itemsize + len(b)] = b
    o = stats_off(n_cam, max_dir, n_labels)
    out[o:o + 16] = struct.pack("<4i", int(st["stats"][1]), 0, 0, 0)
    for t in range(n_cam * n_labels):
        h = st["hdrs"][st["trackers"][t]]
        k = np.zeros(1, TRACKER)
        for f in ("next_id", "max_dist", "max_iou_distance", "max_age", "n_init", "nn_budget", "n_tracks", "err"):
            k[f] = h[f]
        k["min_confidence"], k["nms_max_overlap"] = st["params"][t]
        o = tracker_off(t, n_cam, max_dir, n_labels)
        out[o:o + 64] = k.tobytes()
    for (t, slot, rows), o in zip(tracks, off):
        tr = np.zeros(1, TRACK)
        tr["rec"], tr["mean"], tr["cov"] = st["recs"][slot], st["mean"][slot], st["cov"][slot]
        if st["slots"][slot]["open"]:
            tr["slot"] = st["slots"][slot]
        out[o:o + 704] = tr.tobytes()
        out[o + 704:o + 704 + rows * ROW_BYTES] = st["gallery"][slot, :rows].astype("<f4").tobytes()
    return bytes(out)


def parse(blob):
    """A well-formed blob -> {"header", "cameras": [(CAMERA record, base (max_dir, n_labels))], "retired", "trackers": [{"params": TRACKER record,
    "tracks": TRACK array, "gallery": [rows x 512 float32 per track]}]} with trackers in (camera, label) order."""
    hd = np.frombuffer(blob, HEADER, 1)[0]
    assert hd["magic"] == MAGIC and hd["total_size"] == len(blob), "not a live checkpoint"
    n_cam, n_labels, max_dir = int(hd["n_cam"]), int(hd["n_labels"]), int(hd["max_dir"])
    cams = []
    for c in range(n_cam):
        o = camera_off(c, max_dir, n_labels)
        cams.append((np.frombuffer(blob, CAMERA, 1, o)[0], np.frombuffer(blob, "<i4", max_dir * n_labels, o + CAMERA.itemsize).reshape(max_dir, n_labels)))
    retired = int(np.frombuffer(blob, STATS, 1, stats_off(n_cam, max_dir, n_labels))[0]["retired"])
    o, trackers = tracks_off(n_cam, max_dir, n_labels), []
    for t in range(n_cam * n_labels):
        k = np.frombuffer(blob, TRACKER, 1, tracker_off(t, n_cam, max_dir, n_labels))[0]
        tracks, gal = np.zeros(int(k["n_tracks"]), TRACK), []
        for i in range(int(k["n_tracks"])):
            tracks[i] = np.frombuffer(blob, TRACK, 1, o)[0]
            rows = int(tracks[i]["rec"]["gal_count"])
            gal.append(np.frombuffer(blob, "<f4", rows * FEAT, o + 704).reshape(rows, FEAT))
            o += track_bytes(rows)
        trackers.append({"params": k, "tracks": tracks, "gallery": gal})
    assert o == len(blob)
    return {"header": hd, "cameras": cams, "retired": retired, "trackers": trackers}


# ---- the hand-written state of the CPU tests: 2 cameras x 2 labels ---------------------------------------------------------------
def hand_state():
    """Tracker sections (camera, label) -> pool trackers 3, 0, 5, 2.  (0, 0): a tentative track without gallery rows (closed LiveSlot with
    stale fields) and a confirmed one whose ring has wrapped (nn_budget 3, gal_head 1, open LiveSlot); (0, 1): no track; (1, 0): a
    confirmed track with a partly filled ring and a closed LiveSlot; (1, 1): one confirmed track, open LiveSlot, a full ring at head 0."""
    rng = np.random.default_rng(7)
    st = empty_state(n_cam=2, n_labels=2, max_dir=3, n_trackers=6, list_cap=4, max_tracks=9, budget_cap=5)
    st["trackers"][:] = [3, 0, 5, 2]
    st["params"][:] = [[0.3, 1.0], [0.35, 0.9], [0.3, 1.0], [0.25, 0.8]]
    st["frames_done"][:] = [24, 19]
    st["poly_n"][:], st["n_dir"][:] = [4, 5], [2, 3]
    st["polygons"][0, :8] = [10, 10, 50, 10, 50, 50, 10, 50]
    st["polygons"][1, :10] = [0, 0, 64, 0, 64, 48.5, 32, 60, 0, 48]
    st["dir_lines"][0, :8] = [0, 0, 10, 0, 0, 10, 0, 0]
    st["dir_lines"][1, :12] = [0, 0, 1, 1, 5, 5, 4, 4, 0, 9, 9, 0]
    st["base"][0, :2] = [[3, 1], [0, 2]]
    st["base"][1] = [[1, 0], [0, 0], [7, 4]]
    st["stats"][:] = [2, 18]
    for tr, (nn, n, nid, err) in {3: (3, 2, 12, 0), 0: (3, 0, 1, 2), 5: (4, 1, 6, 0), 2: (3, 1, 40, 0)}.items():     # tracker 0: stopped by an error
        st["hdrs"][tr] = (0.2, 0.7, nid, 2, 1, nn, n, err, 0)
    st["hdrs"][1] = (0.5, 0.5, 99, 9, 9, 2, 3, 0, 0)               # a tracker of no counter: never read
    st["lists"][3, :2], st["lists"][5, :1], st["lists"][2, :1] = [7, 2], [0], [4]
    st["lists"][1, :3] = [1, 3, 5]
    st["recs"][7] = (11, TENTATIVE, 1, 1, 0, 0, 0)
    st["recs"][2] = (4, CONFIRMED, 9, 12, 1, 3, 1)
    st["recs"][0] = (5, CONFIRMED, 2, 2, 0, 2, 2)
    st["recs"][4] = (39, CONFIRMED, 30, 31, 0, 3, 0)
    st["mean"][:] = rng.normal(size=st["mean"].shape) * 100
    st["cov"][:] = rng.normal(size=st["cov"].shape)
    st["gallery"][:] = rng.normal(size=st["gallery"].shape).astype(np.float32)
    st["slots"][2] = (1, 0, 0, 1, 24, [12, 14, 30, 33], [20, 22, 40, 41])
    st["slots"][4] = (1, 1, 1, 2, 19, [1, 2, 3, 4], [5, 6, 7, 8])
    st["slots"][7] = (0, 0, 0, 1, 3, [9, 9, 9, 9], [8, 8, 8, 8])     # closed: its stale fields never reach the blob
    st["slots"][0] = (0, 1, 0, 3, 11, [1, 1, 2, 2], [3, 3, 4, 4])    # closed
    return st


HAND_ROWS = [0, 3, 2, 3]              # gallery rows of the hand state's tracks, blob order
HAND_SLOTS = [7, 2, 0, 4]             # their pool slots


# ---- ctypes mirror of ck::CkptView, over a state's arrays ------------------------------------------------------------------------
class View(C.Structure):
    _fields_ = [("hdrs", C.c_void_p), ("lists", C.c_void_p), ("list_cap", C.c_int), ("recs", C.c_void_p), ("mean", C.c_void_p), ("cov", C.c_void_p),
                ("gallery", C.c_void_p), ("budget_cap", C.c_int), ("max_tracks", C.c_int),
                ("slots", C.c_void_p), ("base", C.c_void_p), ("stats", C.c_void_p), ("polygons", C.c_void_p), ("poly_n", C.c_void_p),
                ("dir_lines", C.c_void_p), ("n_dir", C.c_void_p), ("n_cam", C.c_int), ("n_labels", C.c_int), ("max_dir", C.c_int),
                ("trackers", C.c_void_p), ("params", C.c_void_p), ("frames_done", C.c_void_p)]


def view_of(st):
    v = View()
    for name, _ in View._fields_:
        x = st[name]
        setattr(v, name, x.ctypes.data if isinstance(x, np.ndarray) else int(x))
    return v


# ---- what a validator must refuse --------------------------------------------------------------------------------------------------
def _field(dtype, name, base=0):
    """(offset, NumPy scalar type) of a possibly nested field 'a.b' of a structured type"""
    o = base
    for part in name.split("."):
        sub, fo = dtype.fields[part][:2]
        o, dtype = o + fo, sub
    return o, (dtype.subdtype[0] if dtype.subdtype else dtype)


def corruption_table(blob):
    """[(name, offset, bytes)]: the blob with `bytes` written at `offset` is malformed -- every header and count field out of range, in turn.
    Written for blobs whose first tracker holds at least one track with an open or closed LiveSlot (the hand state, the GPU clip)."""
    p = parse(blob)
    hd = p["header"]
    n_cam, n_labels, max_dir = int(hd["n_cam"]), int(hd["n_labels"]), int(hd["max_dir"])
    out = []

    def put(name, dtype, field, base, value):
        o, t = _field(dtype, field, base)
        if all(n != f"{name}={value}" for n, _, _ in out):                  # two rules may name one value
            out.append((f"{name}={value}", o, np.array([value], t).tobytes()))

    out.append(("magic", 0, b"VCTRK01\0"))
    for f, vals in {"version": [0, 2], "feat_dim": [0, 256], "n_cam": [0, -1, n_cam + 1, 1 << 20], "n_labels": [0, -3, n_labels + 1], "max_dir": [0, MAX_DIRS + 1, -1],
                    "n_tracks": [-1, int(hd["n_tracks"]) + 1, max(int(hd["n_tracks"]) - 1, -1)], "total_size": [len(blob) - 16, len(blob) + 16, 0]}.items():
        for v in vals:
            put("header." + f, HEADER, f, 0, v)
    out.append(("header.pad", 40, b"\1"))
    for c in range(n_cam):
        o = camera_off(c, max_dir, n_labels)
        for f, vals in {"frames_done": [-1], "poly_n": [0, MAX_POINTS + 1, -1], "n_dir": [0, max_dir + 1, -2]}.items():
            for v in vals:
                put(f"camera{c}.{f}", CAMERA, f, o, v)
        if camera_bytes(max_dir, n_labels) > CAMERA.itemsize + 4 * max_dir * n_labels:
            out.append((f"camera{c}.padding", o + camera_bytes(max_dir, n_labels) - 1, b"\x7f"))
    o = stats_off(n_cam, max_dir, n_labels)
    put("stats.retired", STATS, "retired", o, -1)
    out.append(("stats.pad", o + 4, b"\1"))
    to = tracks_off(n_cam, max_dir, n_labels)
    for t, tk in enumerate(p["trackers"]):
        o = tracker_off(t, n_cam, max_dir, n_labels)
        k = tk["params"]
        for f, vals in {"next_id": [0, -5], "max_age": [0], "n_init": [0, -1], "nn_budget": [0, -1], "n_tracks": [-1, int(k["n_tracks"]) + 1, 1 << 21],
                        "err": [-1, 6], "pad": [1]}.items():
            for v in vals:
                put(f"tracker{t}.{f}", TRACKER, f, o, v)
        if k["n_tracks"] > 0:
            put(f"tracker{t}.n_tracks", TRACKER, "n_tracks", o, int(k["n_tracks"]) - 1)
        for i, tr in enumerate(tk["tracks"]):
            rec, name = tr["rec"], f"tracker{t}.track{i}"
            for f, vals in {"rec.id": [0, int(k["next_id"])], "rec.state": [0, 3], "rec.hits": [-1], "rec.age": [-1], "rec.tsu": [-1],
                            "rec.gal_count": [-1, int(k["nn_budget"]) + 1, int(rec["gal_count"]) + 1, int(rec["gal_count"]) - 1],
                            "rec.gal_head": [-1, int(k["nn_budget"])], "slot.open": [2, -1], "pad": [1]}.items():
                for v in vals:
                    put(f"{name}.{f}", TRACK, f, to, v)
            if tr["slot"]["open"]:
                for f, vals in {"slot.cam": [-1, n_cam, (t // n_labels + 1) % max(n_cam, 2)], "slot.label": [-1, n_labels], "slot.at_last": [0]}.items():
                    for v in vals:
                        put(f"{name}.{f}", TRACK, f, to, v)
            else:
                for f in ("slot.cam", "slot.label", "slot.at_last", "slot.last_frame"):
                    put(f"{name}.{f}", TRACK, f, to, 1)
                out.append((f"{name}.slot.first", _field(TRACK, "slot.first", to)[0], b"\1"))
                out.append((f"{name}.slot.last", _field(TRACK, "slot.last", to)[0] + 24, b"\1"))
            to += track_bytes(int(rec["gal_count"]))
    return out


def apply_patch(blob, offset, data):
    b = bytearray(blob)
    b[offset:offset + len(data)] = data
    return bytes(b)


def table_file(blob, table) -> bytes:
    """The file tests/native/live_ckpt_host.cpp's stand-alone program reads: u64 size | blob | u32 n | n x {u64 offset, u32 length, bytes}"""
    out = struct.pack("<Q", len(blob)) + blob + struct.pack("<I", len(table))
    for _, o, data in table:
        out += struct.pack("<QI", o, len(data)) + data
    return out
