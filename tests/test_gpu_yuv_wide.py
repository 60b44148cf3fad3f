"""GPU: the wider YUV ingest formats -- p016 (P010 / P012 / P016 surfaces), i010 (yuv420p10le), i422, i444.  The arithmetic is integer, so
every comparison is bit for bit (assert_array_equal) against the NumPy definition (tests/yuv_wide_ref.py):
  * yuv_to_bgr_kernel (vc_yuv_to_bgr_host) for every format x matrix x range, the 16-byte path and the generic one, tight and padded
    geometry, odd sizes where the format takes them, on uniformly random bytes (planes and padding);
  * every 16-bit word as a luma, a U and a V sample of both 16-bit formats;
  * the frame table and the sized frame table: ONE launch over all six YUV formats and BGR;
  * the stream path: run_stream of a p016 and an i444 clip, and run_streams of an NV12 and a p016 camera, equal the runs on the BGR frames
    the clips convert to;
  * the render path with a p016 device source."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import yuv_ref  # noqa: E402
import yuv_wide_ref as W  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402
from vehicle_counting_amd import _lib as L  # noqa: E402
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource, YuvFrameSource  # noqa: E402
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames  # noqa: E402
from vehicle_counting_amd.weights import synth_reid, synth_yolo  # noqa: E402

NC = 8
TRACK_CFG = dict(MAX_DIST=0.2, MIN_CONFIDENCE=0.25, NMS_MAX_OVERLAP=0.5, MAX_IOU_DISTANCE=0.6, MAX_AGE=30, N_INIT=3, NN_BUDGET=60)
GUARD = 4096
FILL = 0x5A
MODES = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]
KINDS = ("tight", "padded", "padded_odd")
ALL = ("nv12", "i420") + W.WIDE
# the smallest shapes at which the kernel can go wrong: one lane, one and two full 16-pixel groups, a partial group behind one and behind
# two full ones, more than one workgroup (96 x 176: 48 row pairs x 11 groups = 528 lanes); odd heights and widths where the format has them
SHAPES = [(2, 2), (4, 16), (6, 18), (8, 32), (6, 34), (96, 176)]
EXTRA = {"p016": [], "i010": [], "i422": [(1, 2), (3, 18)], "i444": [(1, 2), (3, 18), (1, 1), (3, 17), (5, 33)]}


# ---- kernel ------------------------------------------------------------------------------------------------------------------------
def convert_with_guards(buf, b, h, w, desc):
    """tests/test_gpu_yuv_ingest.py::convert_with_guards: vc_yuv_to_bgr_host writing into the middle of a larger host array"""
    n = b * h * w * 3
    out = np.full(n + 2 * GUARD, FILL, np.uint8)
    dst = C.cast(out.ctypes.data + GUARD, C.POINTER(C.c_uint8))
    L.check(L.lib().vc_yuv_to_bgr_host(C.byref(desc), L.ptr(buf, C.c_uint8), b, h, w, dst))
    return out[GUARD:GUARD + n].reshape(b, h, w, 3), out[:GUARD], out[GUARD + n:]


@pytest.mark.parametrize("matrix,full_range", MODES, ids=[f"{m}_{'full' if f else 'limited'}" for m, f in MODES])
@pytest.mark.parametrize("fmt", W.WIDE)
def test_kernel_matches_the_definition_bit_for_bit(fmt, matrix, full_range):
    rng = np.random.default_rng([W.IDS[fmt], matrix == "bt601", full_range])
    for h, w in SHAPES + EXTRA[fmt]:
        for kind in KINDS:
            for b in (1, 3):
                geo = W.geometry(kind, fmt, h, w)
                buf = rng.integers(0, 256, W.batch_bytes(b, h, w, fmt, **geo), dtype=np.uint8)            # padding bytes random too
                desc = E.yuv_desc(fmt, matrix, full_range, **geo)
                got, before, after = convert_with_guards(buf, b, h, w, desc)
                want = W.yuv_to_bgr(buf, b, h, w, fmt, matrix, full_range, **geo)
                case = f"{fmt} {matrix} full={full_range} {h}x{w} {kind} b={b}"
                np.testing.assert_array_equal(got, want, err_msg=case)
                assert (before == FILL).all() and (after == FILL).all(), case
                np.testing.assert_array_equal(E.yuv_to_bgr(buf, b, h, w, desc=desc), want, err_msg=case)   # the numpy-in / numpy-out wrapper


@pytest.mark.parametrize("fmt", ["p016", "i010"])
def test_every_sample_word(fmt):
    """512 x 512: frame 0's luma plane holds every 16-bit word four times (its chroma random words); in frames 1 and 2 U, then V, holds
    every word once against fixed other planes"""
    h = w = 512
    rng = np.random.default_rng(W.IDS[fmt])
    words = np.arange(65536, dtype=np.uint16)
    every_y = rng.permutation(np.tile(words, 4)).reshape(h, w)
    every_c = rng.permutation(words).reshape(h // 2, w // 2)
    widen = 8 if fmt == "p016" else 2
    flat_y, flat_c = np.full((h, w), 100 << widen, np.uint16), np.full((h // 2, w // 2), 77 << widen, np.uint16)
    rand_c = rng.integers(0, 65536, (2, h // 2, w // 2), dtype=np.uint16)
    frames = []
    for Y, U, V in ((every_y, rand_c[0], rand_c[1]), (flat_y, every_c, flat_c), (flat_y, flat_c, every_c)):
        chroma = [np.stack([U, V], axis=-1)] if fmt == "p016" else [U, V]
        frames.append(np.concatenate([p.astype("<u2").reshape(-1) for p in [Y] + chroma]))
    clip = np.stack(frames)                                                                        # (3, h * w * 3 / 2) uint16, tight
    assert clip.shape == (3, h * w * 3 // 2)
    data = clip.view(np.uint8).reshape(3, -1)
    Yr, Ur, Vr = W.planes(data, 3, h, w, fmt)                                                      # the reference reads the same words back
    assert (np.bincount(Yr[0].reshape(-1), minlength=65536) == 4).all()
    assert (np.bincount(Ur[1].reshape(-1), minlength=65536) == 1).all() and (np.bincount(Vr[2].reshape(-1), minlength=65536) == 1).all()
    for matrix, full in MODES:
        want = W.yuv_to_bgr(data, 3, h, w, fmt, matrix, full)
        np.testing.assert_array_equal(E.yuv_to_bgr(data, 3, h, w, fmt, matrix, full), want, err_msg=f"{fmt} {matrix} full={full}")
    np.testing.assert_array_equal(E.yuv_to_bgr(clip, 3, h, w, fmt), W.yuv_to_bgr(data, 3, h, w, fmt))      # uint16 in


# ---- frame tables ------------------------------------------------------------------------------------------------------------------
def build_batch(rng, specs):
    """specs: per frame (h, w, None (BGR) or (fmt, matrix, full range), geometry kind, host address mod 16), all frames carved out of ONE
    buffer of uniformly random bytes (padding included).  Returns (keep-alive buffer, frame list, dims, per-frame reference (h, w, 3))."""
    sizes = [h * w * 3 if typ is None else W.batch_bytes(1, h, w, typ[0], **W.geometry(kind, typ[0], h, w)) for h, w, typ, kind, _ in specs]
    buf = rng.integers(0, 256, sum(sizes) + 32 * len(specs) + 16, dtype=np.uint8)
    frames, want, pos = [], [], 0
    for (h, w, typ, kind, mod), n in zip(specs, sizes):
        pos += (mod - (buf.ctypes.data + pos)) % 16                                       # the next address congruent to `mod`
        data = buf[pos:pos + n]
        assert data.ctypes.data % 16 == mod
        if typ is None:
            frames.append(E.frame_src("bgr_host", data.ctypes.data))
            want.append(data.reshape(h, w, 3))
        else:
            fmt, matrix, full = typ
            geo = W.geometry(kind, fmt, h, w)
            frames.append(E.frame_src("yuv_host", data.ctypes.data, E.yuv_desc(fmt, matrix, full, **geo)))
            want.append(W.yuv_to_bgr(data, 1, h, w, fmt, matrix, full, **geo)[0])
        pos += n
    return buf, frames, [(h, w) for h, w, *_ in specs], want


def typed(fmts, n):
    """n frame types cycling through `fmts` and BGR, both matrices and both ranges spread over every format"""
    kinds = list(fmts) + [None]
    return [None if kinds[i % len(kinds)] is None else (kinds[i % len(kinds)],) + MODES[(i + 2 * (i // len(kinds))) % 4] for i in range(n)]


def table_cases():
    cases = {}
    # the 16-byte path (aligned address, tight or padded) and the generic one (address = 1 mod 16, or padded_odd) for every format in ONE launch
    t = typed(ALL, 28)
    cases["48x64 b=28"] = [(48, 64, t[f], ("tight", "padded")[(f // 7) % 2], 0) if f < 14 else (48, 64, t[f], KINDS[f % 3], 1 if f < 21 else 0) for f in range(28)]
    # a partial 16-pixel group behind a full one, nothing aligned
    t = typed(ALL, 14)
    cases["6x18 b=14"] = [(6, 18, t[f], KINDS[(f + 1) % 3], (3 * f) % 16) for f in range(14)]
    # an odd height: the last row pair has one row (i422, i444, BGR)
    t = typed(("i422", "i444"), 9)
    cases["3x32 b=9"] = [(3, 32, t[f], KINDS[f % 3], (0, 0, 7)[f % 3]) for f in range(9)]
    # odd height and width (i444, BGR)
    t = typed(("i444",), 6)
    cases["5x33 b=6"] = [(5, 33, t[f], KINDS[f % 3], (5 * f) % 16) for f in range(6)]
    return cases


@pytest.mark.parametrize("name", list(table_cases()))
def test_frame_table_matches_the_definition_frame_by_frame(name):
    specs = table_cases()[name]
    h, w = specs[0][:2]
    if name.startswith("48x64"):                                     # the case covers what it claims
        assert {s[2][0] for s in specs if s[2]} == set(ALL) and any(s[2] is None for s in specs)
        assert {s[2][1:] for s in specs if s[2]} == set(MODES)
        for fmt in ALL:
            assert {(s[3], s[4]) for s in specs if s[2] and s[2][0] == fmt} >= {("tight", 0), ("padded", 0)} and any(s[4] == 1 for s in specs if s[2] and s[2][0] == fmt)
    buf, frames, dims, want = build_batch(np.random.default_rng([h, w, len(specs)]), specs)
    n = len(frames) * h * w * 3
    out = np.full(n + 2 * GUARD, FILL, np.uint8)
    E.frames_to_bgr(frames, h, w, out=out[GUARD:GUARD + n])
    got = out[GUARD:GUARD + n].reshape(len(frames), h, w, 3)
    for f, spec in enumerate(specs):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{name} frame {f}: {spec}")
    assert (out[:GUARD] == FILL).all() and (out[GUARD + n:] == FILL).all(), name


def test_sized_frame_table_with_an_odd_sized_i444_frame():
    big, odd = (48, 64), (47, 63)
    t = typed(ALL, 16)
    full = [(*big, t[f], KINDS[f % 3], (0, 5)[(f // 3) % 2]) for f in range(16)]
    small = [(*odd, ("i444", "bt709", False), "tight", 0), (*odd, None, "tight", 3), (*odd, ("i444", "bt601", True), "padded_odd", 9), (*odd, ("i444", "bt601", False), "padded", 0)]
    specs = small[:1] + full[:5] + small[1:2] + full[5:11] + small[2:3] + full[11:] + small[3:]       # the largest frame neither first nor last
    assert specs[0][:2] == odd and specs[-1][:2] == odd and {s[2][0] for s in specs if s[2]} == set(ALL)
    buf, frames, dims, want = build_batch(np.random.default_rng(4763), specs)
    off, total, cell, net = E.frames_layout_sized(frames, dims, 1)
    assert cell == 48 * 64 * 3 and (47 * 63 * 3) % 16 != 0
    cells = np.full(len(specs) * cell, FILL, np.uint8)
    E.frames_to_bgr_sized(frames, dims, cells)
    cells = cells.reshape(len(specs), cell)
    for f, (h, w) in enumerate(dims):
        np.testing.assert_array_equal(cells[f, : h * w * 3].reshape(h, w, 3), want[f], err_msg=f"frame {f}: {specs[f]}")
        assert (cells[f, h * w * 3:] == FILL).all(), f"frame {f}: the kernel wrote beyond the frame inside its cell"


# ---- stream path -------------------------------------------------------------------------------------------------------------------
def whole_frame_zone(golden_dir, tmp_path, name, h, w):
    """tests/test_gpu_yuv_ingest.py::whole_frame_zone: cam_04's directions with the zone polygon widened to the frame, so that every
    tracked row reaches the CSV."""
    with open(os.path.join(golden_dir, name)) as f:
        z = json.load(f)
    for sh in z["shapes"]:
        if sh["label"] == "zone":
            sh["points"] = [[0.0, 0.0], [float(w), 0.0], [float(w), float(h)], [0.0, float(h)]]
    path = str(tmp_path / f"zone_{h}x{w}.json")
    with open(path, "w") as f:
        json.dump(z, f)
    return path


def assert_same_output(got, want, case):
    """tests/test_gpu_yuv_ingest.py::assert_same_output: one dict per CSV line, all of it equal, and the counts"""
    rows, counts = got
    ref_rows, ref_counts = want
    assert len(rows) == len(ref_rows), case
    for r, q in zip(rows, ref_rows):
        assert set(r) == set(q), case
        for k in r:
            np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(q[k]), err_msg=f"{case}: {k}")
    assert counts == ref_counts, case


H, WID, T, BATCH = 360, 640, 16, 4              # tests/test_gpu_yuv_ingest.py's f32 case (test_gpu_pipeline.py::test_csv_parity), 16 frames


@pytest.fixture(scope="module")
def stream():
    """one fp32 engine (conv numerics do not depend on the tile configuration a batch size selects) with two cameras' trackers, the clip
    as tight NV12 and the BGR frames the device must make of it"""
    import tempfile
    names = ["cam_00", "cam_01"]
    ysd, rsd = synth_yolo("yolov5s", nc=NC, seed=1702, det_scale=4.0, obj_shift=0.0), synth_reid(1702)
    eng = E.Engine(ysd, rsd, precision="f32", num_classes=NC, max_batch=BATCH, max_frame_hw=(H, WID), max_crops=BATCH * 300, max_tracks=4096, nn_budget_cap=60,
                   max_trackers=2 * NC)
    out_dir = tempfile.mkdtemp()
    cfg = types.SimpleNamespace(model_name="yolov5s", min_conf=0.25, min_iou=0.45, max_det=300)
    args = types.SimpleNamespace(weight=None, mapping=None, output_path=out_dir)
    pipe = CountingPipeline(args, cfg, {"cam": {n: {"tracking_config": TRACK_CFG} for n in names}}, engine=eng, class_names=[f"c{i}" for i in range(NC)])
    clip = synth_frames(T, H, WID, n_obj=6, seed=3)
    nv12 = bgr_to_yuv420(clip, "nv12")
    yield types.SimpleNamespace(eng=eng, pipe=pipe, names=names, nv12=nv12, expected=yuv_ref.yuv_to_bgr(nv12, T, H, WID, "nv12"))
    eng.close()


def test_run_stream_of_wide_sources_equals_the_bgr_source(stream, golden_dir, tmp_path):
    zone = whole_frame_zone(golden_dir, tmp_path, "cam_04_halfres.json", H, WID)
    want = stream.pipe.run_stream(FrameSource(stream.expected), "cam_00", zone, batch=BATCH, asynchronous=True)
    assert len(want[0]) >= 10, len(want[0])                                               # a populated CSV, not an empty-equals-empty pass
    for fmt in ("p016", "i444"):
        data = W.from_nv12(fmt, stream.nv12, H, WID)
        np.testing.assert_array_equal(W.yuv_to_bgr(data[:2], 2, H, WID, fmt), stream.expected[:2])        # the clip converts to the same BGR frames
        for host_frames in (False, True):
            got = stream.pipe.run_stream(YuvFrameSource(data, H, WID, fmt=fmt), "cam_00", zone, batch=BATCH, asynchronous=True, host_frames=host_frames)
            assert_same_output(got, want, f"{fmt} host_frames={host_frames}")


def test_run_streams_mixes_an_nv12_and_a_p016_camera(stream, golden_dir, tmp_path):
    zone = whole_frame_zone(golden_dir, tmp_path, "cam_04_halfres.json", H, WID)
    back = np.ascontiguousarray(stream.nv12[::-1])                                        # camera 1: the clip backwards, as 16-bit surfaces
    p016 = W.from_nv12("p016", back, H, WID).view(np.uint16)                              # uint16 in
    sources = [YuvFrameSource(stream.nv12, H, WID, fmt="nv12"), YuvFrameSource(p016, H, WID, fmt="p016")]
    expected = [stream.expected, stream.expected[::-1]]
    want = [stream.pipe.run_stream(FrameSource(np.ascontiguousarray(expected[c])), stream.names[c], zone, batch=BATCH, asynchronous=True) for c in range(2)]
    for c in range(2):
        assert len(want[c][0]) >= 10, (c, len(want[c][0]))
    got = stream.pipe.run_streams(sources, stream.names, [zone] * 2, batch=BATCH, host_frames=True)
    for c in range(2):
        assert_same_output(got[c], want[c], f"camera {c}")


# ---- render path -------------------------------------------------------------------------------------------------------------------
def test_render_from_a_p016_device_source():
    import torch
    b, h, w = 3, 32, 48
    rng = np.random.default_rng(16)
    geo = W.geometry("padded", "p016", h, w)
    surf = rng.integers(0, 256, W.batch_bytes(b, h, w, "p016", **geo), dtype=np.uint8)
    desc = E.yuv_desc("p016", "bt709", False, **geo)
    bgr = W.yuv_to_bgr(surf, b, h, w, "p016", "bt709", False, **geo)
    eng = E.Engine(None, None, max_batch=4, max_frame_hw=(h, w), max_crops=8, max_tracks=16, nn_budget_cap=4)      # a render-only engine
    n = b * h * w * 3 // 2
    outs = {}
    with E.Renderer(eng, max_batch=b, max_hw=(h, w), depth=1) as rnd:
        for kind, src, sd in (("yuv_dev", torch.from_numpy(surf).cuda(), desc), ("bgr_dev", torch.from_numpy(bgr).cuda(), None),
                              ("yuv_host", torch.from_numpy(surf).pin_memory(), desc)):
            out = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8).pin_memory()
            rnd.submit(src.data_ptr(), b, h, w, out.data_ptr() + GUARD, kind=kind, src_desc=sd)
            rnd.collect()
            outs[kind] = out.numpy().copy()
        with pytest.raises(L.VcError, match="ingest-only") as ei:                         # the destination stays NV12 / I420
            rnd.submit(torch.from_numpy(bgr).cuda().data_ptr(), b, h, w, np.zeros(2 * n, np.uint8), kind="bgr_dev", out_desc=E.yuv_desc("p016"))
        assert ei.value.code == 1 and rnd.outstanding == 0
    eng.close()
    assert (outs["bgr_dev"][:GUARD] == FILL).all() and (outs["bgr_dev"][GUARD + n:] == FILL).all() and len(set(outs["bgr_dev"][GUARD:GUARD + n].tolist())) > 16
    np.testing.assert_array_equal(outs["yuv_dev"], outs["bgr_dev"])
    np.testing.assert_array_equal(outs["yuv_host"], outs["bgr_dev"])
