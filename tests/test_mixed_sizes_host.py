"""CPU: the host half of sized batches (cameras of different frame sizes in one detector batch): vc_autoshape_net_size against the
oracle's AutoShape rule, vc_frames_layout_sized_host (cell size, raw-buffer packing with every frame's own size, every refusal with its
own code and the frame it names), and the opt-in of CountingPipeline.run_streams.  No GPU is needed: all of it is pure host code that
runs before any HIP call."""
import types

import numpy as np
import pytest

import yuv_ref
import vehicle_counting_amd.engine as E
from oracle import imageops as oi
from vehicle_counting_amd import _lib as L
from vehicle_counting_amd.pipeline import CountingPipeline, FrameSource

VC_ERR_ARG = 1
BUF = np.zeros(1 << 16, np.uint8)          # every frame points here; nothing reads it without a device
ADDR = BUF.ctypes.data


def refused(fn, code=VC_ERR_ARG):
    with pytest.raises(L.VcError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


# ---- network shape -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,want", [((360, 640), (384, 640)), ((180, 320), (384, 640)), ((540, 960), (384, 640)), ((362, 640), (384, 640)),
                                     ((1080, 1920), (384, 640)), ((720, 1280), (384, 640)), ((480, 640), (480, 640))])
def test_autoshape_net_size_listed_cases(hw, want):
    assert E.autoshape_net_size(*hw, 640) == want
    assert tuple(oi.autoshape_size([hw], 640)) == want


def test_autoshape_net_size_equals_the_oracle_on_random_shapes():
    rng = np.random.default_rng(640)
    for _ in range(400):
        h, w = (int(v) for v in rng.integers(1, 2200, 2))
        size = int(rng.choice([320, 416, 512, 640, 641, 800, 1280]))
        assert E.autoshape_net_size(h, w, size) == tuple(oi.autoshape_size([(h, w)], size)), (h, w, size)
    for bad in ((0, 640, 640), (360, 0, 640), (360, 640, 0)):
        refused(lambda: E.autoshape_net_size(*bad))


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def padded_odd(fmt, h, w):
    """tests/test_frames_layout.py::geometry("padded_odd"): nothing aligned"""
    py, pc = w + 7, (w if fmt == "nv12" else w // 2) + 3
    geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * h + 13)
    if fmt == "i420":
        geo["offset_v"] = geo["offset_c"] + pc * (h // 2) + 5
    return geo


# six frames of four sizes that all run at 384 x 640 (size 640); three of them host YUV with their own geometry
DIMS = [(360, 640), (180, 320), (540, 960), (362, 640), (180, 320), (360, 640)]


def six_frames():
    geos = [None, ("nv12", {}), ("i420", padded_odd("i420", 540, 960)), None, ("nv12", {}), ("nv12", padded_odd("nv12", 360, 640))]
    kinds = ["bgr_host", "yuv_host", "yuv_host", "bgr_dev", "yuv_dev", "yuv_host"]
    frames = [E.frame_src(k, ADDR, None if g is None else E.yuv_desc(g[0], **g[1])) for k, g in zip(kinds, geos)]
    return frames, geos


def test_sized_layout_cell_offsets_and_shape():
    frames, geos = six_frames()
    off, total, cell, net = E.frames_layout_sized(frames, DIMS, 640)
    assert net == (384, 640)
    assert cell == 540 * 960 * 3 and cell % 16 == 0                                         # the largest frame, already a multiple of 16
    assert [int(off[i]) for i in (0, 3, 4)] == [-1, -1, -1]                                 # -1 for everything that is not host YUV
    host, ends = [1, 2, 5], []
    for i in host:
        fmt, geo = geos[i]
        assert off[i] >= 0 and off[i] % 16 == 0
        ends.append(int(off[i]) + yuv_ref.batch_bytes(1, *DIMS[i], fmt, **geo))             # as long as one frame of ITS size and geometry
    assert off[1] < off[2] < off[5] and ends[0] <= off[2] and ends[1] <= off[5]             # ascending and disjoint
    assert total == ends[2]
    # the cell is rounded up to 16; odd BGR sizes are fine; img_size decides which frames go together
    off, total, cell, net = E.frames_layout_sized([E.frame_src("bgr_host", ADDR), E.frame_src("bgr_dev", ADDR)], [(37, 65), (5, 9)], 64)
    assert off.tolist() == [-1, -1] and total == 0 and net == (64, 64)
    assert cell == (37 * 65 * 3 + 15) // 16 * 16 and cell != 37 * 65 * 3
    assert E.frames_layout_sized([E.frame_src("bgr_host", ADDR)] * 2, [(480, 640), (360, 480)], 640)[3] == (480, 640)


def test_sized_layout_refusals():
    frames, _ = six_frames()
    # a frame of another network shape: named, with both shapes
    dims = list(DIMS)
    dims[3] = (480, 640)
    assert "frame 3: 480x640 runs at 480x640, frame 0 at 384x640" in refused(lambda: E.frames_layout_sized(frames, dims, 640))
    # an odd YUV size (the same size is fine for the BGR frame next to it)
    dims = list(DIMS)
    dims[0] = dims[1] = (181, 321)
    msg = refused(lambda: E.frames_layout_sized(frames, dims, 640))
    assert "frame 1:" in msg and "even height and width" in msg
    # null data
    bad = list(frames)
    bad[4] = E.frame_src("yuv_dev", None)
    assert "frame 4: null data" in refused(lambda: E.frames_layout_sized(bad, DIMS, 640))
    # b < 1
    assert "0 frames" in refused(lambda: E.frames_layout_sized([], [], 640))
    # a pitch below the row width of THAT frame's own w: 400 holds a 320-wide row, not a 640-wide one
    desc = E.yuv_desc("nv12", pitch_y=400, pitch_c=400)
    ok = [E.frame_src("bgr_host", ADDR), E.frame_src("yuv_host", ADDR, desc)]
    assert E.frames_layout_sized(ok, [(360, 640), (180, 320)], 640)[0].tolist() == [-1, 0]
    msg = refused(lambda: E.frames_layout_sized(ok, [(180, 320), (360, 640)], 640))
    assert "frame 1:" in msg and "pitch_y" in msg
    # unknown kind, bad size
    assert "frame 0:" in refused(lambda: E.frames_layout_sized([L.FrameSrc(9, ADDR, E.yuv_desc())], [(360, 640)], 640))
    assert "frame 0:" in refused(lambda: E.frames_layout_sized([E.frame_src("bgr_host", ADDR)], [(0, 640)], 640))


def test_sized_ingest_validates_first_and_has_no_cpu_fallback():
    import torch
    cells = np.zeros(2 * 48 * 64 * 3, np.uint8)
    good = [E.frame_src("bgr_host", ADDR), E.frame_src("yuv_host", ADDR, E.yuv_desc("nv12"))]
    assert "frame 1:" in refused(lambda: E.frames_to_bgr_sized([good[0], E.frame_src("yuv_dev", ADDR)], [(48, 64), (36, 64)], cells))
    assert "frame 1:" in refused(lambda: E.frames_to_bgr_sized(good, [(48, 64), (37, 64)], cells))
    if not torch.cuda.is_available():
        refused(lambda: E.frames_to_bgr_sized(good, [(48, 64), (36, 64)], cells), 2)         # VC_ERR_HIP: nothing is computed on the CPU


# ---- run_streams -------------------------------------------------------------------------------------------------------------------
def bare_pipeline(img_size=640):
    """run_streams checks the sizes before it touches the engine: a pipeline without one is enough here"""
    pipe = CountingPipeline.__new__(CountingPipeline)
    pipe.engine = types.SimpleNamespace(cfg=types.SimpleNamespace(img_size=img_size))
    return pipe


def test_run_streams_keeps_the_one_size_rule_by_default():
    a, b = FrameSource(np.zeros((2, 360, 640, 3), np.uint8)), FrameSource(np.zeros((2, 180, 320, 3), np.uint8))
    with pytest.raises(ValueError, match="one size"):
        bare_pipeline().run_streams([a, b], ["cam_00", "cam_01"], [None, None], batch=4, host_frames=True)


def test_run_streams_mixed_sizes_refuses_other_network_shapes():
    a, b = FrameSource(np.zeros((2, 360, 640, 3), np.uint8)), FrameSource(np.zeros((2, 480, 640, 3), np.uint8))
    with pytest.raises(ValueError, match="own call") as ei:
        bare_pipeline().run_streams([a, b], ["cam_00", "cam_01"], [None, None], batch=4, mixed_sizes=True)
    assert "cam_00: 360x640 runs at 384x640" in str(ei.value) and "cam_01: 480x640 runs at 480x640" in str(ei.value)
