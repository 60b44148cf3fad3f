"""CPU: the YUV egress feature without a GPU -- the integer table and known answers of the NumPy definition (tests/yuv_enc_ref.py), its
stated relations to the project's other two definitions (the float test encoder synth.bgr_to_yuv420, the decoder tests/yuv_ref.py),
plane placement, the new C-ABI symbols and their bindings, the library's argument checks (VC_ERR_ARG / VC_ERR_CAPACITY before any HIP
call; a valid call without a GPU is VC_ERR_HIP: there is no CPU fallback) and YuvFrameSink's geometry."""
import ctypes as C

import numpy as np
import pytest

import yuv_enc_ref as enc
import yuv_ref
from vehicle_counting_amd import _lib as L
import vehicle_counting_amd.engine as E
from vehicle_counting_amd.pipeline import CountingPipeline, YuvFrameSink, YuvFrameSource
from vehicle_counting_amd.synth import bgr_to_yuv420, synth_frames

VC_ERR_ARG, VC_ERR_HIP, VC_ERR_STATE, VC_ERR_CAPACITY = 1, 2, 3, 4
PAIRS = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]


def one(b, g, r, matrix="bt601", full_range=False):
    """(Y, U, V) of a flat 2 x 2 block of one colour."""
    Y, U, V = enc.encode_planes(np.broadcast_to(np.array([b, g, r], np.uint8), (1, 2, 2, 3)), matrix, full_range)
    assert len(set(Y.reshape(-1).tolist())) == 1
    return int(Y[0, 0, 0]), int(U[0, 0, 0]), int(V[0, 0, 0])


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def test_table_is_the_rounded_literals_with_the_stated_row_sums():
    for matrix, full in PAIRS:
        table, lit = enc.coefficients(matrix, full), enc.literals(matrix, full)
        assert table == tuple(tuple(int(round(c * (1 << 20))) for c in row) for row in lit), (matrix, full)
        ky, ku, kv = table
        assert sum(ky) == ((1 << 20) if full else 900542), (matrix, full)
        assert sum(ku) == 0 and sum(kv) == 0, (matrix, full)
        assert ku[2] == kv[0] == (524288 if full else 460551)
        # the largest accumulator is 2^28 (full-range chroma of pure blue / red); nothing leaves 32 bits, no factor leaves 24
        assert max(abs(c) for row in table for c in row) < 1 << 23
        hi = max(sum(c * 255 for c in row if c > 0) for row in (ku, kv)) + (1 << 19) + (128 << 20)
        assert hi <= 1 << 28 and (not full or hi == 1 << 28)
        lo = min(sum(c * 255 for c in row if c < 0) for row in (ku, kv)) + (1 << 19) + (128 << 20)
        assert lo >= 0                                           # chroma never needs the lower clamp
    assert (524288 * 255 + (1 << 19) + (128 << 20)) == 1 << 28   # pure blue, U, full range


def test_known_answers():
    for matrix, full in PAIRS:
        assert one(0, 0, 0, matrix, full) == ((0 if full else 16), 128, 128)
        assert one(255, 255, 255, matrix, full) == ((255 if full else 235), 128, 128)
        for v in (1, 77, 128, 200, 254):                          # grey: chroma rows sum to 0, so U = V = 128 exactly
            y, u, w = one(v, v, v, matrix, full)
            assert (u, w) == (128, 128)
            assert y == (v if full else (900542 * v + (1 << 19) + (16 << 20)) >> 20)
    # the six saturated colours (B, G, R) -> (Y, U, V): BT.601 limited are the textbook colour-bar values
    assert one(0, 0, 255) == (81, 90, 240)            # red
    assert one(0, 255, 0) == (145, 54, 34)            # green
    assert one(255, 0, 0) == (41, 240, 110)           # blue
    assert one(0, 255, 255) == (210, 16, 146)         # yellow
    assert one(255, 255, 0) == (170, 166, 16)         # cyan
    assert one(255, 0, 255) == (106, 202, 222)        # magenta
    assert one(0, 0, 255, "bt709") == (63, 102, 240)
    assert one(0, 255, 0, "bt709") == (173, 42, 26)
    assert one(255, 0, 0, "bt709") == (32, 240, 118)
    # full range: pure blue (U) and pure red (V) reach 256 before the clamp
    for matrix in ("bt601", "bt709"):
        ky, ku, kv = enc.coefficients(matrix, True)
        assert (ku[2] * 255 + (1 << 19) + (128 << 20)) >> 20 == 256 and (kv[0] * 255 + (1 << 19) + (128 << 20)) >> 20 == 256
        assert one(255, 0, 0, matrix, True)[1] == 255
        assert one(0, 0, 255, matrix, True)[2] == 255


def test_known_answers_by_plain_integer_arithmetic():
    """The vectorised helper against the formulas spelled out with Python integers, a non-flat 2 x 2 block per case."""
    rng = np.random.default_rng(5)
    clamp = lambda x: min(max(x >> 20, 0), 255)
    for matrix, full in PAIRS:
        ky, ku, kv = enc.coefficients(matrix, full)
        yoff = 0 if full else 16
        blocks = rng.integers(0, 256, (100, 2, 2, 3)).tolist() + [[[[255, 0, 0]] * 2] * 2, [[[0, 0, 255]] * 2] * 2, [[[255, 255, 255], [0, 0, 0]], [[0, 0, 0], [0, 0, 1]]]]
        for blk in blocks:
            Y, U, V = enc.encode_planes(np.array(blk, np.uint8)[None], matrix, full)
            for i in range(2):
                for j in range(2):
                    B, G, R = blk[i][j]
                    acc = ky[0] * R + ky[1] * G + ky[2] * B + (1 << 19) + (yoff << 20)
                    assert 0 <= acc < 2 ** 31 and int(Y[0, i, j]) == clamp(acc)
            Bm, Gm, Rm = ((sum(blk[i][j][c] for i in range(2) for j in range(2)) + 2) >> 2 for c in range(3))
            assert int(U[0, 0, 0]) == clamp(ku[0] * Rm + ku[1] * Gm + ku[2] * Bm + (1 << 19) + (128 << 20))
            assert int(V[0, 0, 0]) == clamp(kv[0] * Rm + kv[1] * Gm + kv[2] * Bm + (1 << 19) + (128 << 20))


def test_limited_range_output_stays_in_range():
    """Limited range never leaves 16..235 / 16..240: each row is linear, so its extremes sit at the corners of the colour cube."""
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    rng = np.random.default_rng(1702)
    sample = np.concatenate([corners, rng.integers(0, 256, (1 << 16, 3), dtype=np.uint8)])
    flat = np.repeat(np.repeat(sample[None, None], 2, axis=1), 2, axis=2).reshape(1, 2, -1, 3)
    for matrix in ("bt601", "bt709"):
        Y, U, V = enc.encode_planes(flat, matrix, False)
        assert Y.min() == 16 and Y.max() == 235
        assert U.min() == 16 and U.max() == 240 and V.min() == 16 and V.max() == 240


# ---- relations to the other two definitions ----------------------------------------------------------------------------------------------
def test_within_one_code_of_the_float_test_encoder():
    clip = synth_frames(3, 48, 64, n_obj=4, seed=7)
    noise = np.random.default_rng(1702).integers(0, 256, (2, 32, 48, 3), dtype=np.uint8)
    for frames in (clip, noise):
        t, h, w, _ = frames.shape
        for matrix, full in PAIRS:
            for fmt in ("nv12", "i420"):
                got = enc.bgr_to_yuv(frames, fmt, matrix, full).reshape(t, -1).astype(int)
                want = bgr_to_yuv420(frames, fmt, matrix, full).astype(int)
                assert np.abs(got - want).max() <= 1, (matrix, full, fmt)


def _flat_sample():
    """2^20 seeded random colours plus the 52^3 lattice 0:256:5 u {255}, each as a flat 2 x 2 block (subsampling loses nothing)."""
    rng = np.random.default_rng(1702)
    rand = rng.integers(0, 256, (1 << 20, 3), dtype=np.uint8)
    axis = np.array(sorted(set(range(0, 256, 5)) | {255}), np.uint8)
    assert len(axis) == 52
    lattice = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([rand, lattice])


def _round_trip_error(colours, matrix, full):
    n = len(colours)
    frame = np.repeat(np.repeat(colours[None, None], 2, axis=1), 2, axis=2).reshape(1, 2, 2 * n, 3)
    back = yuv_ref.yuv_to_bgr(enc.bgr_to_yuv(frame, "i420", matrix, full), 1, 2, 2 * n, "i420", matrix, full)
    return int(np.abs(back.astype(int) - frame).max())


def test_round_trip_through_the_decoder_definition():
    sample = _flat_sample()
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for matrix in ("bt601", "bt709"):
        assert _round_trip_error(sample, matrix, False) <= 2, matrix
        assert _round_trip_error(sample, matrix, True) <= 1, matrix
        assert _round_trip_error(grey, matrix, False) <= 1, matrix
        assert _round_trip_error(grey, matrix, True) == 0, matrix


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_planes_land_where_the_geometry_says():
    rng = np.random.default_rng(3)
    b, h, w = 2, 4, 6
    frames = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    Y, U, V = enc.encode_planes(frames)
    tight = enc.bgr_to_yuv(frames, "nv12").reshape(b, -1)
    assert tight.shape == (b, h * w * 3 // 2)
    np.testing.assert_array_equal(tight[:, : h * w].reshape(b, h, w), Y)
    np.testing.assert_array_equal(tight[:, h * w:].reshape(b, h // 2, w // 2, 2)[..., 0], U)
    np.testing.assert_array_equal(tight[:, h * w:].reshape(b, h // 2, w // 2, 2)[..., 1], V)
    i420 = enc.bgr_to_yuv(frames, "i420").reshape(b, -1)
    np.testing.assert_array_equal(i420[:, h * w: h * w * 5 // 4].reshape(b, h // 2, w // 2), U)
    np.testing.assert_array_equal(i420[:, h * w * 5 // 4:].reshape(b, h // 2, w // 2), V)
    # padded: pitch 8, chroma two rows below the luma plane, 100-byte frames; every byte of no plane keeps the fill
    geo = dict(pitch_y=8, pitch_c=8, offset_c=8 * (h + 2), frame_stride=100)
    buf = enc.bgr_to_yuv(frames, "nv12", fill=0x5A, **geo)
    assert buf.size == yuv_ref.batch_bytes(b, h, w, "nv12", **geo)
    assert buf[100 + 3 * 8 + 5] == Y[1, 3, 5] and buf[100 + 48 + 8 + 4] == U[1, 1, 2] and buf[100 + 48 + 8 + 5] == V[1, 1, 2]
    assert (buf == 0x5A).sum() >= buf.size - b * h * w * 3 // 2 and buf[6] == 0x5A and buf[4 * 8] == 0x5A and buf[99] == 0x5A
    planes = yuv_ref.planes(buf, b, h, w, "nv12", **geo)                                              # and the decoder's reader finds them again
    for got, want in zip(planes, (Y, U, V)):
        np.testing.assert_array_equal(got, want)
    geo = dict(pitch_y=9, pitch_c=5, offset_c=9 * h + 3, offset_v=9 * h + 3 + 5 * 2 + 1, frame_stride=77)
    buf = enc.bgr_to_yuv(frames, "i420", fill=7, **geo)
    for got, want in zip(yuv_ref.planes(buf, b, h, w, "i420", **geo), (Y, U, V)):
        np.testing.assert_array_equal(got, want)
    keep = np.arange(buf.size, dtype=np.uint8)
    again = enc.bgr_to_yuv(frames, "i420", into=keep, **geo)
    untouched = buf == 7
    np.testing.assert_array_equal(again[untouched], keep[untouched])
    np.testing.assert_array_equal(again[~untouched], buf[~untouched])


# ---- the product's surface ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    lib = L.lib()
    for name in ("vc_bgr_to_yuv_host", "vc_bgr_to_yuv_dev", "vc_render_create", "vc_render_destroy", "vc_render_submit", "vc_render_collect"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} has no ctypes prototype"
    assert L.RENDER_SRC_ID == {"bgr_host": 0, "bgr_dev": 1, "yuv_host": 2, "yuv_dev": 3}
    assert callable(E.bgr_to_yuv) and callable(E.bgr_to_yuv_dev)
    for m in ("submit", "collect", "close", "__enter__", "__exit__"):
        assert callable(getattr(E.Renderer, m))
    assert callable(CountingPipeline.render)


def code_of(fn):
    with pytest.raises(L.VcError) as ei:
        fn()
    return ei.value.code


def test_argument_errors_are_refused_before_any_hip_call():
    img = lambda b, h, w: np.zeros((b, h, w, 3), np.uint8)
    assert code_of(lambda: E.bgr_to_yuv(img(1, 5, 8))) == VC_ERR_ARG                                    # odd height
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 7))) == VC_ERR_ARG                                    # odd width
    assert code_of(lambda: E.bgr_to_yuv(img(0, 8, 8))) == VC_ERR_ARG
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), desc=L.YuvDesc(2, 0, 0, 0, 0, 0, 0, 0))) == VC_ERR_ARG   # unknown format
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), desc=L.YuvDesc(0, 2, 0, 0, 0, 0, 0, 0))) == VC_ERR_ARG   # unknown matrix
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), desc=L.YuvDesc(0, 0, 7, 0, 0, 0, 0, 0))) == VC_ERR_ARG
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), pitch_y=6)) == VC_ERR_ARG                         # pitch below the row width
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), pitch_c=6)) == VC_ERR_ARG
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), "i420", pitch_c=3)) == VC_ERR_ARG
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), offset_c=40)) == VC_ERR_ARG                       # chroma inside the luma plane
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), "i420", offset_c=64, offset_v=70)) == VC_ERR_ARG  # U and V overlap
    assert code_of(lambda: E.bgr_to_yuv(img(1, 8, 8), "i420", offset_c=100, offset_v=32)) == VC_ERR_ARG # V inside the luma plane
    assert code_of(lambda: E.bgr_to_yuv(img(2, 8, 8), frame_stride=90)) == VC_ERR_ARG                   # frames overlap (a frame has 96 bytes)
    with pytest.raises(ValueError):
        E.bgr_to_yuv(np.zeros((8, 8, 3), np.uint8))
    lib, d, buf = L.lib(), E.yuv_desc(), np.zeros(1 << 12, np.uint8)
    assert lib.vc_bgr_to_yuv_host(None, L.ptr(buf, C.c_uint8), 1, 8, 8, L.ptr(buf, C.c_uint8)) == VC_ERR_ARG
    assert lib.vc_bgr_to_yuv_host(C.byref(d), None, 1, 8, 8, L.ptr(buf, C.c_uint8)) == VC_ERR_ARG
    assert lib.vc_bgr_to_yuv_host(C.byref(d), L.ptr(buf, C.c_uint8), 1, 8, 8, None) == VC_ERR_ARG
    assert lib.vc_bgr_to_yuv_dev(C.byref(d), None, 1, 8, 8, None) == VC_ERR_ARG
    assert lib.vc_bgr_to_yuv_dev(C.byref(E.yuv_desc(pitch_y=6)), buf.ctypes.data, 1, 8, 8, buf.ctypes.data) == VC_ERR_ARG     # checked before the launch
    # render: a context needs an engine, an engine needs a GPU -- what can be refused without either is refused first
    r = C.c_void_p()
    assert lib.vc_render_create(None, 4, 64, 64, 2, None) == VC_ERR_ARG
    assert lib.vc_render_create(None, 4, 64, 64, 2, C.byref(r)) == VC_ERR_ARG and not r.value           # no engine
    for depth in (0, 5, -1):
        assert lib.vc_render_create(None, 4, 64, 64, depth, C.byref(r)) == VC_ERR_ARG
    assert lib.vc_render_create(None, 0, 64, 64, 2, C.byref(r)) == VC_ERR_ARG
    assert lib.vc_render_create(None, 4, 1, 64, 2, C.byref(r)) == VC_ERR_ARG
    assert lib.vc_render_create(None, 1 << 20, 1 << 15, 1 << 15, 2, C.byref(r)) == VC_ERR_CAPACITY      # a work buffer beyond any device
    src = L.RenderSrc(0, buf.ctypes.data, d)
    assert lib.vc_render_submit(None, C.byref(src), 1, 8, 8, None, None, C.byref(d), buf.ctypes.data, 0) == VC_ERR_ARG
    assert lib.vc_render_collect(None) == VC_ERR_ARG
    assert lib.vc_render_destroy(None) == 0


def test_no_cpu_fallback_for_the_conversion():
    import torch
    if torch.cuda.is_available():
        return                                             # with a GPU the call succeeds: tests/test_gpu_yuv_egress.py
    assert code_of(lambda: E.bgr_to_yuv(np.zeros((1, 8, 8, 3), np.uint8))) == VC_ERR_HIP


def test_yuv_frame_sink_geometry():
    h, w, t = 6, 8, 3
    s = YuvFrameSink(h, w, n_frames=t)
    assert len(s) == t and s.fmt == "nv12" and not s.is_device
    assert (s.desc.format, s.desc.matrix, s.desc.full_range, s.desc.frame_stride) == (0, 0, 0, h * w * 3 // 2)
    assert s.data.shape == (t, h * w * 3 // 2) and s.data.dtype == np.uint8 and not s.data.any()
    assert s.frame(2).shape == (h * w * 3 // 2,) and s.address(2) - s.address(0) == 2 * s.frame_stride == s.frame(2).ctypes.data - s.data.ctypes.data
    assert s.nbytes == s.data.size
    p = YuvFrameSink(h, w, "i420", "bt709", True, pitch=16, n_frames=t)                                 # chroma pitch follows the luma pitch
    assert (p.desc.format, p.desc.matrix, p.desc.full_range, p.desc.pitch_y, p.desc.pitch_c, p.frame_stride) == (1, 1, 1, 16, 8, 16 * 6 + 8 * 6)
    p = YuvFrameSink(h, w, pitch=16, offset_c=16 * 8, frame_stride=400, n_frames=2)
    assert (p.desc.offset_c, p.desc.frame_stride, p.data.shape) == (128, 400, (2, 400))
    # the same geometry words as the source: a sink's bytes read back as a source
    back = YuvFrameSource(p.data, h, w, pitch=16, offset_c=16 * 8, frame_stride=400)
    assert (back.desc.pitch_y, back.desc.pitch_c, back.desc.offset_c, back.desc.frame_stride) == (p.desc.pitch_y, p.desc.pitch_c, p.desc.offset_c, p.desc.frame_stride)
    d = YuvFrameSink(h, w, n_frames=t, device_ptr=0x1000)
    assert d.is_device and d.data is None and d.address(1) == 0x1000 + h * w * 3 // 2
    with pytest.raises(ValueError):
        d.frame(0)
    with pytest.raises(IndexError):
        s.address(t)
    for bad in (lambda: YuvFrameSink(5, w), lambda: YuvFrameSink(h, 7), lambda: YuvFrameSink(h, w, pitch=4), lambda: YuvFrameSink(h, w, "p010"),
                lambda: YuvFrameSink(h, w, matrix="bt2020"), lambda: YuvFrameSink(h, w, frame_stride=60), lambda: YuvFrameSink(h, w, n_frames=0)):
        with pytest.raises(ValueError):
            bad()
