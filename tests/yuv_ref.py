"""NumPy statement of the 4:2:0 YUV -> BGR definition, written from the literals and independent of the
product code.  Helper for tests/test_yuv_ref.py and tests/test_gpu_yuv_ingest.py, not a test.

    u = U - 128, v = V - 128, 32-bit signed arithmetic, >> arithmetic, chroma replicated over its 2 x 2 luma block
    R = clamp((y + (1 << 19) + CVR * v) >> 20, 0, 255)
    G = clamp((y + (1 << 19) + CVG * v + CUG * u) >> 20, 0, 255)
    B = clamp((y + (1 << 19) + CUB * u) >> 20, 0, 255)
    limited range: y = max(0, Y - 16) * CY        full range: y = Y << 20
"""
import numpy as np

SHIFT = 20
#            (matrix, full_range): CY,    CVR,    CVG,       CUG,       CUB
LITERALS = {("bt601", False): (1.164, 1.596, -0.813, -0.391, 2.018),
            ("bt709", False): (1.164, 1.793, -0.533, -0.213, 2.112),
            ("bt601", True): (None, 1.402, -0.714136, -0.344136, 1.772),
            ("bt709", True): (None, 1.5748, -0.468124, -0.187324, 1.8556)}


def coefficients(matrix="bt601", full_range=False):
    """(CY, CVR, CVG, CUG, CUB) as int(literal * 2^20), truncated toward zero; CY is None for full range."""
    return tuple(None if c is None else int(c * (1 << SHIFT)) for c in LITERALS[(matrix, bool(full_range))])


def convert(Y, U, V, matrix="bt601", full_range=False):
    """Y, U, V: integer arrays of one shape (chroma already replicated) -> uint8 array [..., 3] in B, G, R order."""
    cy, cvr, cvg, cug, cub = coefficients(matrix, full_range)
    Y, u, v = np.asarray(Y, np.int32), np.asarray(U, np.int32) - 128, np.asarray(V, np.int32) - 128
    y = (Y << SHIFT) if full_range else np.maximum(Y - 16, 0) * np.int32(cy)
    half = np.int32(1 << (SHIFT - 1))
    r = (y + half + np.int32(cvr) * v) >> SHIFT
    g = (y + half + np.int32(cvg) * v + np.int32(cug) * u) >> SHIFT
    b = (y + half + np.int32(cub) * u) >> SHIFT
    assert y.dtype == np.int32 and r.dtype == np.int32
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def layout(h, w, fmt="nv12", pitch_y=0, pitch_c=0, offset_c=0, offset_v=0, frame_stride=0):
    """The byte geometry with zeros resolved (0 = tightly packed): pitch_y, pitch_c, offset_c, offset_v, frame_stride, frame_end."""
    crow = w if fmt == "nv12" else w // 2
    pitch_y = pitch_y or w
    pitch_c = pitch_c or crow
    offset_c = offset_c or pitch_y * h
    end = offset_c + pitch_c * (h // 2 - 1) + crow
    if fmt == "i420":
        offset_v = offset_v or offset_c + pitch_c * (h // 2)
        end = max(end, offset_v + pitch_c * (h // 2 - 1) + crow)
    else:
        offset_v = 0
    return pitch_y, pitch_c, offset_c, offset_v, frame_stride or end, end


def batch_bytes(b, h, w, fmt="nv12", **geometry):
    *_, stride, end = layout(h, w, fmt, **geometry)
    return (b - 1) * stride + end


def planes(data, b, h, w, fmt="nv12", **geometry):
    """Y [b, h, w], U and V [b, h/2, w/2] read out of the flat byte buffer `data`."""
    assert h % 2 == 0 and w % 2 == 0
    pitch_y, pitch_c, offset_c, offset_v, stride, end = layout(h, w, fmt, **geometry)
    d = np.asarray(data, np.uint8).reshape(-1)
    assert d.size >= (b - 1) * stride + end
    rows, rows_c = np.arange(h)[:, None], np.arange(h // 2)[:, None]
    f0 = (np.arange(b) * stride)[:, None, None]
    Y = d[f0 + rows * pitch_y + np.arange(w)[None, :]]
    if fmt == "nv12":
        U = d[f0 + offset_c + rows_c * pitch_c + 2 * np.arange(w // 2)[None, :]]
        V = d[f0 + offset_c + rows_c * pitch_c + 2 * np.arange(w // 2)[None, :] + 1]
    else:
        U = d[f0 + offset_c + rows_c * pitch_c + np.arange(w // 2)[None, :]]
        V = d[f0 + offset_v + rows_c * pitch_c + np.arange(w // 2)[None, :]]
    return Y, U, V


def yuv_to_bgr(data, b, h, w, fmt="nv12", matrix="bt601", full_range=False, **geometry):
    """b frames of 4:2:0 YUV in `data` (flat uint8) -> (b, h, w, 3) uint8 BGR."""
    Y, U, V = planes(data, b, h, w, fmt, **geometry)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    return convert(Y, up(U), up(V), matrix, full_range)
