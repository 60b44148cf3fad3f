"""NumPy statement of the BGR -> 4:2:0 YUV definition, written from the integer table and independent of the
product code.  Helper for tests/test_yuv_enc_ref.py and tests/test_gpu_yuv_egress.py, not a test.

    integer, 32-bit signed, >> arithmetic, per frame of even h, w
    Y[y][x]     = clamp((KYR*R + KYG*G + KYB*B + (1 << 19) + (YOFF << 20)) >> 20, 0, 255)        from the pixel's own B, G, R
    Rm, Gm, Bm  = (sum of the channel over the 2 x 2 luma block + 2) >> 2                         rounded block mean, per channel
    U[y/2][x/2] = clamp((KUR*Rm + KUG*Gm + KUB*Bm + (1 << 19) + (128 << 20)) >> 20, 0, 255)
    V[y/2][x/2] = clamp((KVR*Rm + KVG*Gm + KVB*Bm + (1 << 19) + (128 << 20)) >> 20, 0, 255)
    YOFF = 16 (limited range) or 0 (full range)
"""
import numpy as np

import yuv_ref

SHIFT = 20
# (matrix, full_range): (KYR, KYG, KYB), (KUR, KUG, KUB), (KVR, KVG, KVB)
TABLE = {("bt601", False): ((269262, 528618, 102662), (-155423, -305128, 460551), (460551, -385654, -74897)),
         ("bt601", True): ((313524, 615514, 119538), (-176933, -347355, 524288), (524288, -439026, -85262)),
         ("bt709", False): ((191455, 644068, 65019), (-105533, -355018, 460551), (460551, -418321, -42230)),
         ("bt709", True): ((222927, 749942, 75707), (-120137, -404151, 524288), (524288, -476214, -48074))}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def literals(matrix, full_range):
    """The real-valued rows the table is rounded from: Kr, Kb of the matrix, scaled by 219 / 255 (luma) and 224 / 255 (chroma) for
    limited range, rounded to 6 decimals."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    y = (kr, kg, kb)
    u = (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5)
    v = (0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)))
    return tuple(tuple(round(c * s, 6) for c in row) for row, s in ((y, sy), (u, sc), (v, sc)))


def coefficients(matrix="bt601", full_range=False):
    return TABLE[(matrix, bool(full_range))]


def _q(acc):
    assert acc.dtype == np.int32
    return np.clip(acc >> SHIFT, 0, 255).astype(np.uint8)


def encode_planes(bgr, matrix="bt601", full_range=False):
    """(b, h, w, 3) uint8 BGR -> Y [b, h, w], U and V [b, h/2, w/2], uint8."""
    f = np.asarray(bgr, np.uint8).astype(np.int32)
    b, h, w, _ = f.shape
    assert h % 2 == 0 and w % 2 == 0
    ky, ku, kv = (tuple(np.int32(c) for c in row) for row in coefficients(matrix, full_range))
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    half, yoff, mid = np.int32(1 << (SHIFT - 1)), np.int32((0 if full_range else 16) << SHIFT), np.int32(128 << SHIFT)
    Y = _q(ky[0] * R + ky[1] * G + ky[2] * B + half + yoff)
    mean = lambda p: (p.reshape(b, h // 2, 2, w // 2, 2).sum(axis=(2, 4), dtype=np.int32) + np.int32(2)) >> 2
    Bm, Gm, Rm = mean(B), mean(G), mean(R)
    U = _q(ku[0] * Rm + ku[1] * Gm + ku[2] * Bm + half + mid)
    V = _q(kv[0] * Rm + kv[1] * Gm + kv[2] * Bm + half + mid)
    return Y, U, V


def scatter(Y, U, V, fmt="nv12", fill=0, into=None, **geometry):
    """Planes -> flat uint8 buffer of b frames laid out by `yuv_ref.layout`; bytes of no plane keep `fill` (or what `into` held)."""
    b, h, w = Y.shape
    pitch_y, pitch_c, offset_c, offset_v, stride, end = yuv_ref.layout(h, w, fmt, **geometry)
    n = (b - 1) * stride + end
    out = np.full(n, fill, np.uint8) if into is None else np.array(into, np.uint8).reshape(-1).copy()
    assert out.size >= n
    rows, rows_c = np.arange(h)[:, None], np.arange(h // 2)[:, None]
    f0 = (np.arange(b) * stride)[:, None, None]
    out[f0 + rows * pitch_y + np.arange(w)[None, :]] = Y
    cx = np.arange(w // 2)[None, :]
    if fmt == "nv12":
        out[f0 + offset_c + rows_c * pitch_c + 2 * cx] = U
        out[f0 + offset_c + rows_c * pitch_c + 2 * cx + 1] = V
    else:
        out[f0 + offset_c + rows_c * pitch_c + cx] = U
        out[f0 + offset_v + rows_c * pitch_c + cx] = V
    return out


def bgr_to_yuv(bgr, fmt="nv12", matrix="bt601", full_range=False, fill=0, into=None, **geometry):
    """(b, h, w, 3) uint8 BGR -> flat uint8 bytes of b frames of 4:2:0 YUV."""
    return scatter(*encode_planes(bgr, matrix, full_range), fmt=fmt, fill=fill, into=into, **geometry)
