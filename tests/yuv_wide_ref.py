"""NumPy statement of the wider YUV ingest formats (include/vcount_hip.h: VC_PIX_P016 / I010 / I422 / I444),
written from the definition and independent of the product code.  Helper for tests/test_yuv_wide_ref.py and
tests/test_gpu_yuv_wide.py, not a test.  An extension of tests/yuv_ref.py, not a second arithmetic:

    1. every sample of every plane is reduced to 8 bits
         p016 (little-endian 16-bit words, significant bits at the top; P010 / P012 surfaces too):  s8 = min(255, (s16 + 128) >> 8)
         i010 (little-endian 16-bit words, 10 significant bits at the bottom; yuv420p10le):         s8 = min(255, ((s16 & 1023) + 2) >> 2)
         8-bit formats:                                                                             s8 = s
    2. the chroma sample of pixel (x, y) is (x >> 1, y >> 1) for nv12 / i420 / p016 / i010, (x >> 1, y) for i422, (x, y) for i444:
       replicated, never interpolated
    3. yuv_ref.convert, verbatim.

Parity with cv2 / swscale is unpinned, as it is for the 8-bit 4:2:0 formats.
"""
import numpy as np

import yuv_ref

IDS = {"nv12": 0, "i420": 1, "p016": 16, "i010": 17, "i422": 18, "i444": 19}
WIDE = ("p016", "i010", "i422", "i444")
#        sample bytes, U and V interleaved in one plane, chroma at half height, chroma at half width
TRAITS = {"nv12": (1, True, True, True), "i420": (1, False, True, True), "p016": (2, True, True, True), "i010": (2, False, True, True),
          "i422": (1, False, False, True), "i444": (1, False, False, False)}


def size_ok(fmt, h, w):
    _, _, vsub, hsub = TRAITS[fmt]
    return h >= 1 and w >= 1 and not (vsub and h % 2) and not (hsub and w % 2)


def reduce8(s16, fmt):
    """step 1 for an array of 16-bit words"""
    s = np.asarray(s16).astype(np.int64)
    if fmt == "p016":
        return np.minimum(255, (s + 128) >> 8).astype(np.uint8)
    if fmt == "i010":
        return np.minimum(255, ((s & 1023) + 2) >> 2).astype(np.uint8)
    raise ValueError(fmt)


def rows(fmt, h, w):
    """(luma row bytes, chroma row bytes, chroma rows)"""
    ss, semi, vsub, hsub = TRAITS[fmt]
    return w * ss, (w if semi or not hsub else w // 2) * ss, (h // 2 if vsub else h)


def layout(h, w, fmt, pitch_y=0, pitch_c=0, offset_c=0, offset_v=0, frame_stride=0):
    """The byte geometry with zeros resolved (0 = tightly packed): pitch_y, pitch_c, offset_c, offset_v, frame_stride, frame_end."""
    rowb, crow, hc = rows(fmt, h, w)
    pitch_y = pitch_y or rowb
    pitch_c = pitch_c or crow
    offset_c = offset_c or pitch_y * h
    end = offset_c + pitch_c * (hc - 1) + crow
    if TRAITS[fmt][1]:
        offset_v = 0
    else:
        offset_v = offset_v or offset_c + pitch_c * hc
        end = max(end, offset_v + pitch_c * (hc - 1) + crow)
    return pitch_y, pitch_c, offset_c, offset_v, frame_stride or end, end


def batch_bytes(b, h, w, fmt, **geometry):
    *_, stride, end = layout(h, w, fmt, **geometry)
    return (b - 1) * stride + end


def geometry(kind, fmt, h, w):
    """The three layouts of tests/test_gpu_yuv_ingest.py::geometry for any format.  tight; padded: 16-byte aligned pitches, offsets and
    frame stride, chroma beyond pitch * h, a gap between planes and frames (a decoder surface); padded_odd: the same with nothing
    aligned, odd pitches and offsets (generic path at every width)."""
    if kind == "tight":
        return {}
    align = lambda v, a: (v + a - 1) // a * a
    rowb, crow, hc = rows(fmt, h, w)
    if kind == "padded":
        py = align(rowb, 256) + 256
        pc = py if crow == rowb else py // 2
        geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * align(h + 5, 16))
        vgap, gap = 32, 4096
    else:
        py, pc = rowb + 7, crow + 3
        py, pc = py + 1 - py % 2, pc + 1 - pc % 2                                    # both odd
        geo = dict(pitch_y=py, pitch_c=pc, offset_c=py * h + 13)
        vgap, gap = 5, 101
    if not TRAITS[fmt][1]:
        geo["offset_v"] = geo["offset_c"] + pc * hc + vgap
    end = batch_bytes(1, h, w, fmt, **geo)
    geo["frame_stride"] = (align(end, 16) if kind == "padded" else end) + gap
    return geo


def _samples(d, base, ss):
    """the samples at byte addresses `base` (an index array) of the flat uint8 buffer d: bytes, or little-endian 16-bit words from two bytes"""
    if ss == 1:
        return d[base].astype(np.int64)
    return d[base].astype(np.int64) | (d[base + 1].astype(np.int64) << 8)


def planes(data, b, h, w, fmt, **geometry):
    """Y [b, h, w], U and V [b, chroma rows, chroma columns] read out of the flat byte buffer `data`, samples as stored (8 or 16 bits)."""
    assert size_ok(fmt, h, w)
    ss, semi, vsub, hsub = TRAITS[fmt]
    pitch_y, pitch_c, offset_c, offset_v, stride, end = layout(h, w, fmt, **geometry)
    d = np.asarray(data, np.uint8).reshape(-1)
    assert d.size >= (b - 1) * stride + end
    hc, wc = (h // 2 if vsub else h), (w // 2 if hsub else w)
    f0 = (np.arange(b, dtype=np.int64) * stride)[:, None, None]
    r, rc = np.arange(h, dtype=np.int64)[:, None], np.arange(hc, dtype=np.int64)[:, None]
    Y = _samples(d, f0 + r * pitch_y + ss * np.arange(w)[None, :], ss)
    if semi:
        U = _samples(d, f0 + offset_c + rc * pitch_c + 2 * ss * np.arange(wc)[None, :], ss)
        V = _samples(d, f0 + offset_c + rc * pitch_c + 2 * ss * np.arange(wc)[None, :] + ss, ss)
    else:
        U = _samples(d, f0 + offset_c + rc * pitch_c + ss * np.arange(wc)[None, :], ss)
        V = _samples(d, f0 + offset_v + rc * pitch_c + ss * np.arange(wc)[None, :], ss)
    return Y, U, V


def yuv_to_bgr(data, b, h, w, fmt, matrix="bt601", full_range=False, **geometry):
    """b frames of `fmt` in `data` (flat uint8) -> (b, h, w, 3) uint8 BGR: reduce, index the chroma, then yuv_ref.convert."""
    Y, U, V = planes(data, b, h, w, fmt, **geometry)
    ss, _, vsub, hsub = TRAITS[fmt]
    if ss == 2:
        Y, U, V = reduce8(Y, fmt), reduce8(U, fmt), reduce8(V, fmt)
    ys, xs = np.arange(h) >> (1 if vsub else 0), np.arange(w) >> (1 if hsub else 0)
    return yuv_ref.convert(Y, U[:, ys][:, :, xs], V[:, ys][:, :, xs], matrix, full_range)


def build(fmt, Y, U, V):
    """Tightly packed frames of `fmt` (flat uint8 per frame: [b, frame bytes]) derived from 8-bit 4:2:0 planes Y [b, h, w], U / V
    [b, h/2, w/2]: << 8 for p016, << 2 for i010, chroma rows replicated for i422, chroma replicated 2 x 2 for i444."""
    Y, U, V = (np.asarray(a, np.uint8) for a in (Y, U, V))
    b = len(Y)
    flat = lambda a: a.reshape(b, -1)
    words = lambda a, sh: (a.astype("<u2") << sh).view(np.uint8).reshape(b, -1)      # little-endian bytes
    uv = np.stack([U, V], axis=-1)                                                   # interleaved
    if fmt == "nv12":
        parts = [flat(Y), flat(uv)]
    elif fmt == "i420":
        parts = [flat(Y), flat(U), flat(V)]
    elif fmt == "p016":
        parts = [words(Y, 8), words(uv, 8)]
    elif fmt == "i010":
        parts = [words(Y, 2), words(U, 2), words(V, 2)]
    elif fmt == "i422":
        parts = [flat(Y), flat(np.repeat(U, 2, axis=1)), flat(np.repeat(V, 2, axis=1))]
    elif fmt == "i444":
        up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
        parts = [flat(Y), flat(up(U)), flat(up(V))]
    else:
        raise ValueError(fmt)
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def from_nv12(fmt, nv12, h, w):
    """`build` from tightly packed NV12 frames [t, h * w * 3 / 2] (what synth.bgr_to_yuv420 returns)."""
    t = len(nv12)
    Y = nv12[:, :h * w].reshape(t, h, w)
    uv = nv12[:, h * w:].reshape(t, h // 2, w // 2, 2)
    return build(fmt, Y, uv[..., 0], uv[..., 1])
