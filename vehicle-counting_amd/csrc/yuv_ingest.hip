// YUV ingest: 4:2:0 frames as a video decoder hands them out (NV12 surfaces in device memory, I420 planes in host memory) converted
// on the device into the packed BGR u8 [b][h][w][3] the engine's ingest slots hold (stream.hip: d_ingest[]).  The reference receives
// BGR because cv2.VideoCapture converts on the CPU behind its back (/root/reference/modules/datasets.py:47-61).
//
// The arithmetic is the definition (integer, so every implementation agrees bit for bit; restated in NumPy by tests/yuv_ref.py):
//   u = U - 128, v = V - 128, chroma replicated over its 2 x 2 luma block (no interpolation), 32-bit signed arithmetic,
//   R = clamp((y + (1 << 19) + CVR * v) >> 20, 0, 255)
//   G = clamp((y + (1 << 19) + CVG * v + CUG * u) >> 20, 0, 255)
//   B = clamp((y + (1 << 19) + CUB * u) >> 20, 0, 255)
//   limited range: y = max(0, Y - 16) * CY;  full range: y = Y << 20;  constants = int(literal * 2^20), truncated toward zero.
// BT.601 limited is OpenCV's COLOR_YUV2BGR_NV12 arithmetic as published; OpenCV is not in this image, so parity with it (and with the
// swscale path inside cv2.VideoCapture) is UNPINNED, like the other cv2 steps.
//
// A pure streaming kernel, 1.5 B read and 3 B written per pixel, no LDS, plain vector stores.  One lane owns 16 pixels x 2 rows so
// that both rows share one chroma fetch: 16 B of Y per row, 16 B of UV (8 B + 8 B for I420), three 16-byte stores per row.  The
// generic variant (any even w, any pitch) owns the same 16 x 2 block, assembles the same words from byte loads and stores bytes.
// Every factor fits 24 bits and every sum 31 bits (|chroma term| <= 2.3e6 * 128, y <= 255 << 20), hence the full-rate 24-bit multiplies.
//
// Wider decoder output (include/vcount_hip.h: P016 = P010 / P012 / P016 surfaces, I010 = yuv420p10le, I422, I444) extends the definition,
// it is not a second one: every sample is first reduced to 8 bits -- P016 s8 = min(255, (s16 + 128) >> 8), I010 s8 = min(255, ((s16 &
// 1023) + 2) >> 2) -- and the chroma sample of pixel (x, y) is (x >> 1, y >> 1), (x >> 1, y) for I422 or (x, y) for I444, replicated, never
// interpolated; then the arithmetic above, verbatim (tests/yuv_wide_ref.py).  Parity with cv2 / swscale is UNPINNED here too.  The same
// body: the format is a template parameter of frame_block that decides the fetch (32 B of luma per row for the 16-bit formats; chroma
// 32 B per row pair for P016, 16 + 16 B for I010, 8 + 8 B per row for I422, 16 + 16 B per row for I444) and the chroma index; 2 to 3 B
// read per pixel.  The generic variant takes any width (odd for I444), any pitch, and an odd h where the format allows one.
#include <algorithm>

#include "engine.h"

namespace vc {

namespace {

// int(literal * 2^20), truncated toward zero: {CY, CVR, CVG, CUG, CUB} per [matrix][full_range]
constexpr int yuv_fix(double v) { return (int)(v * 1048576.0); }
const int kYuvCoef[2][2][5] = {
    {{yuv_fix(1.164), yuv_fix(1.596), yuv_fix(-0.813), yuv_fix(-0.391), yuv_fix(2.018)},            // BT.601 limited: 1220542 1673527 -852492 -409993 2116026
     {1 << 20, yuv_fix(1.402), yuv_fix(-0.714136), yuv_fix(-0.344136), yuv_fix(1.772)}},             // BT.601 full
    {{yuv_fix(1.164), yuv_fix(1.793), yuv_fix(-0.533), yuv_fix(-0.213), yuv_fix(2.112)},            // BT.709 limited
     {1 << 20, yuv_fix(1.5748), yuv_fix(-0.468124), yuv_fix(-0.187324), yuv_fix(1.8556)}}};          // BT.709 full

struct YuvChroma { int r, g, b; };   // chroma terms of one 2 x 2 block, rounding constant included

__device__ __forceinline__ YuvChroma yuv_chroma(int U, int V, const YuvGeom& k) {
    const int u = U - 128, v = V - 128;
    YuvChroma c;
    c.r = __mul24(k.cvr, v) + (1 << 19);
    c.g = __mul24(k.cvg, v) + __mul24(k.cug, u) + (1 << 19);
    c.b = __mul24(k.cub, u) + (1 << 19);
    return c;
}

__device__ __forceinline__ uint32_t yuv_pixel(int Y, const YuvChroma& c, const YuvGeom& k) {    // B | G << 8 | R << 16
    // clamp((x) >> 20, 0, 255) written as clamp(x, 0, (256 << 20) - 1) >> 20: the same value for every x, and the shift is a logical one of
    // a non-negative number.  The arithmetic-shift-then-clamp form is matched by the compiler to gfx950's packed shift-and-saturate
    // instruction (two results in one 16-bit half), and the words assembled from it came out with stray high bits on the hardware.
    const int y = __mul24(max(Y - k.yoff, 0), k.cy), top = (256 << 20) - 1;
    const uint32_t r = (uint32_t)min(max(y + c.r, 0), top) >> 20, g = (uint32_t)min(max(y + c.g, 0), top) >> 20, b = (uint32_t)min(max(y + c.b, 0), top) >> 20;
    return b | (g << 8) | (r << 16);
}

// What a format decides (F: PF_*, engine.h): the sample width, whether U and V share one plane, and which chroma sample a pixel uses.
template <int F> struct PixTraits {
    static constexpr bool wide = F == PF_P016 || F == PF_I010;      // little-endian 16-bit samples, reduced to 8 bits as they are fetched
    static constexpr bool semi = F == PF_NV12 || F == PF_P016;      // one plane of interleaved U,V
    static constexpr bool vsub = F != PF_I422 && F != PF_I444;      // chroma of pixel row y is row y >> 1 (else row y)
    static constexpr bool hsub = F != PF_I444;                      // chroma of pixel column x is column x >> 1 (else column x)
    static constexpr int ss = wide ? 2 : 1;                         // bytes of one sample
};

// A 16-bit sample reduced to 8 bits: P016 min(255, (s + 128) >> 8), I010 min(255, ((s & 1023) + 2) >> 2).  32-bit unsigned, the clamp before
// the shift like yuv_pixel's (the same value for every s: the sums stay below 2^17, and the clamp bound shifts to 255).
template <int F>
__device__ __forceinline__ uint32_t yuv_reduce(uint32_t s) {
    return F == PF_P016 ? min(s + 128u, 0xffffu) >> 8 : min((s & 1023u) + 2u, 1023u) >> 2;
}

template <int F>
__device__ __forceinline__ uint32_t yuv_reduce4(uint32_t lo, uint32_t hi) {     // four 16-bit samples in two words -> four bytes in one
    return yuv_reduce<F>(lo & 0xffffu) | (yuv_reduce<F>(lo >> 16) << 8) | (yuv_reduce<F>(hi & 0xffffu) << 16) | (yuv_reduce<F>(hi >> 16) << 24);
}

// 4 * NW consecutive samples of one plane row, the first n of them valid, as NW words of 8-bit samples.  FAST: one vector load of
// 4 * NW * ss bytes (two 16-byte loads for 32), p aligned to min(16, that); else byte loads of the valid samples only.
template <int F, bool FAST, int NW>
__device__ __forceinline__ void yuv_fetch(const uint8_t* __restrict__ p, int n, uint32_t out[NW]) {
    constexpr bool wide = PixTraits<F>::wide;
    static_assert(NW == 2 || NW == 4, "8 or 16 samples");
    if (FAST) {
        if (NW * (wide ? 2 : 1) == 2) {
            const uint2 a = *(const uint2*)p;
            out[0] = a.x; out[1] = a.y;
        } else {
            const uint4 a = *(const uint4*)p;
            if (!wide) {
                out[0] = a.x; out[1] = a.y; out[NW - 2] = a.z; out[NW - 1] = a.w;
            } else {
                out[0] = yuv_reduce4<F>(a.x, a.y); out[1] = yuv_reduce4<F>(a.z, a.w);
                if (NW == 4) {
                    const uint4 b = ((const uint4*)p)[1];
                    out[NW - 2] = yuv_reduce4<F>(b.x, b.y); out[NW - 1] = yuv_reduce4<F>(b.z, b.w);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * j + i < n) {
                    const uint8_t* q = p + (4 * j + i) * (wide ? 2 : 1);
                    v |= (wide ? yuv_reduce<F>((uint32_t)q[0] | ((uint32_t)q[1] << 8)) : (uint32_t)q[0]) << (8 * i);
                }
            out[j] = v;
        }
    }
}

// 16 pixels of one row: yw = 16 Y bytes -> 48 bytes of BGR as 12 words.  HSUB: ch = the chroma terms of the row, one per pixel pair.
// Else one per pixel: each group of four is formed from its U / V bytes (cu, cv) just before its pixels, so that 4 and not 16 triples
// are live at a time (with 16 the frame-table kernels need 77 VGPRs and drop from 8 to 6 waves per SIMD).
template <bool HSUB>
__device__ __forceinline__ void yuv_row16(const uint32_t yw[4], const YuvChroma* ch, const uint32_t cu[4], const uint32_t cv[4], const YuvGeom& k, uint32_t out[12]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        YuvChroma c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = HSUB ? ch[2 * j + (i >> 1)] : yuv_chroma((cu[j] >> (8 * i)) & 255, (cv[j] >> (8 * i)) & 255, k);
        const uint32_t p0 = yuv_pixel(yw[j] & 255, c[0], k), p1 = yuv_pixel((yw[j] >> 8) & 255, c[1], k);
        const uint32_t p2 = yuv_pixel((yw[j] >> 16) & 255, c[2], k), p3 = yuv_pixel(yw[j] >> 24, c[3], k);
        out[3 * j] = p0 | (p1 << 24);
        out[3 * j + 1] = (p1 >> 8) | (p2 << 16);
        out[3 * j + 2] = (p2 >> 16) | (p3 << 8);
    }
}

// the chroma samples of the 16 pixels from x0 in chroma row crow, 8 bits each: semi-planar cu = U0 V0 U1 V1 ... (4 words, cv unused);
// planar cu / cv = the U / V samples (2 words each when the chroma is at half width, 4 at full width)
template <int F, bool FAST>
__device__ __forceinline__ void chroma_fetch(const uint8_t* __restrict__ sf, const YuvGeom& k, int crow, int x0, int npx, uint32_t cu[4], uint32_t cv[4]) {
    using T = PixTraits<F>;
    const uint8_t* up = sf + k.off_c + (size_t)crow * k.pitch_c;
    const uint8_t* vp = sf + k.off_v + (size_t)crow * k.pitch_c;
    if (T::semi) {
        yuv_fetch<F, FAST, 4>(up + x0 * T::ss, npx, cu);
    } else if (T::hsub) {
        yuv_fetch<F, FAST, 2>(up + (x0 >> 1) * T::ss, npx >> 1, cu);
        yuv_fetch<F, FAST, 2>(vp + (x0 >> 1) * T::ss, npx >> 1, cv);
    } else {
        yuv_fetch<F, FAST, 4>(up + x0 * T::ss, npx, cu);
        yuv_fetch<F, FAST, 4>(vp + x0 * T::ss, npx, cv);
    }
}

// the chroma terms of the 8 pixel pairs of a row whose chroma is at half width
template <int F>
__device__ __forceinline__ void chroma_terms(const uint32_t cu[4], const uint32_t cv[4], const YuvGeom& k, YuvChroma ch[8]) {
    if (PixTraits<F>::semi) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ch[2 * j] = yuv_chroma(cu[j] & 255, (cu[j] >> 8) & 255, k);
            ch[2 * j + 1] = yuv_chroma((cu[j] >> 16) & 255, cu[j] >> 24, k);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) ch[i] = yuv_chroma((cu[i >> 2] >> (8 * (i & 3))) & 255, (cv[i >> 2] >> (8 * (i & 3))) & 255, k);
    }
}

// the 16 x 2 block (row pair rp, column group cg) of the frame that starts at sf, converted into the h x w x 3 frame at df.  The format
// decides how the lane fetches its samples and which chroma row and column a pixel uses; everything after the fetch is shared.  A second
// row that does not exist (odd h: I422 / I444 only) is neither loaded nor stored.
template <int F, bool FAST>
__device__ __forceinline__ void frame_block(const uint8_t* __restrict__ sf, uint8_t* __restrict__ df, const YuvGeom& k, int rp, int cg) {
    using T = PixTraits<F>;
    const int x0 = cg * 16;
    const int npx = min(16, k.w - x0);                      // 16 on the fast path
    const int rows = T::vsub ? 2 : min(2, k.h - 2 * rp);
    const uint8_t* y0p = sf + (size_t)(2 * rp) * k.pitch_y + x0 * T::ss;

    uint32_t yw[2][4], cu[2][4], cv[2][4];
    yuv_fetch<F, FAST, 4>(y0p, npx, yw[0]);
    if (rows == 2) yuv_fetch<F, FAST, 4>(y0p + k.pitch_y, npx, yw[1]);
    if (T::vsub) {
        chroma_fetch<F, FAST>(sf, k, rp, x0, npx, cu[0], cv[0]);
    } else {
        chroma_fetch<F, FAST>(sf, k, 2 * rp, x0, npx, cu[0], cv[0]);
        if (rows == 2) chroma_fetch<F, FAST>(sf, k, 2 * rp + 1, x0, npx, cu[1], cv[1]);
    }

    YuvChroma ch[8];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r < rows) {
            const int cr = T::vsub ? 0 : r;
            if (T::hsub && (r == 0 || !T::vsub)) chroma_terms<F>(cu[cr], cv[cr], k, ch);
            uint32_t o[12];
            yuv_row16<T::hsub>(yw[r], ch, cu[cr], cv[cr], k, o);
            uint8_t* d = df + ((size_t)(2 * rp + r) * k.w + x0) * 3;
            if (FAST) {
                uint4* d4 = (uint4*)d;
                d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
                d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
                d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
            } else {
#pragma unroll
                for (int i = 0; i < 48; ++i)
                    if (i < npx * 3) d[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
}

// grid: one lane per (frame, row pair, 16-pixel column group), flattened in that order so that a wavefront walks along a row pair
template <int F, bool FAST>
__global__ __launch_bounds__(256) void yuv_to_bgr_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, YuvGeom k, int ncg, long long total) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int hp = (k.h + 1) >> 1;
    const long long rowpair = gid / ncg;
    const int cg = (int)(gid - rowpair * ncg);
    const int f = (int)(rowpair / hp), rp = (int)(rowpair - (long long)f * hp);
    frame_block<F, FAST>(src + (size_t)f * k.frame_stride, dst + (size_t)f * k.h * k.w * 3, k, rp, cg);
}

// ---- frame table: one batch whose frames each come from their own place (S decoders' surface pools: own addresses, own pitch, format,
// colour matrix, memory space).  One launch per batch, driven by a table in device memory with one entry per frame (256 frames do not
// fit kernel arguments).  blockIdx.y is the frame, so the entry is workgroup-uniform and neither the format branch nor the 16-byte
// branch diverges.  Per frame the conversion is yuv_to_bgr_kernel's (frame_block, the same 16 x 2 block per lane); a BGR
// entry is a byte copy; an entry of kind FRAME_NONE is a frame that is already in place (a host BGR frame copied straight into the slot).
enum { FRAME_NONE = 0, FRAME_NV12 = 1, FRAME_I420 = 2, FRAME_BGR = 3, FRAME_P016 = 4, FRAME_I010 = 5, FRAME_I422 = 6, FRAME_I444 = 7 };
const int kFrameKind[PF_COUNT] = {FRAME_NV12, FRAME_I420, FRAME_P016, FRAME_I010, FRAME_I422, FRAME_I444};      // by YuvGeom::fmt
struct FrameEntry {
    const uint8_t* src;                                 // device address of the frame
    int kind, fast;                                     // FRAME_*; fast: every address the 16-byte variant forms for THIS frame is aligned
    int pitch_y, pitch_c;
    unsigned long long off_c, off_v;
    int yoff, cy, cvr, cvg, cug, cub;
};
static_assert(sizeof(FrameEntry) == VC_FRAME_ENTRY_BYTES, "FrameEntry is copied to the device as plain bytes");

template <int F>
__device__ __forceinline__ void frame_block_of(const FrameEntry& e, uint8_t* __restrict__ df, const YuvGeom& k, int rp, int cg) {
    if (e.fast) frame_block<F, true>(e.src, df, k, rp, cg);
    else frame_block<F, false>(e.src, df, k, rp, cg);
}

// one frame of a table-driven batch: this lane's share of entry e (workgroup-uniform), converted or copied into the frame at df
__device__ __forceinline__ void frame_convert(const FrameEntry& e, uint8_t* __restrict__ df, int h, int w, int ncg) {
    const size_t frame_bytes = (size_t)h * w * 3;
    const int lid = blockIdx.x * 256 + threadIdx.x;
    if (e.kind == FRAME_BGR) {                              // the frame's lanes stride over its bytes: <= 96 bytes each, as on the YUV side
        const size_t step = (size_t)gridDim.x * 256;
        if (e.fast) {
            const uint4* s4 = (const uint4*)e.src;
            uint4* d4 = (uint4*)df;
            for (size_t i = lid; i < frame_bytes / 16; i += step) d4[i] = s4[i];
        } else {
            for (size_t i = lid; i < frame_bytes; i += step) df[i] = e.src[i];
        }
        return;
    }
    if (lid >= ((h + 1) >> 1) * ncg) return;
    const int rp = lid / ncg, cg = lid - rp * ncg;
    YuvGeom k;
    k.h = h; k.w = w; k.pitch_y = e.pitch_y; k.pitch_c = e.pitch_c; k.off_c = e.off_c; k.off_v = e.off_v;
    k.yoff = e.yoff; k.cy = e.cy; k.cvr = e.cvr; k.cvg = e.cvg; k.cug = e.cug; k.cub = e.cub;
    switch (e.kind) {                                       // workgroup-uniform, like e.fast
    case FRAME_NV12: frame_block_of<PF_NV12>(e, df, k, rp, cg); break;
    case FRAME_I420: frame_block_of<PF_I420>(e, df, k, rp, cg); break;
    case FRAME_P016: frame_block_of<PF_P016>(e, df, k, rp, cg); break;
    case FRAME_I010: frame_block_of<PF_I010>(e, df, k, rp, cg); break;
    case FRAME_I422: frame_block_of<PF_I422>(e, df, k, rp, cg); break;
    case FRAME_I444: frame_block_of<PF_I444>(e, df, k, rp, cg); break;
    default: break;
    }
}

// grid: x = the frame's lanes (row pair, 16-pixel column group) in blocks of 256, y = frame.  dst: frame f at dst + f * h * w * 3.
__global__ __launch_bounds__(256) void frames_to_bgr_kernel(const FrameEntry* __restrict__ tab, uint8_t* __restrict__ dst, int h, int w, int ncg) {
    const FrameEntry e = tab[blockIdx.y];                   // workgroup-uniform
    if (e.kind == FRAME_NONE) return;
    frame_convert(e, dst + (size_t)blockIdx.y * ((size_t)h * w * 3), h, w, ncg);
}

// Sized batches (include/vcount_hip.h): a second table beside the first gives every frame its own size and its cell in dst.  The grid's
// x extent covers the largest frame; workgroups past a smaller frame's own lanes exit.
struct FrameCell {
    unsigned long long dst_off;                             // f * cell
    int h, w;
};
static_assert(sizeof(FrameCell) == 16, "FrameCell is copied to the device as plain bytes");

__global__ __launch_bounds__(256) void frames_to_bgr_sized_kernel(const FrameEntry* __restrict__ tab, const FrameCell* __restrict__ cells, uint8_t* __restrict__ dst) {
    const FrameEntry e = tab[blockIdx.y];                   // workgroup-uniform
    if (e.kind == FRAME_NONE) return;
    const FrameCell c = cells[blockIdx.y];
    frame_convert(e, dst + c.dst_off, c.h, c.w, (c.w + 15) >> 4);
}

template <int F>
void launch_yuv_fmt(bool fast, dim3 grid, hipStream_t s, const uint8_t* src, uint8_t* dst, const YuvGeom& g, int ncg, long long total) {
    if (fast) hipLaunchKernelGGL((yuv_to_bgr_kernel<F, true>), grid, dim3(256), 0, s, src, dst, g, ncg, total);
    else hipLaunchKernelGGL((yuv_to_bgr_kernel<F, false>), grid, dim3(256), 0, s, src, dst, g, ncg, total);
}

}  // namespace

// Validates a descriptor for b frames of h x w and resolves its zeros.  Pure host code: runs before any HIP call.
int yuv_resolve(const vc_yuv_desc* d, int b, int h, int w, YuvGeom& g) {
    VC_CHECK(d, VC_ERR_ARG, "null vc_yuv_desc");
    const bool known = d->format == VC_PIX_NV12 || d->format == VC_PIX_I420 || (d->format >= VC_PIX_P016 && d->format <= VC_PIX_I444);
    VC_CHECK(known, VC_ERR_ARG, "unknown pixel format %d (VC_PIX_NV12 / VC_PIX_I420 / VC_PIX_P016 / VC_PIX_I010 / VC_PIX_I422 / VC_PIX_I444)", d->format);
    VC_CHECK(d->matrix == VC_YUV_BT601 || d->matrix == VC_YUV_BT709, VC_ERR_ARG, "unknown colour matrix %d (VC_YUV_BT601 / VC_YUV_BT709)", d->matrix);
    VC_CHECK(d->full_range == 0 || d->full_range == 1, VC_ERR_ARG, "full_range must be 0 or 1");
    g.fmt = d->format >= VC_PIX_P016 ? PF_P016 + (d->format - VC_PIX_P016) : d->format;
    g.nv12 = g.fmt == PF_NV12;
    const bool semi = g.fmt == PF_NV12 || g.fmt == PF_P016, vsub = g.fmt != PF_I422 && g.fmt != PF_I444, hsub = g.fmt != PF_I444;
    const int ss = g.fmt == PF_P016 || g.fmt == PF_I010 ? 2 : 1;               // bytes of one sample
    VC_CHECK(b >= 1 && h >= (vsub ? 2 : 1) && w >= (hsub ? 2 : 1), VC_ERR_ARG, "bad batch of %d frames %dx%d", b, h, w);
    if (vsub) VC_CHECK(h % 2 == 0 && w % 2 == 0, VC_ERR_ARG, "4:2:0 frames need an even height and width, got %dx%d", h, w);
    if (hsub) VC_CHECK(w % 2 == 0, VC_ERR_ARG, "4:2:2 frames need an even width, got %dx%d", h, w);
    VC_CHECK(ss == 1 || w <= (1 << 29), VC_ERR_ARG, "bad batch of %d frames %dx%d", b, h, w);      // 2 * w is an int
    g.h = h; g.w = w;
    const int rowb = w * ss;                                                   // bytes of one luma row
    const int crow = (semi || !hsub ? w : w / 2) * ss;                         // bytes of one chroma row
    g.pitch_y = d->pitch_y ? d->pitch_y : rowb;
    g.pitch_c = d->pitch_c ? d->pitch_c : crow;
    VC_CHECK(g.pitch_y >= rowb, VC_ERR_ARG, "pitch_y %d is below the row width %d", d->pitch_y, rowb);
    VC_CHECK(g.pitch_c >= crow, VC_ERR_ARG, "pitch_c %d is below the chroma row width %d", d->pitch_c, crow);
    const size_t hc = vsub ? (size_t)h / 2 : (size_t)h;                        // chroma rows
    const size_t len_y = (size_t)g.pitch_y * (h - 1) + rowb, len_c = (size_t)g.pitch_c * (hc - 1) + crow;
    g.off_c = d->offset_c ? d->offset_c : (size_t)g.pitch_y * h;
    g.off_v = semi ? 0 : (d->offset_v ? d->offset_v : g.off_c + (size_t)g.pitch_c * hc);
    const size_t lim = (size_t)1 << 40;                                        // keeps every sum below far from overflow
    VC_CHECK(g.off_c < lim && g.off_v < lim && d->frame_stride < lim, VC_ERR_ARG, "plane offset or frame stride out of range");
    VC_CHECK(g.off_c >= len_y, VC_ERR_ARG, "the chroma plane (offset %zu) overlaps the luma plane (%zu bytes)", g.off_c, len_y);
    g.frame_end = g.off_c + len_c;
    if (!semi) {
        VC_CHECK(g.off_v >= len_y, VC_ERR_ARG, "the V plane (offset %zu) overlaps the luma plane (%zu bytes)", g.off_v, len_y);
        VC_CHECK(g.off_v >= g.off_c + len_c || g.off_c >= g.off_v + len_c, VC_ERR_ARG, "the U and V planes overlap (offsets %zu, %zu)", g.off_c, g.off_v);
        g.frame_end = std::max(g.frame_end, g.off_v + len_c);
    }
    g.frame_stride = d->frame_stride ? d->frame_stride : g.frame_end;
    VC_CHECK(g.frame_stride >= g.frame_end, VC_ERR_ARG, "frame_stride %zu is below the frame's %zu bytes", g.frame_stride, g.frame_end);
    const int* c = kYuvCoef[d->matrix][d->full_range];
    g.matrix = d->matrix; g.full_range = d->full_range;
    g.yoff = d->full_range ? 0 : 16;
    g.cy = c[0]; g.cvr = c[1]; g.cvg = c[2]; g.cug = c[3]; g.cub = c[4];
    return VC_OK;
}

int yuv_resolve_out(const vc_yuv_desc* d, int b, int h, int w, YuvGeom& g) {
    VC_CHECK(!d || d->format < VC_PIX_P016 || d->format > VC_PIX_I444, VC_ERR_ARG,
             "pixel format %d is an ingest-only format: egress writes VC_PIX_NV12 / VC_PIX_I420", d->format);
    return yuv_resolve(d, b, h, w, g);
}

int sized_dims_resolve(const vc_frame_dims* dims, int b, int img_size, SizedDims& out) {
    VC_CHECK(b >= 1, VC_ERR_ARG, "bad batch of %d frames", b);
    VC_CHECK(dims, VC_ERR_ARG, "null frame list");
    VC_CHECK(img_size >= 1, VC_ERR_ARG, "bad img_size %d", img_size);
    out = SizedDims{};
    for (int f = 0; f < b; ++f) {
        const int h = dims[f].h, w = dims[f].w;
        VC_CHECK(h >= 1 && w >= 1 && h <= (1 << 15) && w <= (1 << 15), VC_ERR_ARG, "frame %d: bad frame size %dx%d", f, h, w);
        int nh, nw;
        autoshape_net_size(&h, &w, 1, img_size, nh, nw);
        if (f == 0) { out.net_h = nh; out.net_w = nw; }
        VC_CHECK(nh == out.net_h && nw == out.net_w, VC_ERR_ARG, "frame %d: %dx%d runs at %dx%d, frame 0 at %dx%d", f, h, w, nh, nw, out.net_h, out.net_w);
        out.cell = std::max(out.cell, (size_t)h * w * 3);
        out.max_h = std::max(out.max_h, h); out.max_w = std::max(out.max_w, w);
    }
    out.cell = (out.cell + 15) / 16 * 16;
    return VC_OK;
}

size_t yuv_batch_bytes(const YuvGeom& g, int b) { return (size_t)(b - 1) * g.frame_stride + g.frame_end; }

// src: b frames laid out as g says, dst: [b][h][w][3], both device memory.  The 16-byte variant needs every address it forms aligned.
int launch_yuv_to_bgr(const YuvGeom& g, const uint8_t* src, uint8_t* dst, int b, hipStream_t s) {
    const bool fast = g.w % 16 == 0 && g.pitch_y % 16 == 0 && g.pitch_c % 16 == 0 && g.off_c % 16 == 0 && g.off_v % 16 == 0 &&
                      g.frame_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const int ncg = (g.w + 15) / 16;
    const long long total = (long long)b * ((g.h + 1) / 2) * ncg;
    const long long blocks = (total + 255) / 256;
    VC_CHECK(blocks <= 0x7fffffffll, VC_ERR_CAPACITY, "batch too large for one conversion launch");
    const dim3 grid((unsigned)blocks);
    switch (g.fmt) {
    case PF_NV12: launch_yuv_fmt<PF_NV12>(fast, grid, s, src, dst, g, ncg, total); break;
    case PF_I420: launch_yuv_fmt<PF_I420>(fast, grid, s, src, dst, g, ncg, total); break;
    case PF_P016: launch_yuv_fmt<PF_P016>(fast, grid, s, src, dst, g, ncg, total); break;
    case PF_I010: launch_yuv_fmt<PF_I010>(fast, grid, s, src, dst, g, ncg, total); break;
    case PF_I422: launch_yuv_fmt<PF_I422>(fast, grid, s, src, dst, g, ncg, total); break;
    case PF_I444: launch_yuv_fmt<PF_I444>(fast, grid, s, src, dst, g, ncg, total); break;
    default: VC_CHECK(false, VC_ERR_ARG, "unresolved pixel format %d", g.fmt);
    }
    VC_HIP(hipGetLastError());
    return VC_OK;
}

namespace {

// One frame of a frame list (pure host code): its refusals name it.  g is resolved for the YUV kinds, for the frame's own h x w; a
// YUV_HOST frame takes the next 16-byte-aligned place in the raw buffer (*cur: the bytes packed so far; raw_off[f], -1 for the rest).
int frame_resolve(const vc_frame_src& s, int f, int h, int w, bool host_only, YuvGeom& g, int64_t* raw_off, size_t* cur) {
    VC_CHECK(s.kind == VC_SRC_BGR_HOST || s.kind == VC_SRC_BGR_DEV || s.kind == VC_SRC_YUV_HOST || s.kind == VC_SRC_YUV_DEV, VC_ERR_ARG,
             "frame %d: unknown source kind %d (VC_SRC_*)", f, s.kind);
    VC_CHECK(!host_only || s.kind == VC_SRC_BGR_HOST || s.kind == VC_SRC_YUV_HOST, VC_ERR_ARG, "frame %d: a device source (kind %d) where host frames are expected", f, s.kind);
    VC_CHECK(s.data, VC_ERR_ARG, "frame %d: null data", f);
    if (raw_off) raw_off[f] = -1;
    if (s.kind != VC_SRC_YUV_HOST && s.kind != VC_SRC_YUV_DEV) return VC_OK;
    vc_yuv_desc d = s.desc;
    d.frame_stride = 0;                                     // one frame: the stride has no meaning here
    if (yuv_resolve(&d, 1, h, w, g) != VC_OK) {
        char msg[400];
        snprintf(msg, sizeof(msg), "%s", last_error());
        set_error("frame %d: %s", f, msg);
        return VC_ERR_ARG;
    }
    if (s.kind == VC_SRC_YUV_HOST) {
        *cur = (*cur + 15) / 16 * 16;
        if (raw_off) raw_off[f] = (int64_t)*cur;
        *cur += yuv_batch_bytes(g, 1);
    }
    return VC_OK;
}

// The whole validation of a frame list of h x w frames (before any HIP call).  raw_off[f] / *raw_bytes: the packing of the YUV_HOST
// frames into one raw buffer (vc_frames_layout_host).
int frames_resolve(const vc_frame_src* frames, int b, int h, int w, bool host_only, std::vector<YuvGeom>& geo, int64_t* raw_off, size_t* raw_bytes) {
    VC_CHECK(b >= 1, VC_ERR_ARG, "bad batch of %d frames", b);
    VC_CHECK(frames, VC_ERR_ARG, "null frame list");
    VC_CHECK(h >= 1 && w >= 1, VC_ERR_ARG, "bad frame size %dx%d", h, w);
    geo.assign((size_t)b, YuvGeom{});
    size_t cur = 0;
    for (int f = 0; f < b; ++f) VC_TRY(frame_resolve(frames[f], f, h, w, host_only, geo[f], raw_off, &cur));
    if (raw_bytes) *raw_bytes = cur;
    return VC_OK;
}

// The same for a sized frame list: the rules of its dims first, then every frame with its own size.
int frames_resolve_sized(const vc_frame_src* frames, const vc_frame_dims* dims, int b, int img_size, bool host_only, std::vector<YuvGeom>& geo, int64_t* raw_off,
                         size_t* raw_bytes, SizedDims& sd) {
    VC_CHECK(b >= 1, VC_ERR_ARG, "bad batch of %d frames", b);
    VC_CHECK(frames, VC_ERR_ARG, "null frame list");
    VC_TRY(sized_dims_resolve(dims, b, img_size, sd));
    geo.assign((size_t)b, YuvGeom{});
    size_t cur = 0;
    for (int f = 0; f < b; ++f) VC_TRY(frame_resolve(frames[f], f, dims[f].h, dims[f].w, host_only, geo[f], raw_off, &cur));
    if (raw_bytes) *raw_bytes = cur;
    return VC_OK;
}

// src / dst: the DEVICE addresses the kernel will read and write for this frame
FrameEntry frame_entry(int src_kind, const YuvGeom& g, const uint8_t* src, const uint8_t* dst, int h, int w) {
    FrameEntry t{};
    t.src = src;
    const bool ends = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    if (src_kind == VC_SRC_BGR_HOST || src_kind == VC_SRC_BGR_DEV) {
        t.kind = FRAME_BGR;
        t.fast = ends && ((size_t)h * w * 3) % 16 == 0;
        return t;
    }
    t.kind = kFrameKind[g.fmt];
    // launch_yuv_to_bgr's test with this frame's own addresses in place of the batch's base and stride
    t.fast = g.w % 16 == 0 && g.pitch_y % 16 == 0 && g.pitch_c % 16 == 0 && g.off_c % 16 == 0 && g.off_v % 16 == 0 && ends;
    t.pitch_y = g.pitch_y; t.pitch_c = g.pitch_c; t.off_c = g.off_c; t.off_v = g.off_v;
    t.yoff = g.yoff; t.cy = g.cy; t.cvr = g.cvr; t.cvg = g.cvg; t.cug = g.cug; t.cub = g.cub;
    return t;
}

// d_tab: b entries in device memory, dst: [b][h][w][3] in device memory
int launch_frames_to_bgr(const FrameEntry* d_tab, uint8_t* dst, int b, int h, int w, hipStream_t s) {
    const int ncg = (w + 15) / 16;
    const long long lanes = (long long)((h + 1) / 2) * ncg;                    // of one frame
    const long long blocks = (lanes + 255) / 256;
    VC_CHECK(b <= 65535 && blocks <= 0x7fffffll, VC_ERR_CAPACITY, "batch too large for one conversion launch");
    hipLaunchKernelGGL(frames_to_bgr_kernel, dim3((unsigned)blocks, (unsigned)b), dim3(256), 0, s, d_tab, dst, h, w, ncg);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// d_tab: b entries, d_cells: b cells, both in device memory; dst: b cells of device memory
int launch_frames_to_bgr_sized(const FrameEntry* d_tab, const FrameCell* d_cells, uint8_t* dst, int b, const vc_frame_dims* dims, hipStream_t s) {
    long long lanes = 1;                                                       // of the largest frame
    for (int f = 0; f < b; ++f) lanes = std::max(lanes, (long long)((dims[f].h + 1) / 2) * ((dims[f].w + 15) / 16));
    const long long blocks = (lanes + 255) / 256;
    VC_CHECK(b <= 65535 && blocks <= 0x7fffffll, VC_ERR_CAPACITY, "batch too large for one conversion launch");
    hipLaunchKernelGGL(frames_to_bgr_sized_kernel, dim3((unsigned)blocks, (unsigned)b), dim3(256), 0, s, d_tab, d_cells, dst);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// A frame list's table: b entries, followed for a sized batch (dims != nullptr) by its b cells -- one block, so one copy carries both.
size_t frame_table_bytes(int b, bool sized) { return (size_t)b * (sizeof(FrameEntry) + (sized ? sizeof(FrameCell) : 0)); }

// fills entry f (and, for a sized batch, cell f) of the host table: the frame at DEVICE address src goes to dst + f * stride
void frame_table_set(void* tab, int b, int f, const vc_frame_src& s, const YuvGeom& g, const uint8_t* src, uint8_t* dst, size_t stride, int h, int w, bool sized) {
    ((FrameEntry*)tab)[f] = src ? frame_entry(s.kind, g, src, dst + (size_t)f * stride, h, w) : FrameEntry{};      // no src: FRAME_NONE, already in place
    if (sized) ((FrameCell*)((FrameEntry*)tab + b))[f] = FrameCell{(unsigned long long)f * stride, h, w};
}

// the launch for a table in device memory; dims == nullptr: a uniform batch of h x w frames, dst [b][h][w][3]
int launch_frame_table(const void* d_tab, uint8_t* dst, int b, int h, int w, const vc_frame_dims* dims, hipStream_t s) {
    const FrameEntry* ent = (const FrameEntry*)d_tab;
    return dims ? launch_frames_to_bgr_sized(ent, (const FrameCell*)(ent + b), dst, b, dims, s) : launch_frames_to_bgr(ent, dst, b, h, w, s);
}

// Parity of the two table kernels on a validated list of host frames.  Every frame is uploaded to an address congruent to its host
// pointer mod 16, so that the caller chooses the 16-byte or the generic path by where it puts the frame.  dims == nullptr: b frames of
// h x w into out [b][h][w][3] (stride = h * w * 3).  Otherwise the caller's cells (stride = the cell) are uploaded, converted into and
// read back: what the kernel leaves alone inside a cell comes back as the caller filled it.
int frames_to_bgr_parity(const vc_frame_src* frames, int b, int h, int w, const vc_frame_dims* dims, size_t stride, const std::vector<YuvGeom>& geo, uint8_t* out,
                         const char* kernel) {
    std::vector<size_t> off((size_t)b), len((size_t)b);
    size_t in_bytes = 0;
    for (int f = 0; f < b; ++f) {
        const int fh = dims ? dims[f].h : h, fw = dims ? dims[f].w : w;
        len[f] = frames[f].kind == VC_SRC_YUV_HOST ? yuv_batch_bytes(geo[f], 1) : (size_t)fh * fw * 3;
        off[f] = (in_bytes + 15) / 16 * 16 + (uintptr_t)frames[f].data % 16;
        in_bytes = off[f] + len[f];
    }
    DevScratch mem;
    uint8_t *ds = nullptr, *dt = nullptr;
    GuardedOut dd;
    VC_TRY(mem.alloc(&ds, in_bytes));
    VC_TRY(dd.alloc(mem, (size_t)b * stride, dims ? out : nullptr));
    VC_TRY(mem.alloc(&dt, frame_table_bytes(b, dims != nullptr)));
    std::vector<uint8_t> tab(frame_table_bytes(b, dims != nullptr));
    for (int f = 0; f < b; ++f) {
        VC_HIP(hipMemcpy(ds + off[f], frames[f].data, len[f], hipMemcpyHostToDevice));
        frame_table_set(tab.data(), b, f, frames[f], geo[f], ds + off[f], dd.out(), stride, dims ? dims[f].h : h, dims ? dims[f].w : w, dims != nullptr);
    }
    VC_HIP(hipMemcpy(dt, tab.data(), tab.size(), hipMemcpyHostToDevice));
    VC_TRY(launch_frame_table(dt, dd.out(), b, h, w, dims, nullptr));
    return dd.read_back(out, kernel);
}

// Grows the slot's raw YUV buffer to `bytes` (first YUV batch of the slot, or a pitch wider than any before).  Everything the copy
// stream still has in flight reads the old buffer, hence the wait.
int ingest_raw_reserve(vc_engine* e, int slot, size_t bytes) {
    if (bytes <= e->yuv_raw_bytes[slot]) return VC_OK;
    VC_HIP(hipStreamSynchronize(e->cstream));
    const size_t tight = (size_t)e->cfg.max_batch * e->cfg.max_frame_h * e->cfg.max_frame_w * 3 / 2;
    e->yuv_raw_bytes[slot] = 0;
    VC_TRY(dev_realloc(e, (void**)&e->d_yuv_raw[slot], std::max(bytes, tight)));
    e->yuv_raw_bytes[slot] = std::max(bytes, tight);
    return VC_OK;
}

// One batch from a validated list of per-frame sources into the next ingest slot.  dims == nullptr: a uniform batch of h x w frames,
// frame f at f * h * w * 3.  Otherwise a sized batch: frame f in cell f (stride = the cell), h x w the largest frame, and the slot
// remembers the dims for vc_stream_submit_sized.  On the copy stream: one copy per host frame (BGR straight into its place in the slot,
// YUV into the slot's raw buffer at its raw_off), one copy of the table only if something launches (per-slot pinned table -> per-slot
// device table: the slot rules guarantee that the slot's previous batch, and with it the previous copy of the table, is complete), at
// most one launch, the slot's event.
int stage_frame_list(vc_engine* e, const vc_frame_src* frames, int b, int h, int w, const vc_frame_dims* dims, size_t stride, const std::vector<YuvGeom>& geo,
                     const int64_t* raw_off, size_t raw_bytes, void** frames_dev_out) {
    int slot = 0;
    VC_TRY(ingest_take_slot(e, b, h, w, &slot));
    if (!e->h_frame_tab[slot]) {
        VC_TRY(host_alloc(e, &e->h_frame_tab[slot], frame_table_bytes(e->cfg.max_batch, true)));
        VC_TRY(dev_alloc(e, &e->d_frame_tab[slot], frame_table_bytes(e->cfg.max_batch, true)));
    }
    VC_TRY(ingest_raw_reserve(e, slot, raw_bytes));
    bool launch = false;
    for (int f = 0; f < b; ++f) {
        const vc_frame_src& s = frames[f];
        const int fh = dims ? dims[f].h : h, fw = dims ? dims[f].w : w;
        const uint8_t* src = (const uint8_t*)s.data;
        if (s.kind == VC_SRC_BGR_HOST) {
            VC_HIP(hipMemcpyAsync(e->d_ingest[slot] + (size_t)f * stride, s.data, (size_t)fh * fw * 3, hipMemcpyHostToDevice, e->cstream));
            src = nullptr;                                  // already in place
        } else if (s.kind == VC_SRC_YUV_HOST) {
            uint8_t* raw = e->d_yuv_raw[slot] + raw_off[f];
            VC_HIP(hipMemcpyAsync(raw, s.data, yuv_batch_bytes(geo[f], 1), hipMemcpyHostToDevice, e->cstream));
            src = raw;
        }
        frame_table_set(e->h_frame_tab[slot], b, f, s, geo[f], src, e->d_ingest[slot], stride, fh, fw, dims != nullptr);
        launch = launch || src;
    }
    if (launch) {
        VC_HIP(hipMemcpyAsync(e->d_frame_tab[slot], e->h_frame_tab[slot], frame_table_bytes(b, dims != nullptr), hipMemcpyHostToDevice, e->cstream));
        VC_TRY(launch_frame_table(e->d_frame_tab[slot], e->d_ingest[slot], b, h, w, dims, e->cstream));
    }
    if (dims) e->ingest_dims[slot].assign(dims, dims + b);
    return ingest_publish(e, slot, frames_dev_out);
}

}  // namespace

}  // namespace vc

using namespace vc;

extern "C" {

int vc_yuv_desc_default(vc_yuv_desc* d) {
    VC_CHECK(d, VC_ERR_ARG, "null argument");
    memset(d, 0, sizeof(*d));
    d->format = VC_PIX_NV12; d->matrix = VC_YUV_BT601; d->full_range = 0;
    return VC_OK;
}

// Parity entry point.  The device output sits between two guard blocks that the call checks afterwards: a kernel that wrote
// outside [b][h][w][3] is reported instead of returning a plausible image.
int vc_yuv_to_bgr_host(const vc_yuv_desc* d, const uint8_t* yuv, int b, int h, int w, uint8_t* bgr_out) {
    VC_CHECK(yuv && bgr_out, VC_ERR_ARG, "null argument");
    YuvGeom g;
    VC_TRY(yuv_resolve(d, b, h, w, g));
    const size_t in_bytes = yuv_batch_bytes(g, b);
    DevScratch mem;
    uint8_t* ds = nullptr;
    GuardedOut dd;
    VC_TRY(mem.alloc(&ds, in_bytes));
    VC_TRY(dd.alloc(mem, (size_t)b * h * w * 3));
    VC_HIP(hipMemcpy(ds, yuv, in_bytes, hipMemcpyHostToDevice));
    VC_TRY(launch_yuv_to_bgr(g, ds, dd.out(), b, nullptr));
    return dd.read_back(bgr_out, "yuv_to_bgr_kernel");
}

int vc_yuv_to_bgr_dev(const vc_yuv_desc* d, const void* yuv_dev, int b, int h, int w, void* bgr_dev) {
    VC_CHECK(yuv_dev && bgr_dev, VC_ERR_ARG, "null argument");
    YuvGeom g;
    VC_TRY(yuv_resolve(d, b, h, w, g));
    return launch_yuv_to_bgr(g, (const uint8_t*)yuv_dev, (uint8_t*)bgr_dev, b, nullptr);
}

int vc_stream_stage_yuv_host(vc_engine* e, const vc_yuv_desc* d, const uint8_t* yuv_host, int b, int h, int w, void** frames_dev_out) {
    VC_CHECK(e && yuv_host && frames_dev_out, VC_ERR_ARG, "null argument");
    YuvGeom g;
    VC_TRY(yuv_resolve(d, b, h, w, g));
    int slot = 0;
    VC_TRY(ingest_take_slot(e, b, h, w, &slot));
    const size_t bytes = yuv_batch_bytes(g, b);
    VC_TRY(ingest_raw_reserve(e, slot, bytes));
    VC_HIP(hipMemcpyAsync(e->d_yuv_raw[slot], yuv_host, bytes, hipMemcpyHostToDevice, e->cstream));
    VC_TRY(launch_yuv_to_bgr(g, e->d_yuv_raw[slot], e->d_ingest[slot], b, e->cstream));
    return ingest_publish(e, slot, frames_dev_out);
}

int vc_stream_stage_yuv_dev(vc_engine* e, const vc_yuv_desc* d, const void* yuv_dev, int b, int h, int w, void** frames_dev_out) {
    VC_CHECK(e && yuv_dev && frames_dev_out, VC_ERR_ARG, "null argument");
    YuvGeom g;
    VC_TRY(yuv_resolve(d, b, h, w, g));
    int slot = 0;
    VC_TRY(ingest_take_slot(e, b, h, w, &slot));
    VC_TRY(launch_yuv_to_bgr(g, (const uint8_t*)yuv_dev, e->d_ingest[slot], b, e->cstream));
    return ingest_publish(e, slot, frames_dev_out);
}

int vc_frames_layout_host(const vc_frame_src* frames, int b, int h, int w, int64_t* raw_off, size_t* raw_bytes) {
    VC_CHECK(raw_off && raw_bytes, VC_ERR_ARG, "null argument");
    std::vector<YuvGeom> geo;
    return frames_resolve(frames, b, h, w, false, geo, raw_off, raw_bytes);
}

// Parity entry point of frames_to_bgr_kernel (frames_to_bgr_parity).
int vc_frames_to_bgr_host(const vc_frame_src* frames, int b, int h, int w, uint8_t* bgr_out) {
    VC_CHECK(bgr_out, VC_ERR_ARG, "null argument");
    std::vector<YuvGeom> geo;
    VC_TRY(frames_resolve(frames, b, h, w, true, geo, nullptr, nullptr));
    return frames_to_bgr_parity(frames, b, h, w, nullptr, (size_t)h * w * 3, geo, bgr_out, "frames_to_bgr_kernel");
}

// The kernel on the caller's own device buffers (measurement), null stream, no wait.  With `frames` the table is built and uploaded
// (a blocking copy) into table_dev first; without, table_dev is launched as the last such call left it.
int vc_frames_to_bgr_dev(const vc_frame_src* frames, int b, int h, int w, void* bgr_dev, void* table_dev) {
    VC_CHECK(bgr_dev && table_dev, VC_ERR_ARG, "null argument");
    VC_CHECK(b >= 1 && h >= 1 && w >= 1, VC_ERR_ARG, "bad batch of %d frames %dx%d", b, h, w);
    if (frames) {
        std::vector<YuvGeom> geo;
        VC_TRY(frames_resolve(frames, b, h, w, false, geo, nullptr, nullptr));
        std::vector<FrameEntry> tab((size_t)b);
        for (int f = 0; f < b; ++f) {
            VC_CHECK(frames[f].kind == VC_SRC_BGR_DEV || frames[f].kind == VC_SRC_YUV_DEV, VC_ERR_ARG, "frame %d: a host source (kind %d) where device frames are expected", f, frames[f].kind);
            tab[f] = frame_entry(frames[f].kind, geo[f], (const uint8_t*)frames[f].data, (const uint8_t*)bgr_dev + (size_t)f * h * w * 3, h, w);
        }
        VC_HIP(hipMemcpy(table_dev, tab.data(), (size_t)b * sizeof(FrameEntry), hipMemcpyHostToDevice));
    }
    return launch_frames_to_bgr((const FrameEntry*)table_dev, (uint8_t*)bgr_dev, b, h, w, nullptr);
}

// One batch from per-frame sources (stage_frame_list).
int vc_stream_stage_frames(vc_engine* e, const vc_frame_src* frames, int b, int h, int w, void** frames_dev_out) {
    VC_CHECK(e && frames_dev_out, VC_ERR_ARG, "null argument");
    std::vector<YuvGeom> geo;
    std::vector<int64_t> raw_off((size_t)std::max(b, 1));
    size_t raw_bytes = 0;
    VC_TRY(frames_resolve(frames, b, h, w, false, geo, raw_off.data(), &raw_bytes));
    return stage_frame_list(e, frames, b, h, w, nullptr, (size_t)h * w * 3, geo, raw_off.data(), raw_bytes, frames_dev_out);
}

// ---- sized batches -------------------------------------------------------------------------------------------------------------------
int vc_autoshape_net_size(int h, int w, int img_size, int* net_h, int* net_w) {
    VC_CHECK(net_h && net_w, VC_ERR_ARG, "null argument");
    VC_CHECK(h >= 1 && w >= 1 && img_size >= 1, VC_ERR_ARG, "bad image %dx%d at size %d", h, w, img_size);
    autoshape_net_size(&h, &w, 1, img_size, *net_h, *net_w);
    return VC_OK;
}

int vc_frames_layout_sized_host(const vc_frame_src* frames, const vc_frame_dims* dims, int b, int img_size, int64_t* raw_off, size_t* raw_bytes, size_t* cell,
                                int* net_h, int* net_w) {
    VC_CHECK(raw_off && raw_bytes && cell && net_h && net_w, VC_ERR_ARG, "null argument");
    std::vector<YuvGeom> geo;
    SizedDims sd;
    VC_TRY(frames_resolve_sized(frames, dims, b, img_size, false, geo, raw_off, raw_bytes, sd));
    *cell = sd.cell; *net_h = sd.net_h; *net_w = sd.net_w;
    return VC_OK;
}

// Parity entry point of frames_to_bgr_sized_kernel (frames_to_bgr_parity).  Network shapes are not compared here (img_size 1 gives every
// frame 32 x 32).
int vc_frames_to_bgr_sized_host(const vc_frame_src* frames, const vc_frame_dims* dims, int b, uint8_t* cells) {
    VC_CHECK(cells, VC_ERR_ARG, "null argument");
    std::vector<YuvGeom> geo;
    SizedDims sd;
    VC_TRY(frames_resolve_sized(frames, dims, b, 1, true, geo, nullptr, nullptr, sd));
    return frames_to_bgr_parity(frames, b, sd.max_h, sd.max_w, dims, sd.cell, geo, cells, "frames_to_bgr_sized_kernel");
}

// vc_stream_stage_frames with every frame's own size: frame f lands in cell f of the slot (stage_frame_list).
int vc_stream_stage_frames_sized(vc_engine* e, const vc_frame_src* frames, const vc_frame_dims* dims, int b, void** frames_dev_out) {
    VC_CHECK(e && frames_dev_out, VC_ERR_ARG, "null argument");
    std::vector<YuvGeom> geo;
    std::vector<int64_t> raw_off((size_t)std::max(b, 1));
    size_t raw_bytes = 0;
    SizedDims sd;
    VC_TRY(frames_resolve_sized(frames, dims, b, e->cfg.img_size, false, geo, raw_off.data(), &raw_bytes, sd));
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "engine not finalized");
    VC_CHECK(b <= e->cfg.max_batch && sd.max_h <= e->cfg.max_frame_h && sd.max_w <= e->cfg.max_frame_w && (size_t)b * sd.cell <= ingest_slot_bytes(e), VC_ERR_CAPACITY,
             "batch of %d frames up to %dx%d (%zu-byte cells) exceeds max_batch / max_frame_h / max_frame_w", b, sd.max_h, sd.max_w, sd.cell);
    return stage_frame_list(e, frames, b, sd.max_h, sd.max_w, dims, sd.cell, geo, raw_off.data(), raw_bytes, frames_dev_out);
}

}  // extern "C"
