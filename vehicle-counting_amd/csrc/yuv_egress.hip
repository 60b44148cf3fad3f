// YUV egress: packed BGR u8 [b][h][w][3] frames in device memory (painted by overlay.hip) converted on the device into the 4:2:0
// surfaces an encoder takes -- NV12 (hardware encoders) or I420 (software encoders), pitched or tight.  The inverse of yuv_ingest.hip;
// the reference hands BGR to cv2.VideoWriter, which converts on the CPU behind its back (the reference's modules/datasets.py:132-145).
//
// The arithmetic is the definition (integer, so every implementation agrees bit for bit; restated in NumPy by tests/yuv_enc_ref.py):
//   Y[y][x]     = clamp((KYR*R + KYG*G + KYB*B + (1 << 19) + (YOFF << 20)) >> 20, 0, 255)       from the pixel's own B, G, R
//   Rm, Gm, Bm  = (sum of the channel over the 2 x 2 luma block + 2) >> 2                        rounded block mean, per channel
//   U[y/2][x/2] = clamp((KUR*Rm + KUG*Gm + KUB*Bm + (1 << 19) + (128 << 20)) >> 20, 0, 255)
//   V[y/2][x/2] = clamp((KVR*Rm + KVG*Gm + KVB*Bm + (1 << 19) + (128 << 20)) >> 20, 0, 255)
//   32-bit signed, YOFF = 16 (limited range) or 0 (full range), constants = int(round(literal * 2^20)), table below.
// Every factor fits 24 bits and every sum 29 bits (the largest accumulator is 2^28: full-range pure blue / red chroma, which the clamp
// brings from 256 to 255), hence the full-rate 24-bit multiplies.
//
// A pure streaming kernel, 3 B read and 1.5 B written per pixel, no LDS, plain vector stores.  One lane owns 16 pixels x 2 rows so
// that both rows share one chroma result: three 16-byte loads per row, 16 B of Y per row, 16 B of UV (8 B + 8 B for I420).  The
// generic variant (any even w, any pitch) owns the same 16 x 2 block, assembles the same words from byte loads and stores bytes.
// Bytes of the destination that belong to no plane (pitch padding, gaps between planes and frames) are never written.
#include "engine.h"

namespace vc {

namespace {

// {KYR, KYG, KYB, KUR, KUG, KUB, KVR, KVG, KVB} per [matrix][full_range]: int(round(literal * 2^20)), the literals being Kr, Kb of the
// matrix scaled by 219 / 255 (luma) and 224 / 255 (chroma) for limited range and rounded to 6 decimals.  Luma rows sum
// to 900542 (limited) / 2^20 (full), chroma rows to 0: grey gives U = V = 128 exactly.
const int kEncCoef[2][2][9] = {
    {{269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897},      // BT.601 limited
     {313524, 615514, 119538, -176933, -347355, 524288, 524288, -439026, -85262}},     // BT.601 full
    {{191455, 644068, 65019, -105533, -355018, 460551, 460551, -418321, -42230},       // BT.709 limited
     {222927, 749942, 75707, -120137, -404151, 524288, 524288, -476214, -48074}}};     // BT.709 full

struct EncGeom {                 // what the kernel needs of a YuvGeom, plus the forward constants
    int h, w, pitch_y, pitch_c;
    size_t off_c, off_v, frame_stride;
    int kyr, kyg, kyb, kur, kug, kub, kvr, kvg, kvb, ybias;     // ybias = (1 << 19) + (YOFF << 20)
};

// clamp((x) >> 20, 0, 255) written as clamp(x, 0, (256 << 20) - 1) >> 20, a logical shift of a non-negative number: the
// arithmetic-shift-then-clamp form is matched to gfx950's packed shift-and-saturate instruction, which yuv_ingest.hip found to leave
// stray high bits in words assembled from it.
__device__ __forceinline__ uint32_t enc_q(int acc) { return (uint32_t)min(max(acc, 0), (256 << 20) - 1) >> 20; }

__device__ __forceinline__ uint32_t enc_byte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255; }     // i is a constant after unrolling

__device__ __forceinline__ uint32_t enc_bytes4(const uint8_t* p, int n) {      // up to four bytes, the first n of them valid
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) v |= (uint32_t)p[i] << (8 * i);
    return v;
}

// grid: one lane per (frame, row pair, 16-pixel column group), flattened in that order so that a wavefront walks along a row pair
template <bool NV12, bool FAST>
__global__ __launch_bounds__(256) void bgr_to_yuv_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, EncGeom k, int ncg, long long total) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int hp = k.h >> 1;
    const long long rowpair = gid / ncg;
    const int cg = (int)(gid - rowpair * ncg);
    const int f = (int)(rowpair / hp), rp = (int)(rowpair - (long long)f * hp);
    const int x0 = cg * 16;
    const int npx = min(16, k.w - x0);                      // even; 16 on the fast path
    const uint8_t* s0 = src + (((size_t)f * k.h + 2 * rp) * k.w + x0) * 3;

    uint32_t px[2][12];                                     // 16 pixels of each row: 48 bytes B,G,R,B,G,R,...
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint8_t* s = s0 + (size_t)r * k.w * 3;
        if (FAST) {
            const uint4* s4 = (const uint4*)s;
            const uint4 a = s4[0], b = s4[1], c = s4[2];
            px[r][0] = a.x; px[r][1] = a.y; px[r][2] = a.z; px[r][3] = a.w;
            px[r][4] = b.x; px[r][5] = b.y; px[r][6] = b.z; px[r][7] = b.w;
            px[r][8] = c.x; px[r][9] = c.y; px[r][10] = c.z; px[r][11] = c.w;
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) px[r][j] = enc_bytes4(s + 4 * j, npx * 3 - 4 * j);
        }
    }

    uint32_t yw[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};      // 16 Y bytes per row
    uint32_t cw[4] = {0, 0, 0, 0};                          // NV12: U0 V0 U1 V1 ... (16 bytes); I420: cw[0..1] = 8 U bytes, cw[2..3] = 8 V bytes
#pragma unroll
    for (int c = 0; c < 8; ++c) {                           // one 2 x 2 block per step
        int sb = 2, sg = 2, sr = 2;                         // the rounding term of the block mean
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int p = 2 * c + q;
                const int B = (int)enc_byte(px[r], 3 * p), G = (int)enc_byte(px[r], 3 * p + 1), R = (int)enc_byte(px[r], 3 * p + 2);
                sb += B; sg += G; sr += R;
                yw[r][p >> 2] |= enc_q(__mul24(k.kyr, R) + __mul24(k.kyg, G) + __mul24(k.kyb, B) + k.ybias) << (8 * (p & 3));
            }
        }
        const int Bm = sb >> 2, Gm = sg >> 2, Rm = sr >> 2, cbias = (1 << 19) + (128 << 20);
        const uint32_t U = enc_q(__mul24(k.kur, Rm) + __mul24(k.kug, Gm) + __mul24(k.kub, Bm) + cbias);
        const uint32_t V = enc_q(__mul24(k.kvr, Rm) + __mul24(k.kvg, Gm) + __mul24(k.kvb, Bm) + cbias);
        if (NV12) {
            cw[c >> 1] |= (U | (V << 8)) << (16 * (c & 1));
        } else {
            cw[c >> 2] |= U << (8 * (c & 3));
            cw[2 + (c >> 2)] |= V << (8 * (c & 3));
        }
    }

    uint8_t* df = dst + (size_t)f * k.frame_stride;
    uint8_t* y0p = df + (size_t)(2 * rp) * k.pitch_y + x0;
    uint8_t* y1p = y0p + k.pitch_y;
    uint8_t* c0p = df + k.off_c + (size_t)rp * k.pitch_c + (NV12 ? x0 : (x0 >> 1));     // NV12: the UV row; I420: the U row
    uint8_t* c1p = df + k.off_v + (size_t)rp * k.pitch_c + (x0 >> 1);                   // I420: the V row
    if (FAST) {
        *(uint4*)y0p = make_uint4(yw[0][0], yw[0][1], yw[0][2], yw[0][3]);
        *(uint4*)y1p = make_uint4(yw[1][0], yw[1][1], yw[1][2], yw[1][3]);
        if (NV12) {
            *(uint4*)c0p = make_uint4(cw[0], cw[1], cw[2], cw[3]);
        } else {
            *(uint2*)c0p = make_uint2(cw[0], cw[1]);
            *(uint2*)c1p = make_uint2(cw[2], cw[3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < npx) {
                y0p[i] = (uint8_t)enc_byte(yw[0], i);
                y1p[i] = (uint8_t)enc_byte(yw[1], i);
                if (NV12) c0p[i] = (uint8_t)enc_byte(cw, i);
            }
            if (!NV12 && i < 8 && 2 * i < npx) {
                c0p[i] = (uint8_t)enc_byte(cw, i);
                c1p[i] = (uint8_t)enc_byte(cw, 8 + i);
            }
        }
    }
}

}  // namespace

// src: [b][h][w][3] BGR, dst: b frames laid out as g says, both device memory.  The 16-byte variant needs every address it forms aligned.
int launch_bgr_to_yuv(const YuvGeom& g, const uint8_t* src, uint8_t* dst, int b, hipStream_t s) {
    const bool fast = g.w % 16 == 0 && g.pitch_y % 16 == 0 && g.pitch_c % 16 == 0 && g.off_c % 16 == 0 && g.off_v % 16 == 0 &&
                      g.frame_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const int* c = kEncCoef[g.matrix][g.full_range];
    EncGeom k;
    k.h = g.h; k.w = g.w; k.pitch_y = g.pitch_y; k.pitch_c = g.pitch_c;
    k.off_c = g.off_c; k.off_v = g.off_v; k.frame_stride = g.frame_stride;
    k.kyr = c[0]; k.kyg = c[1]; k.kyb = c[2]; k.kur = c[3]; k.kug = c[4]; k.kub = c[5]; k.kvr = c[6]; k.kvg = c[7]; k.kvb = c[8];
    k.ybias = (1 << 19) + (g.full_range ? 0 : 16 << 20);
    const int ncg = (g.w + 15) / 16;
    const long long total = (long long)b * (g.h / 2) * ncg;
    const long long blocks = (total + 255) / 256;
    VC_CHECK(blocks <= 0x7fffffffll, VC_ERR_CAPACITY, "batch too large for one conversion launch");
    const dim3 grid((unsigned)blocks), block(256);
    if (g.nv12) {
        if (fast) hipLaunchKernelGGL((bgr_to_yuv_kernel<true, true>), grid, block, 0, s, src, dst, k, ncg, total);
        else hipLaunchKernelGGL((bgr_to_yuv_kernel<true, false>), grid, block, 0, s, src, dst, k, ncg, total);
    } else {
        if (fast) hipLaunchKernelGGL((bgr_to_yuv_kernel<false, true>), grid, block, 0, s, src, dst, k, ncg, total);
        else hipLaunchKernelGGL((bgr_to_yuv_kernel<false, false>), grid, block, 0, s, src, dst, k, ncg, total);
    }
    VC_HIP(hipGetLastError());
    return VC_OK;
}

}  // namespace vc

using namespace vc;

extern "C" {

// Parity entry point.  The caller's yuv_out goes to the device first, so the bytes that belong to no plane come back as they were:
// a kernel that wrote padding shows up in the caller's buffer.  The device buffer sits between two guard blocks that the call checks
// afterwards: a kernel that wrote outside the batch is reported instead of returning a plausible surface.
int vc_bgr_to_yuv_host(const vc_yuv_desc* d, const uint8_t* bgr, int b, int h, int w, uint8_t* yuv_out) {
    VC_CHECK(bgr && yuv_out, VC_ERR_ARG, "null argument");
    YuvGeom g;
    VC_TRY(yuv_resolve_out(d, b, h, w, g));
    const size_t in_bytes = (size_t)b * h * w * 3;
    DevScratch mem;
    uint8_t* ds = nullptr;
    GuardedOut dd;
    VC_TRY(mem.alloc(&ds, in_bytes));
    VC_TRY(dd.alloc(mem, yuv_batch_bytes(g, b), yuv_out));
    VC_HIP(hipMemcpy(ds, bgr, in_bytes, hipMemcpyHostToDevice));
    VC_TRY(launch_bgr_to_yuv(g, ds, dd.out(), b, nullptr));
    return dd.read_back(yuv_out, "bgr_to_yuv_kernel");
}

int vc_bgr_to_yuv_dev(const vc_yuv_desc* d, const void* bgr_dev, int b, int h, int w, void* yuv_dev) {
    VC_CHECK(bgr_dev && yuv_dev, VC_ERR_ARG, "null argument");
    YuvGeom g;
    VC_TRY(yuv_resolve_out(d, b, h, w, g));
    return launch_bgr_to_yuv(g, (const uint8_t*)bgr_dev, (uint8_t*)yuv_dev, b, nullptr);
}

}  // extern "C"
