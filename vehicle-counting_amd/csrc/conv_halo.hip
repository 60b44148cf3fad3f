// Halo-staged 3x3 / stride 1 / pad 1 convolution (bf16), first form: conv3x3_halo_kernel, tile configurations 28 - 31 and 36 - 39 of
// conv_cfgs.h.  Same rows of the reference as conv_igemm.hip (the 3x3 convolutions of the YOLOv5 Bottlenecks and of the DeepSORT
// appearance net's BasicBlocks); the second form is conv_halo_v2.hip.
#include "vc_common.h"
#include "conv_device.h"
#include "conv_cfgs.h"

namespace vc {

// ---- halo-staged 3x3 / stride 1 / pad 1 (bf16) ---------------------------------------------------------------------------
// The implicit GEMM (conv_igemm.hip) stages every output pixel's nine taps separately: each input line travels L2 -> LDS nine times, and
// the K loops of the 3x3 layers (93 % L2 hits) sit at half of the L2 bandwidth.  Here the K loop is turned inside out: outer
// loop over 32-channel slices, inner loop over the 9 taps.  A workgroup owns BP consecutive output pixels; per slice it stages
// the input rows those pixels touch ONCE -- rows g0-1 .. g1+1 of the flattened (batch, y) row space are contiguous in NHWC, so
// the patch is a plain run of `npix` pixels starting at pixel (g0-1)*W -- and the nine taps read their MFMA operand from that
// patch at pixel + dy*W + dx.  Taps that fall outside the image (also across the batch seam inside a patch) read a zero
// pixel instead: a 9-bit validity mask per lane, the addresses of all nine taps are loop invariant.  Weights stream through
// the same NS-stage LDS-DMA ring as there, one (tap, slice) tile of [BC][32] per step.  The MFMA / accumulation order per
// output equals the implicit GEMM's only up to the order of the K tiles (tap-major there, slice-major here): results agree
// to fp32 rounding, not bit for bit (same tolerance as between tile configurations with different K chunking... they are
// identical there; here the tests' bf16 / fp32 tolerances apply).
template <int BP, int BC, int WP, int WC, int NS, int XI>
__global__ __launch_bounds__(256, 1) void conv3x3_halo_kernel(const ConvP p) {
    constexpr int KC = 4, ES = 2, BK = 32;
    do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 8 + (0)] = wall_clock64(); } while (0);      // diagnostics (VC_CONV_DBG): phase timestamps like conv_igemm_kernel
    constexpr int PASS = 64;                       // weight rows covered by one DMA instruction of all four waves (16 per wave)
    constexpr int WI = (BC + PASS - 1) / PASS;
    constexpr int WROWS = WI * PASS;
    constexpr int WTP = BP / WP, WTC = BC / WC, PT = WTP / 16, CT = WTC / 16;
    constexpr int ZP = XI * 64 - 1;                // index of the zero pixel: last pixel of a patch buffer, never reached by a patch
    constexpr int XCH = XI * 256;                  // 16-byte chunks per patch buffer
    constexpr uint32_t OOB = 0x80000000u;
    static_assert(WP * WC == 4 && WTP % 16 == 0 && WTC % 16 == 0, "tile shape");
    static_assert((NS - 2) * WI + XI <= 63, "counted vmcnt");
    __shared__ __attribute__((aligned(16))) uint4 lds[2 * XCH + NS * WROWS * KC];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;

    const int nblk = gridDim.x;
    const int tiles_c = (p.Cout + BC - 1) / BC;
    const int tile = xcd_tile_of(blockIdx.x, nblk);
    const int m0 = (tile / tiles_c) * BP;
    const int n0 = (tile % tiles_c) * BC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int W = p.W, H = p.H;

    // patch geometry (workgroup-uniform)
    const int g0 = m0 / W;
    const int g1 = (min(m0 + BP, p.M) - 1) / W;
    const int gp0 = (g0 - 1) * W;                  // first patch pixel (may be negative: row -1 of the first image)
    const int npix = (g1 - g0 + 3) * W;            // <= ZP, checked by the launcher

    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.in), 0, (int)((size_t)p.B * p.H * p.W * p.in_cs * ES), 0x00020000);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.w), 0, (int)((size_t)((p.Cout + 127) / 128 * 128) * p.Kw * ES), 0x00020000);

    // patch staging: instruction i of this wave fills chunks [(i*4 + wave)*64, +64); lane -> (patch pixel, chunk slot)
    uint32_t xsrc[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int e = (i * 4 + wave) * 64 + lane;
        const int pp = e >> 2, cpos = e & 3;
        const int chunk = cpos ^ ((pp >> 1) & 2);                                 // source-side swizzle, see xaddr below
        const int gp = gp0 + pp;
        xsrc[i] = (pp < npix && gp >= 0) ? (uint32_t)((gp * p.in_cs + p.in_co) * ES + chunk * 16) : OOB;
    }
    // weight staging: rows of 4 chunks, 16 rows per wave-instruction (as in conv_igemm_kernel with KC = 4)
    const int prow = wave * 16 + (lane >> 2);
    const int wchunk = (lane & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
    uint32_t woff[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) woff[i] = (uint32_t)(((n0 + prow + PASS * i) * p.Kw + wchunk * 8) * ES);

    // fragment addresses: this lane's pixel of every pixel tile, its nine taps (byte offsets inside a patch buffer)
    const int wp = wave % WP, wc = wave / WP;
    const int frow = lane & 15, fch = lane >> 4;
    uint32_t xaddr[PT][9];
    {
        const float inv_w = 1.0f / (float)W, inv_h = 1.0f / (float)H;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int m = m0 + wp * WTP + i * 16 + frow;
            const bool ok = m < p.M;
            const int mm = ok ? m : m0;
            int g = (int)((float)mm * inv_w);                                     // global row, +-1 fix-up (mm < 2^24)
            g -= (g * W > mm) ? 1 : 0;
            g += ((g + 1) * W <= mm) ? 1 : 0;
            const int x = mm - g * W;
            int b = (int)((float)g * inv_h);
            b -= (b * H > g) ? 1 : 0;
            b += ((b + 1) * H <= g) ? 1 : 0;
            const int y = g - b * H;
            const int pc = mm - gp0;                                              // patch index of the centre tap
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = t / 3 - 1, dx = t % 3 - 1;
                const bool valid = ok && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
                const int px = valid ? pc + dy * W + dx : ZP;
                // chunk slot = fch ^ 2 * bit 2 of the pixel index.  The fragment reads of a tap start at an ARBITRARY patch pixel
                // (lds_slot<4>'s permutation is conflict-free only for bases that are multiples of 16: 33 % of the LDS cycles of this
                // kernel were bank conflicts); this one keeps the four lanes of a ds_read_b128 group that share pixel & 3 on four
                // different 16-byte slots for every base (exhaustive check over bases and the hardware's lane groups).
                xaddr[i][t] = (uint32_t)((px * 4 + (fch ^ ((px >> 1) & 2))) * 16);
            }
        }
    }
    int wfrag[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) wfrag[i] = 16 * lds_slot<4>(wc * WTC + i * 16 + frow, fch);

    f32x4 acc[CT][PT];
#pragma unroll
    for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mfma_inputs_settle<CT * PT>(&acc[0][0]);
    // the residual (ReID conv2 + shortcut, YOLO Bottleneck 3x3 + shortcut) is fetched NOW: this workgroup computes one tile and ends,
    // so the epilogue's residual reads had a full memory latency to themselves (64 -> 64 at 25 x 25: 0.135 ms with, 0.100 ms without)
    u32x2r rpre[PT][CT];
    // (only where the 2 * PT * CT registers it holds through the K loop do not cost a wave of occupancy)
    const bool have_res = PT * CT <= 8 && p.res_mode != RES_NONE && conv_epilogue_fast_bf16<PT, CT>(p) &&
                          ((p.act == ACT_SILU && p.res_mode == RES_AFTER_ACT) || (p.act == ACT_RELU && p.res_mode == RES_BEFORE_ACT));
    if (have_res) conv_residual_fetch<PT, CT>(p, rpre, m0 + wp * WTP, n0 + wc * WTC + fch * 4, frow);

    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)&lds[0];
    constexpr uint32_t XBYTES = XCH * 16, WSTAGE = WROWS * KC * 16;
    const uint32_t wring = lds_base + 2 * XBYTES;
    const int nslices = p.Cin / BK;
    const int nk = nslices * 9;                    // K tiles, slice-major: kt = slice * 9 + tap

    // zero pixels (one per patch buffer): plain LDS stores, ordered before the first barrier
    if (tid < 8) lds[(tid >> 2) * XCH + ZP * 4 + (tid & 3)] = make_uint4(0u, 0u, 0u, 0u);

#define VC_XSTAGE(slice, xb)                                                                                              \
    {                                                                                                                     \
        const uint32_t so = (slice) < nslices ? (uint32_t)((slice) * BK * ES) : OOB;                                       \
        _Pragma("unroll") for (int i = 0; i < XI; ++i)                                                                     \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrd, (lds_ptr_t)&lds[(xb) * XCH + (i * 4 + uwave) * 64], 16,           \
                                                     (int)((xsrc[i] | so) >= OOB ? OOB : xsrc[i] + so), 0, 0, 0);          \
    }
#define VC_WSTAGE(kt, st)                                                                                                 \
    {                                                                                                                     \
        const int kk = (kt);                                                                                               \
        const int sl = kk / 9, tp = kk - sl * 9;                                                                           \
        const uint32_t ko = kk < nk ? (uint32_t)((tp * p.Cin + sl * BK) * ES) : OOB;                                       \
        _Pragma("unroll") for (int i = 0; i < WI; ++i)                                                                     \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wsrd, (lds_ptr_t)&lds[2 * XCH + (st) * WROWS * KC + (PASS * i + uwave * 16) * KC], 16, \
                                                     (int)(ko >= OOB ? OOB : woff[i] + ko), 0, 0, 0);                       \
    }

    do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 8 + (1)] = wall_clock64(); } while (0);
    VC_XSTAGE(0, 0);
#pragma unroll
    for (int st = 0; st < NS - 1; ++st) VC_WSTAGE(st, st);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * WI) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 8 + (2)] = wall_clock64(); } while (0);
    int kt = 0, sbuf = NS - 1;
    uint32_t woffs = wring;                        // LDS address of the weight stage being multiplied
    for (int slice = 0; slice < nslices; ++slice) {
        const uint32_t xb = lds_base + (uint32_t)(slice & 1) * XBYTES;
        VC_XSTAGE(slice + 1, (slice + 1) & 1);     // next slice's patch: its buffer was last read one slice ago
#pragma unroll
        for (int t = 0; t < 9; ++t, ++kt) {
            VC_WSTAGE(kt + NS - 1, sbuf);
            sbuf = sbuf + 1 == NS ? 0 : sbuf + 1;
            u32x4v xr[PT], wr[CT];
#pragma unroll
            for (int i = 0; i < PT; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(xr[i]) : "v"(xb + xaddr[i][t]) : "memory");
#pragma unroll
            for (int i = 0; i < CT; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(wr[i]) : "v"(woffs + wfrag[i]) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < PT; ++i) asm volatile("" : "+v"(xr[i]));
#pragma unroll
            for (int i = 0; i < CT; ++i) asm volatile("" : "+v"(wr[i]));
#pragma unroll
            for (int a = 0; a < CT; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b) mfma_bf16_inplace(acc[a][b], wr[a], xr[b]);
            woffs = woffs + WSTAGE == wring + NS * WSTAGE ? wring : woffs + WSTAGE;
            // weight tile kt+1 has landed once at most the newer weight tiles -- and, while it is still older than this
            // slice's patch prefetch, that prefetch -- are outstanding
            if (t < NS - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * WI + XI) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * WI) : "memory");
            __builtin_amdgcn_s_barrier();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    mfma_results_settle<CT * PT>(&acc[0][0]);
    do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 8 + (3)] = wall_clock64(); } while (0);
#undef VC_XSTAGE
#undef VC_WSTAGE
    conv_epilogue<PT, CT, false>(p, acc, m0 + wp * WTP, n0 + wc * WTC + fch * 4, frow, rpre, have_res);
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 8 + (4)] = wall_clock64(); } while (0); }
}

template <int BP, int BC, int WP, int WC, int NS>
static int launch_halo(ConvP p, hipStream_t s) {
    if (!halo_applicable(p, BP)) return VC_ERR_ARG;                   // quietly: the autotuner skips it, launch_conv falls back
    const int tiles = ((p.M + BP - 1) / BP) * ((p.Cout + BC - 1) / BC);
    p.Kw = p.Kp;
    const int px = halo_patch_pixels(p, BP);
    if (px <= 4 * 64 - 1) launch_timed(p, conv3x3_halo_kernel<BP, BC, WP, WC, NS, 4>, dim3(tiles), dim3(256), 0, s, p);
    else if (px <= 7 * 64 - 1) launch_timed(p, conv3x3_halo_kernel<BP, BC, WP, WC, NS, 7>, dim3(tiles), dim3(256), 0, s, p);
    else launch_timed(p, conv3x3_halo_kernel<BP, BC, WP, WC, NS, 11>, dim3(tiles), dim3(256), 0, s, p);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

int launch_halo_cfg(const ConvP& p, int cfg, hipStream_t s) {
    switch (cfg) {
#define VC_Y(i, bp, bc, wp, wc, ns) case i: return launch_halo<bp, bc, wp, wc, ns>(p, s);
        VC_HALO_CFGS(VC_Y)
#undef VC_Y
    }
    return VC_ERR_ARG;
}

}  // namespace vc
