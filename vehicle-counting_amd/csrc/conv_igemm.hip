// Fused Conv2d(+folded BN bias)+activation(+residual) as an implicit GEMM on the CDNA4 matrix cores.
//
// Replaces, on the reference's hot path:
//   * every ultralytics/yolov5 v6.0 `Conv` / `Bottleneck` / `C3` / `SPPF` / `Detect.m[i]` convolution that
//     /root/reference/networks/yolo.py:70 (`self.model(inputs)`) executes, and
//   * every convolution of the DeepSORT appearance net, /root/reference/networks/deepsort/deep/model.py:5-98
//     (row B5; ReLU / residual-before-ReLU epilogues).
//
// Layout: activations NHWC (channel-sliced views: a buffer may be a slice [co, co+C) of a wider
// concat buffer with channel stride cs, which is how Concat costs nothing), weights [Cout][K] with
// K = (r, s, c) so that a 16-byte chunk of the im2col row is one contiguous NHWC read.
// GEMM orientation: D[channel][pixel] += W[channel][k] * X[pixel][k]; the MFMA "A" operand is the
// weight tile, "B" the im2col pixel tile, so each lane ends up with 4 consecutive output channels
// of one pixel -> one 8-byte (bf16) / 16-byte (f32) NHWC store per 16x16 tile.
//
// bf16 path : v_mfma_f32_16x16x32_bf16, fp32 accumulate, one RNE rounding on store.
// fp32 path : v_mfma_f32_16x16x4_f32 (exact fmaf chain) -- the tight-parity mode (SURVEY.md 8d ladder).
//
// This file: the implicit-GEMM family (conv_igemm_kernel, its split-K form and their launchers).  The halo-staged 3x3 kernels are in
// conv_halo.hip, conv_halo_v2.hip and conv_halo_s2.hip, the weight-stationary 1x1 kernels in conv_pointwise.hip; the table of tile
// configurations is conv_cfgs.h, the dispatch conv_dispatch.hip.
#include <algorithm>
#include <map>
#include <mutex>
#include <cstdlib>

#include "vc_common.h"
#include "conv_device.h"
#include "conv_cfgs.h"
#include "conv_launch.h"

namespace vc {

// BP x BC output tile (pixels x channels) per workgroup of WP x WC wavefronts; KC 16-byte chunks of K per tile row.
//
// Staging: both operands go global -> LDS with `buffer_load_dwordx4 ... lds` (LDS-DMA: no VGPR round trip, no ds_write).
// One wave-instruction writes 64 lanes x 16 B = 1 KiB lane-linearly, i.e. 64/KC consecutive tile rows, so the
// bank-conflict swizzle is applied on the SOURCE side: lane (row, c) fetches logical chunk c ^ swz(row)
// (cdna_hip_programming.md rule 21).  Padding / tile-edge / K-padding taps become out-of-range buffer offsets that the
// hardware answers with zeros (verified by the padded test cases); the per-row validity of all kh*kw taps is one 64-bit
// mask computed once, the tap offset advances incrementally, every LDS address is loop invariant: the K loop is
// {KC/4 x (PT+CT ds_read_b128, PT*CT MFMA)} + (XI+WI) DMA issues + one barrier.
// UP: the first p.up_C input channels of a pointwise conv come from a tensor of half the height and width, nearest-upsampled on the fly
// (nn.Upsample(None, 2, 'nearest') + Concat in front of C3.cv1 | cv2, YOLOv5 layers 11-13 and 15-17): the staged row of output pixel
// (b, y, x) reads pixel (b, y / 2, x / 2) of p.in_up for K tiles below up_C and the concat buffer for the rest, so the upsampled map
// is neither written nor read.  Same values in the same K order: bit-identical to upsample2x_kernel + this kernel.
// SK (round 6, bf16): deterministic split-K for launches with too few output tiles to fill the chip (batch 1 .. 8: 16 workgroups walking
// 72 K steps).  A work item is (output tile, K split s of p.ksplit): it multiplies K tiles [s nk / KS, (s + 1) nk / KS), stores its fp32
// accumulators to p.sk_ws and takes a ticket of its tile; the workgroup that draws the LAST ticket adds the KS partial sums in split
// order 0 .. KS - 1 (whichever workgroup arrives last: the same sum) and runs the epilogue.  No workgroup waits for another one.
// OCC (round 6, configurations 64 - 66): workgroups per CU the register allocation is bounded for.  Two 8-wave workgroups on one CU share no
// barrier: while one is in its epilogue (SiLU + stores, no loads issued, no MFMA) the other is in its K loop -- the phases a single 16-wave
// workgroup runs one after the other overlap across the pair.  (HIP: the second launch-bound is WAVES per SIMD, hence OCC * waves / 4.)
template <int BP, int BC, int WP, int WC, int KC, int NS, int PR, bool UP = false, bool SK = false, int OCC = 1>       // PR: PREC_BF16, PREC_F32 or PREC_FP8
__global__ __launch_bounds__(WP * WC * 64, OCC == 1 ? 1 : OCC * WP * WC / 4) void conv_igemm_kernel(const ConvP p_arg) {
    ConvP p = p_arg;
    if (p_arg.m_dev) {                        // device-side problem size (uniform): fewer pixels, fewer tiles
        const int mm = min(p_arg.M, *p_arg.m_dev);
        p.M = mm;
        p.ntiles = ((mm + BP - 1) / BP) * ((p_arg.Cout + BC - 1) / BC);
    }
    constexpr bool F32 = PR == PREC_F32, FP8 = PR == PREC_FP8;
    constexpr int ES = F32 ? 4 : FP8 ? 1 : 2; // element size
    static_assert(!FP8 || KC == 8, "fp8: one 128-byte LDS row = one K = 128 MX-scaled MFMA step");
    constexpr int CH = 16 / ES;               // elements per 16-byte chunk
    constexpr int BK = KC * CH;               // K elements per tile
    constexpr int RPI = 64 / KC;              // tile rows covered by one wave-instruction
    constexpr int NW = WP * WC;               // waves per workgroup: 4, or 8 / 16 for the 256-row tiles (configs 40-43)
    constexpr int PASS = NW * RPI;            // tile rows covered by one instruction of all waves
    constexpr int XI = BP / PASS;             // DMA instructions per thread for the pixel tile
    constexpr int WI = (BC + PASS - 1) / PASS;
    constexpr int WTP = BP / WP, WTC = BC / WC;
    constexpr int PT = WTP / 16, CT = WTC / 16;
    constexpr uint32_t OOB = 0x80000000u;     // beyond every descriptor's num_records -> the load returns 0
    static_assert(NW == 4 || NW == 8 || NW == 16, "waves per workgroup");
    static_assert(BP % PASS == 0 && BC % RPI == 0 && WTP % 16 == 0 && WTC % 16 == 0, "tile shape");
    constexpr int ROWS = BP + WI * PASS;       // rows of one stage: every wave issues the same XI + WI DMA instructions per tile
    constexpr int PER = XI + WI;
    static_assert(KC == 4 || KC == 8, "K tile");
    static_assert(NS >= 2 && (NS - 2) * PER <= 63, "ring depth: the counted s_waitcnt must fit vmcnt");

    __shared__ __attribute__((aligned(16))) uint4 lds[NS][ROWS * KC];
    if (p.ablate == 6) return;                                 // launch floor (diagnostics)
#define VC_TS(i) do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
    VC_TS(0);

    // Persistent workgroups: the grid is min(tiles, resident workgroups); workgroup b walks the tiles of the virtual blocks
    // b, b + G, b + 2G, ...  The K-tile ring runs THROUGH the tile boundaries -- while a tile's epilogue (bias, SiLU, stores)
    // executes, the first NS-1 K tiles of the next output tile are already in flight -- so the per-tile prologue arithmetic,
    // the first-tile latency and the store tail overlap with useful work instead of being paid serially by a fresh
    // workgroup per tile.
    // XCD-aware tile order: the dispatcher places block b on XCD b % 8 (G is a multiple of 8, so all virtual blocks of a
    // workgroup share its XCD); each XCD gets a contiguous range of tiles so the channel tiles that share one pixel tile
    // hit the same private L2.
    const int ntiles = p.ntiles, G = gridDim.x;
    const int KS = SK ? p.ksplit : 1;         // (uniform)
    const int nitems = ntiles * KS;
    const int tiles_c = (p.Cout + BC - 1) / BC;
    const int tq = ntiles >> 3, tr = ntiles & 7;
#define VC_TILE_OF(v) ((((v) & 7) < tr ? ((v) & 7) * (tq + 1) : tr * (tq + 1) + (((v) & 7) - tr) * tq) + ((v) >> 3))

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int prow = wave * RPI + lane / KC;                 // this thread's row inside a PASS-row slab
    const int cpos = lane % KC;                              // physical chunk slot it fills
    const int kc0 = KC == 4 ? (cpos ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3)) : (cpos ^ (prow & 7));   // logical chunk
    const int HoWo = p.Ho * p.Wo;

    // descriptors: whole input buffer / whole packed weight buffer (sizes < 2 GiB, checked by the launcher)
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.in), 0, (int)((size_t)p.B * p.H * p.W * p.in_cs * ES), 0x00020000);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.w), 0, (int)((size_t)((p.Cout + 127) / 128 * 128) * p.Kw * ES), 0x00020000);

    const float inv_howo = 1.0f / (float)HoWo, inv_wo = 1.0f / (float)p.Wo;
    const bool pointwise = p.kh == 1 && p.kw == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0;    // uniform
    const uint32_t tap_x = (uint32_t)(p.in_cs * ES), tap_y = (uint32_t)((p.W - p.kw + 1) * p.in_cs * ES);
    // When Cin is a multiple of the K tile (every layer but the stems) a K tile lies inside ONE tap, the same for every
    // lane: the tap walk is then scalar state (SALU) instead of a divergent per-lane loop.
    const bool ut = (p.Cin % BK) == 0;

    // ---- state of the tile being STAGED (it runs up to NS-1 K tiles ahead of the tile being multiplied) ----------------
    // per staged pixel row: byte offset of its (iy0, ix0) corner and the validity mask of the kh*kw taps; quotients come from
    // an exact float reciprocal with a +-1 fix-up, the mask from row/column ranges (no run-time integer divisions)
    uint32_t xoff[XI], xoffl[XI], woff[WI];
    uint32_t xoffu[UP ? XI : 1];              // UP: this lane's chunk in the half-size source
    const __amdgpu_buffer_rsrc_t usrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(UP ? p.in_up : p.in), 0, UP ? (int)((size_t)p.B * (p.H / 2) * (p.W / 2) * p.up_cs * ES) : 0, 0x00020000);
    unsigned long long xmask[XI];
    int kc_c = 0, kc_t = 0, kc_s = 0, u_tap = 0, u_s = 0, u_c = 0;
    uint32_t kc_off = 0, u_tapoff = 0;
    int s_v = blockIdx.x, s_kt = 0, s_kt1 = 0, s_issued = 0;
    const int nk = p.Kp / BK;
#define VC_TILE_STATE(v)                                                                                                  \
    if ((v) < nitems) {                                                                                                   \
        const int tile_ = VC_TILE_OF(SK ? (v) / KS : (v));                                                                \
        const int sp_ = SK ? (v) % KS : 0;                                                                                \
        s_kt = SK ? sp_ * nk / KS : 0;                                                                                    \
        s_kt1 = SK ? (sp_ + 1) * nk / KS : nk;                                                                            \
        const int kst_ = s_kt * BK;           /* first K element of this item */                                           \
        const int sm0 = (tile_ / tiles_c) * BP, sn0 = (tile_ % tiles_c) * BC;                                              \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                                                  \
            const int m = sm0 + prow + PASS * i;                                                                          \
            const bool ok = m < p.M;                                                                                      \
            const int mm = ok ? m : 0;                                                                                    \
            if (pointwise) {                  /* 1x1 / stride 1: output pixel m reads input pixel m, one tap */            \
                xoff[i] = (uint32_t)((mm * p.in_cs + p.in_co) * ES);                                                      \
                xmask[i] = ok ? 1ull : 0ull;                                                                              \
                if constexpr (UP) {                                                                                       \
                    int b = (int)((float)mm * inv_howo);                                                                  \
                    b -= (b * HoWo > mm) ? 1 : 0;                                                                         \
                    b += ((b + 1) * HoWo <= mm) ? 1 : 0;                                                                  \
                    const int rem = mm - b * HoWo;                                                                        \
                    int oy = (int)((float)rem * inv_wo);                                                                  \
                    oy -= (oy * p.Wo > rem) ? 1 : 0;                                                                      \
                    oy += ((oy + 1) * p.Wo <= rem) ? 1 : 0;                                                               \
                    const int ox = rem - oy * p.Wo;                                                                       \
                    xoffu[i] = (uint32_t)((((b * (p.H / 2) + (oy >> 1)) * (p.W / 2) + (ox >> 1)) * p.up_cs + p.up_co + kc0 * CH) * ES); \
                }                                                                                                         \
            } else {                                                                                                      \
                int b = (int)((float)mm * inv_howo);    /* mm < 2^24: the float product is within 1 of the quotient */     \
                b -= (b * HoWo > mm) ? 1 : 0;                                                                             \
                b += ((b + 1) * HoWo <= mm) ? 1 : 0;                                                                      \
                const int rem = mm - b * HoWo;                                                                            \
                int oy = (int)((float)rem * inv_wo);                                                                      \
                oy -= (oy * p.Wo > rem) ? 1 : 0;                                                                          \
                oy += ((oy + 1) * p.Wo <= rem) ? 1 : 0;                                                                   \
                const int ox = rem - oy * p.Wo;                                                                           \
                const int iy0 = oy * p.sh - p.ph, ix0 = ox * p.sw - p.pw;                                                 \
                xoff[i] = (uint32_t)((((b * p.H + iy0) * p.W + ix0) * p.in_cs + p.in_co) * ES);                           \
                const int r_lo = max(0, -iy0), r_hi = min(p.kh, p.H - iy0);                                               \
                const int s_lo = max(0, -ix0), s_hi = min(p.kw, p.W - ix0);                                               \
                unsigned long long mk = 0;                                                                                \
                if (ok && s_hi > s_lo) {                                                                                  \
                    const unsigned long long rowbits = ((1ull << (s_hi - s_lo)) - 1ull) << s_lo;                          \
                    for (int r = r_lo; r < r_hi; ++r) mk |= rowbits << (r * p.kw);                                        \
                }                                                                                                         \
                xmask[i] = mk;                                                                                            \
            }                                                                                                             \
            xoffl[i] = xoff[i] + (uint32_t)(kc0 * CH * ES);                                                               \
        }                                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < WI; ++i) woff[i] = (uint32_t)(((sn0 + prow + PASS * i) * p.Kw + kc0 * CH) * ES); \
        {   /* (tap, c) of this thread's chunk and the tap's byte offset (r*W + s)*in_cs*ES, advanced by BK per K step */   \
            const int k = kst_ + kc0 * CH;                                                                                \
            const int tap = k / p.Cin;                                                                                    \
            const int r = tap / p.kw;                                                                                     \
            kc_c = k - tap * p.Cin;                                                                                       \
            kc_t = tap;                                                                                                   \
            kc_s = tap - r * p.kw;                                                                                        \
            kc_off = (uint32_t)((r * p.W + kc_s) * p.in_cs * ES);                                                         \
        }                                                                                                                 \
        u_tap = 0; u_s = 0; u_c = 0; u_tapoff = 0;                                                                        \
        if (SK && kst_ > 0) {                 /* (uniform) the scalar tap walk starts inside the K range */                \
            const int tap = kst_ / p.Cin, r = tap / p.kw;                                                                 \
            u_c = kst_ - tap * p.Cin;                                                                                     \
            u_tap = min(tap, 63);                                                                                         \
            u_s = tap - r * p.kw;                                                                                         \
            u_tapoff = (uint32_t)((r * p.W + u_s) * p.in_cs * ES);                                                        \
        }                                                                                                                 \
    } else {                                  /* no tile left: everything staged from here on is out of range (zeros) */   \
        s_kt = 0; s_kt1 = nk;                                                                                             \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) { xmask[i] = 0ull; xoff[i] = 0; xoffl[i] = 0; }                    \
        _Pragma("unroll") for (int i = 0; i < WI; ++i) woff[i] = OOB;                                                     \
        kc_c = 0; kc_t = 0; kc_s = 0; kc_off = 0; u_tap = 0; u_s = 0; u_c = 0; u_tapoff = 0;                              \
    }

    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    // stage K tile s_kt of the staged tile into ring slot `buf`, then advance (to the next tile of this workgroup at the end)
#define VC_STAGE_NEXT(buf)                                                                                               \
    if ((p.ablate == 1 || p.ablate == 3) && s_issued >= NS) {                                                                               \
    } else if (ut) {                                                                                                            \
        const uint32_t so = u_tapoff + (uint32_t)(u_c * ES);                                                             \
        const bool from_up = UP && u_c < p.up_C;      /* (uniform) this K tile lies in the upsampled half of the concat */   \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                                                 \
            const uint32_t o = ((xmask[i] >> u_tap) & 1ull) ? (from_up ? xoffu[UP ? i : 0] : xoffl[i]) + so : OOB;        \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(from_up ? usrd : xsrd, (lds_ptr_t)&lds[buf][(PASS * i + uwave * RPI) * KC], 16, (int)o, 0, 0, 0); \
        }                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < WI; ++i) {                                                                 \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wsrd, (lds_ptr_t)&lds[buf][BP * KC + (PASS * i + uwave * RPI) * KC], 16,     \
                                                     (int)(woff[i] + (uint32_t)(s_kt * BK * ES)), 0, 0, 0);             \
        }                                                                                                                \
        u_c += BK;                                                                                                       \
        if (u_c == p.Cin) {                                                                                              \
            u_c = 0;                                                                                                     \
            u_tap = min(u_tap + 1, 63);                                                                                  \
            if (++u_s == p.kw) { u_s = 0; u_tapoff += tap_y; } else { u_tapoff += tap_x; }                               \
        }                                                                                                                \
    } else {                                                                                                             \
        const uint32_t tc = kc_off + (uint32_t)(kc_c * ES);                                                              \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                                                 \
            const uint32_t o = ((xmask[i] >> min(kc_t, 63)) & 1ull) ? xoff[i] + tc : OOB;                                \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrd, (lds_ptr_t)&lds[buf][(PASS * i + uwave * RPI) * KC], 16, (int)o, 0, 0, 0); \
        }                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < WI; ++i) {                                                                 \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wsrd, (lds_ptr_t)&lds[buf][BP * KC + (PASS * i + uwave * RPI) * KC], 16,     \
                                                     (int)(woff[i] + (uint32_t)(s_kt * BK * ES)), 0, 0, 0);             \
        }                                                                                                                \
        int cc = kc_c + BK;                                                                                              \
        while (cc >= p.Cin) {                                                                                            \
            cc -= p.Cin;                                                                                                 \
            ++kc_t;                                                                                                      \
            if (++kc_s == p.kw) { kc_s = 0; kc_off += tap_y; } else { kc_off += tap_x; }                                 \
        }                                                                                                                \
        kc_c = cc;                                                                                                       \
    }                                                                                                                    \
    ++s_issued;                                                                                                          \
    if (++s_kt == s_kt1) {                                                                                               \
        s_v += G;                                                                                                        \
        VC_TILE_STATE(s_v);                                                                                              \
    }

    VC_TILE_STATE(s_v);

    const int wp = wave % WP, wc = wave / WP;
    const int frow = lane & 15, fch = lane >> 4;
    int xfrag[KC / 4][PT], wfrag[KC / 4][CT];
#pragma unroll
    for (int h = 0; h < KC / 4; ++h) {
#pragma unroll
        for (int i = 0; i < PT; ++i) xfrag[h][i] = 16 * lds_slot<KC>(wp * WTP + i * 16 + frow, h * 4 + fch);          // byte offsets in a stage
#pragma unroll
        for (int i = 0; i < CT; ++i) wfrag[h][i] = 16 * (BP * KC + lds_slot<KC>(wc * WTC + i * 16 + frow, h * 4 + fch));
    }

    // NS-stage ring: K tiles g+1 .. g+NS-1 of this workgroup's tile sequence are in flight while K tile g is multiplied.
    // LDS-DMA loads return in order, so "the next K tile has landed" is vmcnt <= (NS-2) * PER (the epilogue's loads and stores
    // also sit on the VM counter: they can only make this wait longer, never shorter than needed -- loads complete in order).
    //
    // The fragment reads are inline asm and the barrier is the raw s_barrier: hipcc counts an LDS-DMA as a pending LDS
    // write and puts `s_waitcnt vmcnt(0)` in front of every ds_read (and inside __syncthreads) it can see, which drains
    // the tile that was just issued and serialises DMA and MFMA.  The waits that are needed are written out below.
    VC_TS(1);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)&lds[0][0];
    constexpr uint32_t STAGE_BYTES = ROWS * KC * 16;
#pragma unroll
    for (int st = 0; st < NS - 1; ++st) { VC_STAGE_NEXT(st); }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * PER) : "memory");
    __builtin_amdgcn_s_barrier();
    VC_TS(2);
    int sbuf = NS - 1;
    uint32_t boff = lds_base;
    for (int v = blockIdx.x; v < nitems; v += G) {
        const int tile = VC_TILE_OF(SK ? v / KS : v);
        const int split = SK ? v % KS : 0;
        const int nk_item = SK ? (split + 1) * nk / KS - split * nk / KS : nk;
        const int m0 = (tile / tiles_c) * BP, n0 = (tile % tiles_c) * BC;
        f32x4 acc[CT][PT];
#pragma unroll
        for (int a = 0; a < CT; ++a)
#pragma unroll
            for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk_item; ++kt) {
            VC_STAGE_NEXT(sbuf);                        // into the slot consumed last iteration (all waves passed its barrier)
            sbuf = sbuf + 1 == NS ? 0 : sbuf + 1;
            if constexpr (FP8) {
                // MX-scaled fp8 MFMA, K = 128 per instruction (twice the bf16 rate): a lane's 32 K-bytes are the chunks fch and 4 + fch of
                // its LDS row -- the same two ds_read_b128 the bf16 halves issue; any K assignment works as long as both operands use
                // the same one.  Block scales are 1 (E8M0 0x7f): per-channel weight scales are applied in the epilogue.
                u32x4v xr[2][PT], wr[2][CT];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int i = 0; i < PT; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(xr[h][i]) : "v"(boff + xfrag[h][i]) : "memory");
#pragma unroll
                    for (int i = 0; i < CT; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(wr[h][i]) : "v"(boff + wfrag[h][i]) : "memory");
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                typedef int i32x8 __attribute__((ext_vector_type(8)));
                i32x8 xa[PT], wa[CT];
#pragma unroll
                for (int i = 0; i < PT; ++i) {
                    asm volatile("" : "+v"(xr[0][i])); asm volatile("" : "+v"(xr[1][i]));
                    xa[i] = (i32x8){(int)xr[0][i].x, (int)xr[0][i].y, (int)xr[0][i].z, (int)xr[0][i].w, (int)xr[1][i].x, (int)xr[1][i].y, (int)xr[1][i].z, (int)xr[1][i].w};
                }
#pragma unroll
                for (int i = 0; i < CT; ++i) {
                    asm volatile("" : "+v"(wr[0][i])); asm volatile("" : "+v"(wr[1][i]));
                    wa[i] = (i32x8){(int)wr[0][i].x, (int)wr[0][i].y, (int)wr[0][i].z, (int)wr[0][i].w, (int)wr[1][i].x, (int)wr[1][i].y, (int)wr[1][i].z, (int)wr[1][i].w};
                }
#pragma unroll
                for (int a = 0; a < CT; ++a)
#pragma unroll
                    for (int b = 0; b < PT; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa[a], xa[b], acc[a][b], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
            } else
#pragma unroll
            for (int h = 0; h < KC / 4; ++h) {
                u32x4v xr[PT], wr[CT];
#pragma unroll
                for (int i = 0; i < PT; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(xr[i]) : "v"(boff + xfrag[h][i]) : "memory");
#pragma unroll
                for (int i = 0; i < CT; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(wr[i]) : "v"(boff + wfrag[h][i]) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                Chunk xa[PT], wa[CT];
#pragma unroll
                for (int i = 0; i < PT; ++i) { asm volatile("" : "+v"(xr[i])); xa[i].u = xr[i]; }      // the MFMAs below depend on the wait above
#pragma unroll
                for (int i = 0; i < CT; ++i) { asm volatile("" : "+v"(wr[i])); wa[i].u = wr[i]; }
#pragma unroll
                for (int a = 0; a < CT; ++a)
#pragma unroll
                    for (int b = 0; b < PT; ++b) {
                        if constexpr (F32) {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[a].f[j], xa[b].f[j], acc[a][b], 0, 0, 0);
                        } else {
                            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[a].h, xa[b].h, acc[a][b], 0, 0, 0);
                        }
                    }
            }
            boff = boff + STAGE_BYTES == lds_base + NS * STAGE_BYTES ? lds_base : boff + STAGE_BYTES;
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * PER) : "memory");
            __builtin_amdgcn_s_barrier();
        }
        if constexpr (SK) {
            // Partial sums out, ticket, and for the last arrival: all KS partial sums back in split order.  The hand-over crosses XCDs (each
            // has its own L2), but a release / acquire FENCE at agent scope writes back and invalidates a whole L2 (measured: the split
            // launches ran 3 - 8 x slower than the unsplit ones).  Instead the partial sums themselves travel with agent-scope atomic
            // stores / loads (sc1: write-through / cache-bypassing dword accesses), ordered against the ticket by the VM counter.
            constexpr int NT = NW * 64;
            float* ws = p.sk_ws + (size_t)tile * KS * (CT * PT * NT * 4);
            float* mine = ws + (size_t)split * (CT * PT * NT * 4);
#pragma unroll
            for (int a = 0; a < CT; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) __hip_atomic_store(mine + (((a * PT + b) * 4 + j) * NT + tid), acc[a][b][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this thread's partial sums have reached memory
            __shared__ int sk_ticket;
            __syncthreads();                                      // ... and every other thread's of the workgroup
            if (tid == 0) sk_ticket = __hip_atomic_fetch_add(p.sk_tickets + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const bool last = sk_ticket == KS - 1;        // (uniform)
            if (!last) continue;
            if (tid == 0) __hip_atomic_store(p.sk_tickets + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the tickets are zero again when the launch ends
#pragma unroll
            for (int a = 0; a < CT; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // four splits' partial sums are requested together (64 - 128 loads in flight per lane: one memory latency per group instead of one per
            // split -- the reads were the larger half of a split launch's time), then added in split order; a split past KS reads split
            // KS - 1 again and is not added
            for (int s0 = 0; s0 < KS; s0 += 4) {
                float v[4][CT * PT * 4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float* part = ws + (size_t)min(s0 + u, KS - 1) * (CT * PT * NT * 4);
#pragma unroll
                    for (int i = 0; i < CT * PT * 4; ++i) v[u][i] = __hip_atomic_load(part + (i * NT + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool on = s0 + u < KS;              // (uniform)
#pragma unroll
                    for (int a = 0; a < CT; ++a)
#pragma unroll
                        for (int b = 0; b < PT; ++b)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[a][b][j] = on ? acc[a][b][j] + v[u][(a * PT + b) * 4 + j] : acc[a][b][j];
                }
            }
        }
        // epilogue: D[channel = (lane>>4)*4 + reg][pixel = lane&15]; the next tile's first K tiles are already in flight
        if constexpr (FP8) conv_epilogue_fp8<PT, CT>(p, acc, m0 + wp * WTP, n0 + wc * WTC + fch * 4, frow);
        else conv_epilogue<PT, CT, F32>(p, acc, m0 + wp * WTP, n0 + wc * WTC + fch * 4, frow);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // drain the K tiles issued past the last tile before the LDS is released
    VC_TS(3);
    if (p.dbg) { VC_TS(4); }
#undef VC_STAGE_NEXT
#undef VC_TILE_STATE
#undef VC_TILE_OF
#undef VC_TS
}

// One implicit-GEMM launch: the resident-workgroup count of this kernel instantiation (queried once), the persistent grid, the launch.
template <auto KERNEL, int THREADS>
static void launch_persistent(const ConvP& p, hipStream_t s) {
    const ConvSwitches& sw = conv_switches();
    static const int slots_hw = resident_workgroups(KERNEL, THREADS);
    // p.slots: tests force long tile walks; VC_CONV_DYN_LDS (diagnostics) caps workgroups per CU
    const int grid = (sw.persist && !sw.dyn_lds) ? persistent_grid(p.ntiles, slots_hw, sw.reserve, p.slots, sw.balanced) : p.ntiles;
    launch_timed(p, KERNEL, dim3(grid), dim3(THREADS), sw.dyn_lds, s, p);
}

template <int BP, int BC, int WP, int WC, int KC, int NS, int OCC = 1>
static int launch_one(ConvP p, hipStream_t s) {
    if (OCC != 1 && (p.prec != PREC_BF16 || p.in_up)) return VC_ERR_ARG;      // quietly: the paired-workgroup tiles exist for plain bf16 only
    const int tiles = ((p.M + BP - 1) / BP) * ((p.Cout + BC - 1) / BC);
    const int bk = KC * (p.prec == PREC_F32 ? 4 : p.prec == PREC_FP8 ? 16 : 8);
    p.Kw = p.Kp;                              // weight row stride as packed
    p.Kp = (p.K + bk - 1) / bk * bk;          // K-loop extent: only the tiles that hold real taps
    p.ntiles = tiles;
    constexpr int NT = WP * WC * 64;
    if (p.in_up && p.prec != PREC_BF16) return VC_ERR_ARG;        // (conv_check refuses it with a message)
    bool handled = false;
    if constexpr (OCC == 1) {
    handled = p.prec == PREC_F32 || p.prec == PREC_FP8 || p.in_up;
    if (p.prec == PREC_F32) {
        launch_persistent<conv_igemm_kernel<BP, BC, WP, WC, KC, 2, PREC_F32>, NT>(p, s);
    } else if (p.prec == PREC_FP8) {
        if constexpr (KC == 8 && (BP / WP / 16) % 2 == 0) {        // the fp8 epilogue pairs pixel tiles (PT even)
            launch_persistent<conv_igemm_kernel<BP, BC, WP, WC, KC, NS, PREC_FP8>, NT>(p, s);
        } else {
            return VC_ERR_ARG;                                       // quietly: the autotuner skips it (fp8 runs on the 128-byte-row tiles only)
        }
    } else if (p.in_up) {
        // the upsample fold-in is instantiated for the tiles the wide pointwise layers use (256 x 256 on 16 waves, 128 / 256 x 128 on 2 x 2)
        constexpr bool UP_OK = (BP == 256 && BC == 256 && KC == 4 && NS <= 4) ||
                               (WP == 2 && WC == 2 && BC == 128 && (BP == 128 || BP == 256) && (KC == 8 || (KC == 4 && NS == 2 && BP == 128)));
        if constexpr (UP_OK) {
            launch_persistent<conv_igemm_kernel<BP, BC, WP, WC, KC, NS, PREC_BF16, true>, NT>(p, s);
        } else {
            return VC_ERR_ARG;                                       // quietly: the autotuner skips it
        }
    }
    }
    if (!handled) launch_persistent<conv_igemm_kernel<BP, BC, WP, WC, KC, NS, PREC_BF16, false, false, OCC>, NT>(p, s);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// Split-K workspace: fp32 partial sums + one ticket per output tile, one set per stream (launches of one stream are ordered; the detector's and
// the ReID net's streams run side by side).  Tickets are zeroed once: the kernel leaves them at zero.
struct SkWorkspace { float* ws = nullptr; int* tickets = nullptr; };
static constexpr size_t SK_WS_BYTES = 32u << 20;
static constexpr int SK_MAX_TILES = 16384;
static int sk_workspace(hipStream_t s, SkWorkspace* out) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, SkWorkspace> table;
    int dev = 0;
    VC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    SkWorkspace& w = table[{dev, s}];
    if (!w.ws) {
        if (conv_switches().sk_uncached) {       // memory no XCD's L2 keeps a copy of: the hand-over between workgroups of different XCDs cannot meet a stale line
            VC_HIP(hipExtMallocWithFlags((void**)&w.ws, SK_WS_BYTES, hipDeviceMallocUncached));
            VC_HIP(hipExtMallocWithFlags((void**)&w.tickets, sizeof(int) * SK_MAX_TILES, hipDeviceMallocUncached));
        } else {
            VC_HIP(hipMalloc((void**)&w.ws, SK_WS_BYTES));
            VC_HIP(hipMalloc((void**)&w.tickets, sizeof(int) * SK_MAX_TILES));
        }
        VC_HIP(hipMemset(w.tickets, 0, sizeof(int) * SK_MAX_TILES));
    }
    *out = w;
    return VC_OK;
}

template <int BP, int BC, int WP, int WC, int KC, int NS>
static int launch_one_sk(ConvP p, hipStream_t s) {
    if (!conv_switches().sk || p.prec != PREC_BF16 || p.in_up || p.m_dev) return VC_ERR_ARG;      // quietly: the autotuner skips it
    const int tiles = ((p.M + BP - 1) / BP) * ((p.Cout + BC - 1) / BC);
    const int bk = KC * 8;
    p.Kw = p.Kp;
    p.Kp = (p.K + bk - 1) / bk * bk;
    p.ntiles = tiles;
    const int nk = p.Kp / bk;
    static const int slots_hw = resident_workgroups(conv_igemm_kernel<BP, BC, WP, WC, KC, NS, PREC_BF16, false, true>, WP * WC * 64);
    // worth it only when the tiles leave most of the chip idle and every split still walks a few K tiles
    constexpr size_t item_bytes = (size_t)BP * BC * 4;
    // (measured, tools/sk_time.py: a K step of a 64 x 64 tile costs ~0.43 us -- LDS-DMA issue, not latency: rings of 6 / 8 stages, configurations
    // 60 - 63, change nothing -- a launch ~6 us whatever its size, and the last arrival reads the KS partial sums one memory latency after the
    // other: splits of at least four K steps, at most eight of them)
    int ks = std::min(std::min(slots_hw / std::max(tiles, 1), nk / 4), 8);
    ks = std::min<long>(ks, (long)(SK_WS_BYTES / (item_bytes * (size_t)std::max(tiles, 1))));
    if (ks < 2 || tiles > SK_MAX_TILES) return VC_ERR_ARG;
    SkWorkspace w;
    VC_TRY(sk_workspace(s, &w));
    p.ksplit = ks; p.sk_ws = w.ws; p.sk_tickets = w.tickets;
    launch_timed(p, conv_igemm_kernel<BP, BC, WP, WC, KC, NS, PREC_BF16, false, true>, dim3(tiles * ks), dim3(WP * WC * 64), 0, s, p);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

int launch_igemm_cfg(const ConvP& p, int cfg, hipStream_t s) {
    switch (cfg) {
#define VC_X(i, bp, bc, wp, wc, kc, ns) case i: return launch_one<bp, bc, wp, wc, kc, ns>(p, s);
        VC_CONV_CFGS(VC_X)
        VC_CONV_BIG_CFGS(VC_X)
        VC_CONV_DEEP_CFGS(VC_X)
#undef VC_X
#define VC_K(i, bp, bc, wp, wc, kc, ns) case i: return launch_one_sk<bp, bc, wp, wc, kc, ns>(p, s);
        VC_SK_CFGS(VC_K)
#undef VC_K
#define VC_P(i, bp, bc, wp, wc, kc, ns) case i: return launch_one<bp, bc, wp, wc, kc, ns, 2>(p, s);
        VC_PAIR_CFGS(VC_P)
        VC_PAIR4_CFGS(VC_P)
#undef VC_P
    }
    return VC_ERR_ARG;
}

}  // namespace vc
