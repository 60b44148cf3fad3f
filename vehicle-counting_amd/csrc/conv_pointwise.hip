// Weight-stationary 1x1 / stride 1 convolutions: conv1x1_direct_kernel (weights in registers, bf16: tile configurations 32 - 35 of
// conv_cfgs.h), conv1x1_direct_fp8_kernel (69 - 72), conv1x1_stream_kernel (weights in LDS, 50 - 54) and conv1x1_wreg_kernel (weights in
// registers, pixels through an LDS ring, epilogue under the next tile: 73 - 78).  The pointwise layers of the YOLOv5 C3 blocks; all four
// are bit-identical to conv_igemm_kernel on the shapes they take.
#include <algorithm>
#include <cstdlib>

#include "vc_common.h"
#include "conv_device.h"
#include "conv_cfgs.h"
#include "conv_launch.h"

namespace vc {

// ---- 1x1 / stride 1 with the weights in registers (bf16) -------------------------------------------------------------------
// The narrow pointwise layers (K <= 128) are bound by everything but the matrix work: two K tiles per output tile, each with its
// DMA issue, vmcnt wait and workgroup barrier, around 16 MFMAs.  With K*N this small a wave can keep its share of the weight
// matrix in registers (CT x KS fragments = 32 / 64 VGPRs) for the whole launch and read its MFMA "B" operand -- lane (pixel,
// 16-byte chunk of the pixel's channel run) -- straight from global memory: no LDS, no barrier, waves fully independent, the
// next pixel block's fragments are fetched before this block's MFMAs and epilogue.  A wave owns one channel group of CT*16
// outputs (NG = Cout / (CT*16) groups, 1, 2 or 4) and walks pixel blocks of PT*16 pixels; the NG waves that share a pixel block
// run side by side in one workgroup (the second to fourth read of a pixel hits L2/L1).  K order, MFMA operand order and the
// epilogue are those of conv_igemm_kernel: bit-identical results.
template <int CT, int KS, int PT, int OCC, int ACT>     // OCC = waves per SIMD the register budget is sized for
__global__ __launch_bounds__(256, OCC) void conv1x1_direct_kernel(const ConvP p) {
    constexpr uint32_t OOB = 0x80000000u;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frow = lane & 15, fch = lane >> 4;
    const int NG = p.Cout / (CT * 16);
    const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;           // 4 % NG == 0: a workgroup holds whole sets of groups
    const int g = gw % NG, stride = nw / NG;
    const int nblk = (p.M + PT * 16 - 1) / (PT * 16);
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, (int)((size_t)p.B * p.H * p.W * p.in_cs * 2), 0x00020000);
    Chunk wf[CT][KS];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            wf[ct][ks].u = *(const u32x4v*)((const char*)p.w + ((size_t)((g * CT + ct) * 16 + frow) * p.Kw + ks * 32 + fch * 8) * 2);
    float4 bias[CT];
#pragma unroll
    for (int a = 0; a < CT; ++a) bias[a] = *(const float4*)(p.bias + (g * CT + a) * 16 + fch * 4);
    u32x4 x[PT][KS], xn[PT][KS];
    auto fetch = [&](int blk, u32x4 (&dst)[PT][KS]) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int m = (blk * PT + pt) * 16 + frow;
            const uint32_t base = (blk < nblk && m < p.M) ? (uint32_t)((m * p.in_cs + p.in_co + fch * 8) * 2) : OOB;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dst[pt][ks] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, (int)(base >= OOB ? OOB : base + ks * 64), 0, 0);
        }
    };
    int blk = gw / NG;
    fetch(blk, x);
    for (; blk < nblk; blk += stride) {
        fetch(blk + stride, xn);
        f32x4 acc[CT][PT];
#pragma unroll
        for (int a = 0; a < CT; ++a)
#pragma unroll
            for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int a = 0; a < CT; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b) {
                    Chunk xa;
                    xa.u = (u32x4v){x[b][ks].x, x[b][ks].y, x[b][ks].z, x[b][ks].w};
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a][ks].h, xa.h, acc[a][b], 0, 0, 0);
                }
        conv_epilogue_bf16<PT, CT, ACT, RES_NONE>(p, acc, bias, blk * PT * 16, g * CT * 16 + fch * 4, frow);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) x[pt][ks] = xn[pt][ks];
    }
}

// The same kernel for the fp8 path (round 6): pointwise layers with K <= 256 (Bottleneck.cv1, C3.cv1 | cv2, C3.cv3 of the 320^2 - 80^2 levels of
// YOLOv5l at 1280^2, BASELINE.json configs[4]).  Through the implicit GEMM a K = 128 layer is ONE K step per tile: every 64-pixel tile pays
// its tile bookkeeping, a barrier, a 16 KB weight tile re-streamed through LDS for 8 KB of pixels, and the fp8 layers ran no faster than the
// bf16 ones on half the bytes (128 -> 128 at 160^2: 57 us for 105 MB).  Here the weights of a wave's CT x 16 channels sit in registers as MFMA
// A operands (KS steps of K = 128: 8 registers per fragment), the pixels stream global -> registers, one fetch ahead.  K assignment inside a
// step as in conv_igemm_kernel's fp8 branch (a lane's 32 K-bytes = chunks fch and 4 + fch of the 128-byte slice, both operands): the same
// products in the same MFMA, bit-identical results.  Cin = 64: KS = 1, the upper half of the step is out-of-range offsets (zeros).
template <int CT, int KS, int PT, int OCC>
__global__ __launch_bounds__(256, OCC) void conv1x1_direct_fp8_kernel(const ConvP p) {
    constexpr uint32_t OOB = 0x80000000u;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef int i32x8 __attribute__((ext_vector_type(8)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frow = lane & 15, fch = lane >> 4;
    const int NG = (p.Cout + CT * 16 - 1) / (CT * 16);
    const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;           // 4 % NG == 0: a workgroup holds whole sets of groups
    const int g = gw % NG, stride = nw / NG;
    const int nblk = (p.M + PT * 16 - 1) / (PT * 16);
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, (int)((size_t)p.B * p.H * p.W * p.in_cs), 0x00020000);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)((size_t)((p.Cout + 127) / 128 * 128) * p.Kw), 0x00020000);
    u32x4 wlo[CT][KS], whi[CT][KS];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int row = (g * CT + ct) * 16 + frow;                   // rows past Cout are zero rows of the padded weight buffer
            const int off = row * p.Kw + ks * 128 + fch * 16;
            wlo[ct][ks] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, off, 0, 0);
            whi[ct][ks] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, off + 64, 0, 0);
        }
    u32x4 xl[PT][KS], xh[PT][KS], nl[PT][KS], nh[PT][KS];
    const bool half = p.Cin <= 128 * KS - 64;                           // (uniform) Cin = 64: only the first chunk of the last step holds data
    auto fetch = [&](int blk, u32x4 (&lo)[PT][KS], u32x4 (&hi)[PT][KS]) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int m = (blk * PT + pt) * 16 + frow;
            const uint32_t base = (blk < nblk && m < p.M) ? (uint32_t)(m * p.in_cs + p.in_co + fch * 16) : OOB;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                lo[pt][ks] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, (int)(base >= OOB ? OOB : base + ks * 128), 0, 0);
                hi[pt][ks] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, (int)((base >= OOB || (half && ks == KS - 1)) ? OOB : base + ks * 128 + 64), 0, 0);
            }
        }
    };
    int blk = gw / NG;
    fetch(blk, xl, xh);
    for (; blk < nblk; blk += stride) {
        fetch(blk + stride, nl, nh);
        f32x4 acc[CT][PT];
#pragma unroll
        for (int a = 0; a < CT; ++a)
#pragma unroll
            for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int a = 0; a < CT; ++a) {
                const i32x8 wa = {(int)wlo[a][ks].x, (int)wlo[a][ks].y, (int)wlo[a][ks].z, (int)wlo[a][ks].w, (int)whi[a][ks].x, (int)whi[a][ks].y, (int)whi[a][ks].z, (int)whi[a][ks].w};
#pragma unroll
                for (int b = 0; b < PT; ++b) {
                    const i32x8 xa = {(int)xl[b][ks].x, (int)xl[b][ks].y, (int)xl[b][ks].z, (int)xl[b][ks].w, (int)xh[b][ks].x, (int)xh[b][ks].y, (int)xh[b][ks].z, (int)xh[b][ks].w};
                    acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa, xa, acc[a][b], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
                }
            }
        conv_epilogue_fp8<PT, CT>(p, acc, blk * PT * 16, g * CT * 16 + fch * 4, frow);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { xl[pt][ks] = nl[pt][ks]; xh[pt][ks] = nh[pt][ks]; }
    }
}

// ---- 1x1 / stride 1, streaming form: weights in LDS, a wave owns ALL output channels of its pixels (bf16) -----------------------
// The wide-map pointwise layers (K, N <= 256 at 80^2 / 40^2) move 2 - 7 times the bytes their MFMAs are worth in time, and both other
// forms leave them at ~3.3 TB/s: the implicit GEMM pays a DMA issue, a counted wait and a workgroup barrier per K tile around a dozen
// MFMAs, and the register-weight kernel reads every pixel NG times with 32 KB of unique bytes in flight per CU.  tools/ubench/stream_bw
// puts the ceiling for THIS access shape (fragment loads, epilogue-shaped stores) at 4.5 - 5.0 TB/s.  Here the whole weight matrix sits
// in LDS as ready-made MFMA fragments (CT x KS KB, up to 128 KB: one workgroup of eight waves per CU), a wave takes PT x 16 pixels,
// reads their channel runs straight from global memory into the MFMA "B" operand and keeps all CT x 16 outputs of those pixels in
// its accumulators: every input byte is read once, nothing is staged, no barrier after the prologue.  The pixel fragments of K step
// ks are re-requested for the wave's NEXT block as soon as the step's MFMAs have consumed them, so a block's loads fly under the rest
// of the K loop and the whole epilogue of the block before (8 waves x 16 KB in flight per CU).  K order, operand order and epilogue
// are those of conv_igemm_kernel: bit-identical results.
// Measured (128 frames, isolated, autotuner's timing): 256 -> 256 at 40^2 0.054 - 0.056 ms against 0.060 - 0.062 for the best staged tile,
// 256 -> 128 at 80^2 0.149 - 0.158 against 0.159 - 0.166, 128 -> 128 at 80^2 0.112 - 0.116 (NP = 1, PT = 2) against 0.120 - 0.125; a tie on the
// smaller maps -- 5 - 9 %, not the 30 % the access-shape ceiling would allow.  Neither a second fragment set (a block's loads in flight for
// two block times) nor counting the epilogue's stores as allowed-outstanding (loads and stores do retire in issue order here:
// tools/ubench/vmcnt_order, 0 of 3e9) moved it, so what is left is not staging, load latency or store acknowledgement; both removed.
// END TO END the kernel LOSES: one workgroup with up to 132 KB of LDS per CU keeps the ReID queue's workgroups off the CUs it runs on --
// 17.96 / 18.27 k frames/s with it against 18.55 / 18.81 k without (alternating 60-step runs, one box) although the conv stage sum drops
// from 6.40 to 6.35 ms.  The autotuner therefore offers it only under VC_CONV_STREAM=1 (conv_stream_cfg); it stays for the tests and as the
// measured answer to "would reading every byte once with nothing staged reach the copy rate".
template <int CT, int KS, int PT, int NP, int ACT>
__global__ __launch_bounds__(512, 1) void conv1x1_stream_kernel(const ConvP p) {
    constexpr uint32_t OOB = 0x80000000u;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) uint4 wl[CT * KS * 64 + CT * 4];      // weight fragments [ct][ks][lane], then the bias
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frow = lane & 15, fch = lane >> 4;
    for (int f = wave; f < CT * KS; f += 8) {                 // LDS order [ks][ct]: a K step's fragments are one ds_read offset apart
        const int ks = f / CT, ct = f - ks * CT;
        wl[f * 64 + lane] = *(const uint4*)((const char*)p.w + ((size_t)(ct * 16 + frow) * p.Kw + ks * 32 + fch * 8) * 2);
    }
    float* bl = (float*)(wl + CT * KS * 64);
    for (int i = threadIdx.x; i < CT * 16; i += 512) bl[i] = p.bias[i];
    __syncthreads();
    const int gw = blockIdx.x * 8 + wave, nw = gridDim.x * 8;
    const int nblk = (p.M + PT * 16 - 1) / (PT * 16);
    const uint32_t wl_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)wl + lane * 16;
    // The pixel fragments are loaded by hand too (global_load_dwordx4 + counted s_waitcnt): with loads and stores both pending, hipcc's
    // wait insertion falls back to vmcnt(0) in front of the first MFMA of every block, which drains the next block's loads AND this
    // block's stores once per iteration.  Loads return in order: when step ks of a block's first pass starts, the loads younger than its
    // fragments are the (KS - 1 - ks) * PT of the later K steps (requested during the previous block's last pass), so
    // "vmcnt <= (KS - 1 - ks) * PT" means they have landed; the epilogue's stores also sit on the counter and can only make the wait longer.
    // Rows past M are clamped to the last row (read, multiplied, dropped by the epilogue's m < M).
    u32x4v x[PT][KS];
    const char* inb = (const char*)p.in + (size_t)p.in_co * 2 + fch * 16;
    const char* ra[PT];
    auto rows_of = [&](int blk) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) ra[pt] = inb + (size_t)min((blk * PT + pt) * 16 + frow, p.M - 1) * p.in_cs * 2;
    };
#define VC_XLOAD(pt, ks) asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(x[pt][ks]) : "v"(ra[pt]), "n"((ks) * 64))
    rows_of(gw);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) VC_XLOAD(pt, ks);
    constexpr int CTP = CT / NP;                          // channel tiles per pass: the accumulators of one pass are CTP x PT x 4 registers
    for (int blk = gw; blk < nblk; blk += nw) {
        rows_of(blk + nw);                            // the next block of this wave (past the end: the last row again)
#pragma unroll
        for (int np = 0; np < NP; ++np) {
            f32x4 acc[CTP][PT];
#pragma unroll
            for (int a = 0; a < CTP; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // The weight fragments are read by hand, one ahead of the MFMAs that use them: left to the compiler, the loop-invariant LDS
            // reads are hoisted out of the block loop (CT x KS x 4 registers: 170 - 550 spills).  lgkmcnt(1) = everything but the newest
            // LDS operation has landed, whatever else the compiler has in flight (LDS returns in order): the wait can only be too strict.
            uint32_t wa = wl_addr + np * CTP * 1024;
            asm volatile("" : "+v"(wa));
            u32x4v wcur, wnext;
            asm volatile("ds_read_b128 %0, %1" : "=v"(wcur) : "v"(wa));
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (np == 0) {                        // first pass over this block: its fragments of step ks must have landed
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((KS - 1 - ks) * PT));
#pragma unroll
                    for (int b = 0; b < PT; ++b) asm volatile("" : "+v"(x[b][ks]));
                }
#pragma unroll
                for (int a = 0; a < CTP; ++a) {
                    if (a + 1 < CTP) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wnext) : "v"(wa), "n"((a + 1) * 1024));
                    else if (ks + 1 < KS) { wa += CT * 1024; asm volatile("ds_read_b128 %0, %1" : "=v"(wnext) : "v"(wa)); }
                    if (a + 1 < CTP || ks + 1 < KS) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(wcur));
                    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wcur));
                    Chunk wf;
                    wf.u = wcur;
#pragma unroll
                    for (int b = 0; b < PT; ++b) {
                        Chunk xa;
                        xa.u = x[b][ks];
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf.h, xa.h, acc[a][b], 0, 0, 0);
                    }
                    wcur = wnext;
                }
                if (np == NP - 1) {                   // last pass: this K step's fragments are dead, request the next block's
#pragma unroll
                    for (int b = 0; b < PT; ++b) VC_XLOAD(b, ks);
                }
            }
#pragma unroll
            for (int a = 0; a < CTP; ++a) {
                const float4 b1[1] = {*(const float4*)(bl + (np * CTP + a) * 16 + fch * 4)};
                conv_epilogue_bf16<PT, 1, ACT, RES_NONE>(p, reinterpret_cast<f32x4(&)[1][PT]>(acc[a]), b1, blk * PT * 16, (np * CTP + a) * 16 + fch * 4, frow);
            }
        }
    }
}
#undef VC_XLOAD

// ---- 1x1 / stride 1, third weight-stationary form: weights in registers, pixels through an LDS ring, epilogue under the next tile (bf16) ----
// What the two kernels above showed: with the weights in registers every pixel is read NG times from global memory and 32 KB per CU are in
// flight; with the weights in LDS one workgroup's 132 KB keep the ReID queue's workgroups off the CU; and in both, as in the implicit GEMM,
// the epilogue (bias, SiLU, pack, lane-pair exchange, stores) runs with the matrix pipe and the load queue empty.  Here:
//   * four-wave workgroups, two per CU, at most 64 KB of LDS each: the neighbour still fits, the pair drifts apart;
//   * a wave keeps the weights of its 64 output channels as MFMA A fragments (CT = 4 x KS fragments: 64 / 128 registers) for the whole
//     launch; the four waves are NG = Cout / 64 channel groups x 4 / NG pixel parts of the workgroup's BP = PT * 16 * 4 / NG pixels;
//   * only the pixels go through LDS: whole tiles of BP x K arrive by LDS-DMA in an NS-stage ring that runs through the tile boundaries
//     (fixed stride: workgroup b walks tiles b, b + G, ...), rows past M are out-of-range offsets (zeros); ONE counted vmcnt wait and ONE
//     workgroup barrier per pixel tile.  A row is KS * 64 bytes, a multiple of the 256-byte bank row, so the 16-byte chunk index is
//     XOR-swizzled with row & 15 on the source side (conv_halo.hip's idea on its 64-byte rows): the 16 lanes of every ds_read_b128
//     service group -- rows {0-3, 12-15} of chunk c with rows {4-11} of chunk c ^ 1, and so on -- land on 16 different slots;
//   * the fragment reads are inline ds_read_b128, one fragment (four MFMAs) ahead of the MFMAs that use them, with counted lgkmcnt;
//   * the accumulators of tile i are handed to a second register set, and their epilogue -- conv_epilogue_bf16 per (channel tile, pixel
//     tile pair), expressions unchanged -- is issued group by group between the K steps of tile i + 1.  RES_NONE only: no loads at all,
//     so no load sits behind a store.  The first tile runs over an epilogue whose stores are all masked (mbase = M), which keeps the
//     number of stores per tile a constant; the last tile's epilogue drains alone.
// vmcnt: tile i + 1 was requested NS - 2 tiles ago; younger than its XI loads are the (NS - 2) * XI loads of the tiles after it and the
// stores of NS - 1 epilogues (NGRP each, twice that with a second destination), all issued in program order behind it (a compiler barrier
// after the DMA issue keeps the stores of a tile behind that tile's requests).  Loads and stores retire in issue order
// (tools/ubench/vmcnt_order), so "at most that many outstanding" means it has landed.
// K order, MFMA operand order and epilogue are conv_igemm_kernel's: bit-identical results.
template <int KS, int NG, int PT, int NS, int ACT>
__global__ __launch_bounds__(256, 2) void conv1x1_wreg_kernel(const ConvP p) {
    constexpr int CT = 4;                          // channel tiles per wave: 64 channels
    constexpr int NPP = 4 / NG;                    // pixel parts per workgroup
    constexpr int BP = PT * 16 * NPP;              // pixels per tile
    constexpr int KCH = KS * 4;                    // 16-byte chunks per pixel row
    constexpr int RPI = 64 / KCH;                  // rows one wave-instruction of LDS-DMA fills
    constexpr int XI = BP * KS / 64;               // LDS-DMA instructions per wave and tile
    constexpr int STAGE = BP * KCH;                // 16-byte chunks per stage
    constexpr int NGRP = (PT / 2) * CT;            // epilogue groups per tile, one 16-byte store each (two with a second destination)
    static_assert(NG == 2 || NG == 4, "channel groups per workgroup");
    static_assert(KS == 4 || KS == 8, "K = 128 or 256");
    static_assert(PT % 2 == 0 && (BP * KS) % 64 == 0 && XI >= 1 && PT * 16 * KCH * 16 + 256 < 65536, "tile shape");
    static_assert(NS >= 2 && NS * STAGE * 16 <= 64 * 1024, "the ring: at most 64 KB, two workgroups and a neighbour per CU");
    static_assert((NS - 2) * XI + (NS - 1) * 2 * NGRP <= 63, "the counted s_waitcnt must fit vmcnt");
    __shared__ __attribute__((aligned(256))) uint4 lds[NS * STAGE];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    if (p.ablate == 6) return;                     // launch floor (diagnostics)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int frow = lane & 15, fch = lane >> 4;
    const int g = uwave % NG, pp = uwave / NG;     // (uniform) channel group, pixel part
    const int ntiles = p.ntiles, G = gridDim.x;
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, (int)((size_t)p.B * p.H * p.W * p.in_cs * 2), 0x00020000);

    // staging: instruction i of this wave fills the 1 KB at chunk (i * 4 + wave) * 64 of a stage: rows (i * 4 + wave) * RPI + lane / KCH,
    // physical chunk lane % KCH, which holds the row's logical chunk physical ^ (row & 15).  Instruction i is 4 * RPI rows below instruction
    // 0; with two rows per instruction (RPI = 2) row & 15 of the odd instructions differs in bit 3: a second lane offset
    const int srow = wave * RPI + lane / KCH;      // of instruction 0
    const uint32_t soff0 = (uint32_t)((srow * p.in_cs + p.in_co) * 2 + ((lane % KCH) ^ (srow & 15)) * 16);
    const uint32_t soff1 = RPI == 2 ? (uint32_t)((srow * p.in_cs + p.in_co) * 2 + ((lane % KCH) ^ ((srow & 15) ^ 8)) * 16) : soff0;
    const uint32_t row_bytes = (uint32_t)(p.in_cs * 2);
    int s_v = blockIdx.x, s_buf = 0, s_issued = 0;
    auto stage_next = [&]() {
        if (!((p.ablate == 1 || p.ablate == 3) && s_issued >= NS)) {        // timing experiment: no staging after the first tiles
            // Rows past M (the ragged last tile; every row once no tile is left: m0 = M) lie past the descriptor's num_records = M rows
            // and are answered with zeros.  (M + BP) rows stay below 2^32 bytes: conv_check holds M rows below 2^31.
            const int m0 = s_v < ntiles ? s_v * BP : p.M;
#pragma unroll
            for (int i = 0; i < XI; ++i) {
                const uint32_t o = (uint32_t)(m0 + i * 4 * RPI) * row_bytes + ((RPI == 2 && (i & 1)) ? soff1 : soff0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrd, (lds_ptr_t)&lds[s_buf * STAGE + (i * 4 + uwave) * 64], 16, (int)o, 0, 0, 0);
            }
        }
        ++s_issued;
        s_v += G;
        s_buf = s_buf + 1 == NS ? 0 : s_buf + 1;
        asm volatile("" ::: "memory");             // the stores that follow in program order stay behind these requests
    };
#pragma unroll
    for (int st = 0; st < NS - 1; ++st) stage_next();

    // this wave's weights and bias, once
    Chunk wf[CT][KS];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            wf[ct][ks].u = *(const u32x4v*)((const char*)p.w + ((size_t)((g * CT + ct) * 16 + frow) * p.Kw + ks * 32 + fch * 8) * 2);
    // the bias of the wave's 64 channels in ONE register, channel g * 64 + lane in lane `lane`: an epilogue group fetches its four values
    // through the LDS pipe's crossbar (ds_bpermute_b32, no LDS memory).  Sixteen registers of bias per lane beside 128 of weights and two
    // sets of accumulators spilled.
    float bias_l = p.bias[g * 64 + lane];
    // a use the compiler can see, in front of the loop: its own wait for these loads is paid here and not at the first MFMA of every tile
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(wf[ct][ks].u));
    asm volatile("" : "+v"(bias_l));

    // fragment addresses inside a stage: row pp * PT * 16 + pt * 16 + frow (row & 15 = frow), logical chunk ks * 4 + fch.  Physical chunk
    // (ks * 4 + fch) ^ frow = bits 0-1: fch ^ (frow & 3); bits 2-3: (ks & 3) ^ (frow >> 2); bit 4: ks >> 2.  Stages and rows are multiples
    // of 256 bytes, so bits 6-7 of the byte address are bits 2-3 of the chunk: ONE register, the address for ks = 0 in the stage being
    // multiplied, XORed with (ks & 3) * 64; ks >> 2 and the pixel tile pt (16 rows) are immediate offsets
    uint32_t xa = (uint32_t)(uintptr_t)(lds_ptr_t)&lds[0] + (uint32_t)((pp * PT * 16 + frow) * (KCH * 16) + (fch ^ (frow & 3)) * 16 + (frow >> 2) * 64);
    constexpr uint32_t STAGE_BYTES = STAGE * 16;
    int rbuf = 0;                                  // ring slot being multiplied

    f32x4 acc[CT][PT], prev[CT][PT];
#pragma unroll
    for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int b = 0; b < PT; ++b) prev[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int prev_m = p.M;                              // the epilogue under the first tile stores nothing
    const int nbase = g * CT * 16 + fch * 4;
    auto epilogue_group = [&](int gi) {            // conv_epilogue_bf16's loop body for (pixel tile pair gi / CT, channel tile gi % CT)
        const int b = gi / CT * 2, a = gi % CT;
        float bv[4];
        int bsel = fch * 16;                       // byte index of the lane that holds this lane's first channel of a channel tile
        asm volatile("" : "+v"(bsel));             // volatile statements keep their order: the fetch stays inside its K step (hoisted to the
                                                   // top of the tile, the sixteen values are sixteen live registers again)
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(bsel + (a * 16 + j) * 4, __float_as_int(bias_l)));
        const float4 b1[1] = {make_float4(bv[0], bv[1], bv[2], bv[3])};
        conv_epilogue_bf16<2, 1, ACT, RES_NONE>(p, reinterpret_cast<f32x4(&)[1][2]>(prev[a][b]), b1, prev_m + b * 16, nbase + a * 16, frow);
    };
    // fragment f = ks * PT + pt of a tile: pixel tile pt, K step ks
#define VC_XREAD(dst, f)                                                                                                   \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(xa ^ (uint32_t)((((f) / PT) & 3) * 64)), "n"(((f) % PT) * 16 * KCH * 16 + (((f) / PT) >> 2) * 256) : "memory")

    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * XI) : "memory");       // the first tile has landed
    __builtin_amdgcn_s_barrier();
    for (int v = blockIdx.x; v < ntiles; v += G) {
        stage_next();                              // into the slot read one tile ago (every wave has passed that tile's barrier)
#pragma unroll
        for (int a = 0; a < CT; ++a)
#pragma unroll
            for (int b = 0; b < PT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        u32x4v x[2];                               // one fragment in use, the next one on its way (four MFMAs ahead)
        VC_XREAD(x[0], 0);
#pragma unroll
        for (int f = 0; f < KS * PT; ++f) {
            if (f + 1 < KS * PT) {
                VC_XREAD(x[(f + 1) & 1], f + 1);
                asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");              // LDS returns in order: everything but the newest read
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            asm volatile("" : "+v"(x[f & 1]));                                  // the MFMAs below depend on the wait above
            Chunk xf;
            xf.u = x[f & 1];
#pragma unroll
            for (int a = 0; a < CT; ++a) acc[a][f % PT] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a][f / PT].h, xf.h, acc[a][f % PT], 0, 0, 0);
            // the epilogue of the tile before, a share per K step
            if (f % PT == PT - 1) {
#pragma unroll
                for (int gi = (f / PT) * NGRP / KS; gi < (f / PT + 1) * NGRP / KS; ++gi) epilogue_group(gi);
            }
        }
#pragma unroll
        for (int a = 0; a < CT; ++a)
#pragma unroll
            for (int b = 0; b < PT; ++b) prev[a][b] = acc[a][b];
        prev_m = v * BP + pp * PT * 16;
        {
            const uint32_t step = rbuf + 1 == NS ? 0u - (NS - 1) * STAGE_BYTES : STAGE_BYTES;       // (uniform)
            rbuf = rbuf + 1 == NS ? 0 : rbuf + 1;
            xa += step;
        }
        if (p.split == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * XI + (NS - 1) * NGRP) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * XI + (NS - 1) * 2 * NGRP) : "memory");
        __builtin_amdgcn_s_barrier();
    }
#undef VC_XREAD
#pragma unroll
    for (int gi = 0; gi < NGRP; ++gi) epilogue_group(gi);      // the last tile drains alone
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the tiles requested past the last one, before the LDS is released
}

static bool direct1x1_applicable(const ConvP& p, int ct, int ks) {
    if (p.prec != PREC_BF16 || p.kh != 1 || p.kw != 1 || p.sh != 1 || p.sw != 1 || p.ph != 0 || p.pw != 0) return false;
    if (p.Cin != ks * 32 || p.K != p.Cin || p.Ho != p.H || p.Wo != p.W || p.in_cs % 8 != 0 || p.in_co % 8 != 0 || p.in_up || p.m_dev) return false;
    // the 16-byte-store epilogue only (conv_epilogue_bf16's preconditions), SiLU or no activation, no residual
    if (p.out_f32 || p.res_mode != RES_NONE || (p.act != ACT_SILU && p.act != ACT_NONE) || p.out_cs % 8 != 0 || p.out_co % 8 != 0) return false;
    if (p.split != 0 && (p.split % 8 != 0 || p.out2_cs % 8 != 0 || p.out2_co % 8 != 0)) return false;
    const int ng = p.Cout / (ct * 16);
    return p.Cout % (ct * 16) == 0 && (ng == 1 || ng == 2 || ng == 4);
}

template <int CT, int KS, int PT, int OCC>
static int launch_direct1x1(ConvP p, hipStream_t s) {
    if (!conv_switches().direct || !direct1x1_applicable(p, CT, KS)) return VC_ERR_ARG;          // quietly, like launch_halo
    p.Kw = p.Kp;
    const int ng = p.Cout / (CT * 16);
    const int nblk = (p.M + PT * 16 - 1) / (PT * 16);
    const int need = (nblk * ng + 3) / 4;
    static const int slots_hw = resident_workgroups(conv1x1_direct_kernel<CT, KS, PT, OCC, ACT_SILU>);
    const int slots = p.slots > 0 ? p.slots : std::max(256, slots_hw - conv_slots_reserve());
    p.ntiles = nblk * ng;
    if (p.act == ACT_SILU) launch_timed(p, conv1x1_direct_kernel<CT, KS, PT, OCC, ACT_SILU>, dim3(std::min(need, slots)), dim3(256), 0, s, p);
    else launch_timed(p, conv1x1_direct_kernel<CT, KS, PT, OCC, ACT_NONE>, dim3(std::min(need, slots)), dim3(256), 0, s, p);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

static bool direct8_applicable(const ConvP& p, int ct, int ks) {
    if (p.prec != PREC_FP8 || p.kh != 1 || p.kw != 1 || p.sh != 1 || p.sw != 1 || p.ph != 0 || p.pw != 0) return false;
    if (p.K != p.Cin || p.Cin > ks * 128 || p.Cin <= (ks - 1) * 128 || p.Cin % 64 != 0 || (p.Cin % 128 != 0 && p.Cin != 64)) return false;
    if (p.Ho != p.H || p.Wo != p.W || p.in_cs % 16 != 0 || p.in_co % 16 != 0 || p.in_up || p.m_dev || !p.scale || p.Kw < ks * 128) return false;
    const int ng = (p.Cout + ct * 16 - 1) / (ct * 16);
    return ng == 1 || ng == 2 || ng == 4;                         // (the channel tail of a group is masked by the epilogue; its weight rows are zero padding)
}

template <int CT, int KS, int PT, int OCC>
static int launch_direct8(ConvP p, hipStream_t s) {
    p.Kw = p.Kp;
    if (!conv_switches().direct8 || !direct8_applicable(p, CT, KS)) return VC_ERR_ARG;             // quietly, like launch_halo
    const int ng = (p.Cout + CT * 16 - 1) / (CT * 16);
    const int nblk = (p.M + PT * 16 - 1) / (PT * 16);
    const int need = (nblk * ng + 3) / 4;
    static const int slots_hw = resident_workgroups(conv1x1_direct_fp8_kernel<CT, KS, PT, OCC>);
    const int slots = p.slots > 0 ? p.slots : std::max(256, slots_hw - conv_slots_reserve());
    p.ntiles = nblk * ng;
    launch_timed(p, conv1x1_direct_fp8_kernel<CT, KS, PT, OCC>, dim3(std::min(need, slots)), dim3(256), 0, s, p);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

template <int CT, int KS, int PT, int NP>
static int launch_stream1x1(ConvP p, hipStream_t s) {
    if (!direct1x1_applicable(p, CT, KS) || p.Cout != CT * 16) return VC_ERR_ARG;                     // quietly, like launch_halo
    p.Kw = p.Kp;
    const int nblk = (p.M + PT * 16 - 1) / (PT * 16);
    p.ntiles = nblk;
    const int grid = std::max(1, std::min((nblk + 7) / 8, p.slots > 0 ? std::max(1, p.slots / 8) : device_cus()));   // persistent, one workgroup per CU
    if (p.act == ACT_SILU) launch_timed(p, conv1x1_stream_kernel<CT, KS, PT, NP, ACT_SILU>, dim3(grid), dim3(512), 0, s, p);
    else launch_timed(p, conv1x1_stream_kernel<CT, KS, PT, NP, ACT_NONE>, dim3(grid), dim3(512), 0, s, p);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// what conv1x1_wreg_kernel<KS, NG, ...> takes (tests/wreg_cases.py restates it): a bf16 pointwise conv with K = Cin = KS * 32 and
// Cout = NG * 64, the 16-byte-store epilogue without residual, nothing the kernel does not read (device-side M, upsample fold-in)
bool wreg_applicable(const ConvP& p, int ks, int ng) {
    if (p.prec != PREC_BF16 || p.kh != 1 || p.kw != 1 || p.sh != 1 || p.sw != 1 || p.ph != 0 || p.pw != 0) return false;
    if (p.Cin != ks * 32 || p.K != p.Cin || p.Cout != ng * 64 || p.Ho != p.H || p.Wo != p.W || p.in_up || p.m_dev) return false;
    if (p.in_cs % 8 != 0 || p.in_co % 8 != 0 || p.out_cs % 8 != 0 || p.out_co % 8 != 0) return false;
    if (p.out_f32 || p.res_mode != RES_NONE || (p.act != ACT_SILU && p.act != ACT_RELU && p.act != ACT_NONE)) return false;
    return p.split == 0 || (p.split % 8 == 0 && p.out2_cs % 8 == 0 && p.out2_co % 8 == 0);
}

template <int KS, int NG, int PT, int NS>
static int launch_wreg(ConvP p, hipStream_t s) {
    const ConvSwitches& sw = conv_switches();
    if (!sw.wreg || !wreg_applicable(p, KS, NG)) return VC_ERR_ARG;                                  // quietly, like launch_halo
    constexpr int BP = PT * 16 * (4 / NG);
    p.Kw = p.Kp;
    p.ntiles = (p.M + BP - 1) / BP;
    static const int slots_hw = resident_workgroups(conv1x1_wreg_kernel<KS, NG, PT, NS, ACT_SILU>);
    // p.slots (tests): that many workgroups walk all tiles (no XCD-aware tile order here: any grid size will do)
    const int grid = p.slots > 0 ? std::min(p.ntiles, p.slots) : persistent_grid(p.ntiles, slots_hw, sw.reserve, 0, sw.balanced);
    if (p.act == ACT_SILU) launch_timed(p, conv1x1_wreg_kernel<KS, NG, PT, NS, ACT_SILU>, dim3(grid), dim3(256), 0, s, p);
    else if (p.act == ACT_RELU) launch_timed(p, conv1x1_wreg_kernel<KS, NG, PT, NS, ACT_RELU>, dim3(grid), dim3(256), 0, s, p);
    else launch_timed(p, conv1x1_wreg_kernel<KS, NG, PT, NS, ACT_NONE>, dim3(grid), dim3(256), 0, s, p);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// the first id of the family that takes p, or -1 (VC_TUNE_WREG, engine_run.hip::tuned_cfg)
int wreg_cfg_for(const ConvP& p) {
#define VC_W(i, ks, ng, pt, ns) if (wreg_applicable(p, ks, ng)) return i;
    VC_WREG_CFGS(VC_W)
#undef VC_W
    return -1;
}

int launch_wreg_cfg(const ConvP& p, int cfg, hipStream_t s) {
    switch (cfg) {
#define VC_W(i, ks, ng, pt, ns) case i: return launch_wreg<ks, ng, pt, ns>(p, s);
        VC_WREG_CFGS(VC_W)
#undef VC_W
    }
    return VC_ERR_ARG;
}

int launch_pointwise_cfg(const ConvP& p, int cfg, hipStream_t s) {
    switch (cfg) {
#define VC_Z(i, ct, ks, pt, occ) case i: return launch_direct1x1<ct, ks, pt, occ>(p, s);
        VC_DIRECT_CFGS(VC_Z)
#undef VC_Z
#define VC_S(i, ct, ks, pt, np) case i: return launch_stream1x1<ct, ks, pt, np>(p, s);
        VC_STREAM_CFGS(VC_S)
#undef VC_S
#define VC_F(i, ct, ks, pt, occ) case i: return launch_direct8<ct, ks, pt, occ>(p, s);
        VC_DIRECT8_CFGS(VC_F)
#undef VC_F
    }
    return VC_ERR_ARG;
}

}  // namespace vc
