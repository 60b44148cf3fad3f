// The tile configurations of the convolution kernels: one X-macro list per kernel family and, built from them, the registry
// {id, family} that conv_dispatch.hip dispatches on.  The ids are persistent -- tuner caches (vc_tune_export / vc_tune_import,
// VC_TUNE_CACHE), the tests (VC_CONV_CFG) and the profiles name them -- so a list entry never changes its number.  A family's
// translation unit instantiates the kernels of its lists and exports one launch_<family>_cfg(p, cfg, stream).
#pragma once

namespace vc {

// ---- tile configurations -------------------------------------------------------------------------------------------
// One list drives both the table the autotuner walks and the dispatch switch.  Rings deeper than 2 exist for bf16 only;
// the fp32 parity path maps them to the 2-stage instantiation of the same tile.
#define VC_CONV_CFGS(X)                                                                                          \
    X(0, 256, 32, 4, 1, 4, 2)   X(1, 128, 64, 2, 2, 4, 2)   X(2, 128, 128, 2, 2, 4, 2)  X(3, 64, 64, 2, 2, 4, 2)      \
    X(4, 128, 64, 2, 2, 8, 2)   X(5, 128, 128, 2, 2, 8, 2)  X(6, 64, 64, 2, 2, 8, 2)    X(7, 256, 64, 4, 1, 4, 2)     \
    X(8, 256, 64, 4, 1, 8, 2)   X(9, 256, 128, 2, 2, 4, 2)  X(10, 256, 128, 2, 2, 8, 2) X(11, 64, 128, 1, 4, 4, 2)    \
    X(12, 64, 128, 1, 4, 8, 2)  X(13, 256, 32, 4, 1, 8, 2)                                                          \
    X(14, 64, 64, 2, 2, 4, 4)   X(15, 64, 64, 2, 2, 8, 3)   X(16, 64, 64, 2, 2, 8, 4)   X(17, 128, 64, 2, 2, 4, 4)    \
    X(18, 128, 64, 2, 2, 8, 3)  X(19, 128, 128, 2, 2, 4, 4) X(20, 128, 128, 2, 2, 8, 3) X(21, 64, 128, 1, 4, 4, 4)    \
    X(22, 64, 128, 1, 4, 8, 3)  X(23, 256, 32, 4, 1, 4, 4)  X(24, 256, 64, 4, 1, 4, 4)  X(25, 256, 64, 4, 1, 8, 3)    \
    X(26, 256, 128, 2, 2, 4, 4) X(27, 256, 128, 2, 2, 8, 3)
// halo-staged 3x3 / s1 / p1 (bf16): Y(index, BP, BC, WP, WC, NS)
// 36 - 39: the four waves side by side in pixels (wave tiles 32 x 64 and 64 x 128): half the per-tile tap-address set-up per MFMA
// of the 2 x 2 arrangement -- the narrow layers issue 7 VALU instructions per MFMA, most of them set-up and epilogue (measured:
// 64 -> 64 at 25^2 -8 %, 128 -> 128 at 40^2 -10 %; 256 x 64 and 128 x 128 tiles in this arrangement gained nothing)
#define VC_HALO_CFGS(Y) Y(28, 128, 64, 2, 2, 2) Y(29, 128, 64, 2, 2, 3) Y(30, 128, 128, 2, 2, 2) Y(31, 128, 128, 2, 2, 3) \
                        Y(36, 128, 64, 4, 1, 2) Y(37, 128, 64, 4, 1, 3) Y(38, 256, 128, 4, 1, 2) Y(39, 256, 128, 4, 1, 3)
// 16-wave workgroups on 256 x 256 tiles: half the staged bytes (and LDS-DMA instructions, ~150 issue cycles each) per MFMA of the
// 128 x 128 tile and a 3- or 4-deep ring in 96 / 128 KB (measured per 128 frames: 3x3/s2 128->256 at 80^2 213 -> 169 us, 256->512
// 202 -> 148 us, 1x1 512->512 at 20^2 67 -> 56 us; 256 x 128, 512 x 128 and 512 x 64 tiles with 8 / 16 waves gained nothing)
// 43: the same tile on 128-byte rows (2 x 64 KB): the only 256 x 256 tile of the fp8 path (its K = 128 MFMA step needs KC = 8)
#define VC_CONV_BIG_CFGS(X) X(40, 256, 256, 4, 4, 4, 2) X(41, 256, 256, 4, 4, 4, 3) X(42, 256, 256, 4, 4, 4, 4) X(43, 256, 256, 4, 4, 8, 2)
// halo-staged 3x3 / s2 / p1 (bf16), rectangular tiles of BP pixels: V(index, BP, BC, WP, WC, NS)
// (measured on YOLOv5s, 128 frames: 3-P3 64->128 at 80^2 0.253 -> 0.198 ms with 256-pixel tiles, 18-P4 128->128 0.117 -> 0.096, 5-P4 a tie;
// the 20^2 layers stay on the 256 x 256 implicit GEMM; 2 x 2 waves on 256 pixels never won)
#define VC_S2HALO_CFGS(V) V(44, 128, 128, 2, 2, 2) V(45, 128, 128, 2, 2, 3) V(46, 256, 128, 4, 1, 3) V(47, 128, 128, 2, 2, 4) \
                          V(48, 128, 256, 2, 2, 2) V(49, 256, 128, 4, 1, 2)
// weights-in-registers 1x1 (bf16): Z(index, CT, KS, PT, OCC)
#define VC_DIRECT_CFGS(Z) Z(32, 2, 1, 4, 4) Z(33, 4, 2, 4, 2) Z(34, 4, 2, 2, 3) Z(35, 4, 4, 2, 2)
// weights-in-LDS streaming 1x1 (bf16): S(index, CT, KS, PT, NP): 128 -> 128, 256 -> 256, 256 -> 128, 128 -> 256 channels; NP passes over the
// block's fragments, each for CT / NP channel tiles, keep accumulators + fragments + epilogue inside 256 registers at two waves per SIMD
#define VC_STREAM_CFGS(S) S(50, 8, 4, 4, 2) S(51, 16, 8, 2, 2) S(52, 8, 8, 2, 1) S(53, 16, 4, 2, 2) S(54, 8, 4, 2, 1)
// conv3x3_halo_v2_kernel<4> (conv_halo_v2.hip), one instantiation: W(index)
#define VC_HALO_V2_CFGS(W) W(55)
// deep rings on the small tiles (round 6): a launch of 28 workgroups walking 36 K steps is bound by the latency of its LDS-DMA loads (~1.2 us from
// L2 / HBM on an otherwise idle chip) divided by the tiles in flight; six or eight stages instead of three
#define VC_CONV_DEEP_CFGS(X) X(60, 64, 64, 2, 2, 8, 6) X(61, 64, 64, 2, 2, 8, 8) X(62, 128, 64, 2, 2, 8, 6) X(63, 64, 128, 1, 4, 8, 6)
// split-K instances of the implicit GEMM (bf16, round 6): K(index, BP, BC, WP, WC, KC, NS); offered when the tiles alone cannot fill the chip
#define VC_SK_CFGS(K) K(56, 64, 64, 2, 2, 8, 3) K(57, 64, 64, 2, 2, 8, 4) K(58, 128, 64, 2, 2, 8, 3) K(59, 64, 128, 1, 4, 8, 3)
// paired 8-wave workgroups, two per CU (round 6, conv_igemm_kernel<..., OCC = 2>): P(index, BP, BC, WP, WC, KC, NS)
#define VC_PAIR_CFGS(P) P(64, 256, 128, 4, 2, 4, 3) P(65, 128, 256, 2, 4, 4, 3) P(66, 256, 128, 4, 2, 4, 2)
// 67 - 68: two 4-wave workgroups per CU with 128 x 64 wave tiles (12 fragment reads per 32 MFMAs: 96 B / clk of LDS reads where the 64 x 64 wave
// tile asks for the LDS's whole 128 B / clk), 256 registers per wave
#define VC_PAIR4_CFGS(P) P(67, 256, 128, 2, 2, 4, 3) P(68, 256, 128, 2, 2, 4, 2)
// weights-in-registers 1x1 of the fp8 path (conv1x1_direct_fp8_kernel): F(index, CT, KS, PT, OCC); K <= 128 KS
#define VC_DIRECT8_CFGS(F) F(69, 4, 1, 2, 2) F(70, 4, 2, 2, 2) F(71, 4, 1, 4, 2) F(72, 8, 1, 2, 2)
// weights in registers, pixels through an LDS ring, epilogue under the next tile (conv1x1_wreg_kernel, bf16): W(index, KS, NG, PT, NS) for
// K = KS * 32 in, NG * 64 out; pixel tiles of PT * 16 * 4 / NG rows of KS * 64 bytes, NS of them in the ring (at most 64 KB).
// PT = 2 throughout: four pixel tiles per wave (64 accumulator registers x 2 sets) spill beside the weights, for K = 128 as well.
// 73 / 74: 256 -> 256 (32-pixel tiles); 75: 256 -> 128 (64); 76: 128 -> 256 (32); 77 / 78: 128 -> 128 (64)
#define VC_WREG_CFGS(W) W(73, 8, 4, 2, 3) W(74, 8, 4, 2, 4) W(75, 8, 2, 2, 2) W(76, 4, 4, 2, 4) W(77, 4, 2, 2, 3) W(78, 4, 2, 2, 4)

// ---- the registry ------------------------------------------------------------------------------------------------------
// FAM_IGEMM: conv_igemm.hip; FAM_HALO: conv_halo.hip; FAM_HALO_V2: conv_halo_v2.hip; FAM_HALO_S2: conv_halo_s2.hip; FAM_DIRECT, FAM_STREAM,
// FAM_DIRECT8 and FAM_WREG: conv_pointwise.hip
enum ConvFamily : int { FAM_IGEMM, FAM_HALO, FAM_HALO_V2, FAM_HALO_S2, FAM_DIRECT, FAM_STREAM, FAM_DIRECT8, FAM_WREG };
struct ConvCfgEntry { int id; ConvFamily family; };
#define VC_REG_IGEMM(i, ...) {i, FAM_IGEMM},
#define VC_REG_HALO(i, ...) {i, FAM_HALO},
#define VC_REG_HALO_V2(i, ...) {i, FAM_HALO_V2},
#define VC_REG_HALO_S2(i, ...) {i, FAM_HALO_S2},
#define VC_REG_DIRECT(i, ...) {i, FAM_DIRECT},
#define VC_REG_STREAM(i, ...) {i, FAM_STREAM},
#define VC_REG_DIRECT8(i, ...) {i, FAM_DIRECT8},
#define VC_REG_WREG(i, ...) {i, FAM_WREG},
constexpr ConvCfgEntry kConvCfgs[] = {
    VC_CONV_CFGS(VC_REG_IGEMM) VC_HALO_CFGS(VC_REG_HALO) VC_DIRECT_CFGS(VC_REG_DIRECT) VC_CONV_BIG_CFGS(VC_REG_IGEMM) VC_S2HALO_CFGS(VC_REG_HALO_S2)
    VC_STREAM_CFGS(VC_REG_STREAM) VC_HALO_V2_CFGS(VC_REG_HALO_V2) VC_SK_CFGS(VC_REG_IGEMM) VC_CONV_DEEP_CFGS(VC_REG_IGEMM) VC_PAIR_CFGS(VC_REG_IGEMM)
    VC_PAIR4_CFGS(VC_REG_IGEMM) VC_DIRECT8_CFGS(VC_REG_DIRECT8) VC_WREG_CFGS(VC_REG_WREG)};
#undef VC_REG_IGEMM
#undef VC_REG_HALO
#undef VC_REG_HALO_V2
#undef VC_REG_HALO_S2
#undef VC_REG_DIRECT
#undef VC_REG_STREAM
#undef VC_REG_DIRECT8
#undef VC_REG_WREG
constexpr int kNumConvCfgs = (int)(sizeof(kConvCfgs) / sizeof(kConvCfgs[0]));

// the family of every id, indexed by id; ok = the ids are exactly 0 .. kNumConvCfgs - 1, each once
struct ConvFamilyTable { ConvFamily of[kNumConvCfgs]; bool ok; };
constexpr ConvFamilyTable conv_family_table() {
    ConvFamilyTable t{};
    int seen[kNumConvCfgs] = {};
    t.ok = true;
    for (const ConvCfgEntry& e : kConvCfgs) {
        if (e.id < 0 || e.id >= kNumConvCfgs || seen[e.id]++) { t.ok = false; continue; }
        t.of[e.id] = e.family;
    }
    return t;
}
constexpr ConvFamilyTable kConvFamily = conv_family_table();
static_assert(kConvFamily.ok, "tile configuration ids must be exactly 0 .. N - 1, each once");

#define VC_ID_HALO_V2(i) i
constexpr int kCfgHaloV2 = VC_HALO_V2_CFGS(VC_ID_HALO_V2);      // the one entry of its list
#undef VC_ID_HALO_V2

}  // namespace vc
