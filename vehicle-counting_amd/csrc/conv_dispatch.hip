// Dispatch of a convolution to the kernel families: the registry of tile configurations (conv_cfgs.h) says which family an id belongs
// to, the family's translation unit (conv_igemm.hip, conv_halo.hip, conv_halo_v2.hip, conv_halo_s2.hip, conv_pointwise.hip) launches it.
// Also the heuristic choice for untuned layers, the fall-back when a family refuses a shape, and the argument checks.
#include <algorithm>
#include <cstdlib>

#include "vc_common.h"
#include "conv_cfgs.h"

namespace vc {

int conv_num_cfgs() { return kNumConvCfgs; }

bool conv_stream_cfg(int cfg) { return cfg >= 0 && cfg < kNumConvCfgs && kConvFamily.of[cfg] == FAM_STREAM; }

int conv_k_tile(int prec) { return prec == PREC_F32 ? 32 : prec == PREC_FP8 ? 128 : 64; }    // weights are padded to the widest K tile (KC = 8)

double conv_flops(const ConvP& p) { return 2.0 * (double)p.M * (double)p.Cout * (double)p.K; }

static int conv_heuristic(const ConvP& p) {
    if (p.prec == PREC_FP8) {                  // 128-byte-row tiles only (KC = 8, even pixel tiles per wave)
        if (p.Cout <= 64) return 4;
        const long t = (long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
        return t >= 512 ? 5 : 6;
    }
    if (p.in_up) return 2;                     // the upsample fold-in is instantiated for a subset of the tiles (launch_one): 128 x 128 is one of them
    // narrow layers get tall pixel tiles; late (small-M) layers get small tiles so the grid still covers 256 CUs
    if (p.Cout <= 32) return 0;
    if (p.Cout <= 64) return 1;
    const long t128 = (long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
    return t128 >= 512 ? 2 : 3;
}

int launch_conv_cfg(const ConvP& p, int cfg, hipStream_t s) {
    if (cfg < 0 || cfg >= conv_num_cfgs()) cfg = conv_heuristic(p);
    switch (kConvFamily.of[cfg]) {
        case FAM_IGEMM: return launch_igemm_cfg(p, cfg, s);
        case FAM_HALO: return launch_halo_cfg(p, cfg, s);
        case FAM_HALO_V2: return launch_halo_v2_cfg(p, cfg, s);
        case FAM_HALO_S2: return launch_halo_s2_cfg(p, cfg, s);
        case FAM_DIRECT:
        case FAM_STREAM:
        case FAM_DIRECT8: return launch_pointwise_cfg(p, cfg, s);
        case FAM_WREG: return launch_wreg_cfg(p, cfg, s);
    }
    return VC_ERR_ARG;
}

int conv_check(const ConvP& p);

int launch_conv(const ConvP& p, hipStream_t s) {
    VC_TRY(conv_check(p));
    const int rc = launch_conv_cfg(p, p.cfg, s);
    // A tuned choice is keyed by the power-of-two bucket of M, but some families' applicability depends on the exact batch (v2_applicable:
    // whole rows per tile; the upsample fold-in's tile subset): a launcher refuses before it launches anything, and the heuristic's
    // implicit-GEMM tile takes every shape conv_check admits.
    if (rc == VC_ERR_ARG && p.cfg >= 0 && p.cfg < conv_num_cfgs() && !getenv("VC_CONV_STRICT")) return launch_conv_cfg(p, -1, s);   // (VC_CONV_STRICT: the tile-configuration tests want the refusal)
    return rc;
}

int conv_check(const ConvP& p) {
    const int ch = p.prec == PREC_F32 ? 4 : p.prec == PREC_FP8 ? 16 : 8;
    if (p.prec == PREC_FP8)
        VC_CHECK(p.scale && p.Cout % 8 == 0 && p.out_cs % 8 == 0 && p.out_co % 8 == 0 && (p.split == 0 || (p.split % 8 == 0 && p.out2_cs % 8 == 0 && p.out2_co % 8 == 0)) &&
                 (p.res_mode == RES_NONE || (p.res_cs % 4 == 0 && p.res_co % 4 == 0)), VC_ERR_ARG, "conv fp8: channel scales / 8-channel alignment of the outputs");
    VC_CHECK(p.Cin % ch == 0 && p.in_cs % ch == 0 && p.in_co % ch == 0, VC_ERR_ARG,
             "conv: input channels/stride/offset (%d,%d,%d) must be multiples of %d", p.Cin, p.in_cs, p.in_co, ch);
    VC_CHECK(p.out_cs % 4 == 0 && p.out_co % 4 == 0, VC_ERR_ARG, "conv: output stride/offset must be multiples of 4");
    VC_CHECK(p.split == 0 || (p.split % 4 == 0 && p.out2 && p.out2_cs % 4 == 0 && p.out2_co % 4 == 0 && p.res_mode == RES_NONE), VC_ERR_ARG,
             "conv: bad split destination");
    VC_CHECK(!(p.prec == PREC_FP8 && p.out_bf16 && p.split != 0), VC_ERR_ARG, "conv fp8: the bf16 store has one destination (conv_epilogue_fp8 would put channels >= split behind the first slice)");
    VC_CHECK(p.res_mode == RES_NONE || (p.res_cs % 4 == 0 && p.res_co % 4 == 0), VC_ERR_ARG, "conv: residual alignment");
    VC_CHECK(p.Kp % conv_k_tile(p.prec) == 0 && p.Kp >= p.K, VC_ERR_ARG, "conv: bad K padding %d/%d", p.K, p.Kp);
    VC_CHECK(p.M > 0 && p.Cout > 0, VC_ERR_ARG, "conv: empty problem");
    VC_CHECK(!p.in_up || (p.prec == PREC_BF16 && p.kh == 1 && p.kw == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0 && p.H % 2 == 0 && p.W % 2 == 0 &&
                          p.up_C > 0 && p.up_C < p.Cin && p.up_C % 64 == 0 && p.Cin % 64 == 0 && p.up_cs % 8 == 0 && p.up_co % 8 == 0 && !p.m_dev), VC_ERR_ARG,
             "conv: the upsample fold-in needs a bf16 pointwise conv on an even-sized map with 64-channel-aligned halves");
    VC_CHECK((size_t)p.B * p.H * p.W * p.in_cs * elem_size(p.prec) < (1ull << 31), VC_ERR_CAPACITY, "conv: input tensor exceeds the 2 GiB buffer descriptor");
    VC_CHECK((size_t)((p.Cout + 127) / 128 * 128) * p.Kp * elem_size(p.prec) < (1ull << 31), VC_ERR_CAPACITY, "conv: weights exceed 2 GiB");
    VC_CHECK(p.kh * p.kw <= 40, VC_ERR_ARG, "conv: at most 40 taps (validity mask is 64 bits incl. K padding)");
    VC_CHECK(p.M < (1 << 24), VC_ERR_CAPACITY, "conv: more than 2^24 output pixels in one launch");
    VC_CHECK((size_t)p.M * std::max(p.out_cs, std::max(p.res_cs, p.out2_cs)) * ((p.prec == PREC_F32 || p.out_f32) ? 4 : (p.prec == PREC_FP8 && !p.out_bf16) ? 1 : 2) < (1ull << 31),
             VC_ERR_CAPACITY, "conv: output tensor exceeds 2 GiB (32-bit buffer offsets)");
    return VC_OK;
}

}  // namespace vc
