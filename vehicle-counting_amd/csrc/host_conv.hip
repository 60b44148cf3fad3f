// The convolution kernels on host arrays (include/vcount_hip.h): one launch_conv under the launch views, the stride-2 + pointwise pair, the
// fused C3 / Bottleneck / ReID blocks, the detector's stem and fused front, and the ReID stem.  Entry points only: each stages NumPy-style arrays (host_stage.h), fills its ConvPs
// with the engine's own conv_params (engine_plan.hip), runs one launcher and reads the result back.  None of them touches a vc_engine.
#include <algorithm>
#include <cstdlib>

#include "engine.h"

using namespace vc;

namespace {

int host_param(DevScratch& mem, ConvParam& p, const char* name, int O, int I, int kh, int kw, const float* w, const float* b, int prec = PREC_BF16) {
    p.name = name; p.O = O; p.I = I; p.kh = kh; p.kw = kw; p.set = true;
    p.w.assign(w, w + (size_t)O * I * kh * kw);
    p.b.assign(b, b + O);
    return pack_and_upload(mem.allocs, p, prec);
}

// The launch knobs of the environment, read per call (tools/convdbg.sh, tools/sk_time.py and the tests set them between calls): the tile
// configuration of every launch; for a single launch also the ablation and the persistent grid (tests: a short grid walks all tiles)
void conv_env(ConvP& c, bool single_launch) {
    auto num = [](const char* name, int dflt) { const char* s = getenv(name); return s ? atoi(s) : dflt; };
    c.cfg = num("VC_CONV_CFG", -1);
    if (single_launch) { c.ablate = num("VC_CONV_ABLATE", 0); c.slots = num("VC_CONV_SLOTS", 0); }
}

// Diagnostics of one launch that has run once: VC_CONV_TIME = n: the launch alone on the GPU, best and mean of n repetitions; c.dbg
// (VC_CONV_DBG): the per-workgroup phase stamps the kernel left there
void conv_diagnostics(const ConvP& c, size_t dbg_n) {
    if (getenv("VC_CONV_TIME")) {
        const int reps = std::max(1, atoi(getenv("VC_CONV_TIME")));
        hipEvent_t e0, e1;
        hipEventCreate(&e0); hipEventCreate(&e1);
        float best = 1e30f, sum = 0.f;
        for (int r = 0; r < reps; ++r) {
            hipEventRecord(e0, nullptr);
            launch_conv(c, nullptr);
            hipEventRecord(e1, nullptr);
            hipEventSynchronize(e1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            best = std::min(best, ms); sum += ms;
        }
        hipEventDestroy(e0); hipEventDestroy(e1);
        fprintf(stderr, "[vc conv time] cfg %d M %d N %d K %d: best %.4f ms mean %.4f ms, %.1f TFLOP/s\n", c.cfg, c.M, c.Cout, c.K, best, sum / reps,
                2.0 * c.M * c.Cout * c.K / (best * 1e-3) / 1e12);
    }
    if (!c.dbg) return;
    // per-workgroup phase times (100 MHz timestamps), averaged
    std::vector<long long> h(dbg_n * 8);
    hipMemcpy(h.data(), c.dbg, dbg_n * 64, hipMemcpyDeviceToHost);
    double acc[4] = {0, 0, 0, 0}; long n = 0; long long lo = INT64_MAX, hi = 0;
    for (size_t b = 0; b < dbg_n; ++b) {
        const long long* t = &h[b * 8];
        if (!t[0] || !t[4]) continue;
        for (int i = 0; i < 4; ++i) acc[i] += (double)(t[i + 1] - t[i]);
        lo = std::min(lo, t[0]); hi = std::max(hi, t[4]); ++n;
    }
    std::vector<double> st, du;
    for (size_t b = 0; b < dbg_n; ++b) { const long long* t = &h[b * 8]; if (t[0] && t[4]) { st.push_back((double)(t[0] - lo) / 100); du.push_back((double)(t[4] - t[0]) / 100); } }
    std::sort(st.begin(), st.end()); std::sort(du.begin(), du.end());
    if (n) fprintf(stderr, "[vc conv dbg] start offsets us p10/p50/p90/max %.1f %.1f %.1f %.1f ; lifetimes us p10/p50/p90/max %.1f %.1f %.1f %.1f\n",
                   st[n / 10], st[n / 2], st[n * 9 / 10], st[n - 1], du[n / 10], du[n / 2], du[n * 9 / 10], du[n - 1]);
    if (n) fprintf(stderr, "[vc conv dbg] %ld workgroups, us per workgroup: prologue %.2f first-tile %.2f k-loop %.2f epilogue %.2f ; first start -> last end %.2f us\n",
                   n, acc[0] / n / 100, acc[1] / n / 100, acc[2] / n / 100, acc[3] / n / 100, (double)(hi - lo) / 100);
    for (int w = 0; w < 4; ++w) {   // conv3x3_halo_v2_kernel: per-step cycle stamps of four workgroups
        const long long* tr = &h[400000 + w * 4096];
        if (!tr[0]) continue;
        int steps = 0; while (steps < 800 && tr[steps * 5]) ++steps;
        double d[5] = {0, 0, 0, 0, 0}; int n3 = 0;
        for (int k = 9; k + 1 < steps; ++k, ++n3) { for (int j = 0; j < 4; ++j) d[j] += (double)(tr[k * 5 + j + 1] - tr[k * 5 + j]); d[4] += (double)(tr[(k + 1) * 5] - tr[k * 5 + 4]); }
        if (n3) fprintf(stderr, "[vc conv dbg] wg %d: cycles per step (steps 9..%d), stamp intervals 0-1 %.0f, 1-2 %.0f, 2-3 %.0f, 3-4 %.0f, 4-next %.0f\n", w * 128, steps - 2, d[0] / n3, d[1] / n3, d[2] / n3, d[3] / n3, d[4] / n3);
        if (steps > 30) { fprintf(stderr, "[vc conv dbg]   steps 18..26 total cycles:"); for (int k = 18; k < 27; ++k) fprintf(stderr, " %lld", tr[(k + 1) * 5] - tr[k * 5]); fprintf(stderr, "\n"); }
    }
}

// One convolution launch on host arrays under the views of `v` (include/vcount_hip.h: vc_conv2d_view_host); vc_conv2d_host is its dense
// case.  d->cin may be short of the chunk here (the weights are packed for round_up(cin, chunk) channels, x holds that many).
int conv_view_run(const vc_conv_desc* d, const vc_conv_view* v, const float* x, const float* x_up, const float* w, const float* bias,
                  const float* res, float* y, float* y2) {
    const int prec = d->precision, ch = prec == PREC_F32 ? 4 : prec == PREC_FP8 ? 16 : 8;
    set_error("%s", "");                               // a launcher refuses a shape without a message: the caller must not read an older one
    VC_CHECK(prec == PREC_F32 || prec == PREC_BF16 || prec == PREC_FP8, VC_ERR_ARG, "conv: bad precision");
    VC_CHECK(d->b >= 1 && d->h >= 1 && d->w >= 1 && d->cin >= 1 && d->cout >= 1 && d->kh >= 1 && d->kw >= 1 && d->stride >= 1 && d->pad >= 0, VC_ERR_ARG, "conv: bad shape");
    const int cin_eff = round_up(d->cin, ch);
    const int Ho = (d->h + 2 * d->pad - d->kh) / d->stride + 1, Wo = (d->w + 2 * d->pad - d->kw) / d->stride + 1;
    VC_CHECK(Ho >= 1 && Wo >= 1, VC_ERR_ARG, "conv: empty output");
    const size_t npix_in = (size_t)d->b * d->h * d->w, npix_out = (size_t)d->b * Ho * Wo;
    const int cout_l = prec == PREC_FP8 ? round_up(d->cout, 8) : d->cout;   // the fp8 epilogue stores 8 channels at a time (weight / bias / scale rows are zero-padded)
    const bool with_res = res && d->res_mode != RES_NONE, up = v->up_c > 0;
    // every slice inside its buffer: the kernels address by (stride, offset) alone
    VC_CHECK(v->in_co >= 0 && v->in_cs >= v->in_co + cin_eff, VC_ERR_ARG, "conv view: input slice [%d, %d) outside stride %d", v->in_co, v->in_co + cin_eff, v->in_cs);
    VC_CHECK(v->split >= 0 && v->split < cout_l && (v->split == 0 || y2), VC_ERR_ARG, "conv view: split %d of %d channels", v->split, cout_l);
    VC_CHECK(v->out_co >= 0 && v->out_cs >= v->out_co + (v->split > 0 ? v->split : cout_l), VC_ERR_ARG, "conv view: output slice outside stride %d", v->out_cs);
    VC_CHECK(v->split == 0 || (v->out2_co >= 0 && v->out2_cs >= v->out2_co + cout_l - v->split), VC_ERR_ARG, "conv view: second output slice outside stride %d", v->out2_cs);
    VC_CHECK(!with_res || (v->res_co >= 0 && v->res_cs >= v->res_co + round_up(cout_l, 4)), VC_ERR_ARG, "conv view: residual slice outside stride %d", v->res_cs);
    VC_CHECK(!up || (x_up && v->up_c <= cin_eff && v->up_co >= 0 && v->up_cs >= v->up_co + v->up_c), VC_ERR_ARG, "conv view: upsampled slice outside stride %d", v->up_cs);
    VC_CHECK((!v->out_f32 || prec == PREC_BF16) && (!v->out_bf16 || prec == PREC_FP8), VC_ERR_ARG, "conv view: out_f32 belongs to bf16, out_bf16 to fp8");
    const int oprec = (prec == PREC_F32 || v->out_f32) ? (int)PREC_F32 : (prec == PREC_BF16 || v->out_bf16) ? (int)PREC_BF16 : (int)PREC_FP8;   // element type of the stores
    DevScratch mem;
    ConvParam p;
    VC_TRY(host_param(mem, p, "host", d->cout, d->cin, d->kh, d->kw, w, bias, prec));
    void *dx = nullptr, *dxu = nullptr, *dr = nullptr;
    int* dm = nullptr;
    VC_TRY(upload_elems(mem, x, npix_in * v->in_cs, prec, &dx));                 // activation scale 1
    if (up) VC_TRY(upload_elems(mem, x_up, (size_t)d->b * (d->h / 2) * (d->w / 2) * v->up_cs, prec, &dxu));
    if (with_res) VC_TRY(upload_elems(mem, res, npix_out * v->res_cs, prec, &dr));
    if (v->m_valid >= 0) VC_TRY(mem.upload(&dm, &v->m_valid, sizeof(int)));
    GuardedOut gy, gy2;
    const size_t ny = npix_out * v->out_cs, ny2 = npix_out * (size_t)v->out2_cs;
    VC_TRY(guarded_elems(mem, gy, y, ny, oprec));
    if (v->split > 0) VC_TRY(guarded_elems(mem, gy2, y2, ny2, oprec));
    ConvP c = conv_params(p, {dx, v->in_cs, v->in_co}, {gy.out(), v->out_cs, v->out_co}, d->b, d->h, d->w, d->kh, d->kw, d->stride, d->pad, d->act, 1.0f, 1.0f);
    c.Cout = cout_l;                                   // (above: the fp8 epilogue's 8 channels)
    c.res = dr; c.res_cs = v->res_cs; c.res_co = v->res_co; c.res_mode = with_res ? d->res_mode : RES_NONE;
    c.out_f32 = v->out_f32; c.out_bf16 = v->out_bf16;
    if (v->split > 0) { c.split = v->split; c.out2 = gy2.out(); c.out2_cs = v->out2_cs; c.out2_co = v->out2_co; }
    c.m_dev = dm;
    if (up) { c.in_up = dxu; c.up_C = v->up_c; c.up_cs = v->up_cs; c.up_co = v->up_co; }
    conv_env(c, true);
    const size_t dbg_n = (size_t)1 << 16;
    if (getenv("VC_CONV_DBG") && mem.alloc(&c.dbg, dbg_n * 64) == VC_OK) hipMemset(c.dbg, 0, dbg_n * 64);
    VC_TRY(launch_conv(c, nullptr));                   // a refused launch leaves y / y2 as the caller passed them
    VC_TRY(kernel_wait("conv kernel"));
    conv_diagnostics(c, dbg_n);
    VC_TRY(read_elems(gy, ny, oprec, y, "the conv kernel"));
    if (v->split > 0) VC_TRY(read_elems(gy2, ny2, oprec, y2, "the conv kernel (second destination)"));
    return VC_OK;
}

// ---- the fused block kernels (include/vcount_hip.h: vc_fused_view) -------------------------------------------------------------------------
// Each entry point builds the ConvP chain the engine's plan builds (engine_plan.hip::yolo_c3, reid_build_ops) over buffers of its own and
// hands it to the block's launcher, whose *_applicable decides as it does in the engine, or -- v->unfused -- to launch_conv one
// convolution at a time.
// one bf16 convolution (1x1, or 3x3 / pad 1) of a chain
ConvP chain_conv(const ConvParam& p, void* in, int in_cs, int in_co, void* out, int out_cs, int out_co, int B, int H, int W, int act) {
    ConvP c = conv_params(p, {in, in_cs, in_co}, {out, out_cs, out_co}, B, H, W, p.kh, p.kh, 1, p.kh / 2, act, 1.0f, 1.0f);
    conv_env(c, false);                                // the unfused chain: the tile configuration of every launch
    return c;
}
int chain_unfused(std::initializer_list<ConvP> chain) {
    for (const ConvP& c : chain) VC_TRY(launch_conv(c, nullptr));
    return VC_OK;
}
// an intermediate the fused kernel keeps on chip: its buffer (and the guards around it) still hold the fill
int still_filled(const GuardedOut& g, const char* kernel, const char* what) {
    std::vector<uint8_t> h(g.bytes);
    VC_TRY(g.read_back(h.data(), kernel));
    for (size_t i = 0; i < h.size(); ++i) VC_CHECK(h[i] == 0xA5, VC_ERR_HIP, "%s wrote %s (byte %zu)", kernel, what, i);
    return VC_OK;
}
bool fused_shape_ok(int b, int h, int w) { return b >= 1 && h >= 1 && w >= 1 && (long long)b * h * w <= (1 << 22); }
// Guard blocks that hold every store of an 8 x 16 tile that lost its `y < H` / `x < W` tests: past the last frame's last pixel such a tile
// reaches less than 7 rows and 16 pixels further (bf16 pixels of cs channels)
size_t tile_guard(int w, int cs) { return ((size_t)(8 * w + 16) * cs * 2 + 255) / 256 * 256; }
// channels [co, co + n) inside a pixel of cs channels
bool fused_slice_ok(int cs, int co, int n) { return co >= 0 && cs >= co + n && cs <= 4096; }

// ---- the stem and the fused front (include/vcount_hip.h: vc_front_view) ---------------------------------------------------------------------
// The network input of both entry points, as run_detector_dev hands it to the plan: the letterboxed tensor [b][net_h][net_w][4] bf16 (channel 3
// zero; the pair view reads it as net_w / 2 pixels of 8 channels) from the caller's floats, or u8 frames whose letterbox the kernel folds in
// (mode 0: launch_letterbox writes the tensor).  Inputs lie between guard blocks of 0xFF: a bf16 NaN, the byte 255.
struct FrontInput {
    GuardedOut tensor, frames;
    std::vector<uint8_t> before;         // the bytes of the input the kernels read
    LetterboxGeom g{};
    bool u8 = false;
    const GuardedOut& in() const { return u8 ? frames : tensor; }
};
int front_input(DevScratch& mem, FrontInput& fi, int b, int net_h, int net_w, const float* x, const uint8_t* frames, int h, int w, int swap_rb) {
    const size_t npix = (size_t)b * net_h * net_w;
    fi.u8 = frames != nullptr;
    if (fi.u8) {
        fi.g = letterbox_geom(h, w, net_h, net_w, swap_rb != 0);
        fi.before.assign(frames, frames + (size_t)b * h * w * 3);
        VC_TRY(fi.frames.alloc(mem, fi.before.size(), fi.before.data(), GuardedOut::kGuard, 0xFF));   // (the base is 256-byte aligned: the front kernel wants 4)
        return fi.tensor.alloc(mem, npix * 4 * 2);                                                    // all fill: no direct launch may touch it
    }
    std::vector<float> x4(npix * 4, 0.f);
    for (size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; ++c) x4[i * 4 + c] = x[i * 3 + c];
    fi.before = to_elems(x4.data(), x4.size(), PREC_BF16);
    return fi.tensor.alloc(mem, fi.before.size(), fi.before.data(), GuardedOut::kGuard, 0xFF);
}
// after the launches: the input and its guard blocks are what they were
int front_input_intact(const FrontInput& fi, const char* kernel) {
    std::vector<uint8_t> now(fi.in().bytes);
    VC_TRY(fi.in().read_back(now.data(), kernel));
    VC_CHECK(now == fi.before, VC_ERR_HIP, "%s wrote its input", kernel);
    return VC_OK;
}
bool front_args_ok(int b, int net_h, int net_w, const float* x, const uint8_t* frames, int h, int w) {
    return b >= 1 && net_h >= 2 && net_w >= 2 && net_w % 2 == 0 && (long long)b * net_h * net_w <= (1 << 22) && (x != nullptr) != (frames != nullptr) &&
           (!frames || (h >= 1 && w >= 1 && (long long)b * h * w <= (1 << 24)));
}
// guard blocks that hold every store of a th x tw output tile that lost its bounds tests (pixels of `bytes_per_pixel`)
size_t front_guard(int th, int tw, int wo, size_t bytes_per_pixel) { return ((size_t)(th * wo + tw) * bytes_per_pixel + 255) / 256 * 256; }

}  // namespace

extern "C" {

int vc_conv2d_host(const vc_conv_desc* d, const float* x, const float* w, const float* bias, const float* res, float* y) {
    VC_CHECK(d && x && w && bias && y, VC_ERR_ARG, "null argument");
    const int prec = d->precision;
    VC_CHECK(d->b >= 1 && d->h >= 1 && d->w >= 1 && d->cin >= 1 && d->cout >= 1 && d->kh >= 1 && d->kw >= 1 && d->stride >= 1 && d->pad >= 0, VC_ERR_ARG, "conv: bad shape");
    // the dense case of conv_view_run: input channels padded with zeros to the chunk (the 3 -> 8 stem padding), output rows to 4 (fp8: 8)
    const int cin_eff = round_up(d->cin, prec == PREC_F32 ? 4 : prec == PREC_FP8 ? 16 : 8), cout_s = round_up(d->cout, prec == PREC_FP8 ? 8 : 4);
    const int Ho = (d->h + 2 * d->pad - d->kh) / d->stride + 1, Wo = (d->w + 2 * d->pad - d->kw) / d->stride + 1;
    VC_CHECK(Ho >= 1 && Wo >= 1, VC_ERR_ARG, "conv: empty output");
    const size_t npix_in = (size_t)d->b * d->h * d->w, npix_out = (size_t)d->b * Ho * Wo;
    auto padded = [](const float* src, size_t npix, int C, int Cs) {
        std::vector<float> buf(npix * Cs, 0.f);
        for (size_t i = 0; i < npix; ++i)
            for (int c = 0; c < C; ++c) buf[i * Cs + c] = src[i * C + c];
        return buf;
    };
    const std::vector<float> xs = padded(x, npix_in, d->cin, cin_eff);
    const std::vector<float> rs = res ? padded(res, npix_out, d->cout, cout_s) : std::vector<float>();
    std::vector<float> ys(npix_out * cout_s, 0.f);
    vc_conv_view v{};
    v.in_cs = cin_eff; v.out_cs = cout_s; v.res_cs = cout_s; v.m_valid = -1;
    VC_TRY(conv_view_run(d, &v, xs.data(), nullptr, w, bias, res ? rs.data() : nullptr, ys.data(), nullptr));
    for (size_t i = 0; i < npix_out; ++i)
        for (int c = 0; c < d->cout; ++c) y[i * d->cout + c] = ys[i * cout_s + c];
    return VC_OK;
}

int vc_conv2d_view_host(const vc_conv_desc* d, const vc_conv_view* v, const float* x, const float* x_up, const float* w, const float* bias,
                        const float* res, float* y, float* y2) {
    VC_CHECK(d && v && x && w && bias && y, VC_ERR_ARG, "null argument");
    const int ch = d->precision == PREC_F32 ? 4 : d->precision == PREC_FP8 ? 16 : 8;
    VC_CHECK(d->cin > 0 && d->cin % ch == 0, VC_ERR_ARG, "conv view: cin %d must be a multiple of %d (vc_conv2d_host pads the stem)", d->cin, ch);
    return conv_view_run(d, v, x, x_up, w, bias, res, y, y2);
}

int vc_conv_s2_pw_host(const vc_conv_desc* d, const vc_conv_view* v, const float* x, const float* w, const float* bias, const float* w_pw,
                       const float* bias_pw, float* y, float* y2) {
    VC_CHECK(d && v && x && w && bias && w_pw && bias_pw && y, VC_ERR_ARG, "null argument");
    constexpr int CO = 128;
    VC_CHECK(d->precision == PREC_BF16 && d->kh == 3 && d->kw == 3 && d->stride == 2 && d->pad == 1 && d->cout == CO && d->act == ACT_SILU && d->res_mode == RES_NONE,
             VC_ERR_ARG, "s2 + pointwise: a bf16 3x3 / s2 / p1 conv with SiLU to 128 channels");
    VC_CHECK(d->b >= 1 && d->h >= 2 && d->w >= 2 && d->cin >= 8 && d->cin % 8 == 0, VC_ERR_ARG, "s2 + pointwise: bad shape");
    const int Ho = (d->h + 2 - 3) / 2 + 1, Wo = (d->w + 2 - 3) / 2 + 1;
    const size_t npix_in = (size_t)d->b * d->h * d->w, npix_out = (size_t)d->b * Ho * Wo;
    VC_CHECK(v->in_co >= 0 && v->in_cs >= v->in_co + d->cin, VC_ERR_ARG, "s2 + pointwise: input slice outside stride %d", v->in_cs);
    VC_CHECK(v->split >= 0 && v->split < CO && (v->split == 0 || y2), VC_ERR_ARG, "s2 + pointwise: split %d of %d channels", v->split, CO);
    VC_CHECK(v->out_co >= 0 && v->out_cs >= v->out_co + (v->split > 0 ? v->split : CO), VC_ERR_ARG, "s2 + pointwise: output slice outside stride %d", v->out_cs);
    VC_CHECK(v->split == 0 || (v->out2_co >= 0 && v->out2_cs >= v->out2_co + CO - v->split), VC_ERR_ARG, "s2 + pointwise: second output slice outside stride %d", v->out2_cs);
    DevScratch mem;
    ConvParam p3, p1;
    VC_TRY(host_param(mem, p3, "host 3x3", CO, d->cin, 3, 3, w, bias));
    VC_TRY(host_param(mem, p1, "host 1x1", CO, CO, 1, 1, w_pw, bias_pw));
    void* dx = nullptr;
    VC_TRY(upload_elems(mem, x, npix_in * v->in_cs, PREC_BF16, &dx));
    GuardedOut gmid, gy, gy2;                          // gmid: the 3x3's own output, which the fused kernel keeps on chip
    VC_TRY(gmid.alloc(mem, npix_out * CO * 2));
    const size_t ny = npix_out * v->out_cs, ny2 = npix_out * (size_t)v->out2_cs;
    VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16));
    if (v->split > 0) VC_TRY(guarded_elems(mem, gy2, y2, ny2, PREC_BF16));
    const ConvP c = conv_params(p3, {dx, v->in_cs, v->in_co}, {gmid.out(), CO, 0}, d->b, d->h, d->w, 3, 3, 2, 1, ACT_SILU, 1.0f, 1.0f);
    ConvP q = conv_params(p1, {gmid.out(), CO, 0}, {gy.out(), v->out_cs, v->out_co}, d->b, Ho, Wo, 1, 1, 1, 0, ACT_SILU, 1.0f, 1.0f);
    if (v->split > 0) { q.split = v->split; q.out2 = gy2.out(); q.out2_cs = v->out2_cs; q.out2_co = v->out2_co; }
    VC_CHECK(s2halo_pw_applicable(c, q), VC_ERR_ARG, "s2 + pointwise: the fused kernel does not take this pair");
    VC_TRY(launch_s2halo_pw(c, q, nullptr));
    VC_TRY(kernel_wait("conv3x3s2_halo_kernel"));
    {   // the 3x3's own output stays on chip: its buffer still holds the fill (unless the diagnostic VC_S2PW_STORE asks for the store)
        std::vector<uint8_t> mid(gmid.bytes);
        VC_TRY(gmid.read_back(mid.data(), "conv3x3s2_halo_kernel (the 3x3's own output)"));
        const bool also_store = getenv("VC_S2PW_STORE") && atoi(getenv("VC_S2PW_STORE")) != 0;
        for (size_t i = 0; i < mid.size() && !also_store; ++i)
            VC_CHECK(mid[i] == 0xA5, VC_ERR_HIP, "conv3x3s2_halo_kernel wrote the 3x3's own output (byte %zu)", i);
    }
    VC_TRY(read_elems(gy, ny, PREC_BF16, y, "conv3x3s2_halo_kernel"));
    if (v->split > 0) VC_TRY(read_elems(gy2, ny2, PREC_BF16, y2, "conv3x3s2_halo_kernel (second destination)"));
    return VC_OK;
}

int vc_c3_fused_host(int b, int h, int w, const vc_fused_view* v, float* x, const float* w12, const float* b12, const float* wm1, const float* bm1,
                     const float* wm2, const float* bm2, const float* w3, const float* b3, float* y) {
    VC_CHECK(v && x && w12 && b12 && wm1 && bm1 && wm2 && bm2 && w3 && b3 && (y || v->out_buf == 1), VC_ERR_ARG, "null argument");
    set_error("%s", "");                               // the launcher refuses without a message: the caller must not read an older one
    const int out_cs = v->out_buf == 1 ? v->in_cs : v->out_cs, split = v->split ? v->split : 32;
    VC_CHECK(fused_shape_ok(b, h, w) && (v->out_buf == 0 || v->out_buf == 1) && v->grid >= 0, VC_ERR_ARG, "c3 fused: bad shape");
    VC_CHECK(fused_slice_ok(v->in_cs, v->in_co, 64) && fused_slice_ok(out_cs, v->out_co, 64), VC_ERR_ARG, "c3 fused: a slice lies outside its stride");
    VC_CHECK(split >= 4 && split <= 60 && split % 4 == 0 && (split == 32 || !v->unfused), VC_ERR_ARG, "c3 fused: split %d", split);
    const size_t npix = (size_t)b * h * w, nx = npix * v->in_cs, ny = npix * out_cs;
    DevScratch mem;
    ConvParam P12, PM1, PM2, P3;
    VC_TRY(host_param(mem, P12, "cv1 | cv2", 64, 64, 1, 1, w12, b12));
    VC_TRY(host_param(mem, PM1, "m.cv1", 32, 32, 1, 1, wm1, bm1));
    VC_TRY(host_param(mem, PM2, "m.cv2", 32, 32, 3, 3, wm2, bm2));
    VC_TRY(host_param(mem, P3, "cv3", 64, 64, 1, 1, w3, b3));
    GuardedOut gx, gy, gy1, gb1, gcat;                 // gy1 / gb1 / gcat: y1, b1 and [m | y2] of the unfused graph (c3_<idx>.a, .t, .cat)
    VC_TRY(guarded_elems(mem, gx, x, nx, PREC_BF16, tile_guard(w, v->in_cs)));
    if (!v->out_buf) VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16, tile_guard(w, out_cs)));
    VC_TRY(gy1.alloc(mem, npix * 32 * 2));
    VC_TRY(gb1.alloc(mem, npix * 32 * 2));
    VC_TRY(gcat.alloc(mem, npix * 64 * 2));
    ConvP p12 = chain_conv(P12, gx.out(), v->in_cs, v->in_co, gy1.out(), 32, 0, b, h, w, ACT_SILU);
    p12.split = split; p12.out2 = gcat.out(); p12.out2_cs = 64; p12.out2_co = 32;
    const ConvP pm1 = chain_conv(PM1, gy1.out(), 32, 0, gb1.out(), 32, 0, b, h, w, ACT_SILU);
    ConvP pm2 = chain_conv(PM2, gb1.out(), 32, 0, gcat.out(), 64, 0, b, h, w, ACT_SILU);
    pm2.res = gy1.out(); pm2.res_cs = 32; pm2.res_co = 0; pm2.res_mode = RES_AFTER_ACT;
    const ConvP p3 = chain_conv(P3, gcat.out(), 64, 0, v->out_buf ? gx.out() : gy.out(), out_cs, v->out_co, b, h, w, ACT_SILU);
    VC_TRY(v->unfused ? chain_unfused({p12, pm1, pm2, p3}) : launch_c3_fused(p12, pm1, pm2, p3, nullptr, v->grid));   // refused: x / y as passed
    VC_TRY(kernel_wait("c3_fused_kernel"));
    if (!v->unfused) {
        VC_TRY(still_filled(gy1, "c3_fused_kernel", "y1"));
        VC_TRY(still_filled(gb1, "c3_fused_kernel", "b1"));
        VC_TRY(still_filled(gcat, "c3_fused_kernel", "the concat buffer [m | y2]"));
    }
    VC_TRY(read_elems(gx, nx, PREC_BF16, x, "c3_fused_kernel (the input buffer)"));
    if (!v->out_buf) VC_TRY(read_elems(gy, ny, PREC_BF16, y, "c3_fused_kernel"));
    return VC_OK;
}

int vc_bneck_fused_host(int b, int h, int w, const vc_fused_view* v, float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, float* y, float* z) {
    VC_CHECK(v && x && w1 && b1 && w2 && b2 && (y || v->out_buf == 1), VC_ERR_ARG, "null argument");
    VC_CHECK(!v->cv3 || (w3 && b3 && (z || v->z_buf != 0)), VC_ERR_ARG, "null argument (cv3)");
    set_error("%s", "");
    const char* kernel = v->cv3 ? "bneck_fused_kernel<true>" : "bneck_fused_kernel<false>";
    const int out_cs = v->out_buf == 1 ? v->in_cs : v->out_cs, z_cs = v->z_buf == 1 ? v->in_cs : v->z_buf == 2 ? out_cs : v->z_cs;
    VC_CHECK(fused_shape_ok(b, h, w) && (v->out_buf == 0 || v->out_buf == 1) && v->z_buf >= 0 && v->z_buf <= 2 && v->grid >= 0, VC_ERR_ARG, "bneck fused: bad shape");
    VC_CHECK(fused_slice_ok(v->in_cs, v->in_co, 64) && fused_slice_ok(out_cs, v->out_co, v->cv3 ? 128 : 64) && (!v->cv3 || fused_slice_ok(z_cs, v->z_co, 128)), VC_ERR_ARG,
             "bneck fused: a slice lies outside its stride");
    const size_t npix = (size_t)b * h * w, nx = npix * v->in_cs, ny = npix * out_cs, nz = npix * (size_t)z_cs;
    DevScratch mem;
    ConvParam P1, P2, P3;
    VC_TRY(host_param(mem, P1, "m.cv1", 64, 64, 1, 1, w1, b1));
    VC_TRY(host_param(mem, P2, "m.cv2", 64, 64, 3, 3, w2, b2));
    if (v->cv3) VC_TRY(host_param(mem, P3, "cv3", 128, 128, 1, 1, w3, b3));
    GuardedOut gx, gy, gz, gt;                         // gt: b1 of the unfused graph (c3_<idx>.t)
    VC_TRY(guarded_elems(mem, gx, x, nx, PREC_BF16, tile_guard(w, v->in_cs)));
    std::vector<uint8_t> y_before;                     // CV3 instance: the m slice of y must come back as it went in
    if (!v->out_buf) {
        y_before = to_elems(y, ny, PREC_BF16);
        VC_TRY(gy.alloc(mem, y_before.size(), y_before.data(), tile_guard(w, out_cs)));
    } else {
        y_before = to_elems(x, nx, PREC_BF16);
    }
    const bool own_z = v->cv3 && v->z_buf == 0;
    if (own_z) VC_TRY(guarded_elems(mem, gz, z, nz, PREC_BF16, tile_guard(w, z_cs)));
    VC_TRY(gt.alloc(mem, npix * 64 * 2));
    const GuardedOut& my = v->out_buf ? gx : gy;
    const GuardedOut& zy = v->z_buf == 1 ? gx : v->z_buf == 2 ? my : gz;
    const ConvP pm1 = chain_conv(P1, gx.out(), v->in_cs, v->in_co, gt.out(), 64, 0, b, h, w, ACT_SILU);
    ConvP pm2 = chain_conv(P2, gt.out(), 64, 0, my.out(), out_cs, v->out_co, b, h, w, ACT_SILU);
    if (v->res) { pm2.res = gx.out(); pm2.res_cs = v->in_cs; pm2.res_co = v->in_co; pm2.res_mode = RES_AFTER_ACT; }
    if (v->cv3) {
        const ConvP p3 = chain_conv(P3, my.out(), out_cs, v->out_co, zy.out(), z_cs, v->z_co, b, h, w, ACT_SILU);
        VC_TRY(v->unfused ? chain_unfused({pm1, pm2, p3}) : launch_bneck_cv3_fused(pm1, pm2, p3, nullptr, v->grid));   // refused: x / y / z as passed
    } else {
        VC_TRY(v->unfused ? chain_unfused({pm1, pm2}) : launch_bneck_fused(pm1, pm2, nullptr, v->grid));
    }
    VC_TRY(kernel_wait(kernel));
    if (!v->unfused) VC_TRY(still_filled(gt, kernel, "b1"));
    if (v->cv3 && !v->unfused) {
        std::vector<uint8_t> after(my.bytes);
        VC_TRY(my.read_back(after.data(), kernel));
        const uint16_t *a16 = (const uint16_t*)after.data(), *b16 = (const uint16_t*)y_before.data();
        for (size_t p = 0; p < npix; ++p)
            for (int c = 0; c < 64; ++c) {
                const size_t i = p * out_cs + v->out_co + c;
                VC_CHECK(a16[i] == b16[i], VC_ERR_HIP, "%s wrote m (pixel %zu, channel %d)", kernel, p, c);
            }
    }
    VC_TRY(read_elems(gx, nx, PREC_BF16, x, v->cv3 ? "bneck_fused_kernel<true> (the input buffer)" : "bneck_fused_kernel<false> (the input buffer)"));
    if (!v->out_buf) VC_TRY(read_elems(gy, ny, PREC_BF16, y, kernel));
    if (own_z) VC_TRY(read_elems(gz, nz, PREC_BF16, z, kernel));
    return VC_OK;
}

int vc_reid_block_fused_host(int k, int h, int w, const vc_fused_view* v, float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y) {
    VC_CHECK(v && x && w1 && b1 && w2 && b2 && (y || v->out_buf == 1), VC_ERR_ARG, "null argument");
    set_error("%s", "");
    const int out_cs = v->out_buf == 1 ? v->in_cs : v->out_cs;
    VC_CHECK(fused_shape_ok(k, h, w) && (v->out_buf == 0 || v->out_buf == 1) && v->grid >= 0, VC_ERR_ARG, "reid block fused: bad shape");
    VC_CHECK(fused_slice_ok(v->in_cs, v->in_co, 64) && fused_slice_ok(out_cs, v->out_co, 64), VC_ERR_ARG, "reid block fused: a slice lies outside its stride");
    const size_t npix = (size_t)k * h * w, nx = npix * v->in_cs, ny = npix * out_cs;
    DevScratch mem;
    ConvParam P1, P2;
    VC_TRY(host_param(mem, P1, "conv1", 64, 64, 3, 3, w1, b1));
    VC_TRY(host_param(mem, P2, "conv2", 64, 64, 3, 3, w2, b2));
    GuardedOut gx, gy, gt;                             // gt: t of the unfused graph
    VC_TRY(guarded_elems(mem, gx, x, nx, PREC_BF16));
    if (!v->out_buf) VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16));
    VC_TRY(gt.alloc(mem, npix * 64 * 2));
    const ConvP p1 = chain_conv(P1, gx.out(), v->in_cs, v->in_co, gt.out(), 64, 0, k, h, w, ACT_RELU);
    ConvP p2 = chain_conv(P2, gt.out(), 64, 0, v->out_buf ? gx.out() : gy.out(), out_cs, v->out_co, k, h, w, ACT_RELU);
    p2.res = gx.out(); p2.res_cs = v->in_cs; p2.res_co = v->in_co; p2.res_mode = RES_BEFORE_ACT;
    VC_TRY(v->unfused ? chain_unfused({p1, p2}) : launch_reid_block_fused(p1, p2, nullptr, v->grid));   // refused: x / y as passed
    VC_TRY(kernel_wait("reid_block_fused_kernel"));
    if (!v->unfused) VC_TRY(still_filled(gt, "reid_block_fused_kernel", "t"));
    VC_TRY(read_elems(gx, nx, PREC_BF16, x, "reid_block_fused_kernel (the input buffer)"));
    if (!v->out_buf) VC_TRY(read_elems(gy, ny, PREC_BF16, y, "reid_block_fused_kernel"));
    return VC_OK;
}

int vc_stem_host(int b, int net_h, int net_w, int cout, const vc_front_view* v, const float* x, const uint8_t* frames, int h, int w, const float* w0,
                 const float* b0, float* y, uint8_t* q8) {
    VC_CHECK(v && w0 && b0 && y, VC_ERR_ARG, "null argument");
    set_error("%s", "");                               // the launchers refuse a shape without a message: the caller must not read an older one
    VC_CHECK(front_args_ok(b, net_h, net_w, x, frames, h, w) && cout >= 1 && cout <= 1024 && v->grid_cap >= 0 && (v->mode == 0 || v->mode == 1), VC_ERR_ARG,
             "stem: bad shape");
    VC_CHECK(fused_slice_ok(v->out_cs, v->out_co, cout) && (!q8 || fused_slice_ok(v->q_cs, v->q_co, cout)), VC_ERR_ARG, "stem: a slice lies outside its stride");
    const int Ho = (net_h + 4 - 6) / 2 + 1, Wo = (net_w + 4 - 6) / 2 + 1;
    const size_t npix = (size_t)b * Ho * Wo, ny = npix * v->out_cs, nq = npix * (size_t)v->q_cs;
    DevScratch mem;
    ConvParam P;
    P.pair_stem = true;                                // yolo_define: the stem of every bf16 engine (and of the fp8 one)
    VC_TRY(host_param(mem, P, "model.0.conv", cout, 3, 6, 6, w0, b0));
    FrontInput fi;
    VC_TRY(front_input(mem, fi, b, net_h, net_w, x, frames, h, w, v->swap_rb));
    GuardedOut gy, gq;
    VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16, front_guard(8, 32, Wo, (size_t)v->out_cs * 2)));
    if (q8) VC_TRY(gq.alloc(mem, nq, q8, front_guard(8, 32, Wo, (size_t)v->q_cs)));
    ConvP c = conv_params(P, {fi.tensor.out(), 8, 0}, {gy.out(), v->out_cs, v->out_co}, b, net_h, net_w, 6, 6, 2, 2, ACT_SILU, 1.0f, 1.0f);
    const View yv{gy.out(), b, Ho, Wo, cout, v->out_cs, v->out_co, 2}, qv{q8 ? gq.out() : nullptr, b, Ho, Wo, cout, v->q_cs, v->q_co, 1};
    const char* kernel = v->mode == 0 ? "the unfused stem" : cout == 80 ? "stem_direct_wide_kernel" : "stem_direct_kernel";
    if (v->mode == 1) {                                // refused: y / q8 as passed
        if (fi.u8) VC_TRY(launch_stem_direct_u8(c, fi.frames.out(), fi.g, nullptr, q8 ? &qv : nullptr, v->inv_scale, v->grid_cap));
        else if (!stem_direct_applicable(c)) return VC_ERR_ARG;
        else VC_TRY(launch_stem_direct(c, nullptr, q8 ? &qv : nullptr, v->inv_scale, v->grid_cap));
    } else {                                           // what the engine runs with option "stem_direct" 0: letterbox, launch_conv, the bf16 -> fp8 launch
        conv_env(c, true);
        if (fi.u8) VC_TRY(launch_letterbox(fi.frames.out(), fi.tensor.out(), b, fi.g, PREC_BF16, nullptr));
        VC_TRY(launch_conv(c, nullptr));
        if (q8) VC_TRY(launch_bf16_to_fp8(yv, qv, v->inv_scale, nullptr));
    }
    VC_TRY(kernel_wait(kernel));
    VC_TRY(front_input_intact(fi, kernel));
    if (fi.u8 && v->mode == 1) VC_TRY(still_filled(fi.tensor, kernel, "the letterboxed tensor"));
    std::vector<uint8_t> qh(nq);                       // both outputs checked before either array of the caller changes
    if (q8) VC_TRY(gq.read_back(qh.data(), kernel));
    VC_TRY(read_elems(gy, ny, PREC_BF16, y, kernel));
    if (q8) memcpy(q8, qh.data(), nq);
    return VC_OK;
}

int vc_front_fused_host(int b, int net_h, int net_w, int cout1, const vc_front_view* v, const float* x, const uint8_t* frames, int h, int w, const float* w0,
                        const float* b0, const float* w1, const float* b1, float* y) {
    VC_CHECK(v && w0 && b0 && w1 && b1 && y, VC_ERR_ARG, "null argument");
    set_error("%s", "");
    VC_CHECK(front_args_ok(b, net_h, net_w, x, frames, h, w) && net_h >= 4 && net_w >= 4 && cout1 >= 1 && cout1 <= 1024 && v->grid_cap >= 0 && (v->mode == 0 || v->mode == 1),
             VC_ERR_ARG, "front fused: bad shape");
    VC_CHECK(fused_slice_ok(v->out_cs, v->out_co, cout1), VC_ERR_ARG, "front fused: a slice lies outside its stride");
    constexpr int C0 = 32;
    const int H0 = (net_h + 4 - 6) / 2 + 1, W0 = (net_w + 4 - 6) / 2 + 1, H1 = (H0 + 2 - 3) / 2 + 1, W1 = (W0 + 2 - 3) / 2 + 1;
    const size_t npix0 = (size_t)b * H0 * W0, ny = (size_t)b * H1 * W1 * v->out_cs;
    DevScratch mem;
    ConvParam P0, P1;
    P0.pair_stem = true;
    VC_TRY(host_param(mem, P0, "model.0.conv", C0, 3, 6, 6, w0, b0));
    VC_TRY(host_param(mem, P1, "model.1.conv", cout1, C0, 3, 3, w1, b1));
    FrontInput fi;
    VC_TRY(front_input(mem, fi, b, net_h, net_w, x, frames, h, w, v->swap_rb));
    GuardedOut gl0, gy;                                // gl0: layer 0, which the fused kernel keeps on chip (ybuf["l0"])
    VC_TRY(gl0.alloc(mem, npix0 * C0 * 2));
    VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16, front_guard(16, 16, W1, (size_t)v->out_cs * 2)));
    ConvP p0 = conv_params(P0, {fi.tensor.out(), 8, 0}, {gl0.out(), C0, 0}, b, net_h, net_w, 6, 6, 2, 2, ACT_SILU, 1.0f, 1.0f);
    ConvP p1 = conv_params(P1, {gl0.out(), C0, 0}, {gy.out(), v->out_cs, v->out_co}, b, H0, W0, 3, 3, 2, 1, ACT_SILU, 1.0f, 1.0f);
    const char* kernel = v->mode == 0 ? "the unfused front" : "front_fused_kernel";
    if (v->mode == 1) {                                // refused: y as passed
        if (!front_fused_applicable(p0, p1)) return VC_ERR_ARG;
        p0.slots = v->grid_cap;                        // the field the engine's conv_slots uses; tile_ctr stays null: the fixed stride
        VC_TRY(launch_front_fused(p0, p1, fi.u8 ? fi.frames.out() : nullptr, fi.g, nullptr));
    } else {
        conv_env(p0, false); conv_env(p1, false);
        if (fi.u8) VC_TRY(launch_letterbox(fi.frames.out(), fi.tensor.out(), b, fi.g, PREC_BF16, nullptr));
        VC_TRY(launch_conv(p0, nullptr));
        VC_TRY(launch_conv(p1, nullptr));
    }
    VC_TRY(kernel_wait(kernel));
    VC_TRY(front_input_intact(fi, kernel));
    if (v->mode == 1) {
        VC_TRY(still_filled(gl0, kernel, "layer 0"));
        if (fi.u8) VC_TRY(still_filled(fi.tensor, kernel, "the letterboxed tensor"));
    }
    return read_elems(gy, ny, PREC_BF16, y, kernel);
}

int vc_reid_stem_pool_host(const float* crops, int k, const float* w, const float* bias, float* out) {
    VC_CHECK(crops && w && bias && out && k >= 1, VC_ERR_ARG, "reid stem: bad argument");
    constexpr int S = VC_REID_SIZE, P = (S - 1) / 2 + 1, CO = 64;
    DevScratch mem;
    ConvParam p;
    VC_TRY(host_param(mem, p, "host", CO, 3, 3, 3, w, bias));
    const size_t npix = (size_t)k * S * S;
    std::vector<float> x8(npix * p.cin_eff, 0.f);                     // channels 3 .. cin_eff - 1 stay zero, as in the ReID input buffer
    for (size_t i = 0; i < npix; ++i)
        for (int ch = 0; ch < 3; ++ch) x8[i * p.cin_eff + ch] = crops[i * 3 + ch];
    void* dx = nullptr;
    VC_TRY(upload_elems(mem, x8.data(), x8.size(), PREC_BF16, &dx));
    GuardedOut dd;
    const size_t n = (size_t)k * P * P * CO;
    VC_TRY(dd.alloc(mem, n * 2));
    const ConvP cp = conv_params(p, {dx, p.cin_eff, 0}, {nullptr, CO, 0}, k, S, S, 3, 3, 1, 1, ACT_RELU, 1.0f, 1.0f);   // the conv's own output never exists
    VC_CHECK(reid_stem_applicable(cp, CO, 0), VC_ERR_ARG, "reid stem: the fused kernel does not take this convolution");
    VC_TRY(launch_reid_stem_pool(cp, dd.out(), nullptr));
    return read_elems(dd, n, PREC_BF16, out, "reid_stem_pool_kernel");
}

}  // extern "C"
