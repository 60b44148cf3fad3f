// Execution of the op plans engine_plan.hip builds: tile autotuning, kernel selection and accounting per conv launch, the detector
// and ReID passes.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "engine.h"

namespace vc {

// Pick the fastest tile configuration for a conv launch by timing every candidate once per (layer shape, problem-size
// bucket).  Results are identical across the implicit-GEMM configurations (same K order, fp32 accumulate); the halo-staged 3x3
// variants sum the K tiles slice-major and can differ from them in the last bf16 bit of a few values.
// VC_TUNE_CACHE=<file> persists the choices across processes (used for clean rocprofv3 passes: a first run writes the file, the
// profiled run reads it and launches no tuning candidates; also what makes a bf16 engine bit-reproducible across processes).
// Within a process the choices are shared by all engines of a device (g_tuned): a second engine neither re-times the candidates
// nor picks the other member of a near-tie, so two engines of one process agree bit for bit.
static std::string tune_key(const ConvP& c) {
    int bucket = 1;
    while (bucket < c.M) bucket <<= 1;
    char k[160];
    snprintf(k, sizeof(k), "p%d_ci%d_co%d_k%dx%d_s%d_h%d_w%d_K%d_m%d_sp%d%s", c.prec, c.Cin, c.Cout, c.kh, c.kw, c.sh, c.H, c.W, c.K, bucket, c.split,
             c.in_up ? "_up" : "");      // (the upsample fold-in runs on a subset of the tile configurations)
    return k;
}

static std::mutex g_tune_mu;
static std::map<std::string, int> g_tuned;          // "d<device>_<tune_key>" -> tile configuration

void tune_cache_load(vc_engine* e) {
    const char* path = getenv("VC_TUNE_CACHE");
    if (!path) return;
    FILE* f = fopen(path, "r");
    if (!f) return;
    char k[200];
    int cfg;
    while (fscanf(f, "%199s %d", k, &cfg) == 2) e->tuned[k] = cfg;
    fclose(f);
}

void tune_cache_save(vc_engine* e) {
    const char* path = getenv("VC_TUNE_CACHE");
    if (!path || !e->tuned_dirty) return;
    FILE* f = fopen(path, "w");
    if (!f) return;
    for (const auto& kv : e->tuned) fprintf(f, "%s %d\n", kv.first.c_str(), kv.second);
    fclose(f);
}

// after vc_tune_import: the engines of this process on the same device follow (tuned_cfg consults g_tuned before timing anything)
void tune_cache_publish(vc_engine* e) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    for (const auto& kv : e->tuned) g_tuned["d" + std::to_string(e->cfg.device) + "_" + kv.first] = kv.second;
}

// A cached op resolved its tile configuration at its first launch, for the kernel variant the options selected then (the upsample
// fold-in runs on a subset of the tiles and has its own tune key): after an option switch or an import every op goes back to
// tuned_cfg.
void plans_retune(vc_engine* e) {
    for (auto& kv : e->yolo_plans) for (Op& op : kv.second.ops) op.tuned = -2;
    for (auto& kv : e->reid_plans) for (Op& op : kv.second.ops) op.tuned = -2;
}

static int tuned_cfg(vc_engine* e, const ConvP& c, hipStream_t s) {
    static const bool enabled = !(getenv("VC_AUTOTUNE") && atoi(getenv("VC_AUTOTUNE")) == 0);
    if (!enabled) return -1;
    // VC_TUNE_WREG (tests, A/B; read per op, not per process): no autotuning at all.  1: every conv conv1x1_wreg_kernel takes runs on the
    // family's first id for it, everything else on the heuristic's tile; 0: the heuristic's tile everywhere.  The two differ in that family alone.
    if (const char* fw = getenv("VC_TUNE_WREG")) return atoi(fw) != 0 ? wreg_cfg_for(c) : -1;
    const std::string key = tune_key(c);
    auto it = e->tuned.find(key);
    if (it != e->tuned.end()) return it->second;
    const std::string gkey = "d" + std::to_string(e->cfg.device) + "_" + key;
    {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        auto g = g_tuned.find(gkey);
        if (g != g_tuned.end()) { e->tuned[key] = g->second; e->tuned_dirty = true; return g->second; }
    }
    int best = -1;
    float best_ms = 1e30f;
    static const bool stream_on = getenv("VC_CONV_STREAM") && atoi(getenv("VC_CONV_STREAM")) != 0;   // conv1x1_stream_kernel: wins alone, loses beside the ReID queue (conv_pointwise.hip)
    for (int cfg = 0; cfg < conv_num_cfgs(); ++cfg) {
        if (conv_stream_cfg(cfg) && !stream_on) continue;
        if (launch_conv_cfg(c, cfg, s) != VC_OK) continue;          // warm-up (instruction cache, L2)
        float tmin = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e->ev0, s);
            launch_conv_cfg(c, cfg, s);
            hipEventRecord(e->ev1, s);
            hipEventSynchronize(e->ev1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e->ev0, e->ev1);
            tmin = std::min(tmin, ms);
        }
        static const bool tlog = getenv("VC_TUNE_LOG") != nullptr;      // diagnostics: every candidate's time
        if (tlog) fprintf(stderr, "[vc tune] %s cfg %d %.4f ms\n", key.c_str(), cfg, tmin);
        if (tmin < best_ms) { best_ms = tmin; best = cfg; }
    }
    e->tuned[key] = best;
    e->tuned_dirty = true;
    {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        g_tuned.emplace(gkey, best);
    }
    return best;
}

// in-flight profiling of one conv launch (see vc_engine::prof_async): the launch itself reports its start / stop timestamps
// into an event pair (hipExtLaunchKernel), no host wait
static void conv_timer_arm(vc_engine* e, ConvP& cp, double flops, double bytes, const Op& op) {
    if (!e->prof_async || e->profiling || e->prof_used >= e->prof_pairs.size()) return;
    vc_engine::ProfPair& pp = e->prof_pairs[e->prof_used++];
    pp.flops = flops; pp.bytes = bytes;
    pp.rows = op.rows_level >= 0 && e->h_hc_ring ? e->h_hc_ring + (size_t)e->hc_ring_cur * 4 + op.rows_level : nullptr;
    pp.flops_per_row = op.flops_per_row; pp.bytes_per_row = op.bytes_per_row;
    pp.flops_dense = op.dense_flops >= 0 ? op.dense_flops : -1; pp.bytes_dense = op.dense_bytes >= 0 ? op.dense_bytes : -1;   // -1: same as executed
    cp.ev_start = pp.a; cp.ev_stop = pp.b;
}

// What runs for a CONV op: conv_select decides it anew in every pass (it depends on the options, on e->stem_src and on the ops that follow); the CONV case of
// run_ops_body launches and accounts for whatever it chose.  A new fused kernel is one more `if` in conv_select.
struct ConvCtx {                         // what a launcher works on
    vc_engine* e;
    ConvP& cp;                           // this pass's copy of op[0].conv (upsample fold-in, event pair, cfg)
    Op* op; size_t left;                 // op[0 .. left): the op being launched and the ones after it
    hipStream_t s;
    bool u8_src = false;                 // the letterbox was skipped for this pass: the stem kernels read e->stem_src (run_detector_dev)
    const View* q8 = nullptr;            // stem_direct, fp8 engine: the e4m3 copy of its output that the stem writes as well
};
struct ConvLaunch {
    int (*launch)(ConvCtx&);
    int n_ops;                           // ops the launch does: op[0 .. n_ops)
    int cfg;
    double flops, bytes;                 // the work it is credited with
    int N, K, kh, kw, sh;                // what its op_log line prints
};
static double conv_flops(const Op& o) { return 2.0 * o.conv.M * (double)o.conv.Cout * o.C; }

// fl, by: the work of op[0] alone.  Multi-op fusions first, then the single-launch stems, then the tile kernels.
static int conv_select(ConvCtx& c, double fl, double by, ConvLaunch& L) {
    vc_engine* e = c.e;
    ConvP& cp = c.cp;
    Op& op = *c.op;
    const double es = elem_size(cp.prec);
    auto conv_at = [&](size_t j) -> const Op* { return j < c.left && c.op[j].kind == Op::CONV ? &c.op[j] : nullptr; };
    const Op *nx = c.left > 1 ? &c.op[1] : nullptr, *o1 = conv_at(1), *o2 = conv_at(2), *o3 = conv_at(3);
    const double in_bytes = (double)cp.B * cp.H * cp.W * cp.Cin * es;
    auto w_bytes = [&](const Op& o) { return (double)o.conv.Cout * o.conv.K * es; };
    auto out_bytes = [&](const Op& o) { return (double)o.conv.M * o.conv.Cout * es; };
    L = {nullptr, 1, -1, fl, by, op.conv.Cout, op.conv.K, op.conv.kh, op.conv.kw, op.conv.sh};
    auto fused = [&](int cfg, int n_ops, double flops, double bytes, int N, int K, int k, int sh) {
        L.cfg = cfg; L.n_ops = n_ops; L.flops = flops; L.bytes = bytes; L.N = N; L.K = K; L.kh = L.kw = k; L.sh = sh;
    };

    const bool front_ok = e->opt.front_fused > 0 && o1 && front_fused_applicable(cp, o1->conv);
    c.u8_src = e->stem_src && cp.in == e->ybuf["in"].ptr;
    const bool stem_ok = e->opt.stem_direct != 0 && stem_direct_applicable(cp);
    if (c.u8_src && !((stem_ok && stem_u8_applicable(cp, e->stem_geom)) || (front_ok && front_fused_resize_ok(e->stem_geom)))) {
        // run_detector_dev decided the fold-in from the engine's widths, this op list decides which kernel runs: should they ever
        // disagree (a plan or layout change, option "stem_direct" 0), the letterbox kernel runs now and the pass goes on from its tensor
        ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, c.s);
        VC_TRY(launch_letterbox(e->stem_src, e->ybuf["in"].ptr, cp.B, e->stem_geom, e->aux_prec, c.s));
        e->stem_src = nullptr; e->in_stale = false;
        c.u8_src = false;
    }
    if (e->opt.c3_fused != 0 && o1 && o2 && o3 && c3_fused_applicable(cp, o1->conv, o2->conv, o3->conv)) {
        // the first C3 block in one kernel (c3_fused.hip): y1, y2, b1, m stay in LDS
        fused(103, 4, fl + conv_flops(*o1) + conv_flops(*o2) + conv_flops(*o3),
              in_bytes + w_bytes(op) + w_bytes(*o1) + w_bytes(*o2) + w_bytes(*o3) + out_bytes(*o3), 64, 64, 1, 1);
        cp.ablate = e->opt.c3_ablate;
        cp.slots = e->conv_slots; cp.tile_ctr = tile_ctr_next(e, 2);
        L.launch = [](ConvCtx& x) { return launch_c3_fused(x.cp, x.op[1].conv, x.op[2].conv, x.op[3].conv, x.s); };
    } else if (e->opt.reid_block_fused != 0 && o1 && reid_block_fused_applicable(cp, o1->conv)) {
        // a 64-channel ReID BasicBlock in one kernel (reid_block_fused.hip): x in, both weights, y out
        fused(106, 2, fl + conv_flops(*o1), in_bytes + w_bytes(op) + w_bytes(*o1) + out_bytes(*o1), 64, 1152, 3, 1);
        L.launch = [](ConvCtx& x) { return launch_reid_block_fused(x.cp, x.op[1].conv, x.s); };
    } else if (e->opt.bneck_fused != 0 && e->opt.bneck_cv3 != 0 && o1 && o2 && bneck_cv3_fused_applicable(cp, o1->conv, o2->conv)) {
        // the last 64-channel Bottleneck of a C3 + the block's cv3 in one kernel; cv3 reads the 64 channels of y2 beside the input
        fused(105, 3, fl + conv_flops(*o1) + conv_flops(*o2),
              (double)cp.B * cp.H * cp.W * (cp.Cin + 64) * es + w_bytes(op) + w_bytes(*o1) + w_bytes(*o2) + out_bytes(*o2), 128, 768, 3, 1);
        cp.tile_ctr = tile_ctr_next(e, 4);
        L.launch = [](ConvCtx& x) { return launch_bneck_cv3_fused(x.cp, x.op[1].conv, x.op[2].conv, x.s); };
    } else if (e->opt.bneck_fused != 0 && o1 && bneck_fused_applicable(cp, o1->conv)) {
        // 64-channel Bottleneck in one kernel (bneck_fused.hip)
        fused(104, 2, fl + conv_flops(*o1), in_bytes + w_bytes(op) + w_bytes(*o1) + out_bytes(*o1), 64, 640, 3, 1);
        cp.tile_ctr = tile_ctr_next(e, 4);
        L.launch = [](ConvCtx& x) { return launch_bneck_fused(x.cp, x.op[1].conv, x.s); };
    } else if (e->opt.fuse_s2_pw != 0 && op.sole_reader_next && o1 && s2halo_pw_applicable(cp, o1->conv)) {
        // a 3x3 / s2 conv and the pointwise conv that alone reads it in one launch (conv3x3s2_halo_kernel<..., F2>): YOLOv5s layer 3 +
        // C3.cv1 | cv2 of layer 4; x in, both weights, cv1 | cv2 out
        fused(107, 2, fl + conv_flops(*o1), in_bytes + w_bytes(op) + w_bytes(*o1) + out_bytes(*o1), 128, cp.K + 128, 3, 2);
        L.launch = [](ConvCtx& x) {
            VC_TRY(launch_s2halo_pw(x.cp, x.op[1].conv, x.s));
            static const bool also_store = getenv("VC_S2PW_STORE") && atoi(getenv("VC_S2PW_STORE")) != 0;   // diagnostics: the fused kernel also stores the 3x3's output
            if (!also_store) x.e->s2pw_folded.push_back(x.op->conv);   // its own output stays unwritten (vc_detect_debug_layer produces it on demand)
            return (int)VC_OK;
        };
    } else if (front_ok && (e->opt.front_fused == 2 || c.u8_src)) {      // option: 0 off, 1 only with u8 frames (stream path), 2 always
        // YOLO layers 0 + 1 in one kernel (front_fused.hip): layer 0 never reaches HBM.  The log line keeps the stem's own N / K / k / s.
        L.cfg = 102; L.n_ops = 2; L.flops = fl + conv_flops(*o1); L.bytes = in_bytes + w_bytes(op) + w_bytes(*o1) + out_bytes(*o1);
        cp.ablate = e->opt.ff_ablate;
        cp.slots = e->conv_slots; cp.tile_ctr = tile_ctr_next(e, 1);
        L.launch = [](ConvCtx& x) {
            VC_TRY(launch_front_fused(x.cp, x.op[1].conv, x.u8_src ? x.e->stem_src : nullptr, x.e->stem_geom, x.s));
            x.e->l0_stale = true;                                     // layer 0 lived in LDS only
            return (int)VC_OK;
        };
    } else if (stem_ok) {
        // YOLO stem, bf16: direct convolution (stem_direct.hip).  fp8 engine: the stem also writes the e4m3 copy the next layer reads
        // (TO_FP8 of its own output, folded in)
        L.cfg = 100;
        if (nx && nx->kind == Op::TO_FP8 && nx->a.ptr == cp.out && nx->a.co == cp.out_co) { c.q8 = &nx->b; L.n_ops = 2; }
        L.launch = [](ConvCtx& x) {
            return x.u8_src ? launch_stem_direct_u8(x.cp, x.e->stem_src, x.e->stem_geom, x.s, x.q8, 1.0f / x.e->act_scale)   // letterbox folded in
                            : launch_stem_direct(x.cp, x.s, x.q8, 1.0f / x.e->act_scale);
        };
    } else if (nx && nx->kind == Op::MAXPOOL && nx->a.ptr == cp.out && reid_stem_applicable(cp, nx->b.cs, nx->b.co)) {
        // ReID stem: conv + ReLU + MaxPool in one kernel (reid_stem.hip)
        L.cfg = 101; L.n_ops = 2;
        L.launch = [](ConvCtx& x) { return launch_reid_stem_pool(x.cp, x.op[1].b.ptr, x.s); };
    } else {
        if (op.tuned == -2) op.tuned = cp.m_dev ? -1 : tuned_cfg(e, cp, c.s);   // a device-side row count: the implicit-GEMM heuristic (the only family that honours it)
        L.cfg = op.tuned;
        L.launch = [](ConvCtx& x) { return launch_conv(x.cp, x.s); };
    }
    return VC_OK;
}

// rec: the launch recorder of an armed pass (engine_record.hip), null otherwise -- one pointer test per launch
static int run_ops_body(vc_engine* e, std::vector<Op>& ops, int aux_cat, hipStream_t s_main, bool& side_used, LaunchRecorder* rec) {
    // Op::side ops go to the head stream (detector passes only; not while every launch is bracketed by blocking events): the first of a run
    // of them waits for everything the main stream has been given so far, the caller joins the head stream before it reads their results
    const bool side_ok = s_main == e->dstream && e->hstream && e->opt.head_side && !e->profiling;
    bool prev_side = false;
    const Op* pending_up = nullptr;          // an UPSAMPLE op whose consumer (the next op) reads the half-size map itself
    for (size_t oi = 0; oi < ops.size(); ++oi) {
        Op& op = ops[oi];
        const bool on_side = side_ok && op.side;
        if (on_side && !prev_side) {
            VC_HIP(hipEventRecord(e->ev_fork, s_main));
            VC_HIP(hipStreamWaitEvent(e->hstream, e->ev_fork, 0));
            side_used = true;
        }
        prev_side = on_side;
        hipStream_t s = on_side ? e->hstream : s_main;
        switch (op.kind) {
            case Op::CONV: {
                const double es = elem_size(op.conv.prec);
                const double fl = op.flops_override >= 0 ? op.flops_override : 2.0 * op.conv.M * (double)(op.cout_logical ? op.cout_logical : op.conv.Cout) * op.C;
                double by = op.bytes_override >= 0 ? op.bytes_override
                                                   : ((double)op.conv.B * op.conv.H * op.conv.W * op.conv.Cin + (double)op.conv.Cout * op.conv.K) * es +
                                                         (double)op.conv.M * op.conv.Cout * (op.conv.out_f32 ? 4 : es);
                if (pending_up) by -= 0.75 * (double)op.conv.M * pending_up->a.C * es;   // (folded upsample: three quarters of that half of the input are never read)
                ConvP cp = op.conv;
                if (pending_up) {                                             // Upsample + Concat folded into this pointwise conv (conv_igemm_kernel<..., UP>)
                    const View& u = pending_up->a;
                    cp.in_up = u.ptr; cp.up_C = u.C; cp.up_cs = u.cs; cp.up_co = u.co;
                    pending_up = nullptr;
                }
                ConvCtx cx{e, cp, &op, ops.size() - oi, s};
                ConvLaunch L;
                VC_TRY(conv_select(cx, fl, by, L));
                cp.cfg = L.cfg;
                if (rec) VC_TRY(record_before(rec, e, &op, L.n_ops, L.cfg, &cp, cx.u8_src, on_side, s));
                conv_timer_arm(e, cp, L.flops, L.bytes, op);
                {
                    ProfScope ps(e, VC_PROF_CONV, L.flops, L.bytes, s);
                    VC_TRY(L.launch(cx));
                }
                if (rec) VC_TRY(record_after(rec, s));
                double fl_exec = L.flops;                                     // executed FLOPs: differ where the row count lives on the device
                if (e->profiling && (op.rows_level >= 0 || op.dense_flops >= 0)) {   // sparse head, blocking profile: the scope has synchronised
                    ProfCat& pc = e->prof[VC_PROF_CONV];
                    double be = L.bytes;
                    if (op.rows_level >= 0) {                                 // executed work = fixed part + gathered rows x per-row work
                        int rows = 0;
                        VC_HIP(hipMemcpy(&rows, e->d_hc_count + op.rows_level, sizeof(int), hipMemcpyDeviceToHost));
                        rows = std::min(rows, e->hc_cap[op.rows_level]);
                        fl_exec += rows * op.flops_per_row; be += rows * op.bytes_per_row;
                        pc.flops += fl_exec - L.flops; pc.bytes += be - L.bytes;
                    }
                    // the scope credited (flops, bytes) to the dense-equivalent accumulators as well: replace them by the dense head's figures
                    pc.flops_dense += (op.dense_flops >= 0 ? op.dense_flops : fl_exec) - L.flops;
                    pc.bytes_dense += (op.dense_bytes >= 0 ? op.dense_bytes : be) - L.bytes;
                }
                if (e->profiling && e->op_log.size() < (1u << 20)) {
                    char line[256];
                    snprintf(line, sizeof(line), "%s M=%d N=%d K=%d k=%dx%d s=%d cfg=%d ms=%.4f tflops=%.1f\n", cp.M > 0 ? "conv" : "?", cp.M, L.N, L.K, L.kh, L.kw,
                             L.sh, L.cfg, e->last_ms, fl_exec / (e->last_ms * 1e-3) / 1e12);
                    e->op_log += line;
                }
                oi += L.n_ops - 1;                                            // the ops the launch swallowed are done
                break;
            }
            case Op::SPPF: {
                if (rec) VC_TRY(record_before(rec, e, &op, 1, -1, nullptr, false, on_side, s));
                { ProfScope ps(e, aux_cat, 0, 0, s); VC_TRY(launch_sppf_pool(op.a, op.C, e->prec, e->opt.sppf_sep, s)); }
                if (rec) VC_TRY(record_after(rec, s));
                break;
            }
            case Op::UPSAMPLE: {
                // bf16: when the consumer is the pointwise conv over [upsampled | skip] (C3.cv1 | cv2 of layers 13 / 17) it reads the half-size
                // map itself; the slice of the concat buffer stays unwritten (vc_detect_debug_layer produces it on demand)
                const Op* nx = oi + 1 < ops.size() ? &ops[oi + 1] : nullptr;
                const bool fold = e->opt.fuse_upsample && e->prec == PREC_BF16 && nx && nx->kind == Op::CONV && nx->conv.prec == PREC_BF16 && nx->conv.kh == 1 &&
                                  nx->conv.kw == 1 && nx->conv.sh == 1 && nx->conv.ph == 0 && !nx->conv.m_dev && nx->conv.in == op.b.ptr && nx->conv.in_co == op.b.co &&
                                  nx->conv.in_cs == op.b.cs && nx->conv.H == 2 * op.a.H && nx->conv.W == 2 * op.a.W && op.a.C % 64 == 0 && nx->conv.Cin % 64 == 0 &&
                                  op.a.C < nx->conv.Cin && op.a.cs % 8 == 0 && op.a.co % 8 == 0;
                if (fold) { pending_up = &op; e->up_folded.push_back({op.a, op.b}); break; }
                if (rec) VC_TRY(record_before(rec, e, &op, 1, -1, nullptr, false, on_side, s));
                { ProfScope ps(e, aux_cat, 0, 0, s); VC_TRY(launch_upsample2x(op.a, op.b, e->prec, s)); }
                if (rec) VC_TRY(record_after(rec, s));
                break;
            }
            case Op::MAXPOOL: {                                                   // ReID only
                if (rec) VC_TRY(record_before(rec, e, &op, 1, -1, nullptr, false, on_side, s));
                { ProfScope ps(e, aux_cat, 0, 0, s); VC_TRY(launch_maxpool3s2(op.a, op.b, e->aux_prec, s)); }
                if (rec) VC_TRY(record_after(rec, s));
                break;
            }
            case Op::TO_FP8: {
                if (rec) VC_TRY(record_before(rec, e, &op, 1, -1, nullptr, false, on_side, s));
                { ProfScope ps(e, aux_cat, 0, 0, s); VC_TRY(launch_bf16_to_fp8(op.a, op.b, 1.0f / e->act_scale, s)); }
                if (rec) VC_TRY(record_after(rec, s));
                break;
            }
            case Op::HEAD_COMPACT: {
                if (rec) VC_TRY(record_before(rec, e, &op, 1, -1, nullptr, false, on_side, s));
                {
                    ProfScope ps(e, aux_cat, 0, 0, s);
                    const int i = op.level, M = op.a.B * op.a.H * op.a.W;
                    VC_TRY(launch_head_compact(e->d_obj[i], op.a, M, op.a.H * op.a.W, e->cfg.conf_thres, e->hc_cap[i], e->d_hc_count + i, e->d_hc_list[i], e->d_hc_x[i],
                                               e->post.overflow, s));
                }
                if (rec) VC_TRY(record_after(rec, s));
                break;
            }
        }
    }
    return VC_OK;
}

// The join (head stream -> main stream) of the ops that forked onto the head stream is recorded HERE, on the error path too:
// a pass that failed after the fork must not leave head ops running beside the next pass's memset of the counters they write.
static int run_ops(vc_engine* e, std::vector<Op>& ops, int aux_cat, hipStream_t s_main, LaunchRecorder* rec) {
    bool forked = false;
    const int st = run_ops_body(e, ops, aux_cat, s_main, forked, rec);
    if (forked) {                                            // the P3 / P4 head ops ran on the head stream: whatever follows on the main stream waits for them
        const hipError_t e1 = hipEventRecord(e->ev_join, e->hstream);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(s_main, e->ev_join, 0) : e1;
        if (st == VC_OK && e2 != hipSuccess) { set_error("head stream join failed: %s", hipGetErrorString(e2)); return VC_ERR_HIP; }
    }
    return st;
}

// AutoShape geometry: models/common.py::AutoShape.forward + utils/augmentations.py::letterbox (auto=False)
static int py_round(double x) { return (int)std::nearbyint(x); }     // banker's rounding like Python 3 round()

void autoshape_net_size(const int* h, const int* w, int n, int size, int& nh, int& nw) {
    double mh = 0, mw = 0;
    for (int i = 0; i < n; ++i) {
        const double g = (double)size / std::max(h[i], w[i]);
        mh = std::max(mh, h[i] * g); mw = std::max(mw, w[i] * g);
    }
    nh = (int)std::ceil(mh / 32.0) * 32; nw = (int)std::ceil(mw / 32.0) * 32;
}

LetterboxGeom letterbox_geom(int h0, int w0, int nh, int nw, bool swap_rb) {
    LetterboxGeom g{};
    g.src_h = h0; g.src_w = w0; g.net_h = nh; g.net_w = nw;
    const double r = std::min((double)nh / h0, (double)nw / w0);
    g.unpad_w = py_round(w0 * r); g.unpad_h = py_round(h0 * r);
    const double dw = (nw - g.unpad_w) / 2.0, dh = (nh - g.unpad_h) / 2.0;
    g.top = py_round(dh - 0.1); g.left = py_round(dw - 0.1);
    g.swap_rb = swap_rb ? 1 : 0;
    return g;
}

int yolo_forward(vc_engine* e, int B, int nh, int nw) {
    hipStream_t ds = e->dstream;
    const bool sparse = e->prec == PREC_BF16 && e->opt.sparse_head && !e->want_pred_debug && e->d_hc_count;
    YoloPlan& plan = e->yolo_plans[{B, nh, nw, sparse ? 1 : 0}];
    if (plan.ops.empty()) VC_TRY(yolo_build_ops(e, B, nh, nw, sparse, plan));
    e->last_plan = &plan;                                    // (std::map nodes stay where they are)
    e->l0_stale = false;
    e->up_folded.clear();
    e->s2pw_folded.clear();
    if (sparse) {                                            // the compaction sets overflow flags and counts: clear them ahead of the ops
        e->hc_ring_cur = (int)(e->hc_ring_seq++ % vc_engine::HC_RING);
        VC_HIP(hipMemsetAsync(e->d_zero, 0, e->zero_bytes, ds));
    }
    LaunchRecorder* rec = nullptr;
    if (e->rec_armed) VC_TRY(record_begin(e, VC_NET_YOLO, plan.ops, &rec));
    VC_TRY(run_ops(e, plan.ops, VC_PROF_DETECT_AUX, ds, rec));     // (joins the head stream before it returns: the decode reads the head ops' rows)
    if (sparse && e->prof_async && e->h_hc_ring)     // executed-work accounting: this pass's gathered-row counts, next to the event pairs
        VC_HIP(hipMemcpyAsync(e->h_hc_ring + (size_t)e->hc_ring_cur * 4, e->d_hc_count, 4 * sizeof(int), hipMemcpyDeviceToHost, ds));
    // decode + NMS
    const int nc = e->cfg.num_classes, no = nc + 5, lcs = round_up(3 * no, 8);
    DecodeLevel lv[3];
    int base = 0;
    const int strides[3] = {8, 16, 32};
    for (int i = 0; i < 3; ++i) {
        lv[i].logits = e->d_logits[i]; lv[i].bf16 = e->prec == PREC_F32 ? 0 : 1; lv[i].ny = nh / strides[i]; lv[i].nx = nw / strides[i]; lv[i].cs = lcs;
        lv[i].stride = (float)strides[i];
        for (int a = 0; a < 3; ++a) { lv[i].anchor_w[a] = e->anchors[i][2 * a]; lv[i].anchor_h[a] = e->anchors[i][2 * a + 1]; }
        lv[i].base = base;
        base += 3 * lv[i].ny * lv[i].nx;
    }
    e->last_B = B; e->last_nh = nh; e->last_nw = nw; e->last_ntotal = base;
    float* dbg = nullptr;
    if (e->want_pred_debug) {
        if (!e->d_pred_debug) {
            const int S = round_up(e->cfg.img_size, 32);
            const size_t nmax = (size_t)3 * ((S / 8) * (S / 8) + (S / 16) * (S / 16) + (S / 32) * (S / 32));
            VC_TRY(dev_alloc(e, (void**)&e->d_pred_debug, (size_t)e->cfg.max_batch * nmax * no * sizeof(float)));
        }
        dbg = e->d_pred_debug;
    }
    if (sparse) {
        for (int i = 0; i < 3; ++i) lv[i].logits = e->d_hc_logits[i];
        ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, ds);
        VC_TRY(launch_decode_sparse(lv, e->d_hc_count, e->d_hc_list, e->hc_cap, nc, e->cfg.conf_thres, e->cfg.max_candidates, e->post, ds));
    } else {
        ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, ds);
        VC_TRY(launch_decode(lv, 3, B, nc, e->cfg.conf_thres, e->cfg.max_candidates, e->post, dbg, base, ds));
    }
    // class map set: the dropped classes leave the candidates here, where non_max_suppression applies `classes` -- behind the conf tests, in
    // front of the sort, the NMS and the max_det cut.  The three decodes fill the same buffers; overflow was judged on the unfiltered count.
    const bool mapped = !e->class_map.empty();
    if (mapped) { ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, ds); VC_TRY(launch_cand_class_filter(B, nc, e->cfg.max_candidates, e->d_class_map, e->post, ds)); }
    { ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, ds); VC_TRY(launch_nms(B, e->cfg.max_candidates, e->cfg.max_det, e->cfg.iou_thres, e->d_geom, e->post, ds)); }
    // (the NMS offset its boxes by the ORIGINAL class; the rows leave with the label, modules/detect.py:41-46)
    if (mapped) { ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, ds); VC_TRY(launch_det_relabel(B, nc, e->cfg.max_det, e->d_class_map, e->post, ds)); }
    return VC_OK;
}

int run_detector_dev(vc_engine* e, const uint8_t* d_frames, int B, int h, int w, bool swap_rb) {
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "detector not finalized");
    VC_CHECK(B >= 1, VC_ERR_ARG, "a batch needs at least one frame (got %d)", B);
    VC_CHECK(B <= e->cfg.max_batch, VC_ERR_CAPACITY, "batch %d exceeds max_batch %d", B, e->cfg.max_batch);
    VC_CHECK(h >= 1 && w >= 1, VC_ERR_ARG, "frame size %d x %d", h, w);
    int nh, nw;
    autoshape_net_size(&h, &w, 1, e->cfg.img_size, nh, nw);
    const LetterboxGeom g = letterbox_geom(h, w, nh, nw, swap_rb);
    float* hg = e->h_geom + (size_t)(e->geom_seq++ & 1) * e->cfg.max_batch * 5;      // two pinned slots: two submissions may be in flight
    scale_geom_host(ScaleGeom{nh, nw, h, w}, hg);
    for (int b = 1; b < B; ++b) memcpy(hg + (size_t)b * 5, hg, 5 * sizeof(float));
    VC_HIP(hipMemcpyAsync(e->d_geom, hg, (size_t)B * 5 * sizeof(float), hipMemcpyHostToDevice, e->dstream));
    // bf16, frame already at network scale: the stem reads the u8 frames itself (same arithmetic per pixel, bit-identical stem
    // output) and the 8-byte-per-pixel letterboxed tensor is neither written nor read back
    const bool same_scale = g.unpad_h == g.src_h && g.unpad_w == g.src_w && g.src_w % 2 == 0 && g.left % 2 == 0;
    // frames that need the resize (1280 x 720 -> 384 x 640, Q8): only front_fused_kernel evaluates it at patch-build time, so the fold-in
    // needs that kernel to be the one that runs (YOLOv5s widths, bf16 engine, option on) and the tile's source footprint to fit its staging
    const bool resize_ok = !same_scale && ((uintptr_t)d_frames & 3) == 0 && e->prec == PREC_BF16 && e->opt.front_fused > 0 && e->ch[0] == 32 && e->ch[1] == 64 && front_fused_resize_ok(g);
    const bool fuse = e->aux_prec == PREC_BF16 && (same_scale || resize_ok) && e->ch[0] % 16 == 0 && e->ch[0] <= 80;
    e->stem_src = fuse ? d_frames : nullptr;
    e->stem_geom = g;
    e->in_stale = fuse;
    if (!fuse) { ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, e->dstream); VC_TRY(launch_letterbox(d_frames, e->ybuf["in"].ptr, B, g, e->aux_prec, e->dstream)); }
    const int st = yolo_forward(e, B, nh, nw);
    if (fuse && e->in_stale) e->stem_src = d_frames;    // kept for vc_detect_debug_layer(-1) (not when run_ops fell back to the letterbox kernel)
    return st;
}

// A sized batch (include/vcount_hip.h): the caller has checked that every frame's own network shape is nh x nw.  d_geom per frame, one
// letterbox_frames_kernel launch into ybuf["in"], then the pass every other entry point runs from the letterboxed tensor (the stem
// kernels that read u8 frames take ONE geometry per launch: a sized batch always takes the unfused stem).
int run_detector_dev_sized(vc_engine* e, const uint8_t* d_frames, int B, const vc_frame_dims* dims, size_t cell, int nh, int nw, bool swap_rb) {
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "detector not finalized");
    VC_CHECK(B >= 1, VC_ERR_ARG, "a batch needs at least one frame (got %d)", B);
    VC_CHECK(B <= e->cfg.max_batch, VC_ERR_CAPACITY, "batch %d exceeds max_batch %d", B, e->cfg.max_batch);
    if (!e->h_lb_tab) {
        VC_TRY(host_alloc(e, (void**)&e->h_lb_tab, (size_t)2 * e->cfg.max_batch * sizeof(LetterboxFrame)));
        VC_TRY(dev_alloc(e, (void**)&e->d_lb_tab, (size_t)e->cfg.max_batch * sizeof(LetterboxFrame)));
    }
    const unsigned half = e->geom_seq++ & 1;                                          // two pinned slots: two submissions may be in flight
    float* hg = e->h_geom + (size_t)half * e->cfg.max_batch * 5;
    LetterboxFrame* ht = e->h_lb_tab + (size_t)half * e->cfg.max_batch;
    for (int b = 0; b < B; ++b) {
        scale_geom_host(ScaleGeom{nh, nw, dims[b].h, dims[b].w}, hg + (size_t)b * 5);
        ht[b] = letterbox_frame((long long)((size_t)b * cell), letterbox_geom(dims[b].h, dims[b].w, nh, nw, swap_rb));
    }
    VC_HIP(hipMemcpyAsync(e->d_geom, hg, (size_t)B * 5 * sizeof(float), hipMemcpyHostToDevice, e->dstream));
    VC_HIP(hipMemcpyAsync(e->d_lb_tab, ht, (size_t)B * sizeof(LetterboxFrame), hipMemcpyHostToDevice, e->dstream));
    e->stem_src = nullptr;
    e->in_stale = false;
    { ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, e->dstream);
      VC_TRY(launch_letterbox_frames(d_frames, e->d_lb_tab, e->ybuf["in"].ptr, B, nh, nw, swap_rb ? 1 : 0, e->aux_prec, e->dstream)); }
    return yolo_forward(e, B, nh, nw);
}

#define VC_REID_CHUNK 6400
#define VC_REID_PLAN_CACHE_MAX_K 256       // crop counts whose op plans are kept (k0 is 0 for these: one chunk)
static int reid_forward_chunk(vc_engine* e, int k0, int k, hipStream_t rs, float* feat_out) {
    // The plan cache pays at batch 1 (a few crops per frame, the same counts again and again).  A batch of the stream path has thousands of
    // distinct crop counts: those build a transient plan (21 ops, tens of microseconds beside a multi-millisecond pass) instead of
    // filling the map (~10 KB per entry, a full clear at 8192 entries).
    ReidPlan transient;
    ReidPlan& plan = k <= VC_REID_PLAN_CACHE_MAX_K ? e->reid_plans[{k0, k}] : transient;
    if (plan.ops.empty()) VC_TRY(reid_build_ops(e, k0, k, plan));
    LaunchRecorder* rec = nullptr;
    if (e->rec_armed) VC_TRY(record_begin(e, VC_NET_REID, plan.ops, &rec));
    VC_TRY(run_ops(e, plan.ops, VC_PROF_REID_AUX, rs, rec));
    ProfScope ps(e, VC_PROF_REID_AUX, 0, 0, rs);
    return launch_avgpool_l2norm(plan.out, feat_out, e->aux_prec, rs);               // model.py:70,93
}
// forward from the pre-filled "in" buffer (k x 50 x 50 x cpad) to feat_out.  A conv launch addresses at most 2^24 output pixels
// (conv_check), and the first layer has 2500 per crop: more than VC_REID_CHUNK crops run as several passes over slices of "in"
// (the other activation buffers are reused; the passes are ordered on the stream).
int reid_forward(vc_engine* e, int k, hipStream_t rs, float* feat_out) {
    // ... and its 50 x 50 x 64 output must stay below the 2 GiB a buffer descriptor addresses (fp32: 3200 crops)
    const int chunk = std::min(VC_REID_CHUNK, (int)(((1ull << 31) - 1) / ((size_t)2500 * 64 * elem_size(e->aux_prec))) / 64 * 64);
    for (int k0 = 0; k0 < k; k0 += chunk)
        VC_TRY(reid_forward_chunk(e, k0, std::min(chunk, k - k0), rs, feat_out + (size_t)k0 * VC_FEAT_DIM));
    return VC_OK;
}

int run_reid_on(vc_engine* e, const uint8_t* d_frames, int H, int W, int k, const int* d_crops, float* feat_out, hipStream_t rs, const CropFrame* d_ftab) {
    VC_CHECK(e->finalized && e->cfg.with_reid, VC_ERR_STATE, "ReID net not finalized");
    VC_CHECK(k <= e->cfg.max_crops, VC_ERR_CAPACITY, "%d crops exceed max_crops %d", k, e->cfg.max_crops);
    if (k <= 0) return VC_OK;
    { ProfScope ps(e, VC_PROF_REID_AUX, 0, 0, rs);
      VC_TRY(launch_crop_resize(d_frames, H, W, d_crops, k, e->rbuf["in"].ptr, reid_cpad(e->aux_prec), e->aux_prec, rs, e->opt.crop_per_pixel != 0, d_ftab)); }
    return reid_forward(e, k, rs, feat_out);
}

// blocking-API flavour (vc_embed, vc_deepsort_update, vc_videotracker_run): tracker stream, shared crop / feature buffers
int run_reid_dev(vc_engine* e, const uint8_t* d_frames, int H, int W, int k) {
    VC_HIP(hipStreamSynchronize(e->rstream));          // the activation buffers are shared with the stream path's ReID
    return run_reid_on(e, d_frames, H, W, k, e->d_crops, e->d_feat, e->stream);
}

}  // namespace vc
