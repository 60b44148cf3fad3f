// Engine: owns the device, the streams, the detector and the ReID net (engine_plan.hip defines them and builds their execution
// plans, engine_run.hip runs them) and exposes them through the C ABI in include/vcount_hip.h.  The stateless entry points that run
// one kernel on host arrays (vc_*_host) live in host_conv.hip, host_aux.hip, host_detect.hip and host_track.hip.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>

#include "engine.h"

namespace vc {

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }

int dev_alloc(std::vector<void*>& allocs, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    VC_HIP(hipMalloc(p, bytes));
    allocs.push_back(*p);
    return VC_OK;
}
// Replace *p (an allocation of this engine, or null) by a fresh block of `bytes`; the old block is freed.  The caller makes sure no
// kernel still uses it.  Contents are not carried over.
int dev_realloc(vc_engine* e, void** p, size_t bytes) {
    void* fresh = nullptr;
    VC_HIP(hipMalloc(&fresh, bytes ? bytes : 16));
    bool swapped = false;
    for (void*& q : e->allocs)
        if (*p && q == *p) { (void)hipFree(q); q = fresh; swapped = true; break; }
    if (!swapped) e->allocs.push_back(fresh);
    *p = fresh;
    return VC_OK;
}
int host_alloc(vc_engine* e, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    VC_HIP(hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocPortable));
    e->host_allocs.push_back(*p);
    return VC_OK;
}

ProfScope::ProfScope(vc_engine* e_, int cat_, double flops_, double bytes_, hipStream_t s_)
    : e(e_), cat(cat_), flops(flops_), bytes(bytes_), s(s_ ? s_ : e_->stream) {
    if (e->profiling) hipEventRecord(e->ev0, s);
}
ProfScope::~ProfScope() {
    if (!e->profiling) return;
    hipEventRecord(e->ev1, s);
    hipEventSynchronize(e->ev1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e->ev0, e->ev1);
    ProfCat& c = e->prof[cat];
    c.ms += ms; c.flops += flops; c.bytes += bytes; c.launches += 1;
    c.flops_dense += flops; c.bytes_dense += bytes;
    e->last_ms = ms;
}

// ------------------------------------------------------------------------------------------------ weights
int pack_and_upload(std::vector<void*>& allocs, ConvParam& p, int prec, float act_scale) {
    VC_CHECK(p.set, VC_ERR_STATE, "parameter '%s' was never set", p.name.c_str());
    p.prec = prec;
    const int ch = prec == PREC_F32 ? 4 : prec == PREC_FP8 ? 16 : 8;
    const int kt = conv_k_tile(prec);
    int kw_eff = p.kw;
    if (p.pair_stem) {                       // two 4-channel pixels per chunk: kernel becomes kh x kw/2 over 8 channels
        p.cin_eff = 8;
        kw_eff = p.kw / 2;
    } else {
        p.cin_eff = round_up(p.I, ch);
    }
    p.K = p.kh * kw_eff * p.cin_eff;
    p.Kp = round_up(p.K, kt);
    p.cout_pad = round_up(p.O, 128);
    std::vector<float> packed((size_t)p.cout_pad * p.Kp, 0.f);
    for (int n = 0; n < p.O; ++n)
        for (int c = 0; c < p.I; ++c)
            for (int r = 0; r < p.kh; ++r)
                for (int s = 0; s < p.kw; ++s) {
                    const float v = p.w[(((size_t)n * p.I + c) * p.kh + r) * p.kw + s];
                    size_t k;
                    if (p.pair_stem) k = ((size_t)r * kw_eff + s / 2) * 8 + (s % 2) * 4 + c;
                    else k = ((size_t)r * p.kw + s) * p.cin_eff + c;
                    packed[(size_t)n * p.Kp + k] = v;
                }
    std::vector<float> bias(p.cout_pad, 0.f);
    for (int n = 0; n < p.O; ++n) bias[n] = p.b[n];
    const size_t nel = packed.size();
    VC_TRY(dev_alloc(allocs, &p.d_w, nel * elem_size(prec)));
    VC_TRY(dev_alloc(allocs, (void**)&p.d_b, bias.size() * sizeof(float)));
    if (prec == PREC_F32) {
        VC_HIP(hipMemcpy(p.d_w, packed.data(), nel * 4, hipMemcpyHostToDevice));
    } else if (prec == PREC_FP8) {
        // OCP e4m3fn weights with one scale per output channel (|w|max -> 448); the kernel multiplies the accumulator by
        // weight scale x activation scale in its epilogue (the MFMA's own block scales stay 1)
        std::vector<uint8_t> h(nel);
        std::vector<float> sc(p.cout_pad, 0.f);
        for (int n = 0; n < p.O; ++n) {
            float amax = 0.f;
            for (int k = 0; k < p.Kp; ++k) amax = std::max(amax, std::fabs(packed[(size_t)n * p.Kp + k]));
            const float sw = amax > 0.f ? amax / 448.0f : 1.0f;
            for (int k = 0; k < p.Kp; ++k) h[(size_t)n * p.Kp + k] = f32_to_e4m3(packed[(size_t)n * p.Kp + k] / sw);
            sc[n] = sw * act_scale;
        }
        for (size_t i = (size_t)p.O * p.Kp; i < nel; ++i) h[i] = 0;
        VC_HIP(hipMemcpy(p.d_w, h.data(), nel, hipMemcpyHostToDevice));
        VC_TRY(dev_alloc(allocs, (void**)&p.d_scale, sc.size() * sizeof(float)));
        VC_HIP(hipMemcpy(p.d_scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<uint16_t> h(nel);
        for (size_t i = 0; i < nel; ++i) h[i] = f32_to_bf16(packed[i]);
        VC_HIP(hipMemcpy(p.d_w, h.data(), nel * 2, hipMemcpyHostToDevice));
    }
    VC_HIP(hipMemcpy(p.d_b, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    return VC_OK;
}

}  // namespace vc

// ================================================================================================ C ABI
using namespace vc;

extern "C" {

int vc_version(void) { return 100; }
const char* vc_last_error(void) { return vc::last_error(); }
int vc_device_count(int* n) {
    VC_CHECK(n, VC_ERR_ARG, "null out pointer");
    *n = 0;
    VC_HIP(hipGetDeviceCount(n));
    return VC_OK;
}

int vc_engine_config_default(vc_engine_config* c) {
    VC_CHECK(c, VC_ERR_ARG, "null config");
    memset(c, 0, sizeof(*c));
    c->device = 0; c->precision = VC_PREC_BF16; c->yolo_variant = 0; c->num_classes = 80; c->img_size = 640;
    c->max_batch = 16; c->max_frame_h = 720; c->max_frame_w = 1280;
    c->conf_thres = 0.25f; c->iou_thres = 0.45f; c->max_det = 300; c->max_candidates = 4096;
    c->max_crops = 1024; c->max_tracks = 4096; c->nn_budget_cap = 100; c->with_detector = 1; c->with_reid = 1;
    c->max_trackers = 256; c->tracks_per_tracker = 512;
    return VC_OK;
}

int vc_engine_create(const vc_engine_config* cfg, vc_engine** out) {
    VC_CHECK(cfg && out, VC_ERR_ARG, "null argument");
    VC_CHECK(cfg->yolo_variant >= 0 && cfg->yolo_variant <= 3, VC_ERR_ARG, "yolo_variant must be 0..3");
    VC_CHECK(cfg->precision == VC_PREC_BF16 || cfg->precision == VC_PREC_F32 || cfg->precision == VC_PREC_FP8, VC_ERR_ARG, "bad precision");
    // (no quantisation scales, no folded e4m3 stem copy and no fp8 parity figures exist for the 80 .. 1280-wide layers)
    VC_CHECK(!(cfg->yolo_variant == 3 && cfg->precision == VC_PREC_FP8), VC_ERR_ARG, "the fp8 path is not built for yolov5x (yolo_variant 3): use bf16 or f32");
    VC_CHECK(cfg->max_candidates % 64 == 0 && cfg->max_candidates >= 64 && cfg->max_candidates <= 8192, VC_ERR_ARG,
             "max_candidates must be a multiple of 64 in [64, 8192]");
    VC_CHECK(cfg->max_batch >= 1 && cfg->num_classes >= 1 && cfg->max_det >= 1, VC_ERR_ARG, "bad sizes");
    // The engine runs four streams side by side (detector, ReID, tracker, host-frame copies) next to the application's own.  The HIP
    // runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default): two of the engine's streams on one queue
    // serialise, e.g. a batch's PCIe copy in front of the detector kernels of the batch before it.  Measured on the second engine of a
    // process (the first happens to get distinct queues): 15.1 k -> 17.3 k frames/s with host frames, 17.7 k -> 18.6 k device-resident.
    // GPU_MAX_HW_QUEUES >= 8 is therefore a DEPLOYMENT requirement; the runtime reads it once, when it builds its queue
    // pool, so the embedding application has to export it before its first HIP call.  The library does not touch the process
    // environment (setenv is not thread-safe against concurrent getenv); the Python binding sets a default at import
    // (_lib.py), and an engine created without it says so once when VC_VERBOSE is set.
    {
        static bool warned = false;
        const char* q = getenv("GPU_MAX_HW_QUEUES");
        if (!warned && (!q || atoi(q) < 8) && getenv("VC_VERBOSE")) {     // opt-in (a library does not write to the process's stderr unasked)
            warned = true;
            fprintf(stderr, "libvcount_hip: GPU_MAX_HW_QUEUES is %s; export GPU_MAX_HW_QUEUES=8 before the first HIP call or the engine's streams share hardware queues (INTEGRATION.md)\n", q ? q : "unset");
        }
    }
    int ndev = 0;
    VC_HIP(hipGetDeviceCount(&ndev));
    VC_CHECK(cfg->device >= 0 && cfg->device < ndev, VC_ERR_HIP, "device %d not present (%d visible)", cfg->device, ndev);
    VC_HIP(hipSetDevice(cfg->device));
    vc_engine* e = new vc_engine();
    e->cfg = *cfg;
    e->prec = cfg->precision;
    e->aux_prec = cfg->precision == VC_PREC_FP8 ? (int)PREC_BF16 : cfg->precision;      // stem, logits, pools of the ReID net, ReID convs
    e->act_scale = getenv("VC_FP8_ACT_SCALE") ? (float)atof(getenv("VC_FP8_ACT_SCALE")) : 1.0f;
    {
        auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        e->opt.c3_fused = env_int("VC_C3_FUSED", 1); e->opt.bneck_fused = env_int("VC_BNECK_FUSED", 1); e->opt.bneck_cv3 = env_int("VC_BNECK_CV3", 1);
        e->opt.front_fused = env_int("VC_FRONT_FUSED", 1); e->opt.crop_per_pixel = getenv("VC_CROP_PER_PIXEL") ? 1 : 0;
        e->opt.sparse_head = env_int("VC_SPARSE_HEAD", 1); e->opt.reid_block_fused = env_int("VC_REID_BLOCK_FUSED", 1); e->opt.head_side = env_int("VC_HEAD_SIDE", 1); e->opt.fuse_upsample = env_int("VC_FUSE_UPSAMPLE", 1); e->opt.sppf_sep = env_int("VC_SPPF_SEP", 1); e->opt.fuse_s2_pw = env_int("VC_FUSE_S2PW", 1);
        e->opt.embed_kept_only = env_int("VC_EMBED_KEPT_ONLY", 1);
        e->opt.dyn_tiles = env_int("VC_DYN_TILES", 1); e->opt.dyn_tiles_mask = env_int("VC_DYN_TILES_MASK", vc_engine::kDynTilesKept);
        e->conv_slots = env_int("VC_CONV_SLOTS", 0);
        e->tile_ctr_ring = (unsigned)std::min(std::max(env_int("VC_DYN_TILES_RING", (int)vc_engine::kTileCtrPairs), 1), (int)vc_engine::kTileCtrPairs);
    }
    memcpy(e->anchors, kAnchors, sizeof(kAnchors));
    int st = VC_OK;
    do {
        // the tracker's kernels are tiny and latency-critical (the host waits on them every frame): highest priority,
        // so they are not queued behind the conv waves of the detector / ReID streams they run beside
        int plo = 0, phi = 0;
        hipDeviceGetStreamPriorityRange(&plo, &phi);             // numerically lower = higher priority
        // Optional CU partition (VC_TRACK_CUS=n): the first n CUs are reserved for the tracker stream so that its kernels
        // never wait for a conv workgroup to drain; the conv streams get the remaining CUs.
        const int reserve = getenv("VC_TRACK_CUS") ? atoi(getenv("VC_TRACK_CUS")) : 0;
        bool ok;
        if (reserve > 0) {
            hipDeviceProp_t prop;
            hipGetDeviceProperties(&prop, cfg->device);
            const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
            std::vector<uint32_t> mt(words, 0), mc(words, 0);
            for (int c = 0; c < ncu; ++c) (c < reserve ? mt : mc)[c / 32] |= 1u << (c % 32);
            ok = hipExtStreamCreateWithCUMask(&e->stream, words, mt.data()) == hipSuccess &&
                 hipExtStreamCreateWithCUMask(&e->dstream, words, mc.data()) == hipSuccess &&
                 hipExtStreamCreateWithCUMask(&e->rstream, words, mc.data()) == hipSuccess;
        } else {
            ok = hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, phi) == hipSuccess &&
                 hipStreamCreateWithPriority(&e->dstream, hipStreamNonBlocking, plo) == hipSuccess &&
                 hipStreamCreateWithPriority(&e->rstream, hipStreamNonBlocking, plo) == hipSuccess;
        }
        if (!ok) { set_error("stream create failed"); st = VC_ERR_HIP; break; }
        if ((st = dev_alloc(e, (void**)&e->d_tile_ctr, (size_t)vc_engine::kTileCtrPairs * 64)) != VC_OK) break;
        if (hipMemset(e->d_tile_ctr, 0, (size_t)vc_engine::kTileCtrPairs * 64) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {   // (the engine's streams do not wait for the null stream)
            set_error("tile counter memset failed"); st = VC_ERR_HIP; break;
        }
        // (detector and ReID on ONE queue -- no co-running conv kernels, on the theory that persistent grids sized for the whole chip do not
        // share it well -- measured 16.9 k against 18.5 k frames/s, two alternating runs each: the overlap pays; removed)
        if (hipEventCreateWithFlags(&e->ev_reid[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_reid[1], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_reid[2], hipEventDisableTiming) != hipSuccess) { set_error("event create failed"); st = VC_ERR_HIP; break; }
        if (hipEventCreateWithFlags(&e->ev_det[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_det[1], hipEventDisableTiming) != hipSuccess) { set_error("event create failed"); st = VC_ERR_HIP; break; }
        if (hipStreamCreateWithPriority(&e->hstream, hipStreamNonBlocking, plo) != hipSuccess || hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) { set_error("head stream create failed"); st = VC_ERR_HIP; break; }
        if (hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) { set_error("event create failed"); st = VC_ERR_HIP; break; }
        tune_cache_load(e);
        if (cfg->with_detector) yolo_define(e);
        if (cfg->with_reid) reid_define(e);
        st = tracker_init_pool(e);
    } while (0);
    if (st != VC_OK) { vc_engine_destroy(e); return st; }
    *out = e;
    return VC_OK;
}

int vc_engine_destroy(vc_engine* e) {
    if (!e) return VC_OK;
    tune_cache_save(e);
    hipSetDevice(e->cfg.device);
    render_destroy_all(e);
    if (e->stream) hipStreamSynchronize(e->stream);
    live_destroy_all(e);
    vc_comm_destroy(e);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->dstream) hipStreamSynchronize(e->dstream);
    if (e->rstream) hipStreamSynchronize(e->rstream);
    if (e->cstream) hipStreamSynchronize(e->cstream);
    record_free(e);
    for (void* p : e->allocs) hipFree(p);
    for (void* p : e->host_allocs) hipHostFree(p);
    for (auto& pp : e->prof_pairs) { hipEventDestroy(pp.a); hipEventDestroy(pp.b); }
    if (e->ev0) hipEventDestroy(e->ev0);
    if (e->ev1) hipEventDestroy(e->ev1);
    if (e->stream) hipStreamDestroy(e->stream);
    if (e->dstream) hipStreamDestroy(e->dstream);
    if (e->rstream) hipStreamDestroy(e->rstream);
    if (e->hstream) hipStreamDestroy(e->hstream);
    if (e->ev_fork) hipEventDestroy(e->ev_fork);
    if (e->ev_join) hipEventDestroy(e->ev_join);
    for (hipEvent_t ev : e->ev_det) if (ev) hipEventDestroy(ev);
    for (hipEvent_t ev : e->ev_reid) if (ev) hipEventDestroy(ev);
    for (vc::TrackStage& ts : e->tstage) if (ts.done) hipEventDestroy(ts.done);
    for (hipEvent_t ev : e->ev_ingest) if (ev) hipEventDestroy(ev);
    if (e->cstream) hipStreamDestroy(e->cstream);
    delete e;
    return VC_OK;
}

static Net* pick_net(vc_engine* e, int net) { return net == VC_NET_YOLO ? &e->yolo : (net == VC_NET_REID ? &e->reid : nullptr); }

int vc_engine_param_count(const vc_engine* e, int net, int* n) {
    VC_CHECK(e && n, VC_ERR_ARG, "null argument");
    const Net* nn = pick_net(const_cast<vc_engine*>(e), net);
    VC_CHECK(nn, VC_ERR_ARG, "bad net id %d", net);
    int cnt = 0;
    for (const auto& p : nn->params) cnt += p.hidden ? 0 : 1;
    *n = cnt;
    return VC_OK;
}

int vc_engine_param_info(const vc_engine* e, int net, int index, char* name, int name_cap, int dims[4]) {
    VC_CHECK(e && name && dims, VC_ERR_ARG, "null argument");
    const Net* nn = pick_net(const_cast<vc_engine*>(e), net);
    VC_CHECK(nn && index >= 0, VC_ERR_ARG, "bad net/index");
    int real = -1;
    for (size_t i = 0, k = 0; i < nn->params.size(); ++i) {
        if (nn->params[i].hidden) continue;
        if ((int)k++ == index) { real = (int)i; break; }
    }
    VC_CHECK(real >= 0, VC_ERR_ARG, "parameter index %d out of range", index);
    const ConvParam& p = nn->params[real];
    snprintf(name, name_cap, "%s", p.name.c_str());
    dims[0] = p.O; dims[1] = p.I; dims[2] = p.kh; dims[3] = p.kw;
    return VC_OK;
}

int vc_engine_set_param(vc_engine* e, int net, const char* name, const float* w, const float* bias) {
    VC_CHECK(e && name && w && bias, VC_ERR_ARG, "null argument");
    VC_CHECK(!e->finalized, VC_ERR_STATE, "engine already finalized");
    Net* nn = pick_net(e, net);
    VC_CHECK(nn, VC_ERR_ARG, "bad net id %d", net);
    auto it = nn->index.find(name);
    VC_CHECK(it != nn->index.end(), VC_ERR_NOTFOUND, "no parameter named '%s'", name);
    ConvParam& p = nn->params[it->second];
    VC_CHECK(!p.hidden, VC_ERR_NOTFOUND, "no parameter named '%s'", name);
    p.w.assign(w, w + (size_t)p.O * p.I * p.kh * p.kw);
    p.b.assign(bias, bias + p.O);
    p.set = true;
    return VC_OK;
}

// Detect anchors in pixels, [level P3,P4,P5][anchor][w,h] (ultralytics `model.24.anchors * stride`).  Custom-trained checkpoints
// (the reference loads 'custom' weights, /root/reference/networks/yolo.py:58) may carry autoanchor-evolved values.
int vc_engine_set_anchors(vc_engine* e, const float* anchors18) {
    VC_CHECK(e && anchors18, VC_ERR_ARG, "null argument");
    for (int i = 0; i < 18; ++i) VC_CHECK(anchors18[i] > 0.f && anchors18[i] < 1e5f, VC_ERR_ARG, "anchor %d = %g is not a positive pixel size", i, (double)anchors18[i]);
    memcpy(e->anchors, anchors18, 18 * sizeof(float));
    return VC_OK;
}

int vc_engine_finalize(vc_engine* e) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    VC_CHECK(!e->finalized, VC_ERR_STATE, "engine already finalized");
    VC_HIP(hipSetDevice(e->cfg.device));
    for (auto& p : e->yolo.params) {
        if (p.fuse_a < 0) continue;
        const ConvParam &a = e->yolo.params[p.fuse_a], &b = e->yolo.params[p.fuse_b];
        VC_CHECK(a.set && b.set, VC_ERR_STATE, "parameters '%s' / '%s' were never set", a.name.c_str(), b.name.c_str());
        p.w = a.w; p.w.insert(p.w.end(), b.w.begin(), b.w.end());
        p.b = a.b; p.b.insert(p.b.end(), b.b.begin(), b.b.end());
        p.set = true;
    }
    for (auto& p : e->yolo.params) {                          // sparse head: the objectness rows of a Detect head as an 8-channel conv
        if (p.obj_of < 0) continue;
        const ConvParam& hd = e->yolo.params[p.obj_of];
        VC_CHECK(hd.set, VC_ERR_STATE, "parameter '%s' was never set", hd.name.c_str());
        const int no = hd.O / 3;
        p.w.assign((size_t)8 * p.I, 0.f); p.b.assign(8, 0.f);
        for (int a = 0; a < 3; ++a) {
            memcpy(&p.w[(size_t)a * p.I], &hd.w[(size_t)(a * no + 4) * hd.I], (size_t)p.I * sizeof(float));
            p.b[a] = hd.b[a * no + 4];
        }
        p.set = true;
    }
    {
        std::vector<char> part(e->yolo.params.size(), 0);
        for (auto& p : e->yolo.params) if (p.fuse_a >= 0) { part[p.fuse_a] = 1; part[p.fuse_b] = 1; }
        for (size_t i = 0; i < e->yolo.params.size(); ++i) {
            if (part[i]) { VC_CHECK(e->yolo.params[i].set, VC_ERR_STATE, "parameter '%s' was never set", e->yolo.params[i].name.c_str()); continue; }
            ConvParam& cp = e->yolo.params[i];
            // fp8 mode: every detector conv but the 3-channel stem (Cin must be a multiple of 16 for 16-byte K chunks)
            const bool fp8 = e->prec == PREC_FP8 && cp.I % 16 == 0;
            VC_TRY(pack_and_upload(e->allocs, cp, fp8 ? (int)PREC_FP8 : e->aux_prec, e->act_scale));
        }
    }
    for (auto& p : e->reid.params) VC_TRY(pack_and_upload(e->allocs, p, e->aux_prec));
    e->d_frames_bytes = (size_t)e->cfg.max_batch * e->cfg.max_frame_h * e->cfg.max_frame_w * 3;     // staging for host frames
    VC_TRY(dev_alloc(e, (void**)&e->d_frames, e->d_frames_bytes));
    if (e->cfg.with_detector) VC_TRY(yolo_alloc(e));
    if (e->cfg.with_reid) VC_TRY(reid_alloc(e));
    for (auto& p : e->yolo.params) { p.w.clear(); p.w.shrink_to_fit(); }
    for (auto& p : e->reid.params) { p.w.clear(); p.w.shrink_to_fit(); }
    e->finalized = true;
    return VC_OK;
}

// Kernel-selection switches of a live engine (the parity tests compare a fused kernel with the launches it replaces on the same
// engine).  Initial values come from the environment at vc_engine_create; the launch path itself never calls getenv (what the conv
// launchers consult is one struct read once per process, conv_launch.h::conv_switches: VC_CONV_RESERVE, VC_CONV_PERSIST and the A/B switches).
int vc_engine_set_option(vc_engine* e, const char* name, int value) {
    VC_CHECK(e && name, VC_ERR_ARG, "null argument");
    const std::string n = name;
    if (n == "embed_kept_only") { e->opt.embed_kept_only = value; return VC_OK; }     // host-side choice of what is embedded: no kernel selection changes
    if (n == "c3_fused") e->opt.c3_fused = value;
    else if (n == "bneck_fused") e->opt.bneck_fused = value;
    else if (n == "bneck_cv3") e->opt.bneck_cv3 = value;
    else if (n == "front_fused") e->opt.front_fused = value;
    else if (n == "crop_per_pixel") e->opt.crop_per_pixel = value;
    else if (n == "sparse_head") e->opt.sparse_head = value;
    else if (n == "reid_block_fused") e->opt.reid_block_fused = value;
    else if (n == "dyn_tiles_ring") { VC_CHECK(value >= 1 && value <= (int)vc_engine::kTileCtrPairs, VC_ERR_ARG, "dyn_tiles_ring must be 1 .. %u", vc_engine::kTileCtrPairs); e->tile_ctr_ring = (unsigned)value; return VC_OK; }   // tests: a short ring, pairs come round again at once
    else if (n == "dyn_tiles") e->opt.dyn_tiles = value;              // the fused persistent kernels claim their tiles from a counter (1) or walk them by fixed stride (0)
    else if (n == "dyn_tiles_mask") e->opt.dyn_tiles_mask = value;    // ablation: which of them claim while "dyn_tiles" is on: 1 front, 2 C3, 4 Bottleneck
    else if (n == "head_side") e->opt.head_side = value;
    else if (n == "fuse_upsample") e->opt.fuse_upsample = value;
    else if (n == "sppf_sep") e->opt.sppf_sep = value;
    else if (n == "fuse_s2_pw") e->opt.fuse_s2_pw = value;
    else if (n == "stem_direct") e->opt.stem_direct = value;
    else if (n == "ff_ablate") e->opt.ff_ablate = value;            // diagnostics (wrong results): tools/ff_ablate.py
    else if (n == "c3_ablate") e->opt.c3_ablate = value;
    else if (n == "dot_arena_mb") { VC_CHECK(value >= 0, VC_ERR_ARG, "dot_arena_mb must be >= 0"); e->dot_arena_max_floats = (size_t)value * 262144; }
    else { set_error("unknown option '%s'", name); return VC_ERR_NOTFOUND; }
    plans_retune(e);
    return VC_OK;
}

int vc_tune_export(vc_engine* e, char* buf, size_t cap, size_t* size) {
    VC_CHECK(e && size, VC_ERR_ARG, "null argument");
    std::string text;
    for (const auto& kv : e->tuned) text += kv.first + " " + std::to_string(kv.second) + "\n";
    *size = text.size() + 1;
    if (!buf) return VC_OK;
    VC_CHECK(cap >= text.size() + 1, VC_ERR_CAPACITY, "vc_tune_export: %zu bytes needed", text.size() + 1);
    memcpy(buf, text.c_str(), text.size() + 1);
    return VC_OK;
}

int vc_tune_import(vc_engine* e, const char* text) {
    VC_CHECK(e && text, VC_ERR_ARG, "null argument");
    const char* p = text;
    int n = 0, cfg = 0, used = 0;
    char key[200];
    while (sscanf(p, "%199s %d%n", key, &cfg, &used) == 2) {
        VC_CHECK(cfg >= -1 && cfg < conv_num_cfgs(), VC_ERR_ARG, "vc_tune_import: tile configuration %d of '%s' does not exist in this build", cfg, key);
        e->tuned[key] = cfg;
        p += used; ++n;
    }
    while (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r') ++p;
    VC_CHECK(*p == 0, VC_ERR_ARG, "vc_tune_import: malformed text after %d entries", n);
    tune_cache_publish(e);
    if (n) e->tuned_dirty = true;
    plans_retune(e);
    return VC_OK;
}

int vc_engine_sync(vc_engine* e) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    VC_HIP(hipStreamSynchronize(e->stream));
    VC_HIP(hipStreamSynchronize(e->dstream));
    VC_HIP(hipStreamSynchronize(e->rstream));
    return VC_OK;
}

// ---- detect --------------------------------------------------------------------------------------------
int vc_detect(vc_engine* e, const uint8_t* const* rgb, const int* h, const int* w, int n, float* out_det, int* out_count) {
    VC_CHECK(e && rgb && h && w && out_det && out_count, VC_ERR_ARG, "null argument");
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "detector not finalized");
    VC_CHECK(n >= 1, VC_ERR_ARG, "a batch needs at least one image (got %d)", n);
    VC_CHECK(n <= e->cfg.max_batch, VC_ERR_CAPACITY, "batch %d exceeds max_batch %d", n, e->cfg.max_batch);
    for (int i = 0; i < n; ++i) VC_CHECK(rgb[i] && h[i] >= 1 && w[i] >= 1, VC_ERR_ARG, "image %d: null pointer or size %d x %d", i, h[i], w[i]);
    VC_HIP(hipSetDevice(e->cfg.device));
    int nh, nw;
    autoshape_net_size(h, w, n, e->cfg.img_size, nh, nw);
    size_t off = 0;
    std::vector<float> hg((size_t)n * 5);
    std::vector<size_t> offs(n);
    for (int i = 0; i < n; ++i) {
        VC_CHECK(h[i] > 0 && w[i] > 0, VC_ERR_ARG, "empty image %d", i);
        const size_t bytes = (size_t)h[i] * w[i] * 3;
        VC_CHECK(off + bytes <= e->d_frames_bytes, VC_ERR_CAPACITY, "frames exceed the staging buffer (max_frame_h/w)");
        VC_HIP(hipMemcpyAsync(e->d_frames + off, rgb[i], bytes, hipMemcpyHostToDevice, e->dstream));
        offs[i] = off; off += bytes;
        scale_geom_host(ScaleGeom{nh, nw, h[i], w[i]}, &hg[(size_t)i * 5]);
    }
    VC_HIP(hipMemcpyAsync(e->d_geom, hg.data(), hg.size() * sizeof(float), hipMemcpyHostToDevice, e->dstream));
    VC_HIP(hipStreamSynchronize(e->dstream));        // hg / rgb[] are caller or stack memory
    const size_t px = (size_t)nh * nw * 4 * elem_size(e->aux_prec);
    // this pass reads the letterboxed tensor written below: a u8 source left behind by an earlier stream pass (kept for
    // vc_detect_debug_layer(-1)) must not be picked up by the stem kernels again
    e->stem_src = nullptr; e->in_stale = false;
    for (int i = 0; i < n; ++i) {
        const LetterboxGeom g = letterbox_geom(h[i], w[i], nh, nw, false);
        ProfScope ps(e, VC_PROF_DETECT_AUX, 0, 0, e->dstream);
        VC_TRY(launch_letterbox(e->d_frames + offs[i], (char*)e->ybuf["in"].ptr + (size_t)i * px, 1, g, e->aux_prec, e->dstream));
    }
    VC_TRY(yolo_forward(e, n, nh, nw));
    const int md = e->cfg.max_det;
    VC_HIP(hipMemcpyAsync(e->h_det, e->post.det, (size_t)n * md * 6 * sizeof(float), hipMemcpyDeviceToHost, e->dstream));
    VC_HIP(hipMemcpyAsync(e->h_det_count, e->post.det_count, n * sizeof(int), hipMemcpyDeviceToHost, e->dstream));
    VC_HIP(hipStreamSynchronize(e->dstream));
    for (int i = 0; i < n; ++i)
        VC_CHECK(e->h_det_count[i] >= 0, VC_ERR_CAPACITY, "image %d: more than max_candidates (%d) boxes passed conf_thres; raise vc_engine_config.max_candidates "
                 "(upstream keeps up to max_nms = 30000)", i, e->cfg.max_candidates);
    memcpy(out_det, e->h_det, (size_t)n * md * 6 * sizeof(float));
    memcpy(out_count, e->h_det_count, n * sizeof(int));
    return VC_OK;
}

int vc_detect_debug_shape(const vc_engine* e, int* net_h, int* net_w, int* n_candidates) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    if (net_h) *net_h = e->last_nh;
    if (net_w) *net_w = e->last_nw;
    if (n_candidates) *n_candidates = e->last_ntotal;
    return VC_OK;
}

static int read_view_f32(vc_engine* e, const View& v, float* out, size_t cap, int dims[4]) {
    const size_t n = (size_t)v.B * v.H * v.W * v.C;
    VC_CHECK(n <= cap, VC_ERR_CAPACITY, "debug buffer too small: need %zu floats", n);
    const int es = v.es ? v.es : elem_size(e->prec);
    const size_t rows = (size_t)v.B * v.H * v.W;
    std::vector<uint8_t> raw(rows * v.cs * es);
    VC_HIP(hipStreamSynchronize(e->stream));
    VC_HIP(hipStreamSynchronize(e->dstream));
    VC_HIP(hipMemcpy(raw.data(), v.ptr, raw.size(), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r)
        for (int c = 0; c < v.C; ++c) {
            const size_t o = r * v.cs + v.co + c;
            out[r * v.C + c] = es == 4 ? ((const float*)raw.data())[o] : es == 2 ? bf16_to_f32(((const uint16_t*)raw.data())[o]) : e4m3_to_f32(raw[o]) * e->act_scale;
        }
    dims[0] = v.B; dims[1] = v.H; dims[2] = v.W; dims[3] = v.C;
    return VC_OK;
}

int vc_detect_debug_layer(vc_engine* e, int layer, float* out, size_t cap, int dims[4]) {
    VC_CHECK(e && out && dims, VC_ERR_ARG, "null argument");
    VC_CHECK(e->last_B > 0, VC_ERR_STATE, "no detector run yet");
    VC_CHECK(layer >= -1 && layer < 24, VC_ERR_ARG, "layer must be -1..23");
    if (layer == -1) {
        if (e->in_stale && e->stem_src) {         // the last pass folded the letterbox into the stem: produce the tensor now (the frames must still be there)
            VC_TRY(launch_letterbox(e->stem_src, e->ybuf["in"].ptr, e->last_B, e->stem_geom, e->aux_prec, e->dstream));
            VC_HIP(hipStreamSynchronize(e->dstream));
            e->in_stale = false;
        }
        View v = mkview(e->ybuf["in"], e->last_B, e->last_nh, e->last_nw, 3, 0);
        return read_view_f32(e, v, out, cap, dims);
    }
    if ((layer == 11 || layer == 12 || layer == 15 || layer == 16) && !e->up_folded.empty()) {   // the last pass folded the upsampling into its consumer
        for (const auto& ab : e->up_folded) VC_TRY(launch_upsample2x(ab.first, ab.second, e->prec, e->dstream));
        VC_HIP(hipStreamSynchronize(e->dstream));
        e->up_folded.clear();
    }
    if ((layer == 3 || layer == 5 || layer == 7) && !e->s2pw_folded.empty()) {   // the last pass kept a stride-2 conv's output on chip for its one reader
        for (ConvP c : e->s2pw_folded) { c.cfg = 49; VC_TRY(launch_conv(c, e->dstream)); }   // the fused kernel's own tile and K order (conv3x3s2_halo_kernel<256, 128, 4, 1, 2>)
        VC_HIP(hipStreamSynchronize(e->dstream));
        e->s2pw_folded.clear();
    }
    VC_CHECK(!(layer == 0 && e->l0_stale), VC_ERR_STATE,
             "layer 0 was not written by the last pass (front_fused_kernel keeps it in LDS); vc_engine_set_option(e, \"front_fused\", 0) and run again");
    return read_view_f32(e, e->last_plan->layer_view[layer], out, cap, dims);
}

int vc_detect_debug_pred(vc_engine* e, float* out, size_t cap) {
    VC_CHECK(e, VC_ERR_ARG, "null argument");
    if (!out) { e->want_pred_debug = true; return VC_OK; }       // arm: the next run writes the full decoded tensor
    VC_CHECK(e->d_pred_debug && e->last_B > 0, VC_ERR_STATE, "arm with out=NULL and run the detector first");
    const size_t n = (size_t)e->last_B * e->last_ntotal * (e->cfg.num_classes + 5);
    VC_CHECK(n <= cap, VC_ERR_CAPACITY, "need %zu floats", n);
    VC_HIP(hipStreamSynchronize(e->dstream));
    VC_HIP(hipMemcpy(out, e->d_pred_debug, n * sizeof(float), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_embed_debug_input(vc_engine* e, int k, float* out, size_t cap, int dims[4]) {
    VC_CHECK(e && out && dims, VC_ERR_ARG, "null argument");
    VC_CHECK(e->finalized && e->cfg.with_reid, VC_ERR_STATE, "ReID net not finalized");
    VC_CHECK(k > 0 && k <= e->cfg.max_crops, VC_ERR_ARG, "k must be 1..max_crops");
    return read_view_f32(e, mkview(e->rbuf["in"], k, VC_REID_SIZE, VC_REID_SIZE, 3, 0), out, cap, dims);
}

// ---- embed ---------------------------------------------------------------------------------------------
int vc_embed(vc_engine* e, const uint8_t* bgr, int h, int w, const double* boxes, int k, float* out_feat) {
    VC_CHECK(e && bgr && (k == 0 || (boxes && out_feat)), VC_ERR_ARG, "null argument");
    VC_CHECK(e->finalized && e->cfg.with_reid, VC_ERR_STATE, "ReID net not finalized");
    VC_CHECK(k <= e->cfg.max_crops, VC_ERR_CAPACITY, "%d crops exceed max_crops %d", k, e->cfg.max_crops);
    if (k == 0) return VC_OK;
    VC_HIP(hipSetDevice(e->cfg.device));
    const size_t bytes = (size_t)h * w * 3;
    VC_CHECK(bytes <= e->d_frames_bytes, VC_ERR_CAPACITY, "frame exceeds the staging buffer");
    std::vector<int> crops;
    const int empty = append_crops_cxcywh(0, w, h, boxes, k, crops);
    VC_CHECK(empty < 0, VC_ERR_ARG, "box %d gives an empty crop (the reference's cv2.resize raises here)", empty);
    memcpy(e->h_crops, crops.data(), crops.size() * sizeof(int));
    VC_HIP(hipMemcpyAsync(e->d_frames, bgr, bytes, hipMemcpyHostToDevice, e->stream));
    VC_HIP(hipMemcpyAsync(e->d_crops, e->h_crops, (size_t)k * 5 * sizeof(int), hipMemcpyHostToDevice, e->stream));
    VC_TRY(run_reid_dev(e, e->d_frames, h, w, k));
    VC_HIP(hipMemcpyAsync(e->h_feat, e->d_feat, (size_t)k * VC_FEAT_DIM * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    VC_HIP(hipStreamSynchronize(e->stream));
    memcpy(out_feat, e->h_feat, (size_t)k * VC_FEAT_DIM * sizeof(float));
    return VC_OK;
}

int vc_embed_tensor(vc_engine* e, const float* x, int k, float* out_feat) {
    VC_CHECK(e && x && out_feat, VC_ERR_ARG, "null argument");
    VC_CHECK(e->finalized && e->cfg.with_reid, VC_ERR_STATE, "ReID net not finalized");
    VC_CHECK(k >= 1, VC_ERR_ARG, "at least one crop is needed (got %d)", k);
    VC_CHECK(k <= e->cfg.max_crops, VC_ERR_CAPACITY, "%d crops exceed max_crops %d", k, e->cfg.max_crops);
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_HIP(hipMemcpyAsync(e->d_reid_in_nchw, x, (size_t)k * 3 * 2500 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    VC_HIP(hipStreamSynchronize(e->rstream));
    VC_TRY(launch_nchw_to_nhwc_pad(e->d_reid_in_nchw, k, 3, 50, 50, e->rbuf["in"].ptr, reid_cpad(e->aux_prec), e->aux_prec, e->stream));
    VC_TRY(reid_forward(e, k, e->stream, e->d_feat));
    VC_HIP(hipMemcpyAsync(e->h_feat, e->d_feat, (size_t)k * VC_FEAT_DIM * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    VC_HIP(hipStreamSynchronize(e->stream));
    memcpy(out_feat, e->h_feat, (size_t)k * VC_FEAT_DIM * sizeof(float));
    return VC_OK;
}

// ---- measurement ---------------------------------------------------------------------------------------
int vc_profile_enable(vc_engine* e, int on) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    e->profiling = on == 1;                 // 1: blocking per-launch events for every category (serialises the streams)
    e->prof_async = on == 2;                // 2: in-flight event pairs around conv launches only, resolved by vc_profile_read
    if (on == 2 && e->prof_pairs.empty()) {
        e->prof_pairs.resize(16384);
        for (auto& pp : e->prof_pairs) { VC_HIP(hipEventCreate(&pp.a)); VC_HIP(hipEventCreate(&pp.b)); }
    }
    if (on == 2) e->prof_used = 0;
    return VC_OK;
}
int vc_profile_reset(vc_engine* e) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    for (auto& c : e->prof) c = ProfCat{};
    e->op_log.clear();
    return VC_OK;
}
int vc_profile_ops(vc_engine* e, char* buf, size_t cap) {
    VC_CHECK(e && buf && cap > 0, VC_ERR_ARG, "bad argument");
    snprintf(buf, cap, "%s", e->op_log.c_str());
    return VC_OK;
}
int vc_profile_read(vc_engine* e, int cat, double* ms, int64_t* launches, double* flops, double* bytes) {
    VC_CHECK(e && cat >= 0 && cat < VC_PROF_NCAT, VC_ERR_ARG, "bad category");
    if (cat == VC_PROF_CONV && e->prof_used > 0) {          // resolve the in-flight pairs into the conv category
        VC_HIP(hipStreamSynchronize(e->dstream)); VC_HIP(hipStreamSynchronize(e->rstream)); VC_HIP(hipStreamSynchronize(e->stream));
        std::vector<std::pair<float, float>> iv;           // (start, stop) of every launch relative to the first one's start
        iv.reserve(e->prof_used);
        for (size_t i = 0; i < e->prof_used; ++i) {
            float t = 0.f, t0 = 0.f;
            if (hipEventElapsedTime(&t, e->prof_pairs[i].a, e->prof_pairs[i].b) != hipSuccess) continue;
            ProfCat& c = e->prof[VC_PROF_CONV];
            const vc_engine::ProfPair& pp = e->prof_pairs[i];
            const double rows = pp.rows ? (double)*pp.rows : 0.0;              // the pass's D2H copy of the row count has completed (streams synchronised above)
            const double fe = pp.flops + rows * pp.flops_per_row, be = pp.bytes + rows * pp.bytes_per_row;
            c.ms += t; c.flops += fe; c.bytes += be; c.launches += 1;
            c.flops_dense += pp.flops_dense >= 0 ? pp.flops_dense : fe; c.bytes_dense += pp.bytes_dense >= 0 ? pp.bytes_dense : be;
            if (hipEventElapsedTime(&t0, e->prof_pairs[0].a, e->prof_pairs[i].a) == hipSuccess) iv.emplace_back(t0, t0 + t);
        }
        // how much of the wall-clock window between the first start and the last stop had at least one conv kernel running
        e->prof_conv_union_ms = e->prof_conv_span_ms = 0;
        if (!iv.empty()) {
            std::sort(iv.begin(), iv.end());
            float lo = iv[0].first, hi = iv[0].second, cs = iv[0].first, ce = iv[0].second;
            double uni = 0;
            for (size_t i = 1; i < iv.size(); ++i) {
                lo = std::min(lo, iv[i].first); hi = std::max(hi, iv[i].second);
                if (iv[i].first > ce) { uni += ce - cs; cs = iv[i].first; ce = iv[i].second; }
                else ce = std::max(ce, iv[i].second);
            }
            uni += ce - cs;
            e->prof_conv_union_ms = uni; e->prof_conv_span_ms = hi - lo;
        }
        e->prof_used = 0;
    }
    if (ms) *ms = e->prof[cat].ms;
    if (launches) *launches = e->prof[cat].launches;
    if (flops) *flops = e->prof[cat].flops;
    if (bytes) *bytes = e->prof[cat].bytes;
    return VC_OK;
}

// The same category with the sparse Detect head credited as the DENSE head it replaces (the algorithmic work of the reference's
// Detect.m[i] over every pixel): kept apart from vc_profile_read, whose figures are the work the launches execute.
int vc_profile_read_dense(vc_engine* e, int cat, double* flops_dense, double* bytes_dense) {
    VC_CHECK(e && cat >= 0 && cat < VC_PROF_NCAT && flops_dense && bytes_dense, VC_ERR_ARG, "bad argument");
    VC_CHECK(!(cat == VC_PROF_CONV && e->prof_used > 0), VC_ERR_STATE, "call vc_profile_read first (it resolves the in-flight event pairs)");
    *flops_dense = e->prof[cat].flops_dense; *bytes_dense = e->prof[cat].bytes_dense;
    return VC_OK;
}

int vc_profile_conv_busy(vc_engine* e, double* union_ms, double* span_ms) {
    VC_CHECK(e && union_ms && span_ms, VC_ERR_ARG, "null argument");
    *union_ms = e->prof_conv_union_ms; *span_ms = e->prof_conv_span_ms;
    return VC_OK;
}

}  // extern "C"
