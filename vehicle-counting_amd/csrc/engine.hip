// Engine: owns the device, the streams, the detector and the ReID net (engine_plan.hip defines them and builds their execution
// plans, engine_run.hip runs them) and exposes them through the C ABI in include/vcount_hip.h.
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
int GuardedOut::alloc(DevScratch& mem, size_t out_bytes, const uint8_t* preload, size_t guard_bytes) {
    bytes = out_bytes;
    guard = guard_bytes;
    VC_TRY(mem.alloc(&base, bytes + 2 * guard));
    VC_HIP(hipMemset(base, 0xA5, bytes + 2 * guard));
    if (preload) VC_HIP(hipMemcpy(out(), preload, bytes, hipMemcpyHostToDevice));
    return VC_OK;
}
int GuardedOut::read_back(uint8_t* host_out, const char* kernel) const {
    std::vector<uint8_t> edge(2 * guard);
    if (hipMemcpy(host_out, out(), bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(edge.data(), base, guard, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(edge.data() + guard, out() + bytes, guard, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("%s failed: %s", kernel, hipGetErrorString(hipGetLastError()));
        return VC_ERR_HIP;
    }
    for (size_t i = 0; i < 2 * guard; ++i) VC_CHECK(edge[i] == 0xA5, VC_ERR_HIP, "%s wrote outside its output (guard byte %zu)", kernel, i);
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
static int pack_and_upload(std::vector<void*>& allocs, ConvParam& p, int prec, float act_scale = 1.0f) {
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
        e->opt.dyn_tiles = env_int("VC_DYN_TILES", 1);
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
    vc_comm_destroy(e);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->dstream) hipStreamSynchronize(e->dstream);
    if (e->rstream) hipStreamSynchronize(e->rstream);
    if (e->cstream) hipStreamSynchronize(e->cstream);
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
    else if (n == "dyn_tiles") e->opt.dyn_tiles = value;              // front_fused_kernel claims its tiles from a counter (1) or walks them by fixed stride (0)
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
// deep_sort.py:89-95 _xywh_to_xyxy: int() truncation toward zero, clamp to [0, W-1] / [0, H-1]
static void crop_corners(const double* b, int W, int H, int out[4]) {
    const double x = b[0], y = b[1], w = b[2], h = b[3];
    out[0] = std::max((int)(x - w / 2), 0);
    out[2] = std::min((int)(x + w / 2), W - 1);
    out[1] = std::max((int)(y - h / 2), 0);
    out[3] = std::min((int)(y + h / 2), H - 1);
}

int vc_embed(vc_engine* e, const uint8_t* bgr, int h, int w, const double* boxes, int k, float* out_feat) {
    VC_CHECK(e && bgr && (k == 0 || (boxes && out_feat)), VC_ERR_ARG, "null argument");
    VC_CHECK(e->finalized && e->cfg.with_reid, VC_ERR_STATE, "ReID net not finalized");
    VC_CHECK(k <= e->cfg.max_crops, VC_ERR_CAPACITY, "%d crops exceed max_crops %d", k, e->cfg.max_crops);
    if (k == 0) return VC_OK;
    VC_HIP(hipSetDevice(e->cfg.device));
    const size_t bytes = (size_t)h * w * 3;
    VC_CHECK(bytes <= e->d_frames_bytes, VC_ERR_CAPACITY, "frame exceeds the staging buffer");
    for (int i = 0; i < k; ++i) {
        int c[4];
        crop_corners(boxes + (size_t)i * 4, w, h, c);
        VC_CHECK(c[2] > c[0] && c[3] > c[1], VC_ERR_ARG, "box %d gives an empty crop (the reference's cv2.resize raises here)", i);
        e->h_crops[i * 5 + 0] = 0; e->h_crops[i * 5 + 1] = c[0]; e->h_crops[i * 5 + 2] = c[1]; e->h_crops[i * 5 + 3] = c[2]; e->h_crops[i * 5 + 4] = c[3];
    }
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

// ---- single-function entry points --------------------------------------------------------------------------
// n floats -> elements of `prec` (exact for values the type represents; NaN stays NaN) and back
static std::vector<uint8_t> to_elems(const float* src, size_t n, int prec) {
    const int es = elem_size(prec);
    std::vector<uint8_t> buf(n * es);
    for (size_t i = 0; i < n; ++i) {
        if (es == 4) ((float*)buf.data())[i] = src[i];
        else if (es == 2) ((uint16_t*)buf.data())[i] = f32_to_bf16(src[i]);
        else buf[i] = f32_to_e4m3(src[i]);
    }
    return buf;
}
static void from_elems(const std::vector<uint8_t>& buf, size_t n, int prec, float* dst) {
    const int es = elem_size(prec);
    for (size_t i = 0; i < n; ++i)
        dst[i] = es == 4 ? ((const float*)buf.data())[i] : es == 2 ? bf16_to_f32(((const uint16_t*)buf.data())[i]) : e4m3_to_f32(buf[i]);
}
static int upload_elems(DevScratch& mem, const float* src, size_t n, int prec, void** dst) {
    const std::vector<uint8_t> buf = to_elems(src, n, prec);
    VC_TRY(mem.alloc(dst, buf.size()));
    VC_HIP(hipMemcpy(*dst, buf.data(), buf.size(), hipMemcpyHostToDevice));
    return VC_OK;
}
// the caller's float array as the guarded device buffer a kernel writes into, and back
static int guarded_elems(DevScratch& mem, GuardedOut& g, const float* init, size_t n, int prec, size_t guard = GuardedOut::kGuard) {
    const std::vector<uint8_t> buf = to_elems(init, n, prec);
    return g.alloc(mem, buf.size(), buf.data(), guard);
}
static int read_elems(const GuardedOut& g, size_t n, int prec, float* dst, const char* kernel) {
    std::vector<uint8_t> buf(g.bytes);
    VC_TRY(g.read_back(buf.data(), kernel));
    from_elems(buf, n, prec, dst);
    return VC_OK;
}

// One convolution launch on host arrays under the views of `v` (include/vcount_hip.h: vc_conv2d_view_host); vc_conv2d_host is its dense
// case.  d->cin may be short of the chunk here (the weights are packed for round_up(cin, chunk) channels, x holds that many).
static int conv_view_run(const vc_conv_desc* d, const vc_conv_view* v, const float* x, const float* x_up, const float* w, const float* bias,
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
    p.name = "host"; p.O = d->cout; p.I = d->cin; p.kh = d->kh; p.kw = d->kw; p.set = true;
    p.w.assign(w, w + (size_t)d->cout * d->cin * d->kh * d->kw);
    p.b.assign(bias, bias + d->cout);
    VC_TRY(pack_and_upload(mem.allocs, p, prec));
    void *dx = nullptr, *dxu = nullptr, *dr = nullptr;
    int* dm = nullptr;
    VC_TRY(upload_elems(mem, x, npix_in * v->in_cs, prec, &dx));                 // activation scale 1
    if (up) VC_TRY(upload_elems(mem, x_up, (size_t)d->b * (d->h / 2) * (d->w / 2) * v->up_cs, prec, &dxu));
    if (with_res) VC_TRY(upload_elems(mem, res, npix_out * v->res_cs, prec, &dr));
    if (v->m_valid >= 0) {
        VC_TRY(mem.alloc(&dm, sizeof(int)));
        VC_HIP(hipMemcpy(dm, &v->m_valid, sizeof(int), hipMemcpyHostToDevice));
    }
    GuardedOut gy, gy2;
    const size_t ny = npix_out * v->out_cs, ny2 = npix_out * (size_t)v->out2_cs;
    VC_TRY(guarded_elems(mem, gy, y, ny, oprec));
    if (v->split > 0) VC_TRY(guarded_elems(mem, gy2, y2, ny2, oprec));
    int st = VC_OK;
    {
        ConvP c{};
        c.in = dx; c.w = p.d_w; c.bias = p.d_b; c.res = dr; c.out = gy.out();
        c.B = d->b; c.H = d->h; c.W = d->w; c.Cin = cin_eff; c.in_cs = v->in_cs; c.in_co = v->in_co;
        c.Ho = Ho; c.Wo = Wo; c.Cout = cout_l; c.out_cs = v->out_cs; c.out_co = v->out_co; c.res_cs = v->res_cs; c.res_co = v->res_co;
        c.kh = d->kh; c.kw = d->kw; c.sh = c.sw = d->stride; c.ph = c.pw = d->pad;
        c.K = p.K; c.Kp = p.Kp; c.act = d->act; c.res_mode = with_res ? d->res_mode : RES_NONE; c.out_f32 = v->out_f32; c.prec = prec;
        c.scale = p.d_scale; c.act_scale = 1.0f; c.inv_act_scale = 1.0f; c.out_bf16 = v->out_bf16;
        if (v->split > 0) { c.split = v->split; c.out2 = gy2.out(); c.out2_cs = v->out2_cs; c.out2_co = v->out2_co; }
        c.m_dev = dm;
        if (up) { c.in_up = dxu; c.up_C = v->up_c; c.up_cs = v->up_cs; c.up_co = v->up_co; }
        c.M = d->b * Ho * Wo;
        c.cfg = getenv("VC_CONV_CFG") ? atoi(getenv("VC_CONV_CFG")) : -1;
        c.ablate = getenv("VC_CONV_ABLATE") ? atoi(getenv("VC_CONV_ABLATE")) : 0;
        c.slots = getenv("VC_CONV_SLOTS") ? atoi(getenv("VC_CONV_SLOTS")) : 0;       // tests: a short persistent grid walks all tiles
        long long* dbg = nullptr;
        const size_t dbg_n = (size_t)1 << 16;
        if (getenv("VC_CONV_DBG") && hipMalloc((void**)&dbg, dbg_n * 64) == hipSuccess) { hipMemset(dbg, 0, dbg_n * 64); c.dbg = dbg; }
        st = launch_conv(c, nullptr);
        if (st == VC_OK && hipDeviceSynchronize() != hipSuccess) { set_error("conv kernel failed: %s", hipGetErrorString(hipGetLastError())); st = VC_ERR_HIP; }
        if (st == VC_OK && getenv("VC_CONV_TIME")) {      // diagnostics: the launch alone on the GPU, best and mean of n repetitions
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
        if (dbg) {       // per-workgroup phase times (100 MHz timestamps), averaged
            std::vector<long long> h(dbg_n * 8);
            hipMemcpy(h.data(), dbg, dbg_n * 64, hipMemcpyDeviceToHost);
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
            hipFree(dbg);
        }
    }
    VC_TRY(st);                                         // a refused launch leaves y / y2 as the caller passed them
    VC_TRY(read_elems(gy, ny, oprec, y, "the conv kernel"));
    if (v->split > 0) VC_TRY(read_elems(gy2, ny2, oprec, y2, "the conv kernel (second destination)"));
    return VC_OK;
}

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
    p3.name = "host 3x3"; p3.O = CO; p3.I = d->cin; p3.kh = 3; p3.kw = 3; p3.set = true;
    p3.w.assign(w, w + (size_t)CO * d->cin * 9);
    p3.b.assign(bias, bias + CO);
    p1.name = "host 1x1"; p1.O = CO; p1.I = CO; p1.kh = 1; p1.kw = 1; p1.set = true;
    p1.w.assign(w_pw, w_pw + (size_t)CO * CO);
    p1.b.assign(bias_pw, bias_pw + CO);
    VC_TRY(pack_and_upload(mem.allocs, p3, PREC_BF16));
    VC_TRY(pack_and_upload(mem.allocs, p1, PREC_BF16));
    void* dx = nullptr;
    VC_TRY(upload_elems(mem, x, npix_in * v->in_cs, PREC_BF16, &dx));
    GuardedOut gmid, gy, gy2;                          // gmid: the 3x3's own output, which the fused kernel keeps on chip
    VC_TRY(gmid.alloc(mem, npix_out * CO * 2));
    const size_t ny = npix_out * v->out_cs, ny2 = npix_out * (size_t)v->out2_cs;
    VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16));
    if (v->split > 0) VC_TRY(guarded_elems(mem, gy2, y2, ny2, PREC_BF16));
    ConvP c{}, q{};
    c.in = dx; c.w = p3.d_w; c.bias = p3.d_b; c.out = gmid.out();
    c.B = d->b; c.H = d->h; c.W = d->w; c.Cin = p3.cin_eff; c.in_cs = v->in_cs; c.in_co = v->in_co;
    c.Ho = Ho; c.Wo = Wo; c.Cout = CO; c.out_cs = CO; c.out_co = 0;
    c.kh = c.kw = 3; c.sh = c.sw = 2; c.ph = c.pw = 1;
    c.K = p3.K; c.Kp = p3.Kp; c.act = ACT_SILU; c.res_mode = RES_NONE; c.prec = PREC_BF16;
    c.act_scale = c.inv_act_scale = 1.0f; c.M = d->b * Ho * Wo; c.cfg = -1;
    q.in = gmid.out(); q.w = p1.d_w; q.bias = p1.d_b; q.out = gy.out();
    q.B = d->b; q.H = Ho; q.W = Wo; q.Cin = CO; q.in_cs = CO; q.in_co = 0;
    q.Ho = Ho; q.Wo = Wo; q.Cout = CO; q.out_cs = v->out_cs; q.out_co = v->out_co;
    q.kh = q.kw = 1; q.sh = q.sw = 1; q.ph = q.pw = 0;
    q.K = p1.K; q.Kp = p1.Kp; q.act = ACT_SILU; q.res_mode = RES_NONE; q.prec = PREC_BF16;
    q.act_scale = q.inv_act_scale = 1.0f; q.M = c.M; q.cfg = -1;
    if (v->split > 0) { q.split = v->split; q.out2 = gy2.out(); q.out2_cs = v->out2_cs; q.out2_co = v->out2_co; }
    VC_CHECK(s2halo_pw_applicable(c, q), VC_ERR_ARG, "s2 + pointwise: the fused kernel does not take this pair");
    VC_TRY(launch_s2halo_pw(c, q, nullptr));
    VC_CHECK(hipDeviceSynchronize() == hipSuccess, VC_ERR_HIP, "conv3x3s2_halo_kernel failed: %s", hipGetErrorString(hipGetLastError()));
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

// ---- the fused block kernels on host arrays (include/vcount_hip.h: vc_fused_view) ------------------------------------------------------
// Each entry point builds the ConvP chain the engine's plan builds (engine_plan.hip::yolo_c3, reid_build_ops) over buffers of its own and
// hands it to the block's launcher, whose *_applicable decides as it does in the engine, or -- v->unfused -- to launch_conv one
// convolution at a time.
static int host_param(DevScratch& mem, ConvParam& p, const char* name, int O, int I, int k, const float* w, const float* b) {
    p.name = name; p.O = O; p.I = I; p.kh = p.kw = k; p.set = true;
    p.w.assign(w, w + (size_t)O * I * k * k);
    p.b.assign(b, b + O);
    return pack_and_upload(mem.allocs, p, PREC_BF16);
}
// one bf16 convolution (1x1, or 3x3 / pad 1) of a chain, filled as PlanBuilder::conv fills it
static ConvP chain_conv(const ConvParam& p, const void* in, int in_cs, int in_co, void* out, int out_cs, int out_co, int B, int H, int W, int act) {
    ConvP c{};
    c.in = in; c.w = p.d_w; c.bias = p.d_b; c.out = out;
    c.B = B; c.H = H; c.W = W; c.Cin = p.cin_eff; c.in_cs = in_cs; c.in_co = in_co;
    c.kh = c.kw = p.kh; c.sh = c.sw = 1; c.ph = c.pw = p.kh / 2;
    c.Ho = H; c.Wo = W; c.Cout = p.O; c.out_cs = out_cs; c.out_co = out_co;
    c.K = p.K; c.Kp = p.Kp; c.act = act; c.res_mode = RES_NONE; c.prec = PREC_BF16;
    c.act_scale = c.inv_act_scale = 1.0f; c.M = B * H * W;
    c.cfg = getenv("VC_CONV_CFG") ? atoi(getenv("VC_CONV_CFG")) : -1;                // the unfused chain: the tile configuration of every launch
    return c;
}
static int chain_unfused(std::initializer_list<ConvP> chain) {
    for (const ConvP& c : chain) VC_TRY(launch_conv(c, nullptr));
    return VC_OK;
}
static int chain_finish(int st, const char* kernel) {
    if (st == VC_OK && hipDeviceSynchronize() != hipSuccess) { set_error("%s failed: %s", kernel, hipGetErrorString(hipGetLastError())); return VC_ERR_HIP; }
    return st;
}
// an intermediate the fused kernel keeps on chip: its buffer (and the guards around it) still hold the fill
static int still_filled(const GuardedOut& g, const char* kernel, const char* what) {
    std::vector<uint8_t> h(g.bytes);
    VC_TRY(g.read_back(h.data(), kernel));
    for (size_t i = 0; i < h.size(); ++i) VC_CHECK(h[i] == 0xA5, VC_ERR_HIP, "%s wrote %s (byte %zu)", kernel, what, i);
    return VC_OK;
}
static bool fused_shape_ok(int b, int h, int w) { return b >= 1 && h >= 1 && w >= 1 && (long long)b * h * w <= (1 << 22); }
// Guard blocks that hold every store of an 8 x 16 tile that lost its `y < H` / `x < W` tests: past the last frame's last pixel such a tile
// reaches less than 7 rows and 16 pixels further (bf16 pixels of cs channels)
static size_t tile_guard(int w, int cs) { return ((size_t)(8 * w + 16) * cs * 2 + 255) / 256 * 256; }
// channels [co, co + n) inside a pixel of cs channels
static bool fused_slice_ok(int cs, int co, int n) { return co >= 0 && cs >= co + n && cs <= 4096; }

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
    VC_TRY(host_param(mem, P12, "cv1 | cv2", 64, 64, 1, w12, b12));
    VC_TRY(host_param(mem, PM1, "m.cv1", 32, 32, 1, wm1, bm1));
    VC_TRY(host_param(mem, PM2, "m.cv2", 32, 32, 3, wm2, bm2));
    VC_TRY(host_param(mem, P3, "cv3", 64, 64, 1, w3, b3));
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
    VC_TRY(chain_finish(v->unfused ? chain_unfused({p12, pm1, pm2, p3}) : launch_c3_fused(p12, pm1, pm2, p3, nullptr, v->grid), "c3_fused_kernel"));   // refused: x / y as passed
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
    VC_TRY(host_param(mem, P1, "m.cv1", 64, 64, 1, w1, b1));
    VC_TRY(host_param(mem, P2, "m.cv2", 64, 64, 3, w2, b2));
    if (v->cv3) VC_TRY(host_param(mem, P3, "cv3", 128, 128, 1, w3, b3));
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
    int st;
    if (v->cv3) {
        const ConvP p3 = chain_conv(P3, my.out(), out_cs, v->out_co, zy.out(), z_cs, v->z_co, b, h, w, ACT_SILU);
        st = v->unfused ? chain_unfused({pm1, pm2, p3}) : launch_bneck_cv3_fused(pm1, pm2, p3, nullptr, v->grid);
    } else {
        st = v->unfused ? chain_unfused({pm1, pm2}) : launch_bneck_fused(pm1, pm2, nullptr, v->grid);
    }
    VC_TRY(chain_finish(st, kernel));                  // refused: x / y / z as passed
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
    VC_TRY(host_param(mem, P1, "conv1", 64, 64, 3, w1, b1));
    VC_TRY(host_param(mem, P2, "conv2", 64, 64, 3, w2, b2));
    GuardedOut gx, gy, gt;                             // gt: t of the unfused graph
    VC_TRY(guarded_elems(mem, gx, x, nx, PREC_BF16));
    if (!v->out_buf) VC_TRY(guarded_elems(mem, gy, y, ny, PREC_BF16));
    VC_TRY(gt.alloc(mem, npix * 64 * 2));
    const ConvP p1 = chain_conv(P1, gx.out(), v->in_cs, v->in_co, gt.out(), 64, 0, k, h, w, ACT_RELU);
    ConvP p2 = chain_conv(P2, gt.out(), 64, 0, v->out_buf ? gx.out() : gy.out(), out_cs, v->out_co, k, h, w, ACT_RELU);
    p2.res = gx.out(); p2.res_cs = v->in_cs; p2.res_co = v->in_co; p2.res_mode = RES_BEFORE_ACT;
    VC_TRY(chain_finish(v->unfused ? chain_unfused({p1, p2}) : launch_reid_block_fused(p1, p2, nullptr, v->grid), "reid_block_fused_kernel"));   // refused: x / y as passed
    if (!v->unfused) VC_TRY(still_filled(gt, "reid_block_fused_kernel", "t"));
    VC_TRY(read_elems(gx, nx, PREC_BF16, x, "reid_block_fused_kernel (the input buffer)"));
    if (!v->out_buf) VC_TRY(read_elems(gy, ny, PREC_BF16, y, "reid_block_fused_kernel"));
    return VC_OK;
}

int vc_letterbox_host(const uint8_t* rgb, int h, int w, int net_h, int net_w, int precision, float* out) {
    VC_CHECK(rgb && out, VC_ERR_ARG, "null argument");
    DevScratch mem;
    const LetterboxGeom g = letterbox_geom(h, w, net_h, net_w, false);
    void *ds = nullptr, *dd = nullptr;
    const int es = elem_size(precision);
    VC_TRY(mem.alloc(&ds, (size_t)h * w * 3));
    VC_TRY(mem.alloc(&dd, (size_t)net_h * net_w * 4 * es));
    VC_HIP(hipMemcpy(ds, rgb, (size_t)h * w * 3, hipMemcpyHostToDevice));
    VC_TRY(launch_letterbox((const uint8_t*)ds, dd, 1, g, precision, nullptr));
    std::vector<uint8_t> buf((size_t)net_h * net_w * 4 * es);
    VC_CHECK(hipMemcpy(buf.data(), dd, buf.size(), hipMemcpyDeviceToHost) == hipSuccess, VC_ERR_HIP, "letterbox failed: %s", hipGetErrorString(hipGetLastError()));
    for (size_t i = 0; i < (size_t)net_h * net_w; ++i)
        for (int c = 0; c < 3; ++c)
            out[i * 3 + c] = es == 4 ? ((const float*)buf.data())[i * 4 + c] : bf16_to_f32(((const uint16_t*)buf.data())[i * 4 + c]);
    return VC_OK;
}

// ---- the pool, resample, layout and cast kernels on host arrays (include/vcount_hip.h) ------------------------------------------------
// (to_elems / upload_elems / guarded_elems / read_elems: above, with the convolution entry points)
static bool prec_known(int prec, bool fp8_too) { return prec == PREC_F32 || prec == PREC_BF16 || (fp8_too && prec == PREC_FP8); }

int vc_sppf_pool_host(float* buf, int b, int h, int w, int cs, int co, int c, int precision, int form, int* ran_kernel, int* ran_ws) {
    VC_CHECK(buf && b >= 1 && h >= 1 && w >= 1 && c >= 1 && co >= 0 && cs >= co + 4 * c, VC_ERR_ARG, "sppf: bad shape");
    VC_CHECK(prec_known(precision, true) && (form == 0 || form == 1), VC_ERR_ARG, "sppf: bad precision or form");
    if (ran_kernel) *ran_kernel = 0;
    if (ran_ws) *ran_ws = 0;
    DevScratch mem;
    GuardedOut dd;
    const size_t n = (size_t)b * h * w * cs;
    VC_TRY(guarded_elems(mem, dd, buf, n, precision));
    const View cat{dd.out(), b, h, w, c, cs, co, elem_size(precision)};
    SppfRan ran{0, 0};
    VC_TRY(launch_sppf_pool(cat, c, precision, form, nullptr, &ran));
    VC_TRY(read_elems(dd, n, precision, buf, "the SPPF pool kernel"));
    if (ran_kernel) *ran_kernel = ran.kernel;
    if (ran_ws) *ran_ws = ran.ws;
    return VC_OK;
}

int vc_upsample2x_host(const float* src, int b, int h, int w, int c, float* dst, int cs, int co, int precision) {
    VC_CHECK(src && dst && b >= 1 && h >= 1 && w >= 1 && c >= 1 && co >= 0 && cs >= co + c, VC_ERR_ARG, "upsample: bad shape");
    VC_CHECK(prec_known(precision, true), VC_ERR_ARG, "upsample: bad precision");
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    const size_t n = (size_t)b * 2 * h * 2 * w * cs;
    VC_TRY(upload_elems(mem, src, (size_t)b * h * w * c, precision, &ds));
    VC_TRY(guarded_elems(mem, dd, dst, n, precision));
    const View a{ds, b, h, w, c, c, 0, elem_size(precision)}, d{dd.out(), b, 2 * h, 2 * w, c, cs, co, elem_size(precision)};
    VC_TRY(launch_upsample2x(a, d, precision, nullptr));
    return read_elems(dd, n, precision, dst, "upsample2x_kernel");
}

int vc_maxpool3s2_host(const float* src, int b, int h, int w, int c, float* dst, int cs, int co, int precision) {
    VC_CHECK(src && dst && b >= 1 && h >= 1 && w >= 1 && c >= 1 && co >= 0 && cs >= co + c, VC_ERR_ARG, "maxpool: bad shape");
    VC_CHECK(prec_known(precision, false), VC_ERR_ARG, "maxpool: precision must be VC_PREC_BF16 or VC_PREC_F32");
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const size_t n = (size_t)b * ho * wo * cs;
    VC_TRY(upload_elems(mem, src, (size_t)b * h * w * c, precision, &ds));
    VC_TRY(guarded_elems(mem, dd, dst, n, precision));
    const View a{ds, b, h, w, c, c, 0, elem_size(precision)}, d{dd.out(), b, ho, wo, c, cs, co, elem_size(precision)};
    VC_TRY(launch_maxpool3s2(a, d, precision, nullptr));
    return read_elems(dd, n, precision, dst, "maxpool3s2_kernel");
}

int vc_avgpool_l2norm_host(const float* x, int k, int h, int w, int precision, float* out) {
    VC_CHECK(x && out && k >= 1 && h >= 1 && w >= 1, VC_ERR_ARG, "avgpool: bad shape");
    VC_CHECK(prec_known(precision, false), VC_ERR_ARG, "avgpool: precision must be VC_PREC_BF16 or VC_PREC_F32");
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    VC_TRY(upload_elems(mem, x, (size_t)k * h * w * VC_FEAT_DIM, precision, &ds));
    VC_TRY(dd.alloc(mem, (size_t)k * VC_FEAT_DIM * sizeof(float)));
    const View a{ds, k, h, w, VC_FEAT_DIM, VC_FEAT_DIM, 0, elem_size(precision)};
    VC_TRY(launch_avgpool_l2norm(a, (float*)dd.out(), precision, nullptr));
    return dd.read_back((uint8_t*)out, "avgpool_l2norm_kernel");
}

int vc_nchw_to_nhwc_pad_host(const float* x, int k, int c, int h, int w, int cpad, int precision, float* out) {
    VC_CHECK(x && out && k >= 1 && c >= 1 && h >= 1 && w >= 1, VC_ERR_ARG, "layout: bad shape");
    VC_CHECK(prec_known(precision, false), VC_ERR_ARG, "layout: precision must be VC_PREC_BF16 or VC_PREC_F32");
    VC_CHECK(cpad == reid_cpad(precision) && c <= cpad, VC_ERR_ARG, "layout: cpad must be %d at this precision", reid_cpad(precision));
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    const size_t n = (size_t)k * h * w * cpad;
    VC_TRY(upload_elems(mem, x, (size_t)k * c * h * w, PREC_F32, &ds));
    VC_TRY(dd.alloc(mem, n * elem_size(precision)));
    VC_TRY(launch_nchw_to_nhwc_pad((const float*)ds, k, c, h, w, dd.out(), cpad, precision, nullptr));
    return read_elems(dd, n, precision, out, "nchw_to_nhwc_pad_kernel");
}

int vc_bf16_to_fp8_host(const float* src, int npix, int c, int src_cs, int src_co, float inv_scale, uint8_t* dst, int dst_cs, int dst_co) {
    VC_CHECK(src && dst && npix >= 1 && c >= 1 && src_co >= 0 && src_cs >= src_co + c && dst_co >= 0 && dst_cs >= dst_co + c, VC_ERR_ARG, "bf16 -> fp8: bad shape");
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    VC_TRY(upload_elems(mem, src, (size_t)npix * src_cs, PREC_BF16, &ds));
    VC_TRY(dd.alloc(mem, (size_t)npix * dst_cs, dst));
    const View a{ds, 1, 1, npix, c, src_cs, src_co, 2}, d{dd.out(), 1, 1, npix, c, dst_cs, dst_co, 1};
    VC_TRY(launch_bf16_to_fp8(a, d, inv_scale, nullptr));
    return dd.read_back(dst, "bf16_to_fp8_kernel");
}

int vc_reid_stem_pool_host(const float* crops, int k, const float* w, const float* bias, float* out) {
    VC_CHECK(crops && w && bias && out && k >= 1, VC_ERR_ARG, "reid stem: bad argument");
    constexpr int S = VC_REID_SIZE, P = (S - 1) / 2 + 1, CO = 64;
    DevScratch mem;
    ConvParam p;
    p.name = "host"; p.O = CO; p.I = 3; p.kh = 3; p.kw = 3; p.set = true;
    p.w.assign(w, w + (size_t)CO * 3 * 3 * 3);
    p.b.assign(bias, bias + CO);
    VC_TRY(pack_and_upload(mem.allocs, p, PREC_BF16));
    const size_t npix = (size_t)k * S * S;
    std::vector<float> x8(npix * p.cin_eff, 0.f);                     // channels 3 .. cin_eff - 1 stay zero, as in the ReID input buffer
    for (size_t i = 0; i < npix; ++i)
        for (int ch = 0; ch < 3; ++ch) x8[i * p.cin_eff + ch] = crops[i * 3 + ch];
    void* dx = nullptr;
    VC_TRY(upload_elems(mem, x8.data(), x8.size(), PREC_BF16, &dx));
    GuardedOut dd;
    const size_t n = (size_t)k * P * P * CO;
    VC_TRY(dd.alloc(mem, n * 2));
    ConvP cp{};
    cp.in = dx; cp.w = p.d_w; cp.bias = p.d_b; cp.out = nullptr;      // the conv's own output never exists
    cp.B = k; cp.H = S; cp.W = S; cp.Cin = p.cin_eff; cp.in_cs = p.cin_eff; cp.in_co = 0;
    cp.Ho = S; cp.Wo = S; cp.Cout = CO; cp.out_cs = CO; cp.out_co = 0;
    cp.kh = cp.kw = 3; cp.sh = cp.sw = 1; cp.ph = cp.pw = 1;
    cp.K = p.K; cp.Kp = p.Kp; cp.act = ACT_RELU; cp.res_mode = RES_NONE; cp.out_f32 = 0; cp.prec = PREC_BF16;
    cp.act_scale = cp.inv_act_scale = 1.0f; cp.M = k * S * S; cp.cfg = -1;
    VC_CHECK(reid_stem_applicable(cp, CO, 0), VC_ERR_ARG, "reid stem: the fused kernel does not take this convolution");
    VC_TRY(launch_reid_stem_pool(cp, dd.out(), nullptr));
    return read_elems(dd, n, PREC_BF16, out, "reid_stem_pool_kernel");
}

// ---- sized batches: the letterbox and crop kernels with their per-frame tables, on host arrays --------------------------------------
// frames of their own sizes uploaded into cells (include/vcount_hip.h) -> *cells_out (device, in mem); *cell_out: the cell size.
// Network shapes are not compared here (img_size 1 gives every frame 32 x 32).
static int upload_cells(DevScratch& mem, const uint8_t* const* frames, const vc_frame_dims* dims, int b, uint8_t** cells_out, size_t* cell_out) {
    VC_CHECK(frames, VC_ERR_ARG, "null frame list");
    SizedDims sd;
    VC_TRY(sized_dims_resolve(dims, b, 1, sd));
    for (int f = 0; f < b; ++f) VC_CHECK(frames[f], VC_ERR_ARG, "frame %d: null data", f);
    const size_t cell = sd.cell;
    VC_TRY(mem.alloc(cells_out, (size_t)b * cell));
    VC_HIP(hipMemset(*cells_out, 0xA5, (size_t)b * cell));             // what a kernel that strays outside a frame would pick up
    for (int f = 0; f < b; ++f) VC_HIP(hipMemcpy(*cells_out + (size_t)f * cell, frames[f], (size_t)dims[f].h * dims[f].w * 3, hipMemcpyHostToDevice));
    *cell_out = cell;
    return VC_OK;
}

int vc_letterbox_frames_host(const uint8_t* const* frames, const vc_frame_dims* dims, int b, int net_h, int net_w, int swap_rb, int precision, float* out) {
    VC_CHECK(out, VC_ERR_ARG, "null argument");
    VC_CHECK(net_h >= 1 && net_w >= 4 && net_w % 4 == 0, VC_ERR_ARG, "network tensor %dx%d (the width must be a multiple of 4)", net_h, net_w);
    VC_CHECK(precision == VC_PREC_BF16 || precision == VC_PREC_F32, VC_ERR_ARG, "precision must be VC_PREC_BF16 or VC_PREC_F32");
    DevScratch mem;
    uint8_t* dc = nullptr;
    void *dd = nullptr, *dt = nullptr;
    size_t cell = 0;
    const int es = elem_size(precision);
    VC_TRY(upload_cells(mem, frames, dims, b, &dc, &cell));
    const size_t px = (size_t)b * net_h * net_w;
    VC_TRY(mem.alloc(&dd, px * 4 * es));
    VC_TRY(mem.alloc(&dt, (size_t)b * sizeof(LetterboxFrame)));
    std::vector<LetterboxFrame> tab((size_t)b);
    for (int f = 0; f < b; ++f) tab[f] = letterbox_frame((long long)((size_t)f * cell), letterbox_geom(dims[f].h, dims[f].w, net_h, net_w, swap_rb != 0));
    VC_HIP(hipMemcpy(dt, tab.data(), (size_t)b * sizeof(LetterboxFrame), hipMemcpyHostToDevice));
    VC_TRY(launch_letterbox_frames(dc, (const LetterboxFrame*)dt, dd, b, net_h, net_w, swap_rb ? 1 : 0, precision, nullptr));
    std::vector<uint8_t> buf(px * 4 * es);
    VC_CHECK(hipMemcpy(buf.data(), dd, buf.size(), hipMemcpyDeviceToHost) == hipSuccess, VC_ERR_HIP, "letterbox_frames_kernel failed: %s", hipGetErrorString(hipGetLastError()));
    for (size_t i = 0; i < px; ++i)
        for (int c = 0; c < 3; ++c)
            out[i * 3 + c] = es == 4 ? ((const float*)buf.data())[i * 4 + c] : bf16_to_f32(((const uint16_t*)buf.data())[i * 4 + c]);
    return VC_OK;
}

// The letterbox kernels on the caller's own device buffers (measurement; the counterpart of vc_frames_to_bgr_dev): frames_dev = b packed
// h x w x 3 u8 frames, out_dev = b x net_h x net_w x 4 elements of `precision`.  mode 0: launch_letterbox, the kernels a uniform batch
// runs.  mode 1: a table of b entries for these uniform frames is built and copied to table_dev (b * 64 bytes, a blocking copy), then
// letterbox_frames_kernel runs; mode 2: letterbox_frames_kernel with the table as the last mode-1 call left it.  NULL stream, no wait.
int vc_letterbox_dev(const void* frames_dev, int b, int h, int w, int net_h, int net_w, int swap_rb, int precision, void* out_dev, void* table_dev, int mode) {
    VC_CHECK(frames_dev && out_dev && (mode == 0 || table_dev), VC_ERR_ARG, "null argument");
    VC_CHECK(b >= 1 && h >= 1 && w >= 1 && net_h >= 1 && net_w >= 4 && net_w % 4 == 0 && mode >= 0 && mode <= 2, VC_ERR_ARG, "bad argument");
    VC_CHECK(precision == VC_PREC_BF16 || precision == VC_PREC_F32, VC_ERR_ARG, "precision must be VC_PREC_BF16 or VC_PREC_F32");
    static_assert(sizeof(LetterboxFrame) <= 64, "the caller reserves 64 bytes per table entry");
    const LetterboxGeom g = letterbox_geom(h, w, net_h, net_w, swap_rb != 0);
    if (mode == 0) return launch_letterbox((const uint8_t*)frames_dev, out_dev, b, g, precision, nullptr);
    if (mode == 1) {
        std::vector<LetterboxFrame> tab((size_t)b);
        for (int f = 0; f < b; ++f) tab[f] = letterbox_frame((long long)((size_t)f * h * w * 3), g);
        VC_HIP(hipMemcpy(table_dev, tab.data(), (size_t)b * sizeof(LetterboxFrame), hipMemcpyHostToDevice));
    }
    return launch_letterbox_frames((const uint8_t*)frames_dev, (const LetterboxFrame*)table_dev, out_dev, b, net_h, net_w, swap_rb ? 1 : 0, precision, nullptr);
}

int vc_crop_resize_frames_host(const uint8_t* const* bgr, const vc_frame_dims* dims, int b, const int* frame_of_box, const double* boxes, int k, float* out) {
    VC_CHECK(frame_of_box && boxes && out && k >= 1, VC_ERR_ARG, "bad argument");
    std::vector<int> crops((size_t)k * 5);
    for (int i = 0; i < k; ++i) {
        const int f = frame_of_box[i];
        VC_CHECK(dims && f >= 0 && f < b, VC_ERR_ARG, "box %d: frame %d outside [0, %d)", i, f, b);
        int c[4];
        crop_corners(boxes + (size_t)i * 4, dims[f].w, dims[f].h, c);                 // the frame's own W - 1, H - 1
        VC_CHECK(c[2] > c[0] && c[3] > c[1], VC_ERR_ARG, "box %d gives an empty crop (the reference's cv2.resize raises here)", i);
        crops[(size_t)i * 5] = f;
        memcpy(&crops[(size_t)i * 5 + 1], c, sizeof(c));
    }
    DevScratch mem;
    uint8_t* dc = nullptr;
    void *dd = nullptr, *dt = nullptr, *dk = nullptr;
    size_t cell = 0;
    const size_t px = (size_t)k * VC_REID_SIZE * VC_REID_SIZE;
    VC_TRY(upload_cells(mem, bgr, dims, b, &dc, &cell));
    VC_TRY(mem.alloc(&dd, px * 4 * sizeof(float)));
    VC_TRY(mem.alloc(&dt, (size_t)b * sizeof(CropFrame)));
    VC_TRY(mem.alloc(&dk, crops.size() * sizeof(int)));
    std::vector<CropFrame> tab((size_t)b);
    for (int f = 0; f < b; ++f) tab[f] = CropFrame{(long long)((size_t)f * cell), dims[f].w, 0};
    VC_HIP(hipMemcpy(dt, tab.data(), (size_t)b * sizeof(CropFrame), hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(dk, crops.data(), crops.size() * sizeof(int), hipMemcpyHostToDevice));
    VC_TRY(launch_crop_resize(dc, 0, 0, (const int*)dk, k, dd, 4, VC_PREC_F32, nullptr, false, (const CropFrame*)dt));
    std::vector<float> buf(px * 4);
    VC_CHECK(hipMemcpy(buf.data(), dd, buf.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess, VC_ERR_HIP, "crop_resize_kernel failed: %s", hipGetErrorString(hipGetLastError()));
    for (size_t i = 0; i < px; ++i)
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = buf[i * 4 + c];
    return VC_OK;
}

}  // extern "C"
