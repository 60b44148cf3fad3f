// Render path (the annotated video of the reference's VideoWriter.write_full_to_video -> visualize_merged, modules/datasets.py:132-145
// and utilities/counting/utils.py:299-331): per batch  source -> BGR work buffer -> overlay -> 4:2:0 YUV -> the caller's surface,
// asynchronous, chained out of kernels that exist on their own: yuv_to_bgr_kernel (yuv_ingest.hip), overlay_kernel (overlay.hip) and
// bgr_to_yuv_kernel (yuv_egress.hip).  A frame never exists as BGR on the host.
//
// A context belongs to an engine (device, lifetime) and shares nothing else with it: not the four ingest slots, not the pending
// list, not a detector.  It owns two streams -- `in` (the copy or conversion into the work buffer, the primitive lists, the overlay)
// and `out` (the conversion to YUV and the delivery) -- and `depth` buffer sets handed out round-robin, so that the upload of batch
// n + 1 runs beside the download of batch n.  Orders between the streams and between the users of a buffer set are events; submit
// never waits on the host.  No captured graphs.
#include <algorithm>
#include <deque>

#include "engine.h"

struct vc_render {
    vc_engine* e = nullptr;
    int max_batch = 0, max_h = 0, max_w = 0, depth = 0;
    hipStream_t s_in = nullptr, s_out = nullptr;
    struct Set {
        uint8_t* d_raw = nullptr; size_t raw_bytes = 0;        // raw 4:2:0 bytes of a YUV source in host memory
        uint8_t* d_bgr = nullptr;                              // [max_batch][max_h][max_w][3] work buffer: what the overlay paints
        uint8_t* d_yuv = nullptr; size_t yuv_bytes = 0;        // output surfaces of a batch that is delivered to host memory
        char* h_lists = nullptr; char* d_lists = nullptr; size_t lists_bytes = 0;   // the batch's primitive lists: pinned copy made at submit, device copy
        hipEvent_t ev_in = nullptr, ev_done = nullptr;         // work buffer painted / output complete
        bool used = false;
        vc_live* live = nullptr; int live_token = -1;          // vc_render_submit_live: the counter whose list buffer this batch reads until it is collected
    } set[4];
    unsigned seq = 0;                                          // batches submitted so far: batch n uses set n % depth
    std::deque<int> outstanding;                               // sets of the batches not yet collected, oldest first
};

namespace vc {

namespace {

int grow_dev(uint8_t** p, size_t* have, size_t need) {         // the set is idle when this runs: its last batch has been collected
    if (need <= *have && *p) return VC_OK;
    if (*p) { VC_HIP(hipFree(*p)); *p = nullptr; *have = 0; }
    VC_HIP(hipMalloc((void**)p, std::max<size_t>(need, 16)));
    *have = need;
    return VC_OK;
}

// plane bytes only: rows x width bytes of every plane of every frame, nothing of the padding between them
int copy_planes(const YuvGeom& g, const uint8_t* src, uint8_t* dst, int b, hipStream_t s) {
    const int crow = g.nv12 ? g.w : g.w / 2, hc = g.h / 2;
    const bool tight = g.pitch_y == g.w && g.pitch_c == crow && g.off_c == (size_t)g.w * g.h &&
                       (g.nv12 || g.off_v == g.off_c + (size_t)crow * hc) && g.frame_stride == g.frame_end;
    if (tight) {
        VC_HIP(hipMemcpyAsync(dst, src, yuv_batch_bytes(g, b), hipMemcpyDeviceToHost, s));
        return VC_OK;
    }
    for (int f = 0; f < b; ++f) {
        const size_t o = (size_t)f * g.frame_stride;
        VC_HIP(hipMemcpy2DAsync(dst + o, g.pitch_y, src + o, g.pitch_y, g.w, g.h, hipMemcpyDeviceToHost, s));
        VC_HIP(hipMemcpy2DAsync(dst + o + g.off_c, g.pitch_c, src + o + g.off_c, g.pitch_c, crow, hc, hipMemcpyDeviceToHost, s));
        if (!g.nv12) VC_HIP(hipMemcpy2DAsync(dst + o + g.off_v, g.pitch_c, src + o + g.off_v, g.pitch_c, crow, hc, hipMemcpyDeviceToHost, s));
    }
    return VC_OK;
}

int render_free(vc_render* r) {
    hipSetDevice(r->e->cfg.device);
    if (r->s_in) hipStreamSynchronize(r->s_in);
    if (r->s_out) hipStreamSynchronize(r->s_out);
    for (vc_render::Set& t : r->set) {
        if (t.live) (void)live_overlay_release(t.live, t.live_token);     // a batch never collected: its list buffer is free again
        if (t.d_raw) hipFree(t.d_raw);
        if (t.d_bgr) hipFree(t.d_bgr);
        if (t.d_yuv) hipFree(t.d_yuv);
        if (t.d_lists) hipFree(t.d_lists);
        if (t.h_lists) hipHostFree(t.h_lists);
        if (t.ev_in) hipEventDestroy(t.ev_in);
        if (t.ev_done) hipEventDestroy(t.ev_done);
    }
    if (r->s_in) hipStreamDestroy(r->s_in);
    if (r->s_out) hipStreamDestroy(r->s_out);
    delete r;
    return VC_OK;
}

}  // namespace

void render_destroy_all(vc_engine* e) {
    for (vc_render* r : e->renders) render_free(r);
    e->renders.clear();
}

void render_forget_live(vc_engine* e, vc_live* l) {
    for (vc_render* r : e->renders)
        for (vc_render::Set& t : r->set)
            if (t.live == l) {
                (void)hipStreamSynchronize(r->s_in);             // the overlay launch that reads the counter's lists
                t.live = nullptr; t.live_token = -1;
            }
}

}  // namespace vc

using namespace vc;

// vc_render_submit and vc_render_submit_live: the lists come from the host (copied here) or, with `live`, from the counter's oldest
// unconsumed list buffer in device memory, behind the event recorded after its build launch
static int render_submit(vc_render* r, const vc_render_src* src, int b, int h, int w, const int32_t* prims12, const int32_t* frame_first, vc_live* live,
                         const vc_yuv_desc* out_desc, void* out, int out_is_dev);

extern "C" {

int vc_render_create(vc_engine* e, int max_batch, int max_h, int max_w, int depth, vc_render** out) {
    VC_CHECK(out, VC_ERR_ARG, "null argument");
    *out = nullptr;
    VC_CHECK(max_batch >= 1 && max_h >= 2 && max_w >= 2, VC_ERR_ARG, "bad render capacity: %d frames of %dx%d", max_batch, max_h, max_w);
    VC_CHECK(depth >= 1 && depth <= 4, VC_ERR_ARG, "depth (batches in flight) must be 1..4, got %d", depth);
    VC_CHECK((size_t)max_batch * max_h * max_w <= ((size_t)1 << 36), VC_ERR_CAPACITY, "a work buffer of %d frames of %dx%d is out of range", max_batch, max_h, max_w);
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    VC_HIP(hipSetDevice(e->cfg.device));
    vc_render* r = new vc_render();
    r->e = e; r->max_batch = max_batch; r->max_h = max_h; r->max_w = max_w; r->depth = depth;
    bool ok = hipStreamCreateWithFlags(&r->s_in, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&r->s_out, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < depth && ok; ++i)
        ok = hipEventCreateWithFlags(&r->set[i].ev_in, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&r->set[i].ev_done, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        set_error("render: stream / event create failed: %s", hipGetErrorString(hipGetLastError()));
        render_free(r);
        return VC_ERR_HIP;
    }
    e->renders.push_back(r);
    *out = r;
    return VC_OK;
}

int vc_render_destroy(vc_render* r) {
    if (!r) return VC_OK;
    auto& v = r->e->renders;
    v.erase(std::remove(v.begin(), v.end(), r), v.end());
    return render_free(r);
}

int vc_render_submit(vc_render* r, const vc_render_src* src, int b, int h, int w, const int32_t* prims12, const int32_t* frame_first,
                     const vc_yuv_desc* out_desc, void* out, int out_is_dev) {
    return render_submit(r, src, b, h, w, prims12, frame_first, nullptr, out_desc, out, out_is_dev);
}

int vc_render_submit_live(vc_render* r, vc_live* live, const vc_render_src* src, int b, int h, int w, const vc_yuv_desc* out_desc, void* out, int out_is_dev) {
    VC_CHECK(r && live, VC_ERR_ARG, "null argument");
    VC_CHECK(live->e == r->e, VC_ERR_ARG, "the counter and the render context belong to different engines");
    return render_submit(r, src, b, h, w, nullptr, nullptr, live, out_desc, out, out_is_dev);
}

}  // extern "C"

static int render_submit(vc_render* r, const vc_render_src* src, int b, int h, int w, const int32_t* prims12, const int32_t* frame_first, vc_live* live,
                         const vc_yuv_desc* out_desc, void* out, int out_is_dev) {
    // ---- every refusal comes before anything is enqueued ----
    VC_CHECK(r && src && src->data && out_desc && out, VC_ERR_ARG, "null argument");
    VC_CHECK(src->kind >= VC_SRC_BGR_HOST && src->kind <= VC_SRC_YUV_DEV, VC_ERR_ARG, "unknown source kind %d (VC_SRC_*)", src->kind);
    VC_CHECK((prims12 == nullptr) == (frame_first == nullptr), VC_ERR_ARG, "prims12 and frame_first go together (both NULL = no overlay)");
    const bool src_yuv = src->kind == VC_SRC_YUV_HOST || src->kind == VC_SRC_YUV_DEV;
    YuvGeom go, gi{};
    VC_TRY(yuv_resolve_out(out_desc, b, h, w, go));
    if (src_yuv) VC_TRY(yuv_resolve(&src->desc, b, h, w, gi));
    if (prims12) VC_TRY(overlay_check_lists(b, prims12, frame_first));
    VC_CHECK(b <= r->max_batch && h <= r->max_h && w <= r->max_w, VC_ERR_CAPACITY, "batch of %d frames %dx%d exceeds the render context (%d frames %dx%d)",
             b, h, w, r->max_batch, r->max_h, r->max_w);
    VC_CHECK((int)r->outstanding.size() < r->depth, VC_ERR_STATE, "%d batches are outstanding (depth %d): vc_render_collect first", (int)r->outstanding.size(), r->depth);

    VC_HIP(hipSetDevice(r->e->cfg.device));
    const int si = (int)(r->seq % (unsigned)r->depth);
    vc_render::Set& t = r->set[si];                          // idle: its last batch (seq - depth) has been collected
    const size_t bgr_bytes = (size_t)b * h * w * 3;
    const int n = prims12 ? frame_first[b] : 0;
    const size_t prim_bytes = (size_t)n * 12 * sizeof(int32_t), lists_bytes = prim_bytes + (size_t)(b + 1) * sizeof(int);
    // buffers of each kind on first use
    if (!t.d_bgr) VC_HIP(hipMalloc((void**)&t.d_bgr, (size_t)r->max_batch * r->max_h * r->max_w * 3));
    if (src->kind == VC_SRC_YUV_HOST) VC_TRY(grow_dev(&t.d_raw, &t.raw_bytes, std::max(yuv_batch_bytes(gi, b), (size_t)r->max_batch * r->max_h * r->max_w * 3 / 2)));
    if (!out_is_dev) VC_TRY(grow_dev(&t.d_yuv, &t.yuv_bytes, std::max(yuv_batch_bytes(go, b), (size_t)r->max_batch * r->max_h * r->max_w * 3 / 2)));
    if (n > 0 && lists_bytes > t.lists_bytes) {
        if (t.d_lists) { VC_HIP(hipFree(t.d_lists)); t.d_lists = nullptr; }
        if (t.h_lists) { VC_HIP(hipHostFree(t.h_lists)); t.h_lists = nullptr; }
        t.lists_bytes = 0;
        VC_HIP(hipMalloc((void**)&t.d_lists, lists_bytes * 2));
        VC_HIP(hipHostMalloc((void**)&t.h_lists, lists_bytes * 2, hipHostMallocDefault));
        t.lists_bytes = lists_bytes * 2;
    }

    // the counter's oldest unconsumed lists (the last refusal: nothing unconsumed VC_ERR_STATE, another batch's b / h / w VC_ERR_ARG)
    const void* live_prims = nullptr; const int* live_first = nullptr; hipEvent_t live_built = nullptr; int live_token = -1;
    if (live) VC_TRY(live_overlay_take(live, b, h, w, &live_prims, &live_first, &live_built, &live_token));
    t.live = live; t.live_token = live_token;

    // ---- in: source -> work buffer, overlay ----
    if (t.used) VC_HIP(hipStreamWaitEvent(r->s_in, t.ev_done, 0));      // behind the batch that last used this set (`out` is behind it by stream order)
    switch (src->kind) {
    case VC_SRC_BGR_HOST: VC_HIP(hipMemcpyAsync(t.d_bgr, src->data, bgr_bytes, hipMemcpyHostToDevice, r->s_in)); break;
    case VC_SRC_BGR_DEV: VC_HIP(hipMemcpyAsync(t.d_bgr, src->data, bgr_bytes, hipMemcpyDeviceToDevice, r->s_in)); break;   // never painted in place
    case VC_SRC_YUV_HOST:
        VC_HIP(hipMemcpyAsync(t.d_raw, src->data, yuv_batch_bytes(gi, b), hipMemcpyHostToDevice, r->s_in));
        VC_TRY(launch_yuv_to_bgr(gi, t.d_raw, t.d_bgr, b, r->s_in));
        break;
    default: VC_TRY(launch_yuv_to_bgr(gi, (const uint8_t*)src->data, t.d_bgr, b, r->s_in)); break;
    }
    if (n > 0) {
        memcpy(t.h_lists, prims12, prim_bytes);              // the two lists are copied here: the caller may reuse them at once
        memcpy(t.h_lists + prim_bytes, frame_first, (size_t)(b + 1) * sizeof(int));
        VC_HIP(hipMemcpyAsync(t.d_lists, t.h_lists, lists_bytes, hipMemcpyHostToDevice, r->s_in));
        VC_TRY(launch_overlay(t.d_bgr, b, h, w, t.d_lists, (const int*)(t.d_lists + prim_bytes), r->s_in));
    }
    if (live) {                                              // no host wait, no list copy: the lists are read where the build kernel wrote them
        VC_HIP(hipStreamWaitEvent(r->s_in, live_built, 0));
        VC_TRY(launch_overlay(t.d_bgr, b, h, w, live_prims, live_first, r->s_in));
    }
    VC_HIP(hipEventRecord(t.ev_in, r->s_in));
    // ---- out: work buffer -> YUV -> the caller's surface ----
    VC_HIP(hipStreamWaitEvent(r->s_out, t.ev_in, 0));
    if (out_is_dev) {
        VC_TRY(launch_bgr_to_yuv(go, t.d_bgr, (uint8_t*)out, b, r->s_out));
    } else {
        VC_TRY(launch_bgr_to_yuv(go, t.d_bgr, t.d_yuv, b, r->s_out));
        VC_TRY(copy_planes(go, t.d_yuv, (uint8_t*)out, b, r->s_out));
    }
    VC_HIP(hipEventRecord(t.ev_done, r->s_out));
    t.used = true;
    r->seq++;
    r->outstanding.push_back(si);
    return VC_OK;
}

extern "C" {

int vc_render_collect(vc_render* r) {
    VC_CHECK(r, VC_ERR_ARG, "null argument");
    VC_CHECK(!r->outstanding.empty(), VC_ERR_STATE, "vc_render_collect: no batch is outstanding");
    const int si = r->outstanding.front();
    r->outstanding.pop_front();
    vc_render::Set& t = r->set[si];
    VC_HIP(hipEventSynchronize(t.ev_done));
    if (t.live) {                                            // the counter's list buffer counts as consumed from here on
        vc_live* l = t.live;
        const int token = t.live_token;
        t.live = nullptr; t.live_token = -1;
        VC_TRY(live_overlay_release(l, token));
    }
    return VC_OK;
}

}  // extern "C"
