// The detect tail (detect_post.hip, class_filter.hip) on host arrays (include/vcount_hip.h): the decode kernels, the three NMS kernels and the
// class filter in front of them.  Entry points only: each stages its arrays (host_stage.h), runs the launchers the engine runs and reads the
// result back.  None of them touches a vc_engine.
#include <algorithm>

#include "engine.h"

using namespace vc;

namespace {
// The buffers of the detect tail for the stateless entry points below.  nms = false: the candidate side only (what the decode writes).
int post_alloc(DevScratch& mem, DetectPostBuffers& pb, float** geom, int B, int max_cand, int max_det, bool nms) {
    const size_t mc = (size_t)B * max_cand;
    VC_TRY(mem.alloc(&pb.cand_box, mc * 16)); VC_TRY(mem.alloc(&pb.cand_conf, mc * 4)); VC_TRY(mem.alloc(&pb.cand_cls, mc * 4));
    VC_TRY(mem.alloc(&pb.cand_idx, mc * 4)); VC_TRY(mem.alloc(&pb.cand_count, (size_t)B * 4)); VC_TRY(mem.alloc(&pb.overflow, (size_t)B * 4));
    VC_HIP(hipMemset(pb.cand_count, 0, (size_t)B * 4));
    VC_HIP(hipMemset(pb.overflow, 0, (size_t)B * 4));
    if (!nms) return VC_OK;
    VC_TRY(mem.alloc(&pb.sort_box, mc * 16)); VC_TRY(mem.alloc(&pb.sort_conf, mc * 4)); VC_TRY(mem.alloc(&pb.sort_cls, mc * 4));
    VC_TRY(mem.alloc(&pb.mask, mc * (max_cand / 64) * 8)); VC_TRY(mem.alloc(&pb.det, (size_t)B * max_det * 24));
    VC_TRY(mem.alloc(&pb.det_count, (size_t)B * 4)); VC_TRY(mem.alloc(geom, (size_t)B * 20));
    return VC_OK;
}

// the scale_coords scalars of every frame (geom4[f] = {net_h, net_w, src_h, src_w}; null or net_h <= 0: network pixels, no rescale, no clamp)
int post_geom(float* geom, int B, const int* geom4) {
    std::vector<float> hg((size_t)B * 5);
    for (int f = 0; f < B; ++f) {
        float* g = &hg[(size_t)f * 5];
        if (geom4 && geom4[f * 4] > 0) scale_geom_host(ScaleGeom{geom4[f * 4], geom4[f * 4 + 1], geom4[f * 4 + 2], geom4[f * 4 + 3]}, g);
        else { g[0] = 1.f; g[1] = 0.f; g[2] = 0.f; g[3] = 1e30f; g[4] = 1e30f; }
    }
    VC_HIP(hipMemcpy(geom, hg.data(), hg.size() * 4, hipMemcpyHostToDevice));
    return VC_OK;
}

// launch_nms over filled candidate buffers + download.  out_n[f] is the device's count: -1 for a frame whose overflow flag is set.
int post_nms(DetectPostBuffers& pb, float* geom, int B, int max_cand, int max_det, float iou, const int* geom4, float* out6, int* out_n) {
    VC_TRY(post_geom(geom, B, geom4));
    VC_TRY(launch_nms(B, max_cand, max_det, iou, geom, pb, nullptr));
    VC_TRY(kernel_wait("nms kernels"));
    VC_HIP(hipMemcpy(out_n, pb.det_count, (size_t)B * 4, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(out6, pb.det, (size_t)B * max_det * 24, hipMemcpyDeviceToHost));
    return VC_OK;
}

// Explicit candidate lists ([b][max_cand] arrays, candidate order = position) through the three NMS kernels.  With a class map
// cand_class_filter_kernel runs in front of them and det_relabel_kernel behind them, on the same device buffers (class_filter.hip).  The
// rows and the compacted cand_idx (= the kept candidates' positions) lie between guard blocks.
int nms_candidates(const float* boxes4, const float* conf, const int* cls, const int* counts, int b, const int* label_of_class, int n_classes,
                   float iou, int max_det, int max_cand, const int* geom4, float* out6, int* out_n, int* kept_count, int* kept_idx) {
    DevScratch mem;
    DetectPostBuffers pb{};
    float* geom = nullptr;
    int* d_map = nullptr;
    VC_TRY(post_alloc(mem, pb, &geom, b, max_cand, max_det, true));
    const size_t mc = (size_t)b * max_cand;
    std::vector<int> idx(mc);
    for (size_t i = 0; i < mc; ++i) idx[i] = (int)(i % max_cand);
    GuardedOut gdet, gidx;
    VC_TRY(gdet.alloc(mem, (size_t)b * max_det * 24));
    VC_TRY(gidx.alloc(mem, mc * 4, idx.data()));
    pb.det = gdet.as<float>();
    pb.cand_idx = gidx.as<int>();
    if (label_of_class) VC_TRY(mem.upload(&d_map, label_of_class, (size_t)n_classes * 4));
    VC_HIP(hipMemcpy(pb.cand_box, boxes4, mc * 16, hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(pb.cand_conf, conf, mc * 4, hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(pb.cand_cls, cls, mc * 4, hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(pb.cand_count, counts, (size_t)b * 4, hipMemcpyHostToDevice));
    VC_TRY(post_geom(geom, b, geom4));
    if (d_map) VC_TRY(launch_cand_class_filter(b, n_classes, max_cand, d_map, pb, nullptr));
    VC_TRY(launch_nms(b, max_cand, max_det, iou, geom, pb, nullptr));
    if (d_map) VC_TRY(launch_det_relabel(b, n_classes, max_det, d_map, pb, nullptr));
    VC_TRY(kernel_wait(d_map ? "class filter / nms kernels" : "nms kernels"));
    VC_HIP(hipMemcpy(out_n, pb.det_count, (size_t)b * 4, hipMemcpyDeviceToHost));        // the device's count: -1 for a frame whose overflow flag is set
    if (kept_count) VC_HIP(hipMemcpy(kept_count, pb.cand_count, (size_t)b * 4, hipMemcpyDeviceToHost));
    VC_TRY(gdet.read_back(out6, "nms_scan_kernel / det_relabel_kernel"));
    VC_TRY(gidx.read_back(idx.data(), "cand_class_filter_kernel"));
    if (kept_idx) memcpy(kept_idx, idx.data(), mc * 4);
    return VC_OK;
}

}  // namespace

extern "C" {

int vc_nms_batch_host(const float* boxes4, const float* conf, const int* cls, const int* counts, int b, float iou, int max_det, int max_cand,
                      const int* geom4, float* out6, int* out_n) {
    VC_CHECK(boxes4 && conf && cls && counts && out6 && out_n && b >= 1, VC_ERR_ARG, "bad argument");
    VC_CHECK(nms_capacity_ok(max_cand, max_det), VC_ERR_ARG, "max_cand must be a multiple of 64 in [64,8192], max_det >= 1");
    for (int f = 0; f < b; ++f) VC_CHECK(counts[f] >= 0 && counts[f] <= max_cand, VC_ERR_ARG, "frame %d: count %d outside [0, max_cand]", f, counts[f]);
    return nms_candidates(boxes4, conf, cls, counts, b, nullptr, 0, iou, max_det, max_cand, geom4, out6, out_n, nullptr, nullptr);
}

int vc_class_filter_nms_host(const float* boxes4, const float* conf, const int* cls, const int* counts, int b, const int* label_of_class, int n_classes,
                             float iou, int max_det, int max_cand, const int* geom4, float* out6, int* out_n, int* kept_count, int* kept_idx) {
    VC_CHECK(boxes4 && conf && cls && counts && out6 && out_n && kept_count && b >= 1, VC_ERR_ARG, "bad argument");
    VC_TRY(class_map_check(label_of_class, n_classes, nullptr, nullptr));
    VC_CHECK(nms_capacity_ok(max_cand, max_det), VC_ERR_ARG, "max_cand must be a multiple of 64 in [64,8192], max_det >= 1");
    for (int f = 0; f < b; ++f) {
        VC_CHECK(counts[f] >= 0 && counts[f] <= max_cand, VC_ERR_ARG, "frame %d: count %d outside [0, max_cand]", f, counts[f]);
        for (int i = 0; i < counts[f]; ++i) {
            const int c = cls[(size_t)f * max_cand + i];
            VC_CHECK(c >= 0 && c < n_classes, VC_ERR_ARG, "frame %d candidate %d: class %d outside [0, %d)", f, i, c, n_classes);
        }
    }
    return nms_candidates(boxes4, conf, cls, counts, b, label_of_class, n_classes, iou, max_det, max_cand, geom4, out6, out_n, kept_count, kept_idx);
}

// Greedy class-offset NMS on an explicit candidate list (reference order), through the same three kernels the
// detector uses.  Output rows [x1,y1,x2,y2,conf,cls] (network pixels, no rescale).
int vc_nms_host(const float* boxes4, const float* conf, const int* cls, int n, float iou, int max_det, int max_cand, float* out6,
                int* out_n) {
    VC_CHECK(boxes4 && conf && cls && out6 && out_n && n >= 0, VC_ERR_ARG, "bad argument");
    VC_CHECK(nms_capacity_ok(max_cand, max_det) && n <= max_cand, VC_ERR_ARG, "max_cand must be a multiple of 64 in [64,8192] and >= n");
    // one frame of the batched entry: it reads max_cand rows per array, the caller holds n
    std::vector<float> bx((size_t)max_cand * 4, 0.f), cf(max_cand, 0.f), out((size_t)max_det * 6);
    std::vector<int> cl(max_cand, 0);
    std::copy(boxes4, boxes4 + (size_t)n * 4, bx.begin());
    std::copy(conf, conf + n, cf.begin());
    std::copy(cls, cls + n, cl.begin());
    VC_TRY(vc_nms_batch_host(bx.data(), cf.data(), cl.data(), &n, 1, iou, max_det, max_cand, nullptr, out.data(), out_n));
    std::copy(out.begin(), out.begin() + (size_t)std::min(*out_n, max_det) * 6, out6);
    return VC_OK;
}

int vc_decode_host(const vc_decode_desc* d, const float* const* logits, int* cand_count, int* overflow, float* cand_box, float* cand_conf,
                   int* cand_cls, int* cand_idx, int* hc_count, int* const* hc_list, float iou, int max_det, const int* geom4, float* out6,
                   int* out_n) {
    VC_CHECK(d && logits && logits[0] && logits[1] && logits[2] && cand_count && overflow && cand_box && cand_conf && cand_cls && cand_idx, VC_ERR_ARG,
             "null argument");
    VC_CHECK(d->b >= 1 && d->nc >= 1 && d->mode >= 0 && d->mode <= 2 && d->max_cand >= 1, VC_ERR_ARG, "bad decode description");
    VC_CHECK(!hc_count || (d->mode == 2 && hc_list && hc_list[0] && hc_list[1] && hc_list[2]), VC_ERR_ARG, "gathered lists: sparse mode only");
    const bool chain = out6 != nullptr;
    VC_CHECK(!chain || (out_n && nms_capacity_ok(d->max_cand, max_det)), VC_ERR_ARG, "chained nms: max_cand must be a multiple of 64 in [64,8192]");
    const int B = d->b, nc = d->nc, lcs = round_up(3 * (nc + 5), 8), mc = d->max_cand;
    const bool bf16 = d->mode != 0;
    DevScratch mem;
    DetectPostBuffers pb{};
    float* geom = nullptr;
    VC_TRY(post_alloc(mem, pb, &geom, B, mc, chain ? max_det : 0, chain));
    DecodeLevel lv[3];
    int M[3], base = 0;
    void* d_logits[3];
    std::vector<uint8_t> h16[3];                       // the logits as bf16 elements
    for (int i = 0; i < 3; ++i) {
        VC_CHECK(d->ny[i] >= 1 && d->nx[i] >= 1, VC_ERR_ARG, "level %d: %d x %d", i, d->ny[i], d->nx[i]);
        M[i] = B * d->ny[i] * d->nx[i];
        const size_t nel = (size_t)M[i] * lcs;
        if (bf16) h16[i] = to_elems(logits[i], nel, PREC_BF16);
        VC_TRY(mem.upload(&d_logits[i], bf16 ? (const void*)h16[i].data() : logits[i], nel * (bf16 ? 2 : 4)));
        lv[i].logits = d_logits[i]; lv[i].bf16 = bf16 ? 1 : 0; lv[i].ny = d->ny[i]; lv[i].nx = d->nx[i]; lv[i].cs = lcs; lv[i].stride = d->stride[i];
        for (int a = 0; a < 3; ++a) { lv[i].anchor_w[a] = d->anchors[i * 6 + 2 * a]; lv[i].anchor_h[a] = d->anchors[i * 6 + 2 * a + 1]; }
        lv[i].base = base;
        base += 3 * d->ny[i] * d->nx[i];
    }
    int* d_hc_count = nullptr;
    int* d_list[3] = {nullptr, nullptr, nullptr};
    if (d->mode == 2) {
        VC_TRY(mem.alloc(&d_hc_count, 64));
        VC_HIP(hipMemset(d_hc_count, 0, 64));
        for (int i = 0; i < 3; ++i) {
            // the 8-channel objectness plane the engine's ".obj" conv writes: the three anchors' objectness logits, zero padding
            std::vector<uint16_t> obj((size_t)M[i] * 8, 0);
            for (int m = 0; m < M[i]; ++m)
                for (int a = 0; a < 3; ++a) obj[(size_t)m * 8 + a] = ((const uint16_t*)h16[i].data())[(size_t)m * lcs + a * (nc + 5) + 4];
            void *d_obj = nullptr, *d_xc = nullptr;
            VC_TRY(mem.upload(&d_obj, obj.data(), obj.size() * 2));
            VC_TRY(mem.alloc(&d_list[i], (size_t)M[i] * 4));
            VC_TRY(mem.alloc(&d_xc, (size_t)M[i] * lcs * 2));
            const View x{d_logits[i], B, d->ny[i], d->nx[i], lcs, lcs, 0, 2};
            VC_TRY(launch_head_compact(d_obj, x, M[i], d->ny[i] * d->nx[i], d->conf, M[i], d_hc_count + i, d_list[i], d_xc, pb.overflow, nullptr));
            lv[i].logits = d_xc;
        }
        VC_TRY(launch_decode_sparse(lv, d_hc_count, d_list, M, nc, d->conf, mc, pb, nullptr));
    } else {
        VC_TRY(launch_decode(lv, 3, B, nc, d->conf, mc, pb, nullptr, base, nullptr));
    }
    VC_TRY(kernel_wait("decode kernels"));
    const size_t n = (size_t)B * mc;
    VC_HIP(hipMemcpy(cand_count, pb.cand_count, (size_t)B * 4, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(overflow, pb.overflow, (size_t)B * 4, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(cand_box, pb.cand_box, n * 16, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(cand_conf, pb.cand_conf, n * 4, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(cand_cls, pb.cand_cls, n * 4, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(cand_idx, pb.cand_idx, n * 4, hipMemcpyDeviceToHost));
    if (hc_count) {
        VC_HIP(hipMemcpy(hc_count, d_hc_count, 12, hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; ++i) VC_HIP(hipMemcpy(hc_list[i], d_list[i], (size_t)std::min(hc_count[i], M[i]) * 4, hipMemcpyDeviceToHost));
    }
    if (chain) VC_TRY(post_nms(pb, geom, B, mc, max_det, iou, geom4, out6, out_n));
    return VC_OK;
}

}  // extern "C"
