// Class filter and label map of the detector -- the `classes` argument of non_max_suppression and the relabel behind it.
//
// Restates:
//   networks/yolo.py:20,64                       get_model hands the keys of args.mapping_dict to YoloBackbone as filter_classes -> model.classes
//   utils/general.py::non_max_suppression        `if classes is not None: x = x[(x[:, 5:6] == classes).any(1)]` -- after the best-class pick and the
//                                                conf test, BEFORE the max_nms trim, the NMS and the max_det cut (oracle/yolov5.py)
//   modules/detect.py:41-46                      ImageDetect.run relabels what is left, after the NMS
// A class map is a table label_of_class[nc]: -1 drops every candidate whose best class is c, l >= 0 is the label its detections leave the
// engine with.  cand_class_filter_kernel removes the dropped candidates between the decode and the sort; the NMS then runs on the ORIGINAL
// class (its class offset keeps two classes apart even when they share a label); det_relabel_kernel rewrites the class column of the rows.
#include <algorithm>
#include <cstring>

#include "engine.h"

namespace vc {

// One 256-thread workgroup per frame compacts the frame's candidates in place, in position order (stable).  A chunk of 256 candidates is
// loaded into registers, ranked (__ballot + __popcll per wave, the four wave totals through LDS) and stored behind the candidates kept so
// far: a destination index is never above its source index, so a store never reaches a candidate that a later chunk has yet to load, and
// the barrier between a chunk's loads and its stores keeps it off the candidates of its own chunk.  overflow[b] is not touched: the frame
// overflowed (or not) on its unfiltered candidate count.
__global__ __launch_bounds__(256) void cand_class_filter_kernel(int nc, int max_cand, const int* __restrict__ label_of, DetectPostBuffers pb) {
    extern __shared__ int s_label[];                   // [nc]
    __shared__ int s_tot[4];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = min(pb.cand_count[b], max_cand);
    for (int c = t; c < nc; c += 256) s_label[c] = label_of[c];
    __syncthreads();
    const size_t base = (size_t)b * max_cand;
    int kept = 0;                                      // candidates kept by the chunks before this one (the same in every thread)
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + t;
        float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
        float conf = 0.f;
        int cls = -1, idx = 0;
        if (i < n) {
            box = *(const float4*)(pb.cand_box + (base + i) * 4);
            conf = pb.cand_conf[base + i];
            idx = pb.cand_idx[base + i];
            cls = pb.cand_cls[base + i];
        }
        const bool keep = cls >= 0 && cls < nc && s_label[cls] >= 0;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_tot[wave] = __popcll(mask);
        // a barrier waits for no memory counter: every load of the chunk has landed in its register before another wave may store
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int before = __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) before += s_tot[w];
        const int total = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
        if (keep) {
            const size_t o = base + kept + before;     // kept + before <= i
            *(float4*)(pb.cand_box + o * 4) = box;
            pb.cand_conf[o] = conf;
            pb.cand_cls[o] = cls;
            pb.cand_idx[o] = idx;
        }
        kept += total;
        __syncthreads();                               // s_tot is written again by the next chunk
    }
    if (t == 0) pb.cand_count[b] = kept;
}

// det[b][k][5] = label of the class nms_scan_kernel wrote there, for the rows the frame's count covers (an overflowed frame, count -1, has none)
__global__ __launch_bounds__(256) void det_relabel_kernel(int nc, int max_det, const int* __restrict__ label_of, DetectPostBuffers pb) {
    const int b = blockIdx.x;
    const int n = min(max(pb.det_count[b], 0), max_det);
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        float* o = pb.det + ((size_t)b * max_det + k) * 6;
        const int c = (int)o[5];
        if (c >= 0 && c < nc) o[5] = (float)label_of[c];
    }
}

int launch_cand_class_filter(int B, int nc, int max_cand, const int* label_of_dev, DetectPostBuffers& pb, hipStream_t s) {
    VC_CHECK(B >= 1 && nc >= 1 && nc <= VC_CLASS_MAP_MAX && label_of_dev, VC_ERR_ARG, "class filter: %d frames, %d classes (at most %d)", B, nc, VC_CLASS_MAP_MAX);
    hipLaunchKernelGGL(cand_class_filter_kernel, dim3(B), dim3(256), sizeof(int) * nc, s, nc, max_cand, label_of_dev, pb);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

int launch_det_relabel(int B, int nc, int max_det, const int* label_of_dev, DetectPostBuffers& pb, hipStream_t s) {
    VC_CHECK(B >= 1 && nc >= 1 && label_of_dev, VC_ERR_ARG, "relabel: %d frames, %d classes", B, nc);
    hipLaunchKernelGGL(det_relabel_kernel, dim3(B), dim3(256), 0, s, nc, max_det, label_of_dev, pb);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// The rules of a class map (pure host code): n entries, each -1 or a label in [0, n), at least one kept.
int class_map_check(const int* label_of_class, int n, int* n_labels, int* n_kept) {
    VC_CHECK(label_of_class && n >= 1 && n <= VC_CLASS_MAP_MAX, VC_ERR_ARG, "class map: null table or %d classes (1 .. %d)", n, VC_CLASS_MAP_MAX);
    int top = -1, kept = 0;
    for (int c = 0; c < n; ++c) {
        const int l = label_of_class[c];
        VC_CHECK(l >= -1 && l < n, VC_ERR_ARG, "class map: class %d has label %d, outside [-1, %d)", c, l, n);
        if (l >= 0) { ++kept; top = std::max(top, l); }
    }
    VC_CHECK(kept > 0, VC_ERR_ARG, "class map: every class is dropped");
    if (n_labels) *n_labels = top + 1;
    if (n_kept) *n_kept = kept;
    return VC_OK;
}

}  // namespace vc

using namespace vc;

extern "C" {

int vc_class_map_check_host(const int* label_of_class, int n, int* n_labels, int* n_kept) {
    return class_map_check(label_of_class, n, n_labels, n_kept);
}

int vc_engine_set_class_map(vc_engine* e, const int* label_of_class, int n) {
    int n_labels = 0;
    if (label_of_class) VC_TRY(class_map_check(label_of_class, n, &n_labels, nullptr));      // the table's own rules need no engine
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    VC_CHECK(!label_of_class || n == e->cfg.num_classes, VC_ERR_ARG, "class map: %d entries, the engine has %d classes", n, e->cfg.num_classes);
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "detector not finalized");
    VC_CHECK(e->pending.empty() && e->jobs.empty(), VC_ERR_STATE,
             "class map: %d submissions and %d batches are outstanding on the stream path: consume them first", (int)e->pending.size(), (int)e->jobs.size());
    if (!label_of_class) { e->class_map.clear(); e->n_labels = 0; return VC_OK; }
    VC_HIP(hipSetDevice(e->cfg.device));
    if (!e->d_class_map) {
        VC_TRY(host_alloc(e, (void**)&e->h_class_map, (size_t)n * sizeof(int)));
        VC_TRY(dev_alloc(e, (void**)&e->d_class_map, (size_t)n * sizeof(int)));
    }
    // no detector pass is in flight (vc_detect blocks, the stream path holds nothing): the table follows whatever the detector stream
    // still has, and the pinned copy is free again when the call returns
    memcpy(e->h_class_map, label_of_class, (size_t)n * sizeof(int));
    VC_HIP(hipMemcpyAsync(e->d_class_map, e->h_class_map, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->dstream));
    VC_HIP(hipStreamSynchronize(e->dstream));
    e->class_map.assign(label_of_class, label_of_class + n);
    e->n_labels = n_labels;
    return VC_OK;
}

int vc_engine_class_map(const vc_engine* e, int* label_of_class, int n, int* n_labels) {
    VC_CHECK(e && label_of_class && n_labels, VC_ERR_ARG, "null argument");
    VC_CHECK(n == e->cfg.num_classes, VC_ERR_ARG, "class map: room for %d entries, the engine has %d classes", n, e->cfg.num_classes);
    if (e->class_map.empty()) {
        for (int c = 0; c < n; ++c) label_of_class[c] = c;
        *n_labels = n;
    } else {
        memcpy(label_of_class, e->class_map.data(), (size_t)n * sizeof(int));
        *n_labels = e->n_labels;
    }
    return VC_OK;
}

}  // extern "C"
