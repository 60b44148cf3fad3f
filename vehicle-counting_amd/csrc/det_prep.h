// Detection hand-over, host side: everything between the detector's output rows and the tracker kernel's input that needs no engine.
// The rows are rounded like the reference's JSON round trip (marshal), the crop rectangles are cut (append_crops_*), the boxes are grouped
// by class (group_by_label), DeepSort.update's own filter runs per class (prepare_dets: confidence test + DeepSORT NMS; prepare_frame for a
// whole frame) and, with embed_kept_only, the kept boxes' crops and feature rows are renumbered (compact_kept).  Plain C++: the library
// includes this header (stream.hip, tracker.hip, engine.hip, host_aux.hip) and tests/native/det_prep_host.cpp compiles it a second time
// for the CPU tests, which hold it to oracle/yolov5.py and oracle/deepsort.py.
//
// Reference: networks/yolo.py:72-97 (marshal), modules/track.py:39-59 (xywh -> xyxy, one DeepSort per class with boxes),
// networks/deepsort/deep_sort.py:31-37,68-95 (filter, tlwh, crop corners), networks/deepsort/sort/preprocessing.py:6-73 (NMS, quirk Q6).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

namespace vc {

struct FrameDets { std::vector<double> xyxy, conf; std::vector<int> label; };      // one frame's boxes as VideoTracker.run sees them
struct Prepared { std::vector<double> tlwh, conf; std::vector<int> feat_rows; };    // filtered + NMS'ed detections of one tracker, pick order
typedef std::vector<std::pair<int, Prepared>> FramePrepared;                         // one frame: (label, detections), labels ascending

// DataFrame.to_json(double_precision=10) -> json.loads (quirk Q9), same rounding as oracle/yolov5.py::marshal_like_reference
inline double round10(double v) { return std::nearbyint(v * 1e10) / 1e10; }

// n detector rows [x1, y1, x2, y2, conf, class] (float32) -> the frame's boxes, xywh -> xyxy round trip included
inline void marshal(const float* det6, int n, FrameDets& out) {
    out.xyxy.clear(); out.conf.clear(); out.label.clear();
    for (int i = 0; i < n; ++i) {
        const float* d = det6 + (size_t)i * 6;
        const double x1 = round10((double)d[0]), y1 = round10((double)d[1]), x2 = round10((double)d[2]), y2 = round10((double)d[3]);
        const double w = x2 - x1, h = y2 - y1;                         // networks/yolo.py:82
        out.xyxy.push_back(x1); out.xyxy.push_back(y1);
        out.xyxy.push_back(w + x1); out.xyxy.push_back(h + y1);        // modules/track.py:39-41
        out.conf.push_back(round10((double)d[4]));
        out.label.push_back((int)d[5]);
    }
}

// deep_sort.py:78-87 _xyxy_to_xywh
inline void xyxy_to_cxcywh(const double* b, double* o) {
    const double w = b[2] - b[0], h = b[3] - b[1];
    o[0] = b[0] + w / 2; o[1] = b[1] + h / 2; o[2] = w; o[3] = h;
}

// deep_sort.py:89-95 _xywh_to_xyxy: int() truncation toward zero, clamp to [0, W-1] / [0, H-1]
inline void crop_corners(const double* b, int W, int H, int out[4]) {
    const double x = b[0], y = b[1], w = b[2], h = b[3];
    out[0] = std::max((int)(x - w / 2), 0);
    out[2] = std::min((int)(x + w / 2), W - 1);
    out[1] = std::max((int)(y - h / 2), 0);
    out[3] = std::min((int)(y + h / 2), H - 1);
}

// The crop list: appends [f, x1, y1, x2, y2] for each of the n boxes of frame f (W x H: that frame's own size) and returns the index of
// the first box whose crop is empty (the reference's cv2.resize raises there), -1 if none is.  All n entries are appended either way.
inline int append_crops(int f, int W, int H, const double* boxes, int n, bool boxes_are_xyxy, std::vector<int>& crops) {
    int first_empty = -1;
    for (int i = 0; i < n; ++i) {
        const double* b = boxes + (size_t)i * 4;
        double c[4];
        if (boxes_are_xyxy) { xyxy_to_cxcywh(b, c); b = c; }
        int q[4];
        crop_corners(b, W, H, q);
        if (first_empty < 0 && !(q[2] > q[0] && q[3] > q[1])) first_empty = i;
        const int e[5] = {f, q[0], q[1], q[2], q[3]};
        crops.insert(crops.end(), e, e + 5);
    }
    return first_empty;
}
inline int append_crops_xyxy(int f, int W, int H, const double* xyxy, int n, std::vector<int>& crops) { return append_crops(f, W, H, xyxy, n, true, crops); }
inline int append_crops_cxcywh(int f, int W, int H, const double* cxcywh, int n, std::vector<int>& crops) { return append_crops(f, W, H, cxcywh, n, false, crops); }

// sort/preprocessing.py:6-73 (overlap = inter / area(other), +1 pixel, '>' threshold; quirk Q6)
inline void dsort_nms(const double* tlwh, const double* scores, int n, double max_overlap, std::vector<int>& keep) {
    keep.clear();
    if (n == 0) return;
    std::vector<double> x1(n), y1(n), x2(n), y2(n), area(n);
    for (int i = 0; i < n; ++i) {
        x1[i] = tlwh[i * 4]; y1[i] = tlwh[i * 4 + 1]; x2[i] = tlwh[i * 4 + 2] + tlwh[i * 4]; y2[i] = tlwh[i * 4 + 3] + tlwh[i * 4 + 1];
        area[i] = (x2[i] - x1[i] + 1) * (y2[i] - y1[i] + 1);
    }
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return scores[a] < scores[b]; });
    while (!idx.empty()) {
        const int i = idx.back();
        idx.pop_back();
        keep.push_back(i);
        std::vector<int> rest;
        for (int j : idx) {
            const double w = std::max(0.0, std::min(x2[i], x2[j]) - std::max(x1[i], x1[j]) + 1);
            const double h = std::max(0.0, std::min(y2[i], y2[j]) - std::max(y1[i], y1[j]) + 1);
            if (!((w * h) / area[j] > max_overlap)) rest.push_back(j);
        }
        idx.swap(rest);
    }
}

// DeepSort.update minus the embedding: confidence filter, tlwh, DeepSORT NMS -> detections in pick order; box i owns feature row rows[i].
// The result depends on the boxes, the confidences and the two parameters alone, never on tracker state, so it can run before the crops
// are cut (embed_kept_only: a box dropped here never becomes a Detection, deep_sort.py:31-37, and its feature row is never read)
inline void prepare_dets(const double* xyxy, const double* conf, const int* rows, int k, double min_confidence, double nms_max_overlap, Prepared& out) {
    std::vector<double> tl, cf;
    std::vector<int> fr;
    for (int i = 0; i < k; ++i) {
        if (!(conf[i] > min_confidence)) continue;                   // deep_sort.py:31 (the reference computed features for all, Q5)
        double c[4];
        xyxy_to_cxcywh(xyxy + (size_t)i * 4, c);                     // _xyxy_to_xywh :78-87
        tl.push_back(c[0] - c[2] / 2.); tl.push_back(c[1] - c[3] / 2.); tl.push_back(c[2]); tl.push_back(c[3]);   // _xywh_to_tlwh :68-75
        cf.push_back(conf[i]);
        fr.push_back(rows[i]);
    }
    std::vector<int> keep;
    dsort_nms(tl.data(), cf.data(), (int)cf.size(), nms_max_overlap, keep);
    out.tlwh.clear(); out.conf.clear(); out.feat_rows.clear();
    for (int i : keep) {
        for (int c = 0; c < 4; ++c) out.tlwh.push_back(tl[(size_t)i * 4 + c]);
        out.conf.push_back(cf[i]);
        out.feat_rows.push_back(fr[i]);
    }
}

// The labels present among n boxes, ascending, each with its box indices in box order: group g has label[g] and the boxes
// order[first[g]] .. order[first[g + 1] - 1].  (modules/track.py:50-59 walks the classes in ascending order and masks the boxes of each.)
struct LabelGroups {
    std::vector<int> order, first, label;
    int size() const { return (int)label.size(); }
};
inline void group_by_label(const int* label, int n, LabelGroups& g) {
    g.order.resize(n);
    std::iota(g.order.begin(), g.order.end(), 0);
    std::stable_sort(g.order.begin(), g.order.end(), [&](int a, int b) { return label[a] < label[b]; });
    g.first.clear(); g.label.clear();
    for (int k = 0; k < n; ++k)
        if (k == 0 || label[g.order[k]] != g.label.back()) { g.first.push_back(k); g.label.push_back(label[g.order[k]]); }
    g.first.push_back(n);
}

// Buffers prepare_frame reuses from frame to frame
struct PrepScratch { LabelGroups groups; std::vector<double> bx, cf; std::vector<int> rows; };

// One frame: for every label that occurs, ascending, the label's boxes go through prepare_dets; box i of the frame owns feature row
// row_base + i.  filter_of(label, min_confidence, nms_max_overlap) supplies the label's two parameters, or returns false to leave the
// label out (a label no tracker exists for).  A label whose boxes are all dropped still yields an entry, with zero detections: its
// tracker is stepped.  A frame without boxes yields nothing.
template <class FilterOf>
inline void prepare_frame(const FrameDets& d, int row_base, FilterOf&& filter_of, PrepScratch& s, FramePrepared& out) {
    out.clear();
    group_by_label(d.label.data(), (int)d.label.size(), s.groups);
    for (int g = 0; g < s.groups.size(); ++g) {
        double min_confidence = 0, nms_max_overlap = 0;
        if (!filter_of(s.groups.label[g], min_confidence, nms_max_overlap)) continue;
        const int* idx = &s.groups.order[s.groups.first[g]];
        const int k = s.groups.first[g + 1] - s.groups.first[g];
        s.bx.resize((size_t)k * 4); s.cf.resize(k); s.rows.resize(k);
        for (int i = 0; i < k; ++i) {
            memcpy(&s.bx[(size_t)i * 4], &d.xyxy[(size_t)idx[i] * 4], 4 * sizeof(double));
            s.cf[i] = d.conf[idx[i]];
            s.rows[i] = row_base + idx[i];
        }
        out.emplace_back(s.groups.label[g], Prepared{});
        prepare_dets(s.bx.data(), s.cf.data(), s.rows.data(), k, min_confidence, nms_max_overlap, out.back().second);
    }
}

// embed_kept_only: `crops` holds one entry per box and the feat_rows of frames[0 .. n_frames) index it.  Keeps the entries some detection
// points at, in their existing order, renumbers every feat_rows entry to the entry's new position and returns the kept count.
inline int compact_kept(std::vector<int>& crops, FramePrepared* frames, int n_frames) {
    std::vector<int> row_of(crops.size() / 5, -1);
    for (int f = 0; f < n_frames; ++f)
        for (const auto& lp : frames[f])
            for (int r : lp.second.feat_rows) row_of[r] = 0;
    int kept = 0;
    for (size_t i = 0; i < row_of.size(); ++i)
        if (row_of[i] == 0) {
            memmove(&crops[(size_t)kept * 5], &crops[i * 5], 5 * sizeof(int));
            row_of[i] = kept++;
        }
    crops.resize((size_t)kept * 5);
    for (int f = 0; f < n_frames; ++f)
        for (auto& lp : frames[f])
            for (int& r : lp.second.feat_rows) r = row_of[r];
    return kept;
}

}  // namespace vc
