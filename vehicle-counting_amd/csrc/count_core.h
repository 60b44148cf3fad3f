// Arithmetic of the counting stage, written once for the host post-pass (counting.hip: vc_counts / vc_counter_rows / vc_zone_filter_host),
// for the live-count kernels (live_count.hip) and for the host build the CPU tests compile (tests/native/count_core_host.cpp): the zone
// test, the direction assignment, and the per-track state machine that a row advances.  No HIP, no allocation, no library call but sqrt.
//
// Reference (paths relative to /root/reference/):
//   utilities/counting/bb_polygon.py:14-94    orientation / on_segment / is_intersect / is_point_in_polygon (ray to y = 1e9)
//   utilities/counting/bb_polygon.py:96-114   check_bbox_intersect_polygon: ANY box corner inside shapes[0] (Q12)
//   utilities/counting/utils.py:139-152       find_best_match_direction: strict '>' from 0, first key as fall-back (Q11)
//   modules/track.py:100-116                  VideoCounting.run's loop body: first / last box of a track, rows at its last frame
//   utilities/counting/utils.py:276-297       count_frame_directions: count[direction][label] += 1 where lframe == frame_id
//
// Floating-point contraction is off for everything below: the reference evaluates ax*bx + ay*by and the orientation determinant with one
// rounding per operation (NumPy / Python floats), and a fused multiply-add changes the sign of a determinant that is exactly zero in
// that arithmetic (a corner on a polygon edge).  fp64 sqrt and division are correctly rounded on the host and on gfx950 alike.
#pragma once
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define VC_CC_HD __host__ __device__ __forceinline__
#else
#define VC_CC_HD inline
#endif

namespace vc {
namespace cc {

enum { CC_MAX_POINTS = 64, CC_MAX_DIRS = 16 };          // per camera: what a live counter accepts (vc_live_create)

struct P2 { double x, y; };

VC_CC_HD double dmax(double a, double b) { return a > b ? a : b; }     // Python's max(a, b) / min(a, b) on finite values
VC_CC_HD double dmin(double a, double b) { return a < b ? a : b; }

VC_CC_HD int orient(P2 p, P2 q, P2 r) {
    const double v = (q.y - p.y) * (r.x - q.x) - (q.x - p.x) * (r.y - q.y);
    return v == 0 ? 0 : (v > 0 ? 1 : 2);
}
VC_CC_HD bool on_segment(P2 p, P2 q, P2 r) {
    return q.x <= dmax(p.x, r.x) && q.x >= dmin(p.x, r.x) && q.y <= dmax(p.y, r.y) && q.y >= dmin(p.y, r.y);
}
VC_CC_HD bool intersect(P2 p1, P2 q1, P2 p2, P2 q2) {
    const int o1 = orient(p1, q1, p2), o2 = orient(p1, q1, q2), o3 = orient(p2, q2, p1), o4 = orient(p2, q2, q1);
    if (o1 != o2 && o3 != o4) return true;
    if (o1 == 0 && on_segment(p1, p2, q1)) return true;
    if (o2 == 0 && on_segment(p1, q2, q1)) return true;
    if (o3 == 0 && on_segment(p2, p1, q2)) return true;
    return o4 == 0 && on_segment(p2, q1, q2);
}
// polygon_xy: x0, y0, x1, y1, ... (n points)
VC_CC_HD bool point_in_polygon(const double* polygon_xy, int n, P2 pt) {
    const P2 far{pt.x, 1e9};
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const P2 a{polygon_xy[i * 2], polygon_xy[i * 2 + 1]}, b{polygon_xy[j * 2], polygon_xy[j * 2 + 1]};
        if (intersect(a, b, pt, far)) {
            if (orient(a, pt, b) == 0) return on_segment(a, pt, b);
            ++count;
        }
    }
    return count % 2 == 1;
}
// any corner of box = (x1, y1, x2, y2), in the reference's corner order
VC_CC_HD bool box_in_polygon(const double* polygon_xy, int n, const int64_t* box) {
    const double x1 = (double)box[0], y1 = (double)box[1], x2 = (double)box[2], y2 = (double)box[3];
    return point_in_polygon(polygon_xy, n, P2{x1, y1}) || point_in_polygon(polygon_xy, n, P2{x2, y1}) ||
           point_in_polygon(polygon_xy, n, P2{x2, y2}) || point_in_polygon(polygon_xy, n, P2{x1, y2});
}

// index of the direction line (x0, y0, x1, y1 each) with the largest cosine to (ax, ay): strict '>' from 0, direction 0 as fall-back.
// 0/0 -> NaN and x/0 -> +-inf like the reference's NumPy division; NaN never wins.
VC_CC_HD int best_direction_vec(double ax, double ay, const double* dir_lines, int n_dir) {
    double best = 0;
    int bi = 0;
    for (int d = 0; d < n_dir; ++d) {
        const double* p = dir_lines + (size_t)d * 4;
        const double bx = p[2] - p[0], by = p[3] - p[1];
        const double den = sqrt(ax * ax + ay * ay) * sqrt(bx * bx + by * by);
        const double score = (ax * bx + ay * by) / den;
        if (score > best) { best = score; bi = d; }
    }
    return bi;
}
// ... on the centres of a track's first and last box; fpoint / lpoint (optional) receive the centres
VC_CC_HD int best_direction(const double* dir_lines, int n_dir, const int64_t* fbox, const int64_t* lbox, double* fpoint, double* lpoint) {
    const double fx = (double)(fbox[2] + fbox[0]) / 2, fy = (double)(fbox[3] + fbox[1]) / 2;
    const double lx = (double)(lbox[2] + lbox[0]) / 2, ly = (double)(lbox[3] + lbox[1]) / 2;
    if (fpoint) { fpoint[0] = fx; fpoint[1] = fy; }
    if (lpoint) { lpoint[0] = lx; lpoint[1] = ly; }
    return best_direction_vec(lx - fx, ly - fy, dir_lines, n_dir);
}

// ---- live counting: what is kept of a track while it can still produce rows ------------------------------------------------------
// One record per tracker pool slot.  It is vc_counter's Rec without the row history: the counts read only the first in-zone box,
// the last in-zone box and the number of in-zone rows at the track's last frame.
struct LiveSlot {
    int32_t open, cam, label, at_last;
    int64_t last_frame;
    int64_t first[4], last[4];
};                                                          // 88 bytes

// vc_counter_add for one in-zone row of the track in this slot (the caller has applied the zone test)
VC_CC_HD void live_slot_add(LiveSlot& s, int cam, int label, int64_t frame, const int64_t* box) {
    if (!s.open) {
        s.open = 1; s.cam = cam; s.label = label; s.at_last = 1;
        for (int k = 0; k < 4; ++k) s.first[k] = box[k];
    } else {
        s.at_last = frame == s.last_frame ? s.at_last + 1 : 1;
    }
    s.last_frame = frame;
    for (int k = 0; k < 4; ++k) s.last[k] = box[k];
}

}  // namespace cc
}  // namespace vc
