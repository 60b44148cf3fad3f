// Tracker batch planning, host side: everything track_enqueue (tracker.hip) decides about a batch before it touches a buffer -- the
// device order of the (frame, class) tasks, one workgroup plan per tracker, the step capacity, the LDS assignment-matrix size, whether
// all appearance tables fit (lean or general kernel instance), the rows-arena bound and the layouts of the pinned input and output
// blocks.  Plain integer C++ with no HIP in it and no vc_engine.  Users: kernels.h (the device structs and the two constants, for
// track_kernels.hip, live_count.hip and live_overlay.hip), engine.h (TrackStage holds a TrackBatchPlan), tracker.hip (the planner;
// track_collect and vc_tracker_debug_costs read the plan back) and tests/native/track_batch_plan_host.cpp, which compiles this header
// a second time for the CPU tests that hold every bound below to numbers worked out by hand.
//
// The planner needs TC_HARD_CAP and step_work_bytes of track_core.h, which kernels.h must not pull into every translation unit (it is
// compiled with floating-point contraction off, unlike most of kernels.h's users): the planner half of this header is compiled only
// where VC_TRACK_BATCH_PLANNER is defined in front of the first include (tracker.hip, the CPU test).
#pragma once
#include <algorithm>
#include <cstddef>
#include <numeric>
#include <utility>
#include <vector>

#include "../../include/vcount_hip.h"     // vc_frame_dims

namespace vc {

// One tracker step = (tracker, frame): Tracker.predict() + Tracker.update(detections) on the prepared (confidence-filtered,
// DeepSORT-NMS'ed, deep_sort.py:31-41) detections [det_off, det_off + det_n) of the batch's detection arrays.
// frame_w / frame_h: the size this task's boxes are clamped to (a camera of a sized batch); 0 = TrackBatchArgs.frame_w / frame_h.
struct TrackTask { int tracker, det_off, det_n, frame, label, frame_w, frame_h, pad2; };
// workgroup b of the batch kernel owns one tracker and runs its tasks [task_begin, task_end) in order; the tracker's detections of
// the batch are the contiguous range [det_begin, det_begin + det_n) of the detection arrays (frames ascending)
struct TrackWgPlan { int tracker, task_begin, task_end, det_begin, det_n, pad0, pad1, pad2; };
// one (frame, class) step of a batch as the host sees it
struct TrackTaskHost { int tracker, label, frame, det_off, det_n; };

#define VC_TRACK_DYN_LDS_BYTES (96 * 1024)   // dynamic LDS the tracker kernels may ask for: step work arrays (62.5 KB at 512 tracks + detections) + the assignment matrix
#define VC_ROW_CHUNK 128          // rows of the output arena a tracker workgroup reserves at a time

// The kernel reserves rows in chunks: a workgroup whose step emits m rows and that has fewer left abandons the rest of its chunk and
// grabs track_row_grab(m) fresh ones with one atomic add, so the rows it abandons are always fewer than the rows of the step that
// follows -- consumption is bounded by twice the rows emitted plus one unfinished chunk per workgroup (`rows + chunk` was a
// spurious TERR_ROWS for steady steps of 65..127 rows).  constexpr: host and device alike (track_batch_kernel calls the first).
constexpr int track_row_grab(int m) { return m > VC_ROW_CHUNK ? m : VC_ROW_CHUNK; }
constexpr int track_rows_bound(int rows_in, int n_wg) { return 2 * rows_in + n_wg * VC_ROW_CHUNK; }

// ---- the two pinned blocks: byte offsets, every block 16-byte aligned ---------------------------------------------------------------
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// input block (host-filled, mirrored on the device by one copy).  fno, the frames' numbers for the live counters, is present
// (fno < total) only when a live counter is involved.
struct TrackInLayout { size_t tasks, plans, tlwh, xyah, frow, fno, total; };
inline TrackInLayout track_in_layout(int n_tasks, int n_wg, int n_dets, int n_frames, bool live) {
    TrackInLayout o;
    size_t p = 0;
    o.tasks = p; p = align16(p + (size_t)n_tasks * sizeof(TrackTask));
    o.plans = p; p = align16(p + (size_t)n_wg * sizeof(TrackWgPlan));
    o.tlwh = p; p = align16(p + (size_t)n_dets * 32);
    o.xyah = p; p = align16(p + (size_t)n_dets * 32);
    o.frow = p; p = align16(p + (size_t)n_dets * 4);
    o.fno = p;
    if (live) p = align16(p + (size_t)n_frames * sizeof(long long));
    o.total = p;
    return o;
}
// output block (written by the kernel)
struct TrackOutLayout { size_t rows, row_off, row_n, ntracks, tT, status, total; };
inline TrackOutLayout track_out_layout(int n_tasks, int rows_cap) {
    TrackOutLayout o;
    size_t p = 0;
    o.rows = p; p = align16(p + (size_t)rows_cap * 6 * sizeof(long long));
    o.row_off = p; p = align16(p + (size_t)n_tasks * 4);
    o.row_n = p; p = align16(p + (size_t)n_tasks * 4);
    o.ntracks = p; p = align16(p + (size_t)n_tasks * 4);
    o.tT = p; p = align16(p + (size_t)n_tasks * 4);
    o.status = p; p = align16(p + 16);
    o.total = p;
    return o;
}

// A frame belongs to the camera of frame_tracker[f] (a tracker slot); without frame_tracker, to that of its first task; a frame with
// neither has none (-1).  tasks: the batch's frame-major task list.
inline void track_frame_cameras(const std::vector<TrackTaskHost>& tasks, int n_frames, const int* frame_tracker, std::vector<int>& out) {
    out.assign((size_t)n_frames, -1);
    if (frame_tracker) std::copy(frame_tracker, frame_tracker + n_frames, out.begin());
    else for (size_t i = tasks.size(); i-- > 0;) out[(size_t)tasks[i].frame] = tasks[i].tracker;
}

// What the bounds read of one tracker (engine.h: Tracker) and of the engine.
struct TrackSizes { int known_tracks, pending_dets, nn_budget; };
struct TrackPlanLimits { int budget_cap; long long dot_arena_max_floats; int row_src_cap; };

struct TrackBatchPlan {
    std::vector<TrackTaskHost> tasks;                // (frame, class) order = output order; in: the caller's list, out: det_off filled in
    int n_frames = 0;
    std::vector<int> order;                          // the device's task k is tasks[order[k]] ...
    std::vector<int> dev_index;                      // ... and tasks[i] is the device's task dev_index[i]
    std::vector<TrackTask> dev_tasks;                // device order: grouped by tracker, frames ascending inside a group
    std::vector<TrackWgPlan> wg;                     // one per tracker of the batch, trackers ascending; empty = nothing to launch
    std::vector<std::pair<int, int>> tracker_dets;   // per workgroup: (tracker, detections enqueued) for the pending_dets bookkeeping
    std::vector<int> last_task_of;                   // per workgroup: device index of the tracker's last task
    int n_dets = 0;
    int cap = 0;                                     // TrackBatchArgs::cap
    int lmat_doubles = 0;                            // TrackBatchArgs::lmat_doubles
    bool tables_fit = false;                         // TrackBatchArgs::all_tables
    size_t arena_want = 0;                           // floats of appearance-table arena this batch can use
    int rows_cap = 0;                                // rows of the device's output arena
    bool live = false;                               // a live counter is involved: the input block carries the frames' numbers
    TrackInLayout in{};
    TrackOutLayout out{};
    int n_tasks() const { return (int)tasks.size(); }
    int n_wg() const { return (int)wg.size(); }
};

}  // namespace vc

#ifdef VC_TRACK_BATCH_PLANNER
#include "track_core.h"

namespace vc {

// bp.tasks holds the frame-major task list (tracker, label, frame, -, det_n) of n_frames frames; sizes_of(tracker) -> TrackSizes;
// rows_in: the rows the caller's buffers hold; frame_dims: per frame of a sized batch, else null.  Fills every other member of bp.
template <class SizesOf>
inline void plan_track_batch(TrackBatchPlan& bp, int n_frames, SizesOf sizes_of, const TrackPlanLimits& lim, int rows_in, bool live,
                             const vc_frame_dims* frame_dims) {
    const int n_tasks = bp.n_tasks();
    bp.n_frames = n_frames; bp.live = live;
    bp.wg.clear(); bp.tracker_dets.clear(); bp.last_task_of.clear();
    // device order: grouped by tracker, frames ascending inside a group (stable sort of the frame-major list); the detection arrays
    // follow the same order, so every tracker's detections of the batch are one contiguous range
    std::vector<int>& order = bp.order;
    order.resize((size_t)n_tasks);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bp.tasks[a].tracker < bp.tasks[b].tracker; });
    bp.dev_index.assign((size_t)n_tasks, 0);
    for (int k = 0; k < n_tasks; ++k) bp.dev_index[order[k]] = k;
    int need = 8, n_dets = 0;
    long long mat_need = 0;              // entries of the largest assignment problem a step of this batch is likely to pose (tracks x detections)
    // Do the appearance tables of ALL trackers fit the arena for certain?  Bound from what the host knows: the tracks of the last
    // collected batch (known_tracks) hold at most a full gallery each, and every detection of a batch still in flight (pending_dets)
    // adds at most ONE gallery row -- it either extends one track's ring or starts a track with a single sample (tracker.py:82-91,
    // 133-139).  (Round 2 charged a full gallery per pending detection: at 256 detections per frame that bound was 1.3 GB per tracker,
    // nothing "fitted", and the batch ran on the fallback instance.)  Then the lean kernel instance (no fallback code, 8 waves) runs.
    long long table_floats = 0, table_rows = 0;
    bool all_tables = true;
    for (int k = 0; k < n_tasks;) {
        const int tr = bp.tasks[order[k]].tracker;
        int k1 = k, dets = 0, dmax = 0;
        const int det_begin = n_dets;
        while (k1 < n_tasks && bp.tasks[order[k1]].tracker == tr) {
            TrackTaskHost& t = bp.tasks[order[k1]];
            t.det_off = n_dets; n_dets += t.det_n;
            dets += t.det_n; dmax = std::max(dmax, t.det_n);
            ++k1;
        }
        bp.wg.push_back(TrackWgPlan{tr, k, k1, det_begin, dets, 0, 0, 0});
        const TrackSizes tk = sizes_of(tr);
        const long long old_rows = (long long)tk.known_tracks * std::min(lim.budget_cap, tk.nn_budget) + tk.pending_dets;
        const long long need_f = (old_rows + dets) * dets;
        if (need_f >= (1ll << 31)) all_tables = false;
        table_floats += need_f; table_rows += old_rows;
        // LDS capacity from the tracker's recent size (the kernel falls back to global-memory work arrays for a larger step)
        need = std::max(need, 2 * tk.known_tracks + 2 * dmax + 16);
        mat_need = std::max(mat_need, (long long)(tk.known_tracks + 32) * dmax);
        bp.tracker_dets.emplace_back(tr, dets);
        bp.last_task_of.push_back(k1 - 1);
        k = k1;
    }
    bp.n_dets = n_dets;
    bp.dev_tasks.resize((size_t)n_tasks);
    for (int k = 0; k < n_tasks; ++k) {
        const TrackTaskHost& t = bp.tasks[order[k]];
        bp.dev_tasks[k] = TrackTask{t.tracker, t.det_off, t.det_n, t.frame, t.label, frame_dims ? frame_dims[t.frame].w : 0, frame_dims ? frame_dims[t.frame].h : 0, 0};
    }
    // work-array capacity: 32, else the next multiple of 64 (a power of two, as before round 3, doubled the arrays' LDS for a 310-entry
    // step and left no room for the assignment matrix next to them)
    bp.cap = need <= 32 ? 32 : std::min((int)tc::TC_HARD_CAP, (need + 63) / 64 * 64);
    // Dense steps (BASELINE.json configs[2]: ~90 tracks x ~70 detections): the matrix the assignment scans goes into LDS behind the work
    // arrays -- as much as the kernel's dynamic LDS allows; light batches ask for none (their problems fit the 2 KB static buffers, and
    // a small LDS footprint lets conv workgroups share the tracker's CUs).
    bp.lmat_doubles = 0;
    if (mat_need > 256) {
        const long long room = ((long long)VC_TRACK_DYN_LDS_BYTES - (long long)tc::step_work_bytes(bp.cap)) / 8;
        bp.lmat_doubles = (int)std::max(0ll, std::min(room, (mat_need + 63) / 64 * 64));
    }
    // When every tracker's table fits for certain the lean kernel instance runs; otherwise the arena still grows towards the bound
    // (it used to stay at its 16-byte initial size then, and the per-tracker fit check on the device sent EVERY tracker to
    // the in-walk appearance rows although most tables would have fitted) and the general instance serves the trackers whose tables fit.
    bp.tables_fit = all_tables && table_floats <= lim.dot_arena_max_floats && table_rows <= (long long)lim.row_src_cap;
    bp.arena_want = (size_t)std::min<long long>(std::max<long long>(table_floats, 0), lim.dot_arena_max_floats);
    bp.rows_cap = track_rows_bound(rows_in, bp.n_wg());
    bp.in = track_in_layout(n_tasks, bp.n_wg(), n_dets, n_frames, live);
    bp.out = track_out_layout(n_tasks, bp.rows_cap);
}

}  // namespace vc
#endif  // VC_TRACK_BATCH_PLANNER
