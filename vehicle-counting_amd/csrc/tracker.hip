// DeepSORT tracker, host side: the tracker state is device-resident and every step runs inside track_batch_kernel
// (track_kernels.hip); the host only prepares a batch's detections -- confidence filter and DeepSORT NMS, which do not depend
// on tracker state (det_prep.h) -- packs them with the (frame, class) task list into one host-to-device copy, launches ONE kernel
// per batch and reads the rows the kernel wrote into pinned memory.  One tracker per (camera, class) like the reference
// (modules/track.py:16).  (The single-function entry points -- vc_kalman_*_host, vc_iou_cost_host, vc_cosine_cost_host, vc_lap_host --
// are host_track.hip.)
//
// What a batch needs is decided without the engine by plan_track_batch (track_batch_plan.h: device order, workgroup plans, step capacity,
// assignment-matrix LDS, table fit, arena sizes, block layouts; held to hand-computed numbers by tests/test_track_batch_plan_host.py).
// track_enqueue is the sequence around it -- tasks, plan, overlay begin, reserve buffers, fill the input block, number the frames, upload,
// launch, overlay build, event -- one static function per step above it; TrackStage keeps the plan for track_collect.
//
// Reference (paths relative to /root/reference/networks/deepsort/):
//   deep_sort.py:25-59            DeepSort.update (confidence filter :31, tlwh :68-87, NMS :37-41 -> det_prep.h; predict/update :44-45, rows :46-58)
//   sort/preprocessing.py:6-73    non_max_suppression (quirk Q6)                      -> det_prep.h: dsort_nms (host: state-independent)
//   sort/tracker.py, sort/track.py, sort/linear_assignment.py, sort/nn_matching.py, sort/kalman_filter.py, sort/iou_matching.py
//                                 -> track_core.h + track_kernels.hip (device)
//   modules/track.py:30-70        VideoTracker.run (one DeepSORT per class, classes without boxes are not stepped)
#include <algorithm>
#include <cstring>
#include <cmath>
#include <numeric>
#include <climits>
#include <cstdint>
#include <cstdlib>

#define VC_TRACK_BATCH_PLANNER    // track_batch_plan.h, reached through engine.h: with plan_track_batch, which brings track_core.h in
#include "engine.h"
#include "track_core.h"

namespace vc {

using namespace tc;

// ------------------------------------------------------------------------------------------------ pool
int tracker_init_pool(vc_engine* e) {
    const size_t T = e->cfg.max_tracks, S = e->cfg.nn_budget_cap;
    VC_CHECK(T >= 1 && S >= 1, VC_ERR_ARG, "max_tracks and nn_budget_cap must be positive");
    e->max_trackers = e->cfg.max_trackers > 0 ? e->cfg.max_trackers : 256;
    VC_CHECK(e->max_trackers <= 65535, VC_ERR_ARG, "max_trackers %d: a tracker handle addresses at most 65535 slots", e->max_trackers);
    e->list_cap = e->cfg.tracks_per_tracker > 0 ? e->cfg.tracks_per_tracker : 512;
    e->list_cap = (int)std::min<size_t>((size_t)e->list_cap, T);
    e->pool.max_tracks = (int)T; e->pool.budget_cap = (int)S;
    VC_TRY(dev_alloc(e, (void**)&e->pool.mean, T * 8 * sizeof(double)));
    VC_TRY(dev_alloc(e, (void**)&e->pool.cov, T * 64 * sizeof(double)));
    VC_TRY(dev_alloc(e, (void**)&e->pool.gallery, T * S * VC_FEAT_DIM * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&e->d_hdrs, (size_t)e->max_trackers * sizeof(TrackerHdr)));
    VC_TRY(dev_alloc(e, (void**)&e->d_lists, (size_t)e->max_trackers * e->list_cap * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&e->d_recs, T * sizeof(TrackRecD)));
    VC_TRY(dev_alloc(e, (void**)&e->d_free, 64));
    VC_TRY(dev_alloc(e, (void**)&e->d_free_stack, T * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&e->d_freed, T * sizeof(int)));
    VC_HIP(hipMemset(e->d_hdrs, 0, (size_t)e->max_trackers * sizeof(TrackerHdr)));
    std::vector<int> st(T);
    for (size_t i = 0; i < T; ++i) st[i] = (int)(T - 1 - i);
    VC_HIP(hipMemcpy(e->d_free_stack, st.data(), T * sizeof(int), hipMemcpyHostToDevice));
    const int ctl[2] = {(int)T, 0};
    VC_HIP(hipMemcpy(e->d_free, ctl, sizeof(ctl), hipMemcpyHostToDevice));
    // hoisted appearance dots (track_kernels.hip): table arena (grown on demand by track_enqueue, up to VC_DOT_ARENA_MB /
    // vc_engine_set_option "dot_arena_mb": 1 GB by default; 0 forces the in-walk appearance rows), row bookkeeping
    e->dot_arena_max_floats = getenv("VC_DOT_ARENA_MB") ? (size_t)atol(getenv("VC_DOT_ARENA_MB")) * 262144 : (size_t)256 << 20;
    e->dot_arena_floats = 0;
    VC_TRY(dev_alloc(e, (void**)&e->d_dot_arena, 16));
    e->row_src_cap = (int)std::min<size_t>(T * S, (size_t)1 << 24);
    VC_TRY(dev_alloc(e, (void**)&e->d_row_src, (size_t)e->row_src_cap * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&e->d_gal_row, T * S * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&e->d_dot_ctl, 64));
    e->det_cap = std::max(e->cfg.max_det * 2, 1024);
    VC_TRY(dev_alloc(e, (void**)&e->d_feat_in, (size_t)e->det_cap * VC_FEAT_DIM * sizeof(float)));
    for (TrackStage& s : e->tstage) {
        VC_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        VC_TRY(dev_alloc(e, (void**)&s.d_cursor, 64));
    }
    return VC_OK;
}

// (re)size a staging block; old blocks stay on the engine's free-at-destroy lists (sizes grow geometrically)
static int stage_reserve(vc_engine* e, TrackStage& s, size_t in_bytes, size_t out_bytes) {
    if (in_bytes > s.in_cap) {
        const size_t cap = std::max(in_bytes * 3 / 2, (size_t)1 << 16);
        VC_TRY(host_alloc(e, (void**)&s.h_in, cap));
        VC_TRY(dev_alloc(e, (void**)&s.d_in, cap));
        s.in_cap = cap;
    }
    if (out_bytes > s.out_cap) {
        const size_t cap = std::max(out_bytes * 3 / 2, (size_t)1 << 16);
        VC_TRY(host_alloc(e, (void**)&s.h_out, cap));
        VC_HIP(hipHostGetDevicePointer((void**)&s.hd_out, s.h_out, 0));
        s.out_cap = cap;
    }
    return VC_OK;
}

int track_idle(vc_engine* e) {
    for (TrackStage& s : e->tstage)
        if (s.busy) VC_HIP(hipEventSynchronize(s.done));
    return VC_OK;
}

// ------------------------------------------------------------------------------------------------ track_enqueue, step by step
// the tasks in (frame, class) order -- the order rows are handed back in -- and the detections each one brings
static int batch_tasks(vc_engine* e, const std::vector<std::vector<FrameClassDets>>& frames, std::vector<TrackTaskHost>& tasks,
                       std::vector<const FrameClassDets*>& src) {
    tasks.clear();
    for (size_t f = 0; f < frames.size(); ++f)
        for (const FrameClassDets& g : frames[f]) {
            VC_CHECK(tracker_ok(e->trackers, g.tracker), VC_ERR_NOTFOUND, "bad tracker id %d", g.tracker);
            tasks.push_back(TrackTaskHost{g.tracker, g.label, (int)f, 0, (int)g.dets.conf.size()});
            src.push_back(&g);
        }
    return VC_OK;
}

// live counters (live_count.hip): does one own a tracker of this batch, or the camera of one of its frames?  Then the batch carries its
// frames' numbers, and the kernel writes the slot behind every row
static bool batch_is_live(const vc_engine* e, const std::vector<TrackTaskHost>& tasks, int b, const int* frame_tracker) {
    bool live = false;
    if (e->lives.empty()) return live;
    for (const TrackTaskHost& t : tasks) live = live || e->trackers[t.tracker]->live != nullptr;
    if (frame_tracker) for (int f = 0; f < b; ++f) live = live || (tracker_ok(e->trackers, frame_tracker[f]) && e->trackers[frame_tracker[f]]->live);
    return live;
}

// every buffer the planned batch needs, grown before anything is written or enqueued
static int reserve_buffers(vc_engine* e, TrackStage& s) {
    const TrackBatchPlan& bp = s.plan;
    const size_t n_wg = (size_t)bp.n_wg(), n_dets = (size_t)bp.n_dets;
    VC_TRY(stage_reserve(e, s, bp.in.total, bp.out.total));
    if (bp.live && (size_t)bp.rows_cap > s.row_slot_cap) {      // like the staging blocks: the old one stays allocated, a batch in flight may use it
        s.row_slot_cap = (size_t)bp.rows_cap * 3 / 2;
        VC_TRY(dev_alloc(e, (void**)&s.d_row_slot, s.row_slot_cap * sizeof(int)));
    }
    // buffers of the hoisted appearance dots (engine-wide: the tracker stream runs one batch at a time)
    if (n_wg > e->dot_plans_cap || n_dets > e->nfeat_cap) {
        VC_TRY(track_idle(e));
        VC_HIP(hipStreamSynchronize(e->stream));
        if (n_wg > e->dot_plans_cap) { e->dot_plans_cap = n_wg * 2; VC_TRY(dev_alloc(e, (void**)&e->d_dot_plans, e->dot_plans_cap * sizeof(TrackDotPlan))); }
        if (n_dets > e->nfeat_cap) {
            e->nfeat_cap = n_dets * 3 / 2 + 64;
            VC_TRY(dev_alloc(e, (void**)&e->d_nfeat, e->nfeat_cap * VC_FEAT_DIM * sizeof(float)));
            VC_TRY(dev_alloc(e, (void**)&e->d_det_ss, e->nfeat_cap * sizeof(float)));
        }
    }
    const size_t scratch = n_wg * track_scratch_per_wg();
    if (scratch > e->track_scratch_bytes) {
        VC_TRY(track_idle(e));                                                // the old block may still be in use
        const size_t bytes = scratch * 3 / 2;
        VC_TRY(dev_alloc(e, (void**)&e->d_track_scratch, bytes));
        e->track_scratch_bytes = bytes;
    }
    // appearance-table arena: grown to what this batch can use (plan_track_batch: bounded by dot_arena_max_floats, also when not every table fits)
    if (bp.arena_want > e->dot_arena_floats) {
        VC_TRY(track_idle(e));
        VC_HIP(hipStreamSynchronize(e->stream));
        const size_t want = std::min(e->dot_arena_max_floats, std::max(bp.arena_want * 3 / 2, (size_t)1 << 22));
        VC_TRY(dev_realloc(e, (void**)&e->d_dot_arena, want * sizeof(float)));
        e->dot_arena_floats = want;
    }
    return VC_OK;
}

// tasks, plans and the detections (tlwh, xyah, feature row) in device order; the frame numbers are number_frames'
static void fill_input_block(TrackStage& s, const std::vector<const FrameClassDets*>& src) {
    const TrackBatchPlan& bp = s.plan;
    memcpy(s.h_in + bp.in.tasks, bp.dev_tasks.data(), bp.dev_tasks.size() * sizeof(TrackTask));
    memcpy(s.h_in + bp.in.plans, bp.wg.data(), bp.wg.size() * sizeof(TrackWgPlan));
    double* tl = (double*)(s.h_in + bp.in.tlwh);
    double* xy = (double*)(s.h_in + bp.in.xyah);
    int* fr = (int*)(s.h_in + bp.in.frow);
    for (int i : bp.order) {
        const Prepared& d = src[i]->dets;
        int g = bp.tasks[i].det_off;
        for (size_t k = 0; k < d.conf.size(); ++k, ++g) {
            const double* t = &d.tlwh[k * 4];
            memcpy(tl + (size_t)g * 4, t, 32);
            double* o = xy + (size_t)g * 4;                               // sort/detection.py:42-50 to_xyah
            o[0] = t[0] + t[2] / 2; o[1] = t[1] + t[3] / 2; o[2] = t[2] / t[3]; o[3] = t[3];
            fr[g] = d.feat_rows[k];
        }
    }
}

// a frame takes the next number of its camera (track_frame_cameras), 1-based and continuing across batches (modules/datasets.py:61);
// a frame of a camera without a counter gets 0, no row of it is read
static void number_frames(vc_engine* e, const std::vector<int>& frame_trk, long long* fno) {
    for (size_t f = 0; f < frame_trk.size(); ++f) fno[f] = live_next_frame(e, frame_trk[f]);
}

// the input block to the device, and the cursors of the launch cleared behind it
static int upload_inputs(vc_engine* e, TrackStage& s, hipEvent_t wait) {
    hipStream_t ts = e->stream;
    if (wait) VC_HIP(hipStreamWaitEvent(ts, wait, 0));
    VC_HIP(hipMemcpyAsync(s.d_in, s.h_in, s.plan.in.total, hipMemcpyHostToDevice, ts));
    VC_HIP(hipMemsetAsync(s.d_cursor, 0, 64, ts));           // [0] row cursor, [4..6] status
    VC_HIP(hipMemsetAsync(e->d_dot_ctl, 0, 64, ts));
    VC_HIP(hipMemsetAsync(e->d_dot_plans, 0, (size_t)s.plan.n_wg() * sizeof(TrackDotPlan), ts));
    return VC_OK;
}

static TrackBatchArgs batch_args(vc_engine* e, const TrackStage& s, int st, const float* d_feat, int W, int H) {
    const TrackBatchPlan& bp = s.plan;
    TrackBatchArgs a{};
    a.pool = e->pool;
    a.hdrs = e->d_hdrs; a.lists = e->d_lists; a.list_cap = e->list_cap; a.recs = e->d_recs;
    a.free_top = e->d_free; a.freed_count = e->d_free + 1; a.free_stack = e->d_free_stack; a.freed = e->d_freed;
    a.plans = (const TrackWgPlan*)(s.d_in + bp.in.plans); a.tasks = (const TrackTask*)(s.d_in + bp.in.tasks);
    a.det_tlwh = (const double*)(s.d_in + bp.in.tlwh); a.det_xyah = (const double*)(s.d_in + bp.in.xyah); a.det_featrow = (const int*)(s.d_in + bp.in.frow);
    a.feat = d_feat;
    // what the plan kernel may hand out: the block that is allocated, and no more than the option allows NOW -- a "dot_arena_mb" lowered on
    // an engine whose arena had already grown used to bound the host's plan only, and the device went on fitting tables into the old block
    a.dot_plans = e->d_dot_plans; a.dot_arena = e->d_dot_arena; a.dot_arena_floats = (long long)std::min(e->dot_arena_floats, e->dot_arena_max_floats);
    a.row_src = e->d_row_src; a.row_src_cap = e->row_src_cap; a.gal_row = e->d_gal_row; a.nfeat = e->d_nfeat; a.det_ss = e->d_det_ss;
    a.dot_ctl = e->d_dot_ctl; a.n_det_total = bp.n_dets;
    a.rows = (long long*)(s.hd_out + bp.out.rows); a.rows_cap = bp.rows_cap; a.row_cursor = s.d_cursor;
    a.task_row_off = (int*)(s.hd_out + bp.out.row_off); a.task_row_n = (int*)(s.hd_out + bp.out.row_n);
    a.task_ntracks = (int*)(s.hd_out + bp.out.ntracks); a.task_T = (int*)(s.hd_out + bp.out.tT);
    a.status = s.d_cursor + 4;                               // device memory (atomics), copied next to the rows behind the launch
    a.scratch = e->d_track_scratch; a.scratch_per_wg = track_scratch_per_wg(); a.cap = bp.cap; a.frame_w = W; a.frame_h = H;
    a.all_tables = bp.tables_fit ? 1 : 0;
    a.row_slot = bp.live ? s.d_row_slot : nullptr;
    a.lmat_doubles = bp.lmat_doubles;
    static const bool no_reg = getenv("VC_TRACK_NO_REG") != nullptr;
    a.no_reg = no_reg ? 1 : 0;
    // a blocking single step of one tracker: vc_tracker_debug_costs may read the rows back, so they go to the scratch whatever their
    // size.  Every other blocking launch (several classes, or vc_videotracker_run_features' run of frames) chooses per step like the
    // stream path does, which is what lets the tests walk a tracker across that switch inside one launch.
    a.dbg_costs = st == 3 && bp.n_tasks() == 1 && bp.n_wg() == 1 ? 1 : 0;
    return a;
}

// diagnostics (VC_TRACK_DBG): phase times of every task, printed per batch.  dbg_begin: the kernel's timestamp buffer, null when off
static long long* dbg_begin(int n_tasks, hipStream_t ts) {
    static const bool dbg_on = getenv("VC_TRACK_DBG") != nullptr;
    long long* dbg = nullptr;
    if (dbg_on && hipMalloc((void**)&dbg, (size_t)n_tasks * 128) == hipSuccess) hipMemsetAsync(dbg, 0, (size_t)n_tasks * 128, ts);
    return dbg;
}

static void dbg_report(long long* dbg, const TrackBatchPlan& bp, hipStream_t ts) {
    const int n_tasks = bp.n_tasks();
    std::vector<long long> h((size_t)n_tasks * 16);
    hipStreamSynchronize(ts);
    hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost);
    hipFree(dbg);
    double acc[5] = {0, 0, 0, 0, 0}, sumT = 0, sumD = 0;
    int maxwg = 0;
    for (const TrackWgPlan& pl : bp.wg) maxwg = std::max(maxwg, pl.task_end - pl.task_begin);
    for (int k = 0; k < n_tasks; ++k) {
        for (int i = 0; i < 5; ++i) acc[i] += (double)(h[(size_t)k * 16 + i + 1] - h[(size_t)k * 16 + i]) / 100.0;
        sumT += (double)h[(size_t)k * 16 + 6]; sumD += (double)h[(size_t)k * 16 + 7];
    }
    fprintf(stderr, "[vc track dbg] %d tasks in %d workgroups (longest %d tasks), LDS cap %d; us per task: predict %.1f cost %.1f match %.1f apply %.1f finish %.1f; mean T %.1f D %.1f\n",
            n_tasks, bp.n_wg(), maxwg, bp.cap, acc[0] / n_tasks, acc[1] / n_tasks, acc[2] / n_tasks, acc[3] / n_tasks, acc[4] / n_tasks, sumT / n_tasks, sumD / n_tasks);
    long long t_lo = INT64_MAX, t_hi = 0;
    double worst = 0; const TrackWgPlan* wp = nullptr;
    for (const TrackWgPlan& pl : bp.wg) {
        const long long b0 = h[(size_t)pl.task_begin * 16], b1 = h[(size_t)(pl.task_end - 1) * 16 + 5];
        t_lo = std::min(t_lo, b0); t_hi = std::max(t_hi, b1);
        if ((double)(b1 - b0) > worst) { worst = (double)(b1 - b0); wp = &pl; }
    }
    if (!wp) return;
    double a2[5] = {0, 0, 0, 0, 0}, sT = 0, sD = 0, gaps = 0, mp[3] = {0, 0, 0};
    const int nt = wp->task_end - wp->task_begin;
    for (int k = wp->task_begin; k < wp->task_end; ++k) {
        for (int i = 0; i < 5; ++i) a2[i] += (double)(h[(size_t)k * 16 + i + 1] - h[(size_t)k * 16 + i]) / 100.0;
        for (int i = 0; i < 3; ++i) mp[i] += (double)(h[(size_t)k * 16 + 9 + i] - h[(size_t)k * 16 + 8 + i]) / 100.0;
        sT += (double)h[(size_t)k * 16 + 6]; sD += (double)h[(size_t)k * 16 + 7];
        if (k > wp->task_begin) gaps += (double)(h[(size_t)k * 16] - h[(size_t)(k - 1) * 16 + 5]) / 100.0;
    }
    fprintf(stderr, "[vc track dbg]   match split of that workgroup, us per task: setup %.1f cascade %.1f iou stage %.1f\n", mp[0] / nt, mp[1] / nt, mp[2] / nt);
    fprintf(stderr, "[vc track dbg]   kernel span %.0f us; slowest workgroup (tracker %d): %d tasks, %.0f us, per task predict %.1f cost %.1f match %.1f apply %.1f finish %.1f gap %.1f; mean T %.1f D %.1f\n",
            (double)(t_hi - t_lo) / 100.0, wp->tracker, nt, worst / 100.0, a2[0] / nt, a2[1] / nt, a2[2] / nt, a2[3] / nt, a2[4] / nt, gaps / nt, sT / nt, sD / nt);
}

// Overlay lists (live_overlay.hip) for the counters live_overlay_begin found: behind the apply launch and in front of s.done -- the build
// reads this stage's tasks and rows, which the stage's next batch overwrites.  a: null for a batch without a task (anno, text and frame
// number only).  A launch of its own in the profile: a counter without the overlay shows none.
static int overlay_build(vc_engine* e, std::vector<LiveOverlayPlan>& ov, const TrackStage& s, const long long* fno, const TrackBatchArgs* a, int H, int W) {
    if (ov.empty()) return VC_OK;
    ProfScope ps(e, VC_PROF_TRACK);
    return live_overlay_finish(e, ov, s.frame_trk, fno, a, s.plan.n_tasks(), s.plan.n_frames, H, W, e->stream);
}

int track_enqueue(vc_engine* e, int st, const std::vector<std::vector<FrameClassDets>>& frames, const float* d_feat, int W, int H,
                  int rows_cap, hipEvent_t wait, const vc_frame_dims* frame_dims, const int* frame_tracker) {
    TrackStage& s = e->tstage[st];
    VC_CHECK(!s.busy, VC_ERR_STATE, "tracker staging slot %d is still in flight", st);
    TrackBatchPlan& bp = s.plan;
    const int b = (int)frames.size();
    hipStream_t ts = e->stream;
    std::vector<const FrameClassDets*> src;
    VC_TRY(batch_tasks(e, frames, bp.tasks, src));
    plan_track_batch(bp, b, [&](int tr) { const Tracker& tk = *e->trackers[tr]; return TrackSizes{tk.known_tracks, tk.pending_dets, tk.p.nn_budget}; },
                     TrackPlanLimits{e->pool.budget_cap, (long long)e->dot_arena_max_floats, e->row_src_cap}, rows_cap,
                     batch_is_live(e, bp.tasks, b, frame_tracker), frame_dims);
    // The counters of this batch's cameras whose overlay is enabled -- none unless vc_live_overlay_enable has run, and then the launch
    // below is exactly what it was.  Lists are built for uniform batches only.
    std::vector<LiveOverlayPlan> ov;
    s.frame_trk.clear();
    if (!e->lives.empty()) track_frame_cameras(bp.tasks, b, frame_tracker, s.frame_trk);
    if (!frame_dims && !e->lives.empty()) VC_TRY(live_overlay_begin(e, s.frame_trk, ts, ov));
    if (bp.wg.empty()) {                                     // nothing to step; the frames still count for their cameras' live counters
        std::vector<long long> fno((size_t)b, 0);
        if (bp.live) number_frames(e, s.frame_trk, fno.data());
        VC_TRY(overlay_build(e, ov, s, fno.data(), nullptr, H, W));
        s.busy = true; VC_HIP(hipEventRecord(s.done, ts)); return VC_OK;
    }
    VC_TRY(reserve_buffers(e, s));
    fill_input_block(s, src);
    long long* fno = (long long*)(s.h_in + bp.in.fno);
    std::vector<LiveCountArgs> live_args;
    if (bp.live) {
        number_frames(e, s.frame_trk, fno);
        std::vector<int> used;
        for (const TrackWgPlan& pl : bp.wg) used.push_back(pl.tracker);
        live_batch_args(e, used, (const long long*)(s.d_in + bp.in.fno), live_args);
    }
    for (auto& td : bp.tracker_dets) e->trackers[td.first]->pending_dets += td.second;
    VC_TRY(upload_inputs(e, s, wait));
    TrackBatchArgs a = batch_args(e, s, st, d_feat, W, H);
    a.dbg = dbg_begin(bp.n_tasks(), ts);
    {
        ProfScope ps(e, VC_PROF_TRACK);
        VC_TRY(launch_track_batch(a, bp.n_wg(), ts, live_args.data(), (int)live_args.size()));
    }
    VC_TRY(overlay_build(e, ov, s, fno, &a, H, W));
    if (a.dbg) dbg_report(a.dbg, bp, ts);
    VC_HIP(hipMemcpyAsync(s.h_out + bp.out.status, s.d_cursor + 4, 16, hipMemcpyDeviceToHost, ts));
    VC_HIP(hipEventRecord(s.done, ts));
    s.busy = true;
    return VC_OK;
}

int track_collect(vc_engine* e, int st, int64_t* out_rows6, int cap_rows_per_frame, int* out_m) {
    TrackStage& s = e->tstage[st];
    VC_CHECK(s.busy, VC_ERR_STATE, "no tracker batch in staging slot %d", st);
    VC_HIP(hipEventSynchronize(s.done));
    s.busy = false;
    const TrackBatchPlan& bp = s.plan;
    const TrackOutLayout& ol = bp.out;
    for (int f = 0; f < bp.n_frames; ++f) out_m[f] = 0;
    if (bp.n_tasks() == 0) return VC_OK;
    const int* row_off = (const int*)(s.h_out + ol.row_off);
    const int* row_n = (const int*)(s.h_out + ol.row_n);
    const int* ntr = (const int*)(s.h_out + ol.ntracks);
    const int* status = (const int*)(s.h_out + ol.status);
    const long long* rows = (const long long*)(s.h_out + ol.rows);
    for (size_t i = 0; i < bp.tracker_dets.size(); ++i) {                       // size bounds for the next batches
        Tracker& tk = *e->trackers[bp.tracker_dets[i].first];
        tk.pending_dets -= bp.tracker_dets[i].second;
        tk.known_tracks = ntr[bp.last_task_of[i]];
    }
    if (status[0] != TERR_NONE) {
        const char* what = status[0] == TERR_TRACK_CAP ? "live tracks + detections exceed the per-tracker capacity (vc_engine_config.tracks_per_tracker)"
                         : status[0] == TERR_POOL     ? "track pool exhausted (vc_engine_config.max_tracks)"
                         : status[0] == TERR_ROWS     ? "more output rows than the caller's buffers hold (cap_rows)"
                         : status[0] == TERR_TABLE    ? "appearance table missing although the host's bound said it fits (internal)"
                                                      : "infeasible assignment problem";
        set_error("tracker %d: %s; the tracker is stopped until vc_tracker_reset", status[1], what);
        return VC_ERR_CAPACITY;
    }
    for (int i = 0; i < bp.n_tasks(); ++i) {                                    // (frame, class) order
        const int k = bp.dev_index[i], f = bp.tasks[i].frame, m = row_n[k];
        VC_CHECK(out_m[f] + m <= cap_rows_per_frame, VC_ERR_CAPACITY, "frame %d needs room for %d rows", f, out_m[f] + m);
        memcpy(out_rows6 + ((size_t)f * cap_rows_per_frame + out_m[f]) * 6, rows + (size_t)row_off[k] * 6, (size_t)m * 6 * sizeof(int64_t));
        out_m[f] += m;
    }
    return VC_OK;
}

// DeepSort.update's filter for a frame whose trackers are known: every class of [0, num_classes) that has boxes, under the parameters
// of its own tracker (handle trackers[c]); box i of the frame owns feature row row_base + i.  Boxes of other labels are ignored like
// the reference's mask loop ignores them.  A class with a bad handle is prepared too (under zeros): frame_tasks refuses it.
void prepare_for_trackers(vc_engine* e, const int* trackers, int num_classes, const FrameDets& d, int row_base, PrepScratch& scratch, FramePrepared& out) {
    prepare_frame(d, row_base, [&](int c, double& min_confidence, double& nms_max_overlap) {
        if (c < 0 || c >= num_classes) return false;
        const int ts = tracker_slot(e->trackers, trackers[c]);
        if (ts >= 0) { min_confidence = e->trackers[ts]->p.min_confidence; nms_max_overlap = e->trackers[ts]->p.nms_max_overlap; }
        return true;
    }, scratch, out);
}

// A prepared frame -> its tracker tasks, appended in class order (modules/track.py:50-59: a class without boxes is not stepped; one whose
// boxes were all dropped is, with zero detections).  A frame prepared at look-ahead time (stream.hip::issue_reid) holds every label that
// occurred: those outside [0, num_classes) are skipped.  The detections are moved out of `prep`.
int frame_tasks(vc_engine* e, const int* trackers, int num_classes, FramePrepared& prep, std::vector<FrameClassDets>& out) {
    for (auto& lp : prep) {
        const int c = lp.first;
        if (c < 0 || c >= num_classes) continue;
        const int ts = tracker_slot(e->trackers, trackers[c]);
        VC_CHECK(ts >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle %d for class %d", trackers[c], c);
        out.push_back(FrameClassDets{c, ts, std::move(lp.second)});
    }
    return VC_OK;
}

// Shared by vc_deepsort_update / vc_videotracker_run: one frame already on the device, blocking.  Every label of `d` lies in
// [0, num_classes); the boxes of class c go to the tracker with handle trackers[c].  Output rows [x1,y1,x2,y2,id,label].
// The trackers are known here, so DeepSort.update's own filter (prepare_dets: deep_sort.py:31-37) runs BEFORE the crops are uploaded and,
// with the engine option embed_kept_only, only the boxes it keeps are embedded: a dropped box never becomes a Detection, so the
// feature row the reference computes for it (Q5) is never read.  The capacity and empty-crop checks still cover every box.
int frame_track(vc_engine* e, const uint8_t* d_frame_base, int frame_index, int H, int W, const int* trackers, int num_classes, const FrameDets& d,
                std::vector<int64_t>& rows6) {
    const int n = (int)d.conf.size();
    VC_CHECK(n <= e->cfg.max_crops, VC_ERR_CAPACITY, "%d crops exceed max_crops %d", n, e->cfg.max_crops);
    std::vector<int> crops;
    const int empty = append_crops_xyxy(frame_index, W, H, d.xyxy.data(), n, crops);         // deep_sort.py:78-95
    VC_CHECK(empty < 0, VC_ERR_ARG, "box %d gives an empty crop (the reference's cv2.resize raises here)", empty);
    PrepScratch scratch;
    FramePrepared prep;
    prepare_for_trackers(e, trackers, num_classes, d, 0, scratch, prep);
    const int k = e->opt.embed_kept_only ? compact_kept(crops, &prep, 1) : n;                // kept boxes get consecutive feature rows, in box order
    std::vector<std::vector<FrameClassDets>> frames(1);
    VC_TRY(frame_tasks(e, trackers, num_classes, prep, frames[0]));
    int total_tracks = 0;
    for (const FrameClassDets& fc : frames[0]) total_tracks += e->trackers[fc.tracker]->known_tracks + (int)fc.dets.conf.size();
    e->boxes_detected += n; e->crops_embedded += k;
    if (k > 0) {
        memcpy(e->h_crops, crops.data(), (size_t)k * 5 * sizeof(int));
        VC_HIP(hipMemcpyAsync(e->d_crops, e->h_crops, (size_t)k * 5 * sizeof(int), hipMemcpyHostToDevice, e->stream));
        VC_TRY(run_reid_dev(e, d_frame_base, H, W, k));
    }
    const int cap = std::max(total_tracks, 16);
    const int cam_tracker = tracker_slot(e->trackers, trackers[0]);             // the frame counts for its camera's live counter even without a task
    VC_TRY(track_enqueue(e, 3, frames, e->d_feat, W, H, cap, nullptr, nullptr, &cam_tracker));
    std::vector<int64_t> buf((size_t)cap * 6);
    int m = 0;
    VC_TRY(track_collect(e, 3, buf.data(), cap, &m));
    rows6.assign(buf.begin(), buf.begin() + (size_t)m * 6);
    return VC_OK;
}

// ---- tracker state on the host (blocking paths: the engine is idle) ---------------------------------------------------------------
struct HostTrackerState { TrackerHdr hdr; std::vector<int> list; std::vector<TrackRecD> recs; };

static int download_tracker(vc_engine* e, int id, HostTrackerState& st) {
    VC_TRY(track_idle(e));
    VC_HIP(hipStreamSynchronize(e->stream));
    VC_HIP(hipMemcpy(&st.hdr, e->d_hdrs + id, sizeof(TrackerHdr), hipMemcpyDeviceToHost));
    const int n = st.hdr.n_tracks;
    st.list.resize(n); st.recs.resize(n);
    if (n) VC_HIP(hipMemcpy(st.list.data(), e->d_lists + (size_t)id * e->list_cap, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    for (int t = 0; t < n; ++t) VC_HIP(hipMemcpy(&st.recs[t], e->d_recs + st.list[t], sizeof(TrackRecD), hipMemcpyDeviceToHost));
    return VC_OK;
}

// free-slot stack, host side (engine idle): take n slots / give slots back
int host_take_slots(vc_engine* e, int n, std::vector<int>& out) {
    int ctl[2];
    VC_HIP(hipMemcpy(ctl, e->d_free, sizeof(ctl), hipMemcpyDeviceToHost));
    VC_CHECK(ctl[0] >= n, VC_ERR_CAPACITY, "track pool too small for %d more tracks (max_tracks = %d)", n, e->cfg.max_tracks);
    out.resize(n);
    if (n) VC_HIP(hipMemcpy(out.data(), e->d_free_stack + (ctl[0] - n), (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    ctl[0] -= n;
    VC_HIP(hipMemcpy(e->d_free, ctl, sizeof(int), hipMemcpyHostToDevice));
    return VC_OK;
}
int host_give_slots(vc_engine* e, const std::vector<int>& slots) {
    if (slots.empty()) return VC_OK;
    int ctl[2];
    VC_HIP(hipMemcpy(ctl, e->d_free, sizeof(ctl), hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(e->d_free_stack + ctl[0], slots.data(), slots.size() * sizeof(int), hipMemcpyHostToDevice));
    ctl[0] += (int)slots.size();
    VC_HIP(hipMemcpy(e->d_free, ctl, sizeof(int), hipMemcpyHostToDevice));
    return VC_OK;
}

static TrackerHdr make_hdr(const vc_tracker_params& p) {
    TrackerHdr h{};
    h.max_dist = p.max_dist; h.max_iou_distance = p.max_iou_distance; h.next_id = 1;
    h.max_age = p.max_age; h.n_init = p.n_init; h.nn_budget = p.nn_budget; h.n_tracks = 0; h.err = TERR_NONE;
    return h;
}

}  // namespace vc

// ================================================================================================ C ABI
using namespace vc;

extern "C" {

int vc_tracker_create(vc_engine* e, const vc_tracker_params* p, int* id) {
    VC_CHECK(e && p && id, VC_ERR_ARG, "null argument");
    VC_CHECK(p->nn_budget >= 1 && p->nn_budget <= e->cfg.nn_budget_cap, VC_ERR_CAPACITY,
             "nn_budget %d outside [1, nn_budget_cap=%d] (an unbounded budget is not supported)", p->nn_budget, e->cfg.nn_budget_cap);
    VC_CHECK(p->max_age >= 1 && p->n_init >= 1, VC_ERR_ARG, "max_age and n_init must be >= 1");
    int slot = -1;                       // an id given back by vc_tracker_destroy is used again before the table grows
    for (int i = 0; i < (int)e->trackers.size() && slot < 0; ++i) if (e->trackers[i]->released) slot = i;
    VC_CHECK(slot >= 0 || (int)e->trackers.size() < e->max_trackers, VC_ERR_CAPACITY,
             "more than max_trackers (%d) trackers (vc_tracker_destroy gives an id back)", e->max_trackers);
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));           // batches in flight index e->trackers
    const TrackerHdr h = make_hdr(*p);
    if (slot < 0) { slot = (int)e->trackers.size(); e->trackers.push_back(std::unique_ptr<Tracker>(new Tracker())); }
    VC_HIP(hipMemcpy(e->d_hdrs + slot, &h, sizeof(h), hipMemcpyHostToDevice));
    Tracker& t = *e->trackers[slot];
    t.p = *p; t.known_tracks = 0; t.pending_dets = 0; t.released = false;
    *id = slot | (t.gen << 16);
    return VC_OK;
}

// The reference builds a new VideoTracker (one DeepSort per class) for every video (modules/__init__.py:32-36) and drops the old one:
// the drop-in's DeepSort gives its tracker back here, so that a process that walks a folder of videos does not run out of ids.
int vc_tracker_destroy(vc_engine* e, int handle) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    VC_CHECK(!e->trackers[id]->live, VC_ERR_STATE, "vc_tracker_destroy: the tracker is attached to a live counter (vc_live_destroy first)");
    VC_TRY(vc_tracker_reset(e, handle)); // waits for the batches in flight, returns the track slots to the pool
    e->trackers[id]->released = true;
    e->trackers[id]->gen = (e->trackers[id]->gen + 1) & 0x7fff;      // handles of this incarnation are refused from now on
    return VC_OK;
}

int vc_tracker_reset(vc_engine* e, int handle) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    // its tracks would leave the pool behind the counter's back: their slots are open there
    VC_CHECK(!e->trackers[id]->live, VC_ERR_STATE, "vc_tracker_reset: the tracker is attached to a live counter (vc_live_destroy first)");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    HostTrackerState st;
    VC_TRY(download_tracker(e, id, st));
    VC_TRY(host_give_slots(e, st.list));
    const TrackerHdr h = make_hdr(e->trackers[id]->p);
    VC_HIP(hipMemcpy(e->d_hdrs + id, &h, sizeof(h), hipMemcpyHostToDevice));
    e->trackers[id]->known_tracks = 0;
    e->trackers[id]->pending_dets = 0;
    return VC_OK;
}

int vc_tracker_step(vc_engine* e, int handle, const double* tlwh, const double* conf, const float* feat, int k) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    VC_CHECK(k == 0 || (tlwh && conf && feat), VC_ERR_ARG, "null argument");
    VC_CHECK(k >= 0 && k <= e->det_cap, VC_ERR_CAPACITY, "%d detections exceed capacity %d", k, e->det_cap);
    if (!e->lives.empty()) VC_TRY(live_overlay_room(e, &handle, 1));
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    if (k > 0) VC_HIP(hipMemcpyAsync(e->d_feat_in, feat, (size_t)k * VC_FEAT_DIM * sizeof(float), hipMemcpyHostToDevice, e->stream));
    std::vector<std::vector<FrameClassDets>> frames(1);
    FrameClassDets fc{0, id, {}};
    fc.dets.tlwh.assign(tlwh, tlwh + (size_t)k * 4);
    fc.dets.conf.assign(conf, conf + k);
    fc.dets.feat_rows.resize(k);
    std::iota(fc.dets.feat_rows.begin(), fc.dets.feat_rows.end(), 0);
    frames[0].push_back(std::move(fc));
    const int cap = e->trackers[id]->known_tracks + k + 16;
    VC_TRY(track_enqueue(e, 3, frames, e->d_feat_in, 1 << 30, 1 << 30, cap, nullptr));
    std::vector<int64_t> buf((size_t)cap * 6);
    int m = 0;
    return track_collect(e, 3, buf.data(), cap, &m);
}

int vc_tracker_count(vc_engine* e, int handle, int* n) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && n && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    HostTrackerState st;
    VC_TRY(download_tracker(e, id, st));
    *n = st.hdr.n_tracks;
    return VC_OK;
}

int vc_tracker_state(vc_engine* e, int handle, int cap, int64_t* ids, int* state, int* hits, int* age, int* tsu, double* mean8,
                     double* cov64, int* gallery_count) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    HostTrackerState st;
    VC_TRY(download_tracker(e, id, st));
    VC_CHECK(st.hdr.n_tracks <= cap, VC_ERR_CAPACITY, "need room for %d tracks", st.hdr.n_tracks);
    for (int t = 0; t < st.hdr.n_tracks; ++t) {
        const TrackRecD& tr = st.recs[t];
        const int slot = st.list[t];
        if (ids) ids[t] = tr.id;
        if (state) state[t] = tr.state;
        if (hits) hits[t] = tr.hits;
        if (age) age[t] = tr.age;
        if (tsu) tsu[t] = tr.tsu;
        if (gallery_count) gallery_count[t] = tr.state == CONFIRMED ? tr.gal_count : 0;
        if (mean8) VC_HIP(hipMemcpy(mean8 + (size_t)t * 8, e->pool.mean + (size_t)slot * 8, 8 * sizeof(double), hipMemcpyDeviceToHost));
        if (cov64) VC_HIP(hipMemcpy(cov64 + (size_t)t * 64, e->pool.cov + (size_t)slot * 64, 64 * sizeof(double), hipMemcpyDeviceToHost));
    }
    return VC_OK;
}

// The cost matrices of the LAST blocking step of this engine (vc_tracker_step / vc_deepsort_update on ONE tracker), as the batch
// kernel left them in its scratch: app[t * D + d] = gated appearance cost of list position t (valid for tracks that were
// confirmed when the step began), iou[t * D + d] = 1 - IoU (valid for the IoU candidates).  T = tracks before the step.
int vc_tracker_debug_costs(vc_engine* e, int cap_entries, double* app, double* iou, int* T, int* D) {
    VC_CHECK(e && app && iou && T && D, VC_ERR_ARG, "null argument");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    const TrackStage& s = e->tstage[3];
    VC_CHECK(s.plan.n_tasks() == 1 && s.plan.n_wg() == 1 && !s.busy, VC_ERR_STATE, "the last blocking call did not step exactly one tracker");
    *T = ((const int*)(s.h_out + s.plan.out.tT))[0];
    *D = s.plan.tasks[0].det_n;
    const size_t n = (size_t)*T * *D;
    VC_CHECK(n <= (size_t)cap_entries, VC_ERR_CAPACITY, "need room for %zu entries", n);
    VC_HIP(hipStreamSynchronize(e->stream));
    const size_t mat = TC_MAT;                                       // scratch of workgroup 0: [appearance | IoU | ...], rows of D entries
    if (n) {
        VC_HIP(hipMemcpy(app, e->d_track_scratch, n * sizeof(double), hipMemcpyDeviceToHost));
        VC_HIP(hipMemcpy(iou, e->d_track_scratch + mat, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return VC_OK;
}

// ---- tracker snapshot / restore (tracker state for stream migration) -----------------------------------------
// Everything Tracker.predict/update reads: parameters, id counter, and per track the FSM counters, the Kalman mean / covariance
// (fp64, bit for bit) and the valid rows of the appearance gallery ring.  Little-endian, packed; restoring on another engine (or
// GPU) and feeding the same detections continues the stream with identical ids and states (tests/test_gpu_tracker.py).
namespace {
struct SnapHeader { char magic[8]; int32_t feat_dim, n_tracks; int64_t next_id; double max_dist, min_confidence, nms_max_overlap, max_iou_distance; int32_t max_age, n_init, nn_budget, pad; };
struct SnapTrack { int64_t id; int32_t state, hits, age, tsu, gal_count, gal_head; double last_conf; double mean[8]; double cov[64]; };
const char kSnapMagic[8] = {'V', 'C', 'T', 'R', 'K', '0', '1', 0};
}  // namespace

int vc_tracker_snapshot(vc_engine* e, int handle, void* buf, size_t cap, size_t* size) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && size && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    HostTrackerState st;
    VC_TRY(download_tracker(e, id, st));
    const vc_tracker_params& tp = e->trackers[id]->p;
    size_t need = sizeof(SnapHeader);
    for (const TrackRecD& tr : st.recs) need += sizeof(SnapTrack) + (size_t)std::min(tr.gal_count, tp.nn_budget) * VC_FEAT_DIM * sizeof(float);
    *size = need;
    if (!buf) return VC_OK;                       // size query
    VC_CHECK(cap >= need, VC_ERR_CAPACITY, "snapshot needs %zu bytes", need);
    char* o = (char*)buf;
    SnapHeader h{};
    memcpy(h.magic, kSnapMagic, 8);
    h.feat_dim = VC_FEAT_DIM; h.n_tracks = st.hdr.n_tracks; h.next_id = st.hdr.next_id;
    h.max_dist = tp.max_dist; h.min_confidence = tp.min_confidence; h.nms_max_overlap = tp.nms_max_overlap;
    h.max_iou_distance = tp.max_iou_distance; h.max_age = tp.max_age; h.n_init = tp.n_init; h.nn_budget = tp.nn_budget;
    memcpy(o, &h, sizeof(h)); o += sizeof(h);
    for (int i = 0; i < st.hdr.n_tracks; ++i) {
        const TrackRecD& tr = st.recs[i];
        const int slot = st.list[i];
        SnapTrack t{};
        t.id = tr.id; t.state = tr.state; t.hits = tr.hits; t.age = tr.age; t.tsu = tr.tsu; t.gal_count = tr.gal_count; t.gal_head = tr.gal_head;
        t.last_conf = 0.0;
        VC_HIP(hipMemcpy(t.mean, e->pool.mean + (size_t)slot * 8, sizeof(t.mean), hipMemcpyDeviceToHost));
        VC_HIP(hipMemcpy(t.cov, e->pool.cov + (size_t)slot * 64, sizeof(t.cov), hipMemcpyDeviceToHost));
        memcpy(o, &t, sizeof(t)); o += sizeof(t);
        const size_t rows = (size_t)std::min(tr.gal_count, tp.nn_budget);
        if (rows) VC_HIP(hipMemcpy(o, e->pool.gallery + (size_t)slot * e->pool.budget_cap * VC_FEAT_DIM, rows * VC_FEAT_DIM * sizeof(float), hipMemcpyDeviceToHost));
        o += rows * VC_FEAT_DIM * sizeof(float);
    }
    return VC_OK;
}

int vc_tracker_restore(vc_engine* e, int handle, const void* buf, size_t size) {
    const int id = e ? tracker_slot(e->trackers, handle) : -1;
    VC_CHECK(e && buf && id >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle");
    VC_CHECK(!e->trackers[id]->live, VC_ERR_STATE, "vc_tracker_restore: the tracker is attached to a live counter (vc_live_destroy first)");
    VC_CHECK(size >= sizeof(SnapHeader), VC_ERR_ARG, "snapshot truncated");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    const char* in = (const char*)buf;
    SnapHeader h;
    memcpy(&h, in, sizeof(h)); in += sizeof(h);
    VC_CHECK(memcmp(h.magic, kSnapMagic, 8) == 0 && h.feat_dim == VC_FEAT_DIM && h.n_tracks >= 0, VC_ERR_ARG, "not a tracker snapshot");
    VC_CHECK(h.nn_budget >= 1 && h.nn_budget <= e->cfg.nn_budget_cap, VC_ERR_CAPACITY, "snapshot nn_budget %d exceeds nn_budget_cap %d", h.nn_budget, e->cfg.nn_budget_cap);
    VC_CHECK(h.max_age >= 1 && h.n_init >= 1 && h.next_id >= 1, VC_ERR_ARG, "snapshot corrupt (parameters)");
    VC_CHECK(h.n_tracks <= e->list_cap, VC_ERR_CAPACITY, "snapshot holds %d tracks, tracks_per_tracker is %d", h.n_tracks, e->list_cap);
    // validate the whole blob before touching the tracker
    {
        const char* q = in;
        for (int i = 0; i < h.n_tracks; ++i) {
            VC_CHECK((size_t)(q - (const char*)buf) + sizeof(SnapTrack) <= size, VC_ERR_ARG, "snapshot truncated");
            SnapTrack t;
            memcpy(&t, q, sizeof(t)); q += sizeof(t);
            VC_CHECK(t.gal_count >= 0 && t.gal_count <= h.nn_budget && t.gal_head >= 0 && t.gal_head < h.nn_budget, VC_ERR_ARG, "snapshot corrupt (gallery ring)");
            VC_CHECK(t.state == TENTATIVE || t.state == CONFIRMED, VC_ERR_ARG, "snapshot corrupt (track state %d)", t.state);
            VC_CHECK(t.hits >= 0 && t.age >= 0 && t.tsu >= 0 && t.id >= 1 && t.id < h.next_id, VC_ERR_ARG, "snapshot corrupt (track counters)");
            q += (size_t)t.gal_count * VC_FEAT_DIM * sizeof(float);
        }
        VC_CHECK((size_t)(q - (const char*)buf) == size, VC_ERR_ARG, "snapshot size mismatch");
    }
    HostTrackerState old;
    VC_TRY(download_tracker(e, id, old));
    VC_TRY(host_give_slots(e, old.list));
    std::vector<int> slots;
    VC_TRY(host_take_slots(e, h.n_tracks, slots));
    Tracker& tk = *e->trackers[id];
    tk.p.max_dist = h.max_dist; tk.p.min_confidence = h.min_confidence; tk.p.nms_max_overlap = h.nms_max_overlap;
    tk.p.max_iou_distance = h.max_iou_distance; tk.p.max_age = h.max_age; tk.p.n_init = h.n_init; tk.p.nn_budget = h.nn_budget;
    TrackerHdr dh = make_hdr(tk.p);
    dh.next_id = h.next_id; dh.n_tracks = h.n_tracks;
    for (int i = 0; i < h.n_tracks; ++i) {
        SnapTrack t;
        memcpy(&t, in, sizeof(t)); in += sizeof(t);
        TrackRecD tr{};
        tr.id = t.id; tr.state = t.state; tr.hits = t.hits; tr.age = t.age; tr.tsu = t.tsu; tr.gal_count = t.gal_count; tr.gal_head = t.gal_head;
        const int slot = slots[i];
        VC_HIP(hipMemcpy(e->d_recs + slot, &tr, sizeof(tr), hipMemcpyHostToDevice));
        VC_HIP(hipMemcpy(e->pool.mean + (size_t)slot * 8, t.mean, sizeof(t.mean), hipMemcpyHostToDevice));
        VC_HIP(hipMemcpy(e->pool.cov + (size_t)slot * 64, t.cov, sizeof(t.cov), hipMemcpyHostToDevice));
        const size_t rows = (size_t)t.gal_count;
        if (rows) VC_HIP(hipMemcpy(e->pool.gallery + (size_t)slot * e->pool.budget_cap * VC_FEAT_DIM, in, rows * VC_FEAT_DIM * sizeof(float), hipMemcpyHostToDevice));
        in += rows * VC_FEAT_DIM * sizeof(float);
    }
    if (h.n_tracks) VC_HIP(hipMemcpy(e->d_lists + (size_t)id * e->list_cap, slots.data(), (size_t)h.n_tracks * sizeof(int), hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(e->d_hdrs + id, &dh, sizeof(dh), hipMemcpyHostToDevice));
    tk.known_tracks = h.n_tracks;
    tk.pending_dets = 0;
    return VC_OK;
}

int vc_deepsort_update(vc_engine* e, int id, const uint8_t* bgr, int h, int w, const double* bbox_xyxy, const double* conf, int k,
                       int64_t* out_rows7, int cap_rows, int* out_m) {
    VC_CHECK(e && bgr && out_m && tracker_slot(e->trackers, id) >= 0, VC_ERR_ARG, "bad argument (null pointer, bad or stale tracker handle)");
    VC_CHECK(k >= 1 && bbox_xyxy && conf, VC_ERR_ARG, "DeepSort.update needs at least one box (the reference only calls it then)");
    if (!e->lives.empty()) VC_TRY(live_overlay_room(e, &id, 1));
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    const size_t bytes = (size_t)h * w * 3;
    VC_CHECK(bytes <= e->d_frames_bytes, VC_ERR_CAPACITY, "frame exceeds the staging buffer");
    VC_HIP(hipMemcpyAsync(e->d_frames, bgr, bytes, hipMemcpyHostToDevice, e->stream));
    FrameDets d;                                                // one tracker: every box is class 0 of one
    d.xyxy.assign(bbox_xyxy, bbox_xyxy + (size_t)k * 4); d.conf.assign(conf, conf + k); d.label.assign(k, 0);
    std::vector<int64_t> rows6;
    VC_TRY(frame_track(e, e->d_frames, 0, h, w, &id, 1, d, rows6));
    const int m = (int)(rows6.size() / 6);
    VC_CHECK(m <= cap_rows, VC_ERR_CAPACITY, "need room for %d rows", m);
    for (int i = 0; i < m; ++i) {
        for (int c = 0; c < 5; ++c) out_rows7[i * 7 + c] = rows6[(size_t)i * 6 + c];
        out_rows7[i * 7 + 5] = -1;       // track_feat slot: features of confirmed tracks were just cleared (quirk Q7)
        out_rows7[i * 7 + 6] = 0;        // int(confidence) with confidence in (0, 1)
    }
    *out_m = m;
    return VC_OK;
}

int vc_videotracker_run(vc_engine* e, const int* trackers, int num_classes, const uint8_t* bgr, int h, int w, const double* boxes_xywh,
                        const int64_t* labels, const double* scores, int n, int64_t* out_rows6, int cap_rows, int* out_m) {
    VC_CHECK(e && trackers && bgr && out_m, VC_ERR_ARG, "null argument");
    VC_CHECK(n >= 1 && boxes_xywh && labels && scores, VC_ERR_ARG, "VideoTracker.run needs at least one box (quirk Q1)");
    if (!e->lives.empty()) VC_TRY(live_overlay_room(e, trackers, num_classes));
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    const size_t bytes = (size_t)h * w * 3;
    VC_CHECK(bytes <= e->d_frames_bytes, VC_ERR_CAPACITY, "frame exceeds the staging buffer");
    VC_HIP(hipMemcpyAsync(e->d_frames, bgr, bytes, hipMemcpyHostToDevice, e->stream));
    // boxes of classes outside [0, num_classes) are ignored exactly like the reference's mask loop (modules/track.py:50-59), and only used
    // boxes are embedded: frame_track gets the in-range boxes in class-major order
    std::vector<int> lab(n);
    for (int i = 0; i < n; ++i) lab[i] = labels[i] >= 0 && labels[i] < num_classes ? (int)labels[i] : -1;
    LabelGroups groups;
    group_by_label(lab.data(), n, groups);
    FrameDets used;
    for (int k = groups.first[groups.label[0] < 0 ? 1 : 0]; k < n; ++k) {
        const double* b = boxes_xywh + (size_t)groups.order[k] * 4;
        const double xyxy[4] = {b[0], b[1], b[2] + b[0], b[3] + b[1]};                      // modules/track.py:39-41
        used.xyxy.insert(used.xyxy.end(), xyxy, xyxy + 4);
        used.conf.push_back(scores[groups.order[k]]);
        used.label.push_back(lab[groups.order[k]]);
    }
    std::vector<int64_t> rows6;
    if (!used.conf.empty()) VC_TRY(frame_track(e, e->d_frames, 0, h, w, trackers, num_classes, used, rows6));
    const int m = (int)(rows6.size() / 6);
    VC_CHECK(m <= cap_rows, VC_ERR_CAPACITY, "need room for %d rows", m);
    memcpy(out_rows6, rows6.data(), rows6.size() * sizeof(int64_t));
    *out_m = m;
    return VC_OK;
}

int vc_dsort_nms_host(const double* tlwh, const double* scores, int n, double max_overlap, int* keep, int* n_keep) {
    VC_CHECK(n_keep && (n == 0 || (tlwh && scores && keep)), VC_ERR_ARG, "null argument");
    std::vector<int> k;
    dsort_nms(tlwh, scores, n, max_overlap, k);
    for (size_t i = 0; i < k.size(); ++i) keep[i] = k[i];
    *n_keep = (int)k.size();
    return VC_OK;
}

}  // extern "C"
