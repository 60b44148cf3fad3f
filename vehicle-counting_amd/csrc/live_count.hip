// Running per-camera counts on the device, beside the tracker ("an all-gather of per-camera count tensors ... at end-of-run
// (or per reporting interval)"): the counts of a stream that never ends, without keeping a row of it.
//
// The rule: the counts read at any moment equal vc_counts of a vc_counter (counting.hip) that was fed exactly the rows of
// all batches enqueued so far -- the reference's end state (/root/reference/utilities/counting/utils.py:276-297 count_frame_directions
// over the table of modules/track.py:81-137 VideoCounting.run) for the video cut at that point, integer for integer, with
// utilities/counting/utils.py:139-152 (strict '>' from 0, first direction as fall-back, NaN from a zero-length vector: Q11) and
// utilities/counting/bb_polygon.py:96-114 (any box corner inside shapes[0]: Q12).  The arithmetic is count_core.h, the body counting.hip
// runs on the host.
//
// What is kept: per tracker pool slot (indexed like TrackBatchArgs::recs) the record vc_counter keeps per track minus its row history
// (cc::LiveSlot: open, camera, label, first in-zone box, last in-zone box, last frame, rows at the last frame), and per counter
// base[n_cam][max_dir][n_labels].  A track whose slot the tracker kernel freed can never produce another row, so its contribution is
// final: it is added to base and the slot is closed.  Memory is max_tracks records and one int32 tensor, whatever the stream's length.
//
//   live_count_apply_kernel   per tracker launch, between track_batch_kernel and merge_free_kernel (launch_track_batch):
//                             1. the batch's rows in task order onto the slot of their track (TrackBatchArgs::row_slot names it; rows with
//                                no corner in their camera's polygon are skipped, as in vc_counter_add);
//                             2. every slot of freed[0, freed_count) that is open: base[cam][best_direction][label] += at_last, closed.
//                             A track can be confirmed and deleted inside one batch: 1 before 2.
//   live_count_read_kernel    counts = base + the contribution of every open slot, into a tensor that stays on the device.
//
// Shape: ONE workgroup of 16 waves.  A wave takes a tracker (a TrackWgPlan) and walks its tasks in order; within a task the lanes load
// and zone-test the rows in parallel, then the in-zone rows are applied in row order, each by the lane that OWNS the slot (slot % 64):
// a slot belongs to one tracker, a tracker to one wave, so a record is only ever touched by one lane, in program order -- no atomics
// and no ordering between lanes is needed for step 1.  Step 2 follows a workgroup barrier.  The work is a few thousand rows per batch
// at most; one workgroup keeps the two steps in one launch without a grid-wide barrier.
#include <algorithm>
#include <cstring>

#include "engine.h"

#pragma clang fp contract(off)

#include "count_core.h"

namespace vc {

using cc::LiveSlot;

namespace {

__device__ __forceinline__ long long shfl_i64(long long v, int src) {
    const int lo = __shfl((int)(unsigned)(unsigned long long)v, src), hi = __shfl((int)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ int live_index(const LiveCountArgs& a, int cam, int d, int label) { return (cam * a.max_dir + d) * a.n_labels + label; }

__device__ __forceinline__ int slot_direction(const LiveCountArgs& a, const LiveSlot& s) {
    return cc::best_direction(a.dir_lines + (size_t)s.cam * cc::CC_MAX_DIRS * 4, a.n_dir[s.cam], s.first, s.last, nullptr, nullptr);
}

}  // namespace

__global__ __launch_bounds__(1024) void live_count_apply_kernel(const LiveCountArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    // ---- step 1 ----------------------------------------------------------------------------------------------------------------
    for (int p = wave; p < a.n_plans; p += n_waves) {                     // wave-uniform
        const TrackWgPlan plan = a.plans[p];
        if (plan.tracker < 0 || plan.tracker >= a.n_trackers) continue;
        const int cam = a.owner[plan.tracker];
        if (cam < 0 || cam >= a.n_cam) continue;                          // another counter's tracker, or none's
        const double* poly = a.polygons + (size_t)cam * cc::CC_MAX_POINTS * 2;
        const int pn = a.poly_n[cam];
        for (int task = plan.task_begin; task < plan.task_end; ++task) {
            const TrackTask tk = a.tasks[task];
            const int n = a.task_row_n[task], off = a.task_row_off[task];
            const long long frame = a.frame_no[tk.frame];
            if (n <= 0 || off < 0 || off > a.rows_cap - n) continue;           // (wave-uniform) nothing emitted, or a refused step
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                long long box[4] = {0, 0, 0, 0};
                int slot = -1, label = -1;
                bool in = false;
                if (i < n) {
                    const long long* r = a.rows + (size_t)(off + i) * 6;
                    box[0] = r[0]; box[1] = r[1]; box[2] = r[2]; box[3] = r[3];
                    label = (int)r[5];
                    slot = a.row_slot[off + i];
                    in = slot >= 0 && slot < a.max_tracks && label >= 0 && label < a.n_labels && cc::box_in_polygon(poly, pn, (const int64_t*)box);
                }
                unsigned long long m = __ballot(in);
                while (m) {                                                // in-zone rows in row order (wave-uniform loop)
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int sj = __shfl(slot, j), lj = __shfl(label, j);
                    long long bj[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) bj[k] = shfl_i64(box[k], j);
                    if ((sj & 63) == lane) cc::live_slot_add(a.slots[sj], cam, lj, (int64_t)frame, (const int64_t*)bj);
                }
            }
        }
    }
    __syncthreads();
    // ---- step 2 ----------------------------------------------------------------------------------------------------------------
    const int nf = *a.freed_count;
    for (int i = threadIdx.x; i < nf; i += blockDim.x) {
        const int slot = a.freed[i];
        if (slot < 0 || slot >= a.max_tracks) continue;
        LiveSlot& s = a.slots[slot];
        if (!s.open) continue;                                             // never in the zone, or another counter's
        const int d = slot_direction(a, s);
        __hip_atomic_fetch_add(a.base + live_index(a, s.cam, d, s.label), s.at_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a.stats + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.open = 0;
    }
}

__global__ __launch_bounds__(1024) void live_count_read_kernel(const LiveCountArgs a) {
    const int n = a.n_cam * a.max_dir * a.n_labels;
    for (int i = threadIdx.x; i < n; i += blockDim.x) a.counts[i] = a.base[i];
    if (threadIdx.x == 0) a.stats[0] = 0;
    __syncthreads();
    for (int slot = threadIdx.x; slot < a.max_tracks; slot += blockDim.x) {
        const LiveSlot& s = a.slots[slot];
        if (!s.open) continue;
        __hip_atomic_fetch_add(a.counts + live_index(a, s.cam, slot_direction(a, s), s.label), s.at_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a.stats, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int launch_live_count_apply(const LiveCountArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(live_count_apply_kernel, dim3(1), dim3(1024), 0, s, a);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

int launch_live_count_read(const LiveCountArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(live_count_read_kernel, dim3(1), dim3(1024), 0, s, a);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// The zones of n_cam cameras as the kernels read them: polygons padded to CC_MAX_POINTS points, direction lines to CC_MAX_DIRS.
// polygons / dir_lines arrive concatenated in camera order (poly_n[c] points, n_dir[c] lines).  Pure host code.
int live_pack_zones(int n_cam, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir, std::vector<double>& poly_out,
                    std::vector<double>& dirs_out, int* max_dir) {
    VC_CHECK(n_cam >= 1 && polygons && poly_n && dir_lines && n_dir && max_dir, VC_ERR_ARG, "bad argument");
    poly_out.assign((size_t)n_cam * cc::CC_MAX_POINTS * 2, 0.0);
    dirs_out.assign((size_t)n_cam * cc::CC_MAX_DIRS * 4, 0.0);
    *max_dir = 0;
    size_t po = 0, dof = 0;
    for (int c = 0; c < n_cam; ++c) {
        VC_CHECK(poly_n[c] >= 1 && n_dir[c] >= 1, VC_ERR_ARG, "camera %d: a zone needs at least one polygon point and one direction", c);
        VC_CHECK(poly_n[c] <= cc::CC_MAX_POINTS, VC_ERR_CAPACITY, "camera %d: %d polygon points, a live counter takes at most %d", c, poly_n[c], (int)cc::CC_MAX_POINTS);
        VC_CHECK(n_dir[c] <= cc::CC_MAX_DIRS, VC_ERR_CAPACITY, "camera %d: %d directions, a live counter takes at most %d", c, n_dir[c], (int)cc::CC_MAX_DIRS);
        std::copy(polygons + po * 2, polygons + (po + poly_n[c]) * 2, poly_out.begin() + (size_t)c * cc::CC_MAX_POINTS * 2);
        std::copy(dir_lines + dof * 4, dir_lines + (dof + n_dir[c]) * 4, dirs_out.begin() + (size_t)c * cc::CC_MAX_DIRS * 4);
        po += poly_n[c]; dof += n_dir[c];
        *max_dir = std::max(*max_dir, n_dir[c]);
    }
    return VC_OK;
}

}  // namespace vc

using namespace vc;

// struct vc_live: engine.h (live_overlay.hip shares it)

namespace vc {

// tracker.hip: the counters that own a tracker of the batch, with the batch's frame numbers (device), ready for launch_track_batch
void live_batch_args(vc_engine* e, const std::vector<int>& batch_trackers, const long long* d_frame_no, std::vector<LiveCountArgs>& out) {
    out.clear();
    for (vc_live* l : e->lives) {
        bool used = false;
        for (int t : batch_trackers) if (e->trackers[t]->live == l) { used = true; break; }
        if (!used) continue;
        LiveCountArgs a = l->dev;
        a.frame_no = d_frame_no;
        out.push_back(a);
    }
}

// the 1-based number of the next frame of the camera this tracker belongs to (0: the tracker is not attached)
long long live_next_frame(vc_engine* e, int tracker_slot_) {
    if (tracker_slot_ < 0 || tracker_slot_ >= (int)e->trackers.size()) return 0;
    const Tracker& t = *e->trackers[tracker_slot_];
    if (!t.live) return 0;
    return ++t.live->frames_done[t.live_cam];
}

static void live_free(vc_live* l) {
    live_overlay_free(l);                                // waits for the render contexts that still read its lists
    live_ckpt_free(l);                                   // waits for a checkpoint in flight
    for (void* p : l->allocs) (void)hipFree(p);
    if (l->h_out) (void)hipHostFree(l->h_out);
    delete l;
}

void live_destroy_all(vc_engine* e) {
    for (vc_live* l : e->lives) live_free(l);
    e->lives.clear();
    for (auto& t : e->trackers) { t->live = nullptr; t->live_cam = -1; }
}

static int live_read(vc_live* l) {                       // counts + stats -> pinned memory, after everything enqueued so far
    vc_engine* e = l->e;
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(launch_live_count_read(l->dev, e->stream));
    const int n = l->n_cam * l->max_dir * l->n_labels;
    VC_HIP(hipMemcpyAsync(l->h_out, l->dev.counts, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(hipMemcpyAsync(l->h_out + n, l->dev.stats, 8, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(hipStreamSynchronize(e->stream));
    return VC_OK;
}

}  // namespace vc

extern "C" {

int vc_live_create(vc_engine* e, int n_cam, int n_labels, const int* trackers, const double* polygons, const int* poly_n, const double* dir_lines,
                   const int* n_dir, vc_live** out) {
    VC_CHECK(e && trackers && out && n_cam >= 1 && n_labels >= 1, VC_ERR_ARG, "bad argument");
    std::vector<double> poly, dirs;
    int max_dir = 0;
    VC_TRY(live_pack_zones(n_cam, polygons, poly_n, dir_lines, n_dir, poly, dirs, &max_dir));
    std::vector<int> slots((size_t)n_cam * n_labels);
    for (size_t i = 0; i < slots.size(); ++i) {
        slots[i] = tracker_slot(e->trackers, trackers[i]);
        VC_CHECK(slots[i] >= 0, VC_ERR_NOTFOUND, "bad or stale tracker handle %d (camera %d, label %d)", trackers[i], (int)(i / n_labels), (int)(i % n_labels));
        VC_CHECK(!e->trackers[slots[i]]->live, VC_ERR_STATE, "tracker %d (camera %d, label %d) is already attached to a live counter", trackers[i],
                 (int)(i / n_labels), (int)(i % n_labels));
        for (size_t k = 0; k < i; ++k) VC_CHECK(slots[k] != slots[i], VC_ERR_STATE, "tracker %d is named twice", trackers[i]);
    }
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));                 // batches in flight were launched without this counter
    VC_HIP(hipStreamSynchronize(e->stream));
    vc_live* l = new vc_live();
    l->e = e; l->n_cam = n_cam; l->n_labels = n_labels; l->max_dir = max_dir; l->trackers = slots;
    l->frames_done.assign(n_cam, 0);
    l->n_dir.assign(n_dir, n_dir + n_cam);
    l->poly_n.assign(poly_n, poly_n + n_cam); l->h_poly = poly; l->h_dirs = dirs;
    const int n = n_cam * max_dir * n_labels, T = e->cfg.max_tracks;
    std::vector<int> owner((size_t)e->max_trackers, -1);
    for (size_t i = 0; i < slots.size(); ++i) owner[slots[i]] = (int)(i / n_labels);
    double *d_poly = nullptr, *d_dirs = nullptr;
    int *d_pn = nullptr, *d_nd = nullptr, *d_owner = nullptr, *d_base = nullptr, *d_counts = nullptr, *d_stats = nullptr;
    LiveSlot* d_slots = nullptr;
    auto fail = [&](int code) { live_free(l); return code; };
    auto up = [&](void** p, const void* src, size_t bytes) -> int {
        VC_TRY(dev_alloc(l->allocs, p, bytes));
        if (src) VC_HIP(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice)); else VC_HIP(hipMemset(*p, 0, bytes));
        return VC_OK;
    };
    int rc = VC_OK;
    if ((rc = up((void**)&d_poly, poly.data(), poly.size() * 8)) || (rc = up((void**)&d_dirs, dirs.data(), dirs.size() * 8)) ||
        (rc = up((void**)&d_pn, poly_n, (size_t)n_cam * 4)) || (rc = up((void**)&d_nd, n_dir, (size_t)n_cam * 4)) ||
        (rc = up((void**)&d_owner, owner.data(), owner.size() * 4)) || (rc = up((void**)&d_slots, nullptr, (size_t)T * sizeof(LiveSlot))) ||
        (rc = up((void**)&d_base, nullptr, (size_t)n * 4)) || (rc = up((void**)&d_counts, nullptr, (size_t)n * 4)) || (rc = up((void**)&d_stats, nullptr, 64)))
        return fail(rc);
    if (hipHostMalloc((void**)&l->h_out, (size_t)(n + 2) * 4) != hipSuccess) { set_error("hipHostMalloc failed for a live counter"); return fail(VC_ERR_HIP); }
    LiveCountArgs& a = l->dev;
    a.polygons = d_poly; a.poly_n = d_pn; a.dir_lines = d_dirs; a.n_dir = d_nd; a.n_cam = n_cam; a.n_labels = n_labels; a.max_dir = max_dir;
    a.owner = d_owner; a.n_trackers = e->max_trackers; a.slots = d_slots; a.max_tracks = T; a.base = d_base; a.counts = d_counts; a.stats = d_stats;
    for (size_t i = 0; i < slots.size(); ++i) { e->trackers[slots[i]]->live = l; e->trackers[slots[i]]->live_cam = (int)(i / n_labels); }
    e->lives.push_back(l);
    *out = l;
    return VC_OK;
}

int vc_live_destroy(vc_live* l) {
    if (!l) return VC_OK;
    vc_engine* e = l->e;
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    VC_HIP(hipStreamSynchronize(e->stream));
    for (int s : l->trackers) { e->trackers[s]->live = nullptr; e->trackers[s]->live_cam = -1; }
    e->lives.erase(std::remove(e->lives.begin(), e->lives.end(), l), e->lives.end());
    live_free(l);
    return VC_OK;
}

int vc_live_counts(vc_live* l, int32_t* out, int64_t* frames_done) {
    VC_CHECK(l && out, VC_ERR_ARG, "null argument");
    VC_TRY(live_read(l));
    memcpy(out, l->h_out, (size_t)l->n_cam * l->max_dir * l->n_labels * 4);
    if (frames_done) for (int c = 0; c < l->n_cam; ++c) frames_done[c] = l->frames_done[c];
    return VC_OK;
}

int vc_live_counts_dev(vc_live* l, const int32_t** dev_ptr) {
    VC_CHECK(l && dev_ptr, VC_ERR_ARG, "null argument");
    VC_TRY(live_read(l));
    *dev_ptr = l->dev.counts;
    return VC_OK;
}

int vc_live_stats(vc_live* l, int* open_tracks, int* retired_tracks) {
    VC_CHECK(l && open_tracks && retired_tracks, VC_ERR_ARG, "null argument");
    VC_TRY(live_read(l));
    const int n = l->n_cam * l->max_dir * l->n_labels;
    *open_tracks = l->h_out[n]; *retired_tracks = l->h_out[n + 1];
    return VC_OK;
}

// One launch of each kernel on host arrays (the parity entry point of tests/test_gpu_live_count.py): the counter's zones, the state a
// previous batch left (slots88: max_tracks records of 88 bytes = cc::LiveSlot; base; stats2), one batch -- rows, their slots, tasks
// [n_tasks][5] = (tracker, frame index into frame_no, label, first row, rows) grouped by tracker as the tracker kernel's plans are, the
// freed list -- and back: slots88, base, stats2 updated, counts written.  Everything the kernels write lies between guard blocks.
int vc_live_count_host(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir,
                       int n_trackers, const int* tracker_cam, int max_tracks, const int64_t* rows6, const int* row_slot, int n_rows,
                       const int* tasks5, int n_tasks, const int64_t* frame_no, int n_frames, const int* freed, int n_freed,
                       void* slots88, int32_t* base, int32_t* stats2, int32_t* counts) {
    VC_CHECK(tracker_cam && slots88 && base && stats2 && counts && n_labels >= 1 && n_trackers >= 1 && max_tracks >= 1, VC_ERR_ARG, "bad argument");
    VC_CHECK(n_rows >= 0 && n_tasks >= 0 && n_frames >= 0 && n_freed >= 0 && (n_rows == 0 || (rows6 && row_slot)) && (n_tasks == 0 || (tasks5 && frame_no)) &&
             (n_freed == 0 || freed), VC_ERR_ARG, "bad argument");
    std::vector<double> poly, dirs;
    int max_dir = 0;
    VC_TRY(live_pack_zones(n_cam, polygons, poly_n, dir_lines, n_dir, poly, dirs, &max_dir));
    std::vector<TrackTask> tasks(std::max(n_tasks, 1));
    std::vector<int> off(std::max(n_tasks, 1)), cnt(std::max(n_tasks, 1));
    std::vector<TrackWgPlan> plans;
    for (int t = 0; t < n_tasks; ++t) {
        const int* q = tasks5 + (size_t)t * 5;
        VC_CHECK(q[0] >= 0 && q[0] < n_trackers && q[1] >= 0 && q[1] < n_frames && q[3] >= 0 && q[4] >= 0 && q[3] + q[4] <= n_rows, VC_ERR_ARG, "task %d out of range", t);
        tasks[t] = TrackTask{q[0], 0, 0, q[1], q[2], 0, 0, 0};
        off[t] = q[3]; cnt[t] = q[4];
        if (plans.empty() || plans.back().tracker != q[0]) {
            for (const TrackWgPlan& pl : plans) VC_CHECK(pl.tracker != q[0], VC_ERR_ARG, "task %d: the tasks of tracker %d are not contiguous", t, q[0]);
            plans.push_back(TrackWgPlan{q[0], t, t + 1, 0, 0, 0, 0, 0});
        } else plans.back().task_end = t + 1;
    }
    for (int i = 0; i < n_freed; ++i) VC_CHECK(freed[i] >= 0 && freed[i] < max_tracks, VC_ERR_ARG, "freed slot %d out of range", freed[i]);
    for (int i = 0; i < n_trackers; ++i) VC_CHECK(tracker_cam[i] >= -1 && tracker_cam[i] < n_cam, VC_ERR_ARG, "tracker %d: camera %d outside [-1, %d)", i, tracker_cam[i], n_cam);
    for (int i = 0; i < max_tracks; ++i) {                    // an open record addresses base / counts by its camera and label
        const LiveSlot& s = ((const LiveSlot*)slots88)[i];
        VC_CHECK(!s.open || (s.cam >= 0 && s.cam < n_cam && s.label >= 0 && s.label < n_labels), VC_ERR_ARG, "slot %d: camera %d / label %d out of range", i, s.cam, s.label);
    }
    const int n = n_cam * max_dir * n_labels;
    DevScratch mem;
    GuardedOut g_slots, g_base, g_counts, g_stats;
    LiveCountArgs a{};
    double *d_poly = nullptr, *d_dirs = nullptr;
    int *d_pn = nullptr, *d_nd = nullptr, *d_owner = nullptr, *d_rslot = nullptr, *d_off = nullptr, *d_cnt = nullptr, *d_freed = nullptr, *d_nfreed = nullptr;
    long long *d_rows = nullptr, *d_fno = nullptr;
    TrackTask* d_tasks = nullptr; TrackWgPlan* d_plans = nullptr;
    const long long zero = 0;
    VC_TRY(mem.upload(&d_poly, poly.data(), poly.size() * 8));
    VC_TRY(mem.upload(&d_dirs, dirs.data(), dirs.size() * 8));
    VC_TRY(mem.upload(&d_pn, poly_n, (size_t)n_cam * 4));
    VC_TRY(mem.upload(&d_nd, n_dir, (size_t)n_cam * 4));
    VC_TRY(mem.upload(&d_owner, tracker_cam, (size_t)n_trackers * 4));
    VC_TRY(mem.upload(&d_rows, n_rows ? (const void*)rows6 : (const void*)&zero, std::max((size_t)n_rows * 48, (size_t)8)));
    VC_TRY(mem.upload(&d_rslot, n_rows ? (const void*)row_slot : (const void*)&zero, std::max((size_t)n_rows * 4, (size_t)4)));
    VC_TRY(mem.upload(&d_tasks, tasks.data(), tasks.size() * sizeof(TrackTask)));
    VC_TRY(mem.upload(&d_plans, plans.empty() ? (const void*)tasks.data() : (const void*)plans.data(), std::max(plans.size(), (size_t)1) * sizeof(TrackWgPlan)));
    VC_TRY(mem.upload(&d_off, off.data(), off.size() * 4));
    VC_TRY(mem.upload(&d_cnt, cnt.data(), cnt.size() * 4));
    VC_TRY(mem.upload(&d_fno, n_frames ? (const void*)frame_no : (const void*)&zero, std::max((size_t)n_frames * 8, (size_t)8)));
    VC_TRY(mem.upload(&d_freed, n_freed ? (const void*)freed : (const void*)&zero, std::max((size_t)n_freed * 4, (size_t)4)));
    VC_TRY(mem.upload(&d_nfreed, &n_freed, 4));
    VC_TRY(g_slots.alloc(mem, (size_t)max_tracks * sizeof(LiveSlot), slots88));
    VC_TRY(g_base.alloc(mem, (size_t)n * 4, base));
    VC_TRY(g_stats.alloc(mem, 8, stats2));
    VC_TRY(g_counts.alloc(mem, (size_t)n * 4));
    a.polygons = d_poly; a.poly_n = d_pn; a.dir_lines = d_dirs; a.n_dir = d_nd; a.n_cam = n_cam; a.n_labels = n_labels; a.max_dir = max_dir;
    a.owner = d_owner; a.n_trackers = n_trackers; a.slots = g_slots.as<LiveSlot>(); a.max_tracks = max_tracks;
    a.base = g_base.as<int>(); a.counts = g_counts.as<int>(); a.stats = g_stats.as<int>(); a.frame_no = d_fno;
    a.plans = d_plans; a.n_plans = (int)plans.size(); a.tasks = d_tasks; a.rows = d_rows; a.row_slot = d_rslot; a.task_row_off = d_off; a.task_row_n = d_cnt; a.rows_cap = n_rows;
    a.freed = d_freed; a.freed_count = d_nfreed;
    VC_TRY(launch_live_count_apply(a, nullptr));
    VC_TRY(kernel_wait("live_count_apply_kernel"));
    VC_TRY(launch_live_count_read(a, nullptr));
    VC_TRY(kernel_wait("live_count_read_kernel"));
    VC_TRY(g_slots.read_back(slots88, "live_count_apply_kernel (slots)"));
    VC_TRY(g_base.read_back(base, "live_count_apply_kernel (base)"));
    VC_TRY(g_stats.read_back(stats2, "live_count kernels (stats)"));
    return g_counts.read_back(counts, "live_count_read_kernel (counts)");
}

int vc_live_allgather(vc_engine* e, vc_live* l, int32_t* out) {
    VC_CHECK(e && l && out && l->e == e, VC_ERR_ARG, "bad argument");
    return live_allgather(e, l->dev, out);       // counting.hip, beside vc_allgather_counts
}

}  // extern "C"
