// Live annotated video: the overlay lists of a batch built on the device, beside the live counter (live_count.hip).
//
// The definition is overlay.py::LiveVisualizer; the arithmetic is overlay_build.h, shared with the host.  When the tracker
// launch of a batch has run, everything its picture needs is in device memory: the rows and their pool slots, each track's first in-zone
// box (cc::LiveSlot::first), the frame numbers, the zones and the counts.  The kernels below turn that into the prims12 / frame_first
// lists overlay_kernel paints (overlay.hip), in a per-batch arena a render context reads behind an event -- no host hop.
//
//   live_overlay_count_kernel   one workgroup per frame: the frame's rows (through the tasks whose `frame` it is, labels ascending -- the
//                               order vc_stream_collect hands them back in), the zone test and every row's primitive count; the counts
//                               of anno, count text and frame number; their sum -> frame_cnt[f].
//   live_overlay_build_kernel   one workgroup per frame: a scan over frame_cnt gives the frame its place in the arena (workgroup 0 also
//                               writes frame_first); then the frame's parts in chunks of 256 -- a workgroup prefix sum over the chunk's
//                               counts gives every part its offset, and its lane writes it with plain 16-byte vector stores.
// Two launches rather than one: the arena is compact and in frame order, so no frame can be placed before every earlier frame has been
// counted, and the kernels use no grid-wide wait.  A frame that does not fit raises flags[0]; it and every later frame own nothing.
//
// Ordering facts, asserted where they are used: FIRST BOX and COUNTS BEFORE THE BATCH (below).
#include <algorithm>
#include <cstring>
#include <deque>

#include "engine.h"

#pragma clang fp contract(off)

#include "count_core.h"
#include "overlay_build.h"

namespace vc {

using cc::LiveSlot;

enum { LO_THREADS = 256, LO_MAX_LABELS = 256, LO_MAX_BATCH = 1024 };
static_assert((int)ob::OB_MAX_DIRS == (int)cc::CC_MAX_DIRS, "overlay_build.h strides the direction arrays like count_core.h");

namespace {

struct FrameRows {                       // LDS: the tasks of one frame by label, and where each label's rows start among the frame's rows
    int task_of_label[LO_MAX_LABELS];
    int row_base[LO_MAX_LABELS + 1];
};

// the frame's tasks of camera `cam`, at most one per label (a tracker belongs to one (camera, label), a task to one (tracker, frame))
__device__ void frame_rows_setup(const LiveOverlayArgs& a, int f, int cam, FrameRows& fr) {
    for (int l = threadIdx.x; l < a.n_labels; l += blockDim.x) fr.task_of_label[l] = -1;
    __syncthreads();
    for (int t = threadIdx.x; t < a.n_tasks; t += blockDim.x) {
        const TrackTask tk = a.tasks[t];
        if (tk.frame != f || tk.tracker < 0 || tk.tracker >= a.n_trackers || a.owner[tk.tracker] != cam || tk.label < 0 || tk.label >= a.n_labels) continue;
        const int n = a.task_row_n[t], off = a.task_row_off[t];
        if (n <= 0 || off < 0 || off > a.rows_cap - n) continue;                   // nothing emitted, or a refused step (as live_count_apply_kernel)
        fr.task_of_label[tk.label] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int l = 0; l < a.n_labels; ++l) {
            fr.row_base[l] = acc;
            if (fr.task_of_label[l] >= 0) acc += a.task_row_n[fr.task_of_label[l]];
        }
        fr.row_base[a.n_labels] = acc;
    }
    __syncthreads();
}

// row r of the frame (emit order) -> its index in the rows arena
__device__ __forceinline__ int frame_row_index(const LiveOverlayArgs& a, const FrameRows& fr, int r) {
    int lo = 0, hi = a.n_labels;                                                   // the last label whose rows start at or before r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (fr.row_base[mid] <= r) lo = mid; else hi = mid;
    }
    return a.task_row_off[fr.task_of_label[lo]] + (r - fr.row_base[lo]);
}
// (labels without rows share their row_base with the next label; the search above lands on the LAST label with row_base <= r, which is
// the one that owns r because an empty label's base equals its successor's)

__device__ int block_scan_inclusive(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    __syncthreads();                                                               // s_wave of the previous call has been read
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < n_waves; ++i) { if (i < wave) before += s_wave[i]; all += s_wave[i]; }
    *total = all;
    return v + before;
}

__device__ __forceinline__ bool text_on(const LiveOverlayArgs& a, int cam) { return a.counts_before && (!a.text_cam || a.text_cam[cam]); }

}  // namespace

__global__ __launch_bounds__(LO_THREADS) void live_overlay_count_kernel(const LiveOverlayArgs a) {
    __shared__ FrameRows fr;
    __shared__ int s_wave[LO_THREADS / 64];
    const int f = blockIdx.x, cam = a.cam_of_frame[f];
    if (cam < 0 || cam >= a.n_cam) {                                               // (workgroup-uniform) not a camera of this counter
        if (threadIdx.x == 0) a.frame_cnt[f] = 0;
        return;
    }
    frame_rows_setup(a, f, cam, fr);
    const double* poly = a.polygons + (size_t)cam * cc::CC_MAX_POINTS * 2;
    const int pn = a.poly_n[cam], R = fr.row_base[a.n_labels], n_dir = a.n_dir[cam];
    int mine = 0;
    for (int r = threadIdx.x; r < R; r += blockDim.x) {
        const int idx = frame_row_index(a, fr, r);
        const long long* row = a.rows + (size_t)idx * 6;
        const int64_t box[4] = {row[0], row[1], row[2], row[3]};
        const int slot = a.row_slot[idx];
        const int cnt = slot >= 0 && slot < a.max_tracks && cc::box_in_polygon(poly, pn, box) ? ob::count_row(row[4], row[5]) : 0;
        a.row_cnt[idx] = cnt;
        mine += cnt;
    }
    if (threadIdx.x == 0)
        mine += ob::count_anno(poly, pn, a.dir_lines + (size_t)cam * cc::CC_MAX_DIRS * 4, n_dir, a.dir_keys + (size_t)cam * cc::CC_MAX_DIRS) + ob::count_frame_no(a.frame_no[f]);
    if (text_on(a, cam))
        for (int part = threadIdx.x; part < ob::text_parts(n_dir, a.n_labels); part += blockDim.x) {
            int d, pass, seg;
            ob::text_part(part, a.n_labels, &d, &pass, &seg);
            mine += ob::count_count_seg(a.dir_keys[(size_t)cam * cc::CC_MAX_DIRS + d], a.counts_before + ((size_t)cam * a.max_dir + d) * a.n_labels, pass, seg);
        }
    int total;
    (void)block_scan_inclusive(mine, s_wave, &total);
    if (threadIdx.x == 0) a.frame_cnt[f] = total;
}

__global__ __launch_bounds__(LO_THREADS) void live_overlay_build_kernel(const LiveOverlayArgs a) {
    __shared__ FrameRows fr;
    __shared__ int s_wave[LO_THREADS / 64];
    __shared__ int s_cnt[LO_MAX_BATCH];
    __shared__ int s_base, s_fit;
    const int f = blockIdx.x;
    for (int g = threadIdx.x; g < a.b; g += blockDim.x) s_cnt[g] = a.frame_cnt[g];
    __syncthreads();
    if (threadIdx.x == 0) {
        // the one small scan over the frames: a frame owns [acc, acc + its count) if that ends inside the arena; the first that does not,
        // and every frame after it, own nothing (their place would begin beyond it)
        long long acc = 0;
        bool open = true;
        int base = 0, fit = 0;
        if (f == 0) a.frame_first[0] = 0;
        for (int g = 0; g < a.b; ++g) {
            const bool fits = open && acc + s_cnt[g] <= (long long)a.cap_prims;
            if (g == f) { base = (int)acc; fit = fits ? 1 : 0; }
            if (fits) acc += s_cnt[g]; else open = false;
            if (f == 0) a.frame_first[g + 1] = (int)acc;
        }
        if (f == 0 && !open) a.flags[0] = 1;
        s_base = base; s_fit = fit;
    }
    __syncthreads();
    const int cam = a.cam_of_frame[f];
    if (!s_fit || cam < 0 || cam >= a.n_cam || s_cnt[f] == 0) return;               // (workgroup-uniform)
    frame_rows_setup(a, f, cam, fr);
    const double* poly = a.polygons + (size_t)cam * cc::CC_MAX_POINTS * 2;
    const double* dirs = a.dir_lines + (size_t)cam * cc::CC_MAX_DIRS * 4;
    const int* keys = a.dir_keys + (size_t)cam * cc::CC_MAX_DIRS;
    const int pn = a.poly_n[cam], n_dir = a.n_dir[cam], R = fr.row_base[a.n_labels];
    const int TP = text_on(a, cam) ? ob::text_parts(n_dir, a.n_labels) : 0, P = 1 + R + TP + 1;
    const int end = s_base + s_cnt[f];                                              // <= cap_prims: nothing below writes at or beyond it
    int carry = s_base;
    for (int p0 = 0; p0 < P; p0 += blockDim.x) {                                    // (workgroup-uniform loop)
        const int p = p0 + threadIdx.x;
        int cnt = 0, idx = -1, d = 0, pass = 0, seg = 0;
        if (p == 0) cnt = ob::count_anno(poly, pn, dirs, n_dir, keys);
        else if (p <= R) { idx = frame_row_index(a, fr, p - 1); cnt = a.row_cnt[idx]; }
        else if (p <= R + TP) {
            ob::text_part(p - 1 - R, a.n_labels, &d, &pass, &seg);
            cnt = ob::count_count_seg(keys[d], a.counts_before + ((size_t)cam * a.max_dir + d) * a.n_labels, pass, seg);
        } else if (p == P - 1) cnt = ob::count_frame_no(a.frame_no[f]);
        int total;
        const int at = carry + block_scan_inclusive(cnt, s_wave, &total) - cnt;
        if (cnt > 0 && at + cnt <= end) {
            ob::Out o{a.prims + (size_t)at * 12, 0};
            if (p == 0) ob::emit_anno(o, poly, pn, dirs, n_dir, keys);
            else if (p <= R) {
                const long long* row = a.rows + (size_t)idx * 6;
                const int64_t box[4] = {row[0], row[1], row[2], row[3]};
                // FIRST BOX: the row was kept by the zone test, so step 1 of live_count_apply_kernel for THIS batch has opened its slot
                // at the latest with this row -- `first` is the track's first in-zone box, never later than the row drawn.  It stays
                // readable after step 2 has closed a freed slot (open = 0 leaves `first` alone), and slots are not reused inside a
                // launch: this launch goes after the apply launch, before or after merge_free_kernel.
                const LiveSlot& s = a.slots[a.row_slot[idx]];
                const int64_t first[4] = {s.first[0], s.first[1], s.first[2], s.first[3]};
                ob::emit_row(o, a.h, a.w, box, first, row[4], row[5]);
            } else if (p <= R + TP) {
                // COUNTS BEFORE THE BATCH: counts_before was written by a read enqueued in front of this batch's apply launch
                ob::emit_count_seg(o, a.h, n_dir, d, keys[d], a.counts_before + ((size_t)cam * a.max_dir + d) * a.n_labels, pass, seg);
            } else ob::emit_frame_no(o, a.frame_no[f]);
        }
        carry += total;
    }
}

int launch_live_overlay(const LiveOverlayArgs& a, hipStream_t s) {
    VC_CHECK(a.b >= 1 && a.b <= LO_MAX_BATCH && a.n_labels >= 1 && a.n_labels <= LO_MAX_LABELS && a.cap_prims >= 0, VC_ERR_CAPACITY,
             "live overlay: %d frames (at most %d), %d labels (at most %d)", a.b, (int)LO_MAX_BATCH, a.n_labels, (int)LO_MAX_LABELS);
    hipLaunchKernelGGL(live_overlay_count_kernel, dim3(a.b), dim3(LO_THREADS), 0, s, a);
    hipLaunchKernelGGL(live_overlay_build_kernel, dim3(a.b), dim3(LO_THREADS), 0, s, a);
    VC_HIP(hipGetLastError());
    return VC_OK;
}

// live_count.hip
int live_pack_zones(int n_cam, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir, std::vector<double>& poly_out,
                    std::vector<double>& dirs_out, int* max_dir);
int launch_live_count_read(const LiveCountArgs& a, hipStream_t s);

// ---- the builder of a live counter ------------------------------------------------------------------------------------------------
struct LiveOverlay {
    int max_batch = 0, max_rows_per_frame = 0, depth = 0, cap_prims = 0;
    int* d_keys = nullptr; int* d_counts = nullptr; int* d_stats = nullptr;
    int* d_row_cnt = nullptr; size_t row_cnt_cap = 0;
    struct Buf {
        int* d_prims = nullptr; int* d_first = nullptr; int* d_frame_cnt = nullptr; int* d_flags = nullptr;
        char* h_meta = nullptr; char* d_meta = nullptr;     // frame_no[max_batch] int64 | cam_of_frame[max_batch] | text_cam[n_cam]
        int* h_res = nullptr;                               // pinned: [0] overflow flag, [1] frame_first[b]
        hipEvent_t built = nullptr;
        int b = 0, h = 0, w = 0;
        int state = 0;                                      // 0 free, 1 holds unconsumed lists, 2 being read by a render context
    } buf[4];
    std::deque<int> pending;                                // buffers in state 1, oldest first
    std::vector<void*> allocs;
};

namespace {

int free_buf(const LiveOverlay& o) {
    for (int i = 0; i < o.depth; ++i) if (o.buf[i].state == 0) return i;
    return -1;
}

// dir_keys concatenated per camera -> [n_cam][CC_MAX_DIRS]
int pack_keys(int n_cam, const int* n_dir, const int* dir_keys, std::vector<int>& out) {
    out.assign((size_t)n_cam * cc::CC_MAX_DIRS, 0);
    size_t k = 0;
    for (int c = 0; c < n_cam; ++c)
        for (int d = 0; d < n_dir[c]; ++d, ++k) {
            VC_CHECK(dir_keys[k] >= 0 && dir_keys[k] <= 99, VC_ERR_ARG, "camera %d: direction key %d outside 0..99 (a zone file names directions with two digits)", c, dir_keys[k]);
            out[(size_t)c * cc::CC_MAX_DIRS + d] = dir_keys[k];
        }
    return VC_OK;
}

}  // namespace

int live_overlay_room(vc_engine* e, const int* tracker_handles, int n) {
    for (int i = 0; i < n; ++i) {
        const int ts = tracker_slot(e->trackers, tracker_handles[i]);
        if (ts < 0 || !e->trackers[ts]->live || !e->trackers[ts]->live->ov) continue;
        const LiveOverlay& o = *e->trackers[ts]->live->ov;
        VC_CHECK(free_buf(o) >= 0, VC_ERR_STATE, "all %d overlay list buffers hold lists nobody has consumed (vc_live_overlay_lists / vc_render_submit_live + vc_render_collect)", o.depth);
    }
    return VC_OK;
}

int live_overlay_begin(vc_engine* e, const std::vector<int>& frame_trk, hipStream_t s, std::vector<LiveOverlayPlan>& plans) {
    plans.clear();
    for (vc_live* l : e->lives) {
        if (!l->ov) continue;
        bool used = false;
        for (int t : frame_trk) if (tracker_ok(e->trackers, t) && e->trackers[t]->live == l) { used = true; break; }
        if (!used) continue;
        VC_CHECK(free_buf(*l->ov) >= 0, VC_ERR_STATE, "all %d overlay list buffers hold lists nobody has consumed", l->ov->depth);
        VC_CHECK((int)frame_trk.size() <= l->ov->max_batch, VC_ERR_CAPACITY, "a batch of %d frames exceeds the overlay's max_batch %d", (int)frame_trk.size(), l->ov->max_batch);
        LiveOverlayPlan p{l, {}};
        for (long long done : l->frames_done) p.text_cam.push_back(done > 0 ? 1 : 0);       // the reference's prev_text = None before a camera's first frame
        // COUNTS BEFORE THE BATCH: base + open slots as they stand now, in front of this batch's apply launch, into the overlay's own tensor
        // (the counter's `counts` belongs to vc_live_counts*)
        LiveCountArgs ra = l->dev;
        ra.counts = l->ov->d_counts; ra.stats = l->ov->d_stats;
        VC_TRY(launch_live_count_read(ra, s));
        plans.push_back(std::move(p));
    }
    return VC_OK;
}

int live_overlay_finish(vc_engine* e, std::vector<LiveOverlayPlan>& plans, const std::vector<int>& frame_trk, const long long* frame_no,
                        const TrackBatchArgs* ta, int n_tasks, int b, int h, int w, hipStream_t s) {
    for (LiveOverlayPlan& p : plans) {
        vc_live* l = p.live;
        LiveOverlay& o = *l->ov;
        VC_CHECK(b <= o.max_batch, VC_ERR_CAPACITY, "a batch of %d frames exceeds the overlay's max_batch %d", b, o.max_batch);
        const int bi = free_buf(o);
        VC_CHECK(bi >= 0, VC_ERR_STATE, "all %d overlay list buffers hold lists nobody has consumed", o.depth);
        LiveOverlay::Buf& bf = o.buf[bi];
        const size_t rows_cap = ta ? (size_t)ta->rows_cap : 0;
        if (rows_cap > o.row_cnt_cap) {                      // like TrackStage::d_row_slot: the old block stays, a launch in flight may use it
            o.row_cnt_cap = rows_cap * 3 / 2;
            VC_TRY(dev_alloc(o.allocs, (void**)&o.d_row_cnt, o.row_cnt_cap * sizeof(int)));
        }
        long long* fno = (long long*)bf.h_meta;
        int* cam = (int*)(bf.h_meta + (size_t)o.max_batch * 8);
        int* tcam = cam + o.max_batch;
        for (int f = 0; f < b; ++f) {
            const int t = frame_trk[f];
            const bool mine = tracker_ok(e->trackers, t) && e->trackers[t]->live == l;
            cam[f] = mine ? e->trackers[t]->live_cam : -1;
            fno[f] = mine ? frame_no[f] : 0;
        }
        for (int c = 0; c < l->n_cam; ++c) tcam[c] = p.text_cam[c];
        const size_t meta_bytes = (size_t)o.max_batch * 12 + (size_t)l->n_cam * 4;
        VC_HIP(hipMemcpyAsync(bf.d_meta, bf.h_meta, meta_bytes, hipMemcpyHostToDevice, s));
        VC_HIP(hipMemsetAsync(bf.d_flags, 0, 16, s));
        LiveOverlayArgs a{};
        const LiveCountArgs& lc = l->dev;
        a.polygons = lc.polygons; a.poly_n = lc.poly_n; a.dir_lines = lc.dir_lines; a.n_dir = lc.n_dir; a.dir_keys = o.d_keys;
        a.n_cam = l->n_cam; a.n_labels = l->n_labels; a.max_dir = l->max_dir; a.owner = lc.owner; a.n_trackers = lc.n_trackers;
        a.slots = lc.slots; a.max_tracks = lc.max_tracks; a.counts_before = o.d_counts;
        a.frame_no = (const long long*)bf.d_meta; a.cam_of_frame = (const int*)(bf.d_meta + (size_t)o.max_batch * 8); a.text_cam = a.cam_of_frame + o.max_batch;
        if (ta) {
            a.tasks = ta->tasks; a.n_tasks = n_tasks; a.rows = ta->rows; a.row_slot = ta->row_slot; a.task_row_off = ta->task_row_off;
            a.task_row_n = ta->task_row_n; a.rows_cap = ta->rows_cap;
        }
        a.b = b; a.h = h; a.w = w;
        a.row_cnt = o.d_row_cnt; a.frame_cnt = bf.d_frame_cnt; a.prims = bf.d_prims; a.cap_prims = o.cap_prims; a.frame_first = bf.d_first; a.flags = bf.d_flags;
        VC_TRY(launch_live_overlay(a, s));
        VC_HIP(hipMemcpyAsync(bf.h_res, bf.d_flags, 4, hipMemcpyDeviceToHost, s));
        VC_HIP(hipMemcpyAsync(bf.h_res + 1, bf.d_first + b, 4, hipMemcpyDeviceToHost, s));
        VC_HIP(hipEventRecord(bf.built, s));
        bf.b = b; bf.h = h; bf.w = w; bf.state = 1;
        o.pending.push_back(bi);
    }
    return VC_OK;
}

int live_overlay_take(vc_live* l, int b, int h, int w, const void** d_prims, const int** d_first, hipEvent_t* built, int* token) {
    VC_CHECK(l->ov, VC_ERR_STATE, "the counter's overlay is not enabled (vc_live_overlay_enable)");
    LiveOverlay& o = *l->ov;
    VC_CHECK(!o.pending.empty(), VC_ERR_STATE, "no unconsumed overlay lists (a uniform tracker launch builds them)");
    LiveOverlay::Buf& bf = o.buf[o.pending.front()];
    VC_CHECK(bf.b == b && bf.h == h && bf.w == w, VC_ERR_ARG, "the oldest unconsumed lists are those of %d frames of %dx%d, not %d of %dx%d", bf.b, bf.h, bf.w, b, h, w);
    *d_prims = bf.d_prims; *d_first = bf.d_first; *built = bf.built; *token = o.pending.front();
    bf.state = 2;
    o.pending.pop_front();
    return VC_OK;
}

int live_overlay_release(vc_live* l, int token) {
    if (!l || !l->ov || token < 0 || token >= l->ov->depth || l->ov->buf[token].state != 2) return VC_OK;
    LiveOverlay::Buf& bf = l->ov->buf[token];
    bf.state = 0;
    VC_HIP(hipEventSynchronize(bf.built));                   // long past: the render batch behind it has completed
    VC_CHECK(bf.h_res[0] == 0, VC_ERR_CAPACITY, "a frame of the rendered batch did not fit the overlay arena (%d primitives): it and the frames after it were not annotated", l->ov->cap_prims);
    return VC_OK;
}

void live_overlay_free(vc_live* l) {
    if (!l->ov) return;
    render_forget_live(l->e, l);
    LiveOverlay* o = l->ov;
    for (LiveOverlay::Buf& bf : o->buf) {
        if (bf.h_meta) (void)hipHostFree(bf.h_meta);
        if (bf.h_res) (void)hipHostFree(bf.h_res);
        if (bf.built) (void)hipEventDestroy(bf.built);
    }
    for (void* p : o->allocs) (void)hipFree(p);
    delete o;
    l->ov = nullptr;
}

namespace {

// ---- what the two parity entries share: checks, and the batch in the form both builders read ---------------------------------------------
struct HostBatch {
    std::vector<double> poly, dirs;
    std::vector<int> keys;
    int max_dir = 0;
};

int host_check(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir, const int* dir_keys,
               int n_trackers, const int* tracker_cam, int max_tracks, const void* slots88, const int64_t* rows6, const int* row_slot, int n_rows,
               const int* tasks5, int n_tasks, const int64_t* frame_no, const int* cam_of_frame, int b, int h, int w, int32_t* prims12, int cap_prims,
               int32_t* frame_first, HostBatch& hb) {
    VC_CHECK(dir_keys && tracker_cam && slots88 && frame_no && cam_of_frame && frame_first && n_labels >= 1 && n_trackers >= 1 && max_tracks >= 1, VC_ERR_ARG, "bad argument");
    VC_CHECK(n_rows >= 0 && n_tasks >= 0 && (n_rows == 0 || (rows6 && row_slot)) && (n_tasks == 0 || tasks5) && cap_prims >= 0 && (cap_prims == 0 || prims12) &&
             h >= 1 && w >= 1, VC_ERR_ARG, "bad argument");
    VC_CHECK(b >= 1 && b <= LO_MAX_BATCH && n_labels <= LO_MAX_LABELS, VC_ERR_CAPACITY, "live overlay: %d frames (at most %d), %d labels (at most %d)", b,
             (int)LO_MAX_BATCH, n_labels, (int)LO_MAX_LABELS);
    VC_TRY(live_pack_zones(n_cam, polygons, poly_n, dir_lines, n_dir, hb.poly, hb.dirs, &hb.max_dir));
    VC_TRY(pack_keys(n_cam, n_dir, dir_keys, hb.keys));
    for (int i = 0; i < n_trackers; ++i) VC_CHECK(tracker_cam[i] >= -1 && tracker_cam[i] < n_cam, VC_ERR_ARG, "tracker %d: camera %d outside [-1, %d)", i, tracker_cam[i], n_cam);
    for (int f = 0; f < b; ++f) VC_CHECK(cam_of_frame[f] >= -1 && cam_of_frame[f] < n_cam, VC_ERR_ARG, "frame %d: camera %d outside [-1, %d)", f, cam_of_frame[f], n_cam);
    for (int i = 0; i < n_rows; ++i) VC_CHECK(row_slot[i] >= 0 && row_slot[i] < max_tracks, VC_ERR_ARG, "row %d: slot %d out of range", i, row_slot[i]);
    for (int t = 0; t < n_tasks; ++t) {
        const int* q = tasks5 + (size_t)t * 5;
        VC_CHECK(q[0] >= 0 && q[0] < n_trackers && q[1] >= 0 && q[1] < b && q[2] >= 0 && q[2] < n_labels && q[3] >= 0 && q[4] >= 0 && q[3] + q[4] <= n_rows, VC_ERR_ARG,
                 "task %d out of range", t);
        for (int u = 0; u < t; ++u) {
            const int* p = tasks5 + (size_t)u * 5;
            VC_CHECK(!(p[1] == q[1] && p[2] == q[2] && tracker_cam[p[0]] == tracker_cam[q[0]]), VC_ERR_ARG, "tasks %d and %d: a frame has one task per camera and label", u, t);
        }
    }
    return VC_OK;
}

}  // namespace

}  // namespace vc

using namespace vc;

extern "C" {

int vc_glyph_bits_host(int ch, uint64_t* bits) {
    VC_CHECK(bits, VC_ERR_ARG, "null argument");
    *bits = ob::glyph_bits(ch);
    return VC_OK;
}

// The lists of one batch through the CPU build of overlay_build.h: no HIP call.  Arguments as vc_live_overlay_host.
int vc_overlay_build_host(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir,
                          const int* dir_keys, int n_trackers, const int* tracker_cam, int max_tracks, const void* slots88,
                          const int32_t* counts_before, const int64_t* rows6, const int* row_slot, int n_rows, const int* tasks5, int n_tasks,
                          const int64_t* frame_no, const int* cam_of_frame, int b, int h, int w, int32_t* prims12, int cap_prims, int32_t* frame_first) {
    HostBatch hb;
    VC_TRY(host_check(n_cam, n_labels, polygons, poly_n, dir_lines, n_dir, dir_keys, n_trackers, tracker_cam, max_tracks, slots88, rows6, row_slot, n_rows, tasks5,
                      n_tasks, frame_no, cam_of_frame, b, h, w, prims12, cap_prims, frame_first, hb));
    const LiveSlot* slots = (const LiveSlot*)slots88;
    std::vector<int32_t> one;
    std::vector<int64_t> rows, first;
    std::vector<unsigned char> keep;
    long long acc = 0;
    bool open = true;
    frame_first[0] = 0;
    for (int f = 0; f < b; ++f) {
        const int cam = cam_of_frame[f];
        one.clear();
        if (cam >= 0) {
            const double* poly = hb.poly.data() + (size_t)cam * cc::CC_MAX_POINTS * 2;
            rows.clear(); first.clear(); keep.clear();
            for (int label = 0; label < n_labels; ++label)                  // the frame's tasks, labels ascending
                for (int t = 0; t < n_tasks; ++t) {
                    const int* q = tasks5 + (size_t)t * 5;
                    if (q[1] != f || q[2] != label || tracker_cam[q[0]] != cam) continue;
                    for (int i = q[3]; i < q[3] + q[4]; ++i) {
                        rows.insert(rows.end(), rows6 + (size_t)i * 6, rows6 + (size_t)i * 6 + 6);
                        first.insert(first.end(), slots[row_slot[i]].first, slots[row_slot[i]].first + 4);
                        keep.push_back(cc::box_in_polygon(poly, poly_n[cam], rows6 + (size_t)i * 6) ? 1 : 0);
                    }
                }
            const int32_t* counts_cam = counts_before ? counts_before + (size_t)cam * hb.max_dir * n_labels : nullptr;
            const double* dirs = hb.dirs.data() + (size_t)cam * cc::CC_MAX_DIRS * 4;
            const int* keys = hb.keys.data() + (size_t)cam * cc::CC_MAX_DIRS;
            ob::Out cnt{nullptr, 0};
            ob::emit_frame(cnt, h, w, poly, poly_n[cam], dirs, n_dir[cam], keys, n_labels, counts_cam, rows.data(), first.data(), keep.data(), (int)keep.size(), frame_no[f]);
            one.resize((size_t)cnt.n * 12 + 4);
            int32_t* al = one.data();
            while ((uintptr_t)al & 15) ++al;
            ob::Out o{al, 0};
            ob::emit_frame(o, h, w, poly, poly_n[cam], dirs, n_dir[cam], keys, n_labels, counts_cam, rows.data(), first.data(), keep.data(), (int)keep.size(), frame_no[f]);
            if (open && acc + o.n <= (long long)cap_prims) {
                memcpy(prims12 + (size_t)acc * 12, al, (size_t)o.n * 48);
                acc += o.n;
            } else open = false;
        }
        frame_first[f + 1] = (int32_t)acc;
    }
    VC_CHECK(open, VC_ERR_CAPACITY, "the lists need more than %d primitives: the first frame that did not fit and every later one own nothing", cap_prims);
    return VC_OK;
}

// One launch of live_overlay_count_kernel and one of live_overlay_build_kernel on host arrays (tests/test_gpu_live_overlay.py): zones
// as for vc_live_create, dir_keys as for vc_live_overlay_enable; slots88 the per-slot records AFTER the batch's apply launch; counts_before
// [n_cam][max_dir][n_labels] or NULL for "no text"; the batch as for vc_live_count_host, with the camera of every frame.  prims12
// receives the whole arena (cap_prims x 12, what no frame owns keeps the byte 0xA5), frame_first b + 1 entries.
int vc_live_overlay_host(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir,
                         const int* dir_keys, int n_trackers, const int* tracker_cam, int max_tracks, const void* slots88,
                         const int32_t* counts_before, const int64_t* rows6, const int* row_slot, int n_rows, const int* tasks5, int n_tasks,
                         const int64_t* frame_no, const int* cam_of_frame, int b, int h, int w, int32_t* prims12, int cap_prims, int32_t* frame_first) {
    HostBatch hb;
    VC_TRY(host_check(n_cam, n_labels, polygons, poly_n, dir_lines, n_dir, dir_keys, n_trackers, tracker_cam, max_tracks, slots88, rows6, row_slot, n_rows, tasks5,
                      n_tasks, frame_no, cam_of_frame, b, h, w, prims12, cap_prims, frame_first, hb));
    std::vector<TrackTask> tasks(std::max(n_tasks, 1));
    std::vector<int> off(std::max(n_tasks, 1)), cnt(std::max(n_tasks, 1));
    for (int t = 0; t < n_tasks; ++t) {
        const int* q = tasks5 + (size_t)t * 5;
        tasks[t] = TrackTask{q[0], 0, 0, q[1], q[2], 0, 0, 0};
        off[t] = q[3]; cnt[t] = q[4];
    }
    const int n = n_cam * hb.max_dir * n_labels;
    const long long zero = 0;
    DevScratch mem;
    GuardedOut g_prims, g_first, g_fcnt, g_rcnt, g_flags;
    LiveOverlayArgs a{};
    double *d_poly = nullptr, *d_dirs = nullptr;
    int *d_pn = nullptr, *d_nd = nullptr, *d_keys = nullptr, *d_owner = nullptr, *d_rslot = nullptr, *d_off = nullptr, *d_cnt = nullptr, *d_cam = nullptr, *d_counts = nullptr;
    long long *d_rows = nullptr, *d_fno = nullptr;
    TrackTask* d_tasks = nullptr;
    LiveSlot* d_slots = nullptr;
    VC_TRY(mem.upload(&d_poly, hb.poly.data(), hb.poly.size() * 8));
    VC_TRY(mem.upload(&d_dirs, hb.dirs.data(), hb.dirs.size() * 8));
    VC_TRY(mem.upload(&d_pn, poly_n, (size_t)n_cam * 4));
    VC_TRY(mem.upload(&d_nd, n_dir, (size_t)n_cam * 4));
    VC_TRY(mem.upload(&d_keys, hb.keys.data(), hb.keys.size() * 4));
    VC_TRY(mem.upload(&d_owner, tracker_cam, (size_t)n_trackers * 4));
    VC_TRY(mem.upload(&d_slots, slots88, (size_t)max_tracks * sizeof(LiveSlot)));
    if (counts_before) VC_TRY(mem.upload(&d_counts, counts_before, (size_t)n * 4));
    VC_TRY(mem.upload(&d_rows, n_rows ? (const void*)rows6 : (const void*)&zero, std::max((size_t)n_rows * 48, (size_t)8)));
    VC_TRY(mem.upload(&d_rslot, n_rows ? (const void*)row_slot : (const void*)&zero, std::max((size_t)n_rows * 4, (size_t)4)));
    VC_TRY(mem.upload(&d_tasks, tasks.data(), tasks.size() * sizeof(TrackTask)));
    VC_TRY(mem.upload(&d_off, off.data(), off.size() * 4));
    VC_TRY(mem.upload(&d_cnt, cnt.data(), cnt.size() * 4));
    VC_TRY(mem.upload(&d_fno, frame_no, (size_t)b * 8));
    VC_TRY(mem.upload(&d_cam, cam_of_frame, (size_t)b * 4));
    VC_TRY(g_prims.alloc(mem, (size_t)cap_prims * 48));
    VC_TRY(g_first.alloc(mem, (size_t)(b + 1) * 4));
    VC_TRY(g_fcnt.alloc(mem, (size_t)b * 4));
    VC_TRY(g_rcnt.alloc(mem, std::max((size_t)n_rows * 4, (size_t)4)));
    const int no_flag[4] = {0, 0, 0, 0};
    VC_TRY(g_flags.alloc(mem, 16, no_flag));
    a.polygons = d_poly; a.poly_n = d_pn; a.dir_lines = d_dirs; a.n_dir = d_nd; a.dir_keys = d_keys; a.n_cam = n_cam; a.n_labels = n_labels; a.max_dir = hb.max_dir;
    a.owner = d_owner; a.n_trackers = n_trackers; a.slots = d_slots; a.max_tracks = max_tracks; a.counts_before = d_counts; a.text_cam = nullptr;
    a.tasks = d_tasks; a.n_tasks = n_tasks; a.rows = d_rows; a.row_slot = d_rslot; a.task_row_off = d_off; a.task_row_n = d_cnt; a.rows_cap = n_rows;
    a.frame_no = d_fno; a.cam_of_frame = d_cam; a.b = b; a.h = h; a.w = w;
    a.row_cnt = g_rcnt.as<int>(); a.frame_cnt = g_fcnt.as<int>(); a.prims = g_prims.as<int>(); a.cap_prims = cap_prims; a.frame_first = g_first.as<int>(); a.flags = g_flags.as<int>();
    VC_TRY(launch_live_overlay(a, nullptr));
    VC_TRY(kernel_wait("live_overlay kernels"));
    std::vector<int> scratch(std::max((size_t)n_rows, (size_t)b) + 4);
    int flags[4];
    VC_TRY(g_rcnt.read_back(scratch.data(), "live_overlay_count_kernel (row counts)"));
    VC_TRY(g_fcnt.read_back(scratch.data(), "live_overlay_count_kernel (frame counts)"));
    VC_TRY(g_flags.read_back(flags, "live_overlay_build_kernel (flags)"));
    VC_TRY(g_first.read_back(frame_first, "live_overlay_build_kernel (frame_first)"));
    if (cap_prims) VC_TRY(g_prims.read_back(prims12, "live_overlay_build_kernel (prims)"));
    VC_CHECK(flags[0] == 0, VC_ERR_CAPACITY, "the lists need more than %d primitives: the first frame that did not fit and every later one own nothing", cap_prims);
    return VC_OK;
}

int vc_live_overlay_enable(vc_live* l, const int* dir_keys, int max_batch, int max_rows_per_frame, int depth) {
    VC_CHECK(l && dir_keys, VC_ERR_ARG, "null argument");
    VC_CHECK(!l->ov, VC_ERR_STATE, "vc_live_overlay_enable: the counter's overlay is enabled already");
    VC_CHECK(depth >= 1 && depth <= 4, VC_ERR_ARG, "depth (list buffers) must be 1..4, got %d", depth);
    VC_CHECK(max_batch >= 1 && max_rows_per_frame >= 0, VC_ERR_ARG, "bad capacity: %d frames of %d rows", max_batch, max_rows_per_frame);
    VC_CHECK(max_batch <= LO_MAX_BATCH && l->n_labels <= LO_MAX_LABELS, VC_ERR_CAPACITY, "live overlay: %d frames (at most %d), %d labels (at most %d)", max_batch,
             (int)LO_MAX_BATCH, l->n_labels, (int)LO_MAX_LABELS);
    std::vector<int> keys;
    VC_TRY(pack_keys(l->n_cam, l->n_dir.data(), dir_keys, keys));
    vc_engine* e = l->e;
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));                 // batches in flight were launched without the overlay
    VC_HIP(hipStreamSynchronize(e->stream));
    // the arena holds max_batch frames of the largest anno, max_rows_per_frame rows of the longest id and label, the count text at ten
    // digits per count and a nineteen-digit frame number
    long long per_frame = 0;
    {
        std::vector<double> poly((size_t)l->n_cam * cc::CC_MAX_POINTS * 2), dirs((size_t)l->n_cam * cc::CC_MAX_DIRS * 4);
        std::vector<int> pn(l->n_cam);
        VC_HIP(hipMemcpy(poly.data(), l->dev.polygons, poly.size() * 8, hipMemcpyDeviceToHost));
        VC_HIP(hipMemcpy(dirs.data(), l->dev.dir_lines, dirs.size() * 8, hipMemcpyDeviceToHost));
        VC_HIP(hipMemcpy(pn.data(), l->dev.poly_n, pn.size() * 4, hipMemcpyDeviceToHost));
        const std::vector<int32_t> big((size_t)l->n_labels, INT32_MAX);
        for (int c = 0; c < l->n_cam; ++c) {
            long long n = ob::count_anno(poly.data() + (size_t)c * cc::CC_MAX_POINTS * 2, pn[c], dirs.data() + (size_t)c * cc::CC_MAX_DIRS * 4, l->n_dir[c], keys.data() + (size_t)c * cc::CC_MAX_DIRS);
            for (int part = 0; part < ob::text_parts(l->n_dir[c], l->n_labels); ++part) {
                int d, pass, seg;
                ob::text_part(part, l->n_labels, &d, &pass, &seg);
                n += ob::count_count_seg(keys[(size_t)c * cc::CC_MAX_DIRS + d], big.data(), pass, seg);
            }
            per_frame = std::max(per_frame, n);
        }
        per_frame += (long long)max_rows_per_frame * ob::count_row(INT64_MAX, l->n_labels - 1) + ob::count_frame_no(INT64_MAX);
    }
    VC_CHECK(per_frame * max_batch < (1ll << 26), VC_ERR_CAPACITY, "an overlay arena of %d frames x %lld primitives is out of range", max_batch, per_frame);
    LiveOverlay* o = new LiveOverlay();
    o->max_batch = max_batch; o->max_rows_per_frame = max_rows_per_frame; o->depth = depth; o->cap_prims = (int)(per_frame * max_batch);
    l->ov = o;
    auto fail = [&](int code) { live_overlay_free(l); return code; };
    const size_t n = (size_t)l->n_cam * l->max_dir * l->n_labels, meta = (size_t)max_batch * 12 + (size_t)l->n_cam * 4;
    int rc = VC_OK;
    if ((rc = dev_alloc(o->allocs, (void**)&o->d_keys, keys.size() * 4)) || (rc = dev_alloc(o->allocs, (void**)&o->d_counts, n * 4)) ||
        (rc = dev_alloc(o->allocs, (void**)&o->d_stats, 64)))
        return fail(rc);
    if (hipMemcpy(o->d_keys, keys.data(), keys.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_error("hipMemcpy failed for the overlay's direction keys"); return fail(VC_ERR_HIP); }
    for (int i = 0; i < depth; ++i) {
        LiveOverlay::Buf& bf = o->buf[i];
        if ((rc = dev_alloc(o->allocs, (void**)&bf.d_prims, std::max((size_t)o->cap_prims * 48, (size_t)48))) ||
            (rc = dev_alloc(o->allocs, (void**)&bf.d_first, (size_t)(max_batch + 1) * 4)) || (rc = dev_alloc(o->allocs, (void**)&bf.d_frame_cnt, (size_t)max_batch * 4)) ||
            (rc = dev_alloc(o->allocs, (void**)&bf.d_flags, 16)) || (rc = dev_alloc(o->allocs, (void**)&bf.d_meta, meta)))
            return fail(rc);
        if (hipHostMalloc((void**)&bf.h_meta, meta) != hipSuccess || hipHostMalloc((void**)&bf.h_res, 16) != hipSuccess ||
            hipEventCreateWithFlags(&bf.built, hipEventDisableTiming) != hipSuccess) {
            set_error("overlay list buffer %d: pinned memory / event create failed: %s", i, hipGetErrorString(hipGetLastError()));
            return fail(VC_ERR_HIP);
        }
    }
    return VC_OK;
}

int vc_live_overlay_lists(vc_live* l, int32_t* prims12, int cap_prims, int32_t* frame_first, int cap_frames, int* b, int* n_prims) {
    VC_CHECK(l && frame_first && b && n_prims && (cap_prims == 0 || prims12), VC_ERR_ARG, "null argument");
    VC_CHECK(l->ov, VC_ERR_STATE, "the counter's overlay is not enabled (vc_live_overlay_enable)");
    LiveOverlay& o = *l->ov;
    VC_CHECK(!o.pending.empty(), VC_ERR_STATE, "no unconsumed overlay lists (a uniform tracker launch builds them)");
    LiveOverlay::Buf& bf = o.buf[o.pending.front()];
    VC_HIP(hipSetDevice(l->e->cfg.device));
    VC_HIP(hipEventSynchronize(bf.built));
    const int n = bf.h_res[1];
    VC_CHECK(bf.b <= cap_frames && n <= cap_prims, VC_ERR_ARG, "the oldest lists hold %d frames and %d primitives, room for %d and %d", bf.b, n, cap_frames, cap_prims);
    bf.state = 0;                                            // consumed, whatever follows
    o.pending.pop_front();
    VC_CHECK(bf.h_res[0] == 0, VC_ERR_CAPACITY, "a frame of the batch did not fit the overlay arena (%d primitives)", o.cap_prims);
    if (n) VC_HIP(hipMemcpy(prims12, bf.d_prims, (size_t)n * 48, hipMemcpyDeviceToHost));
    VC_HIP(hipMemcpy(frame_first, bf.d_first, (size_t)(bf.b + 1) * 4, hipMemcpyDeviceToHost));
    *b = bf.b; *n_prims = n;
    return VC_OK;
}

}  // extern "C"
