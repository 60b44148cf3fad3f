// Checkpoint of a live counter: device-packed snapshot and resume of a stream (vc_live_checkpoint* / vc_live_restore).
//
// The blob (live_ckpt.h) holds everything the counter's trackers and the counter read from now on.  It is packed ON THE DEVICE IN STREAM
// ORDER, behind the batches enqueued so far, without draining the pipeline:
//
//   e->stream   ... track_batch_kernel, live_count_apply_kernel (batch n) | upload(frames_done, params) | plan | pack | event P | batch n+1 ...
//   copy stream                                                             wait P | copy kernel: staging -> pinned (blob, info) | event C
//
//   live_ckpt_plan_kernel    ONE workgroup: walks the counter's trackers (hdrs[t].n_tracks, the list, every record's gal_count), scans the
//                            track counts and then the section sizes (a chunk per thread, the chunk sums in LDS) into the per-track offset table, writes header, camera, stats and tracker sections and the
//                            total.  A total beyond the staging capacity: the overflow flag, and nothing beyond the header.
//   live_ckpt_pack_kernel    grid-wide, a workgroup per track: record, mean, covariance, LiveSlot and the valid gallery rows from the
//                            scattered pool slots to their offsets, 16 bytes per lane (a 2 KB gallery row = 128 lanes, fully coalesced).
//   live_ckpt_copy_kernel    on the copy stream: the blob's `total` bytes -- the size lives on the device, the host's bound on it (a track per
//                            detection in flight) is tens of times larger -- from the staging buffer into mapped pinned memory, 16 bytes per
//                            lane, and the info block behind them.  A few workgroups: the PCIe link bounds it, not the CUs.
//   live_ckpt_unpack_kernel  the reverse, driven by the slot table the host builds from the validated blob; also lists, hdrs, recs, the
//                            counter's slots[] and base.
//
// Why the order is enough: plan and pack read the pool, the lists and the counter's records on the stream that alone writes them, so they
// see exactly the state behind the last enqueued tracker launch and its apply launch; the next tracker launch may overwrite the pool as
// soon as pack has finished, which the same stream guarantees.  The copy to the host waits for event P on a stream of its own and reads
// only the staging buffer, which nothing writes until the next vc_live_checkpoint_begin -- refused until vc_live_checkpoint_end has
// waited for event C.  No call here synchronises the tracker stream except vc_live_restore, which is rare and drains first.
#include <algorithm>
#include <cstring>

#include "engine.h"
#include "track_core.h"

#pragma clang fp contract(off)

#include "live_ckpt.h"

namespace vc {

using namespace ck;

static_assert(sizeof(tc::TrackerHdr) == sizeof(CkptHdr) && offsetof(tc::TrackerHdr, next_id) == offsetof(CkptHdr, next_id) &&
              offsetof(tc::TrackerHdr, n_tracks) == offsetof(CkptHdr, n_tracks) && offsetof(tc::TrackerHdr, nn_budget) == offsetof(CkptHdr, nn_budget) &&
              offsetof(tc::TrackerHdr, err) == offsetof(CkptHdr, err), "CkptHdr mirrors tc::TrackerHdr");
static_assert(sizeof(tc::TrackRecD) == sizeof(CkptRec) && offsetof(tc::TrackRecD, gal_head) == offsetof(CkptRec, gal_head), "CkptRec mirrors tc::TrackRecD");
static_assert((int)tc::TENTATIVE == CK_TENTATIVE && (int)tc::CONFIRMED == CK_CONFIRMED && (int)tc::TERR_TABLE == CK_TERR_LAST && VC_FEAT_DIM == CK_FEAT_DIM, "checkpoint constants");

// one track of the offset table the plan kernel leaves for the pack kernel
struct CkptPackRef { unsigned long long off; int slot, rows; };
// info block: what the host reads beside the blob
struct CkptInfo { unsigned long long total; int overflow, n_tracks; };

enum { CKPT_PLAN_THREADS = 1024, CKPT_COPY_THREADS = 256, CKPT_PACK_BLOCKS = 512, CKPT_D2H_BLOCKS = 64 };

__global__ __launch_bounds__(CKPT_PLAN_THREADS) void live_ckpt_plan_kernel(const CkptView v, char* blob, unsigned long long cap, CkptPackRef* table,
                                                                           int* trk_first, CkptInfo* info) {
    __shared__ unsigned long long part[CKPT_PLAN_THREADS];
    const int tid = threadIdx.x, n_trk = v.n_cam * v.n_labels;
    // first table entry of every tracker: a chunk of trackers per thread, the chunks' sums scanned in LDS
    auto tracks_of = [&](int t) { const int k = v.hdrs[v.trackers[t]].n_tracks; return k < 0 ? 0 : (k > v.list_cap ? v.list_cap : k); };
    const int tchunk = (n_trk + CKPT_PLAN_THREADS - 1) / CKPT_PLAN_THREADS;
    const int t0 = min(tid * tchunk, n_trk), t1 = min(t0 + tchunk, n_trk);
    {
        int cnt = 0;
        for (int t = t0; t < t1; ++t) cnt += tracks_of(t);
        part[tid] = (unsigned long long)cnt;
        __syncthreads();
        if (tid == 0) {
            unsigned long long o = 0;
            for (int j = 0; j < CKPT_PLAN_THREADS; ++j) { const unsigned long long b = part[j]; part[j] = o; o += b; }
        }
        __syncthreads();
        int o = (int)part[tid];
        for (int t = t0; t < t1; ++t) { trk_first[t] = o; o += tracks_of(t); }
        if (tid == CKPT_PLAN_THREADS - 1) trk_first[n_trk] = o;       // its chunk is the last one, or empty behind the last
    }
    __syncthreads();
    const int n = trk_first[n_trk];
    for (int i = tid; i < n; i += CKPT_PLAN_THREADS) {                 // slot and gallery rows of every track
        int lo = 0, hi = n_trk - 1;                                    // the last tracker whose first entry is <= i
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (trk_first[mid] <= i) lo = mid; else hi = mid - 1; }
        const int tr = v.trackers[lo];
        int slot = v.lists[(size_t)tr * v.list_cap + (i - trk_first[lo])];
        int rows = 0;
        if (slot < 0 || slot >= v.max_tracks) slot = -1;               // never: the section is then written as zeros
        else rows = ckpt_track_rows(v.recs[slot].gal_count, v.hdrs[tr].nn_budget < v.budget_cap ? v.hdrs[tr].nn_budget : v.budget_cap);
        table[i].slot = slot; table[i].rows = rows;
    }
    __syncthreads();
    const int chunk = (n + CKPT_PLAN_THREADS - 1) / CKPT_PLAN_THREADS;
    const int i0 = min(tid * chunk, n), i1 = min(i0 + chunk, n);
    unsigned long long mine = 0;
    for (int i = i0; i < i1; ++i) mine += ckpt_track_bytes(table[i].rows);
    part[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        unsigned long long o = ckpt_tracks_off(v.n_cam, v.max_dir, v.n_labels);
        for (int j = 0; j < CKPT_PLAN_THREADS; ++j) { const unsigned long long b = part[j]; part[j] = o; o += b; }
        info->total = o; info->overflow = o > cap ? 1 : 0; info->n_tracks = n;
        ckpt_put_header(blob, v, n, o);
    }
    __syncthreads();
    unsigned long long o = part[tid];
    for (int i = i0; i < i1; ++i) { table[i].off = o; o += ckpt_track_bytes(table[i].rows); }
    if (info->overflow) return;                                        // written by thread 0 in front of the barrier above
    for (int c = tid; c < v.n_cam; c += CKPT_PLAN_THREADS) ckpt_put_camera(blob, v, c);
    if (tid == CKPT_PLAN_THREADS - 1) ckpt_put_stats(blob, v);
    for (int t = tid; t < n_trk; t += CKPT_PLAN_THREADS) ckpt_put_tracker(blob, v, t);
}

__device__ __forceinline__ void copy16(char* dst, const char* src, size_t n_vec) {
    const uint4* s = (const uint4*)src;
    uint4* d = (uint4*)dst;
    for (size_t k = threadIdx.x; k < n_vec; k += CKPT_COPY_THREADS) d[k] = s[k];
}

__global__ __launch_bounds__(CKPT_COPY_THREADS) void live_ckpt_pack_kernel(const CkptView v, char* blob, const CkptPackRef* table, const CkptInfo* info) {
    if (info->overflow) return;
    const int n = info->n_tracks;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {                  // block-uniform
        const CkptPackRef r = table[i];
        char* o = blob + r.off;
        if (r.slot < 0) { for (int k = threadIdx.x; k < (int)(sizeof(CkptTrack) / 16); k += CKPT_COPY_THREADS) ((uint4*)o)[k] = uint4{0, 0, 0, 0}; continue; }
        // what ckpt_put_track_head writes, by lanes: the record as two 16-byte words (wave 0), the LiveSlot as eleven 8-byte words, zero
        // unless open, and the padding word behind it (wave 1)
        if (threadIdx.x < 2) ((uint4*)o)[threadIdx.x] = ((const uint4*)(v.recs + r.slot))[threadIdx.x];
        else if (threadIdx.x >= 64 && threadIdx.x < 76) {
            const int w = threadIdx.x - 64;
            const unsigned long long* s = (const unsigned long long*)(v.slots + r.slot);
            ((unsigned long long*)(o + offsetof(CkptTrack, slot)))[w] = (w < 11 && v.slots[r.slot].open) ? s[w] : 0ull;
        }
        copy16(o + offsetof(CkptTrack, mean), (const char*)(v.mean + (size_t)r.slot * 8), 4);
        copy16(o + offsetof(CkptTrack, cov), (const char*)(v.cov + (size_t)r.slot * 64), 32);
        copy16(o + sizeof(CkptTrack), (const char*)(v.gallery + (size_t)r.slot * v.budget_cap * CK_FEAT_DIM), (size_t)r.rows * (CK_ROW_BYTES / 16));
    }
}

// staging -> mapped pinned memory, exactly the blob (nothing but the header after an overflow); the info block for the host
__global__ __launch_bounds__(CKPT_COPY_THREADS) void live_ckpt_copy_kernel(const char* stage, char* host_blob, const CkptInfo* info, CkptInfo* host_info) {
    const unsigned long long bytes = info->overflow ? sizeof(CkptHeader) : info->total;
    const size_t n_vec = (size_t)(bytes / 16);                         // every section is a multiple of 16 bytes
    const uint4* s = (const uint4*)stage;
    uint4* d = (uint4*)host_blob;
    for (size_t k = (size_t)blockIdx.x * CKPT_COPY_THREADS + threadIdx.x; k < n_vec; k += (size_t)gridDim.x * CKPT_COPY_THREADS) d[k] = s[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) *host_info = *info;
}

// what the unpack kernel does beside the tracks: tracker headers, bases, the retired count, slots to close (old tracks whose slot no new track took)
struct CkptUnpackMisc {
    const int* trk_map;      // [b_n_cam * n_labels] tracker (pool index) of every blob tracker, -1 = not restored
    const int* cam_map;      // [b_n_cam] the counter's camera of every blob camera, -1 = not restored
    const int* close; int n_close;
    int b_n_cam, b_max_dir, n_tracks;
    int set_retired;         // the restore covers the whole counter from the whole blob: the retired count becomes the blob's
};

__global__ __launch_bounds__(CKPT_COPY_THREADS) void live_ckpt_unpack_kernel(const CkptView v, const char* blob, const CkptUnpackRef* table, const CkptUnpackMisc m) {
    for (int i = blockIdx.x; i < m.n_tracks + 1; i += gridDim.x) {     // block-uniform
        if (i == m.n_tracks) {
            for (int t = threadIdx.x; t < m.b_n_cam * v.n_labels; t += CKPT_COPY_THREADS)
                if (m.trk_map[t] >= 0) ckpt_get_tracker(blob, t, m.b_n_cam, m.b_max_dir, v.n_labels, v.hdrs[m.trk_map[t]]);
            for (int c = threadIdx.x; c < m.b_n_cam; c += CKPT_COPY_THREADS)
                if (m.cam_map[c] >= 0) ckpt_get_base(blob, c, m.b_max_dir, v.n_labels, m.cam_map[c], v);
            if (threadIdx.x == 0 && m.set_retired) v.stats[1] = ckpt_load<CkptStats>(blob + ckpt_stats_off(m.b_n_cam, m.b_max_dir, v.n_labels)).retired;
            for (int k = threadIdx.x; k < m.n_close; k += CKPT_COPY_THREADS) v.slots[m.close[k]] = cc::LiveSlot{};
            continue;
        }
        const CkptUnpackRef r = table[i];
        const char* o = blob + r.off;
        // what ckpt_get_track_head does, by lanes: record, LiveSlot (word 0 = open | cam << 32: an open record takes the counter's camera), list entry
        if (threadIdx.x < 2) ((uint4*)(v.recs + r.slot))[threadIdx.x] = ((const uint4*)o)[threadIdx.x];
        else if (threadIdx.x >= 64 && threadIdx.x < 75) {
            const int w = threadIdx.x - 64;
            unsigned long long x = ((const unsigned long long*)(o + offsetof(CkptTrack, slot)))[w];
            if (w == 0 && (unsigned)x) x = (x & 0xffffffffull) | ((unsigned long long)(unsigned)r.cam << 32);
            ((unsigned long long*)(v.slots + r.slot))[w] = x;
        } else if (threadIdx.x == 128) v.lists[(size_t)r.tracker * v.list_cap + r.pos] = r.slot;
        copy16((char*)(v.mean + (size_t)r.slot * 8), o + offsetof(CkptTrack, mean), 4);
        copy16((char*)(v.cov + (size_t)r.slot * 64), o + offsetof(CkptTrack, cov), 32);
        copy16((char*)(v.gallery + (size_t)r.slot * v.budget_cap * CK_FEAT_DIM), o + sizeof(CkptTrack), (size_t)r.rows * (CK_ROW_BYTES / 16));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct LiveCkpt {
    size_t max_bytes = 0;
    char* d_stage = nullptr; char* h_blob = nullptr; char* hd_blob = nullptr;   // device staging; pinned host copy and its device address
    CkptPackRef* d_table = nullptr; int* d_trk_first = nullptr; int* d_trackers = nullptr;
    CkptInfo* d_info = nullptr; CkptInfo* h_info = nullptr; CkptInfo* hd_info = nullptr;
    char* d_up = nullptr; char* h_up = nullptr; size_t up_bytes = 0;   // frames_done[n_cam] int64 | params[n_cam * n_labels]
    hipEvent_t packed = nullptr, copied = nullptr;
    hipStream_t cstream = nullptr;
    bool in_flight = false;
    std::vector<void*> allocs;
};

static CkptView ckpt_view(const vc_live* l) {
    const vc_engine* e = l->e;
    CkptView v{};
    v.hdrs = (CkptHdr*)e->d_hdrs; v.lists = e->d_lists; v.list_cap = e->list_cap; v.recs = (CkptRec*)e->d_recs;
    v.mean = e->pool.mean; v.cov = e->pool.cov; v.gallery = e->pool.gallery; v.budget_cap = e->pool.budget_cap; v.max_tracks = e->pool.max_tracks;
    v.slots = l->dev.slots; v.base = l->dev.base; v.stats = l->dev.stats;
    v.polygons = l->dev.polygons; v.poly_n = l->dev.poly_n; v.dir_lines = l->dev.dir_lines; v.n_dir = l->dev.n_dir;
    v.n_cam = l->n_cam; v.n_labels = l->n_labels; v.max_dir = l->max_dir;
    if (l->ck) {
        v.trackers = l->ck->d_trackers;
        v.frames_done = (const long long*)l->ck->d_up;
        v.params = (const CkptHostParams*)(l->ck->d_up + (size_t)l->n_cam * 8);
    }
    return v;
}

void live_ckpt_free(vc_live* l) {
    LiveCkpt* c = l->ck;
    if (!c) return;
    if (c->cstream) (void)hipStreamSynchronize(c->cstream);           // a checkpoint in flight: its copy reads the staging buffer
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->h_blob) (void)hipHostFree(c->h_blob);
    if (c->h_info) (void)hipHostFree(c->h_info);
    if (c->h_up) (void)hipHostFree(c->h_up);
    if (c->packed) (void)hipEventDestroy(c->packed);
    if (c->copied) (void)hipEventDestroy(c->copied);
    if (c->cstream) (void)hipStreamDestroy(c->cstream);
    delete c;
    l->ck = nullptr;
}

static int ckpt_enable(vc_live* l, size_t max_bytes) {
    vc_engine* e = l->e;
    const int n_trk = l->n_cam * l->n_labels;
    const size_t fixed = (size_t)ckpt_fixed_bytes(l->n_cam, l->max_dir, l->n_labels);
    VC_CHECK(max_bytes >= fixed, VC_ERR_CAPACITY, "max_bytes %zu: the sections of %d cameras x %d labels alone take %zu bytes", max_bytes, l->n_cam, l->n_labels, fixed);
    LiveCkpt* c = l->ck = new LiveCkpt();
    c->max_bytes = (max_bytes + 15) & ~(size_t)15;
    c->up_bytes = (size_t)l->n_cam * 8 + (size_t)n_trk * sizeof(CkptHostParams);
    VC_TRY(dev_alloc(c->allocs, (void**)&c->d_stage, c->max_bytes));
    VC_TRY(dev_alloc(c->allocs, (void**)&c->d_table, (size_t)n_trk * e->list_cap * sizeof(CkptPackRef)));
    VC_TRY(dev_alloc(c->allocs, (void**)&c->d_trk_first, (size_t)(n_trk + 1) * sizeof(int)));
    VC_TRY(dev_alloc(c->allocs, (void**)&c->d_trackers, (size_t)n_trk * sizeof(int)));
    VC_TRY(dev_alloc(c->allocs, (void**)&c->d_info, 64));
    VC_TRY(dev_alloc(c->allocs, (void**)&c->d_up, c->up_bytes));
    VC_HIP(hipMemcpy(c->d_trackers, l->trackers.data(), (size_t)n_trk * sizeof(int), hipMemcpyHostToDevice));
    VC_HIP(hipHostMalloc((void**)&c->h_blob, c->max_bytes));
    VC_HIP(hipHostMalloc((void**)&c->h_info, 64));
    VC_HIP(hipHostGetDevicePointer((void**)&c->hd_blob, c->h_blob, 0));
    VC_HIP(hipHostGetDevicePointer((void**)&c->hd_info, c->h_info, 0));
    VC_HIP(hipHostMalloc((void**)&c->h_up, c->up_bytes));
    VC_HIP(hipEventCreateWithFlags(&c->packed, hipEventDisableTiming));
    VC_HIP(hipEventCreateWithFlags(&c->copied, hipEventDisableTiming));
    VC_HIP(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    return VC_OK;
}

static int ckpt_begin(vc_live* l) {
    vc_engine* e = l->e;
    LiveCkpt& c = *l->ck;
    VC_HIP(hipSetDevice(e->cfg.device));
    long long* fd = (long long*)c.h_up;                                   // frames_done as of this call
    CkptHostParams* hp = (CkptHostParams*)(c.h_up + (size_t)l->n_cam * 8);
    for (int i = 0; i < l->n_cam; ++i) fd[i] = l->frames_done[i];
    for (size_t i = 0; i < l->trackers.size(); ++i) { const vc_tracker_params& p = e->trackers[l->trackers[i]]->p; hp[i] = CkptHostParams{p.min_confidence, p.nms_max_overlap}; }
    hipStream_t ts = e->stream;
    VC_HIP(hipMemcpyAsync(c.d_up, c.h_up, c.up_bytes, hipMemcpyHostToDevice, ts));
    const CkptView v = ckpt_view(l);
    hipLaunchKernelGGL(live_ckpt_plan_kernel, dim3(1), dim3(CKPT_PLAN_THREADS), 0, ts, v, c.d_stage, (unsigned long long)c.max_bytes, c.d_table, c.d_trk_first, c.d_info);
    VC_HIP(hipGetLastError());
    hipLaunchKernelGGL(live_ckpt_pack_kernel, dim3(CKPT_PACK_BLOCKS), dim3(CKPT_COPY_THREADS), 0, ts, v, c.d_stage, c.d_table, c.d_info);
    VC_HIP(hipGetLastError());
    VC_HIP(hipEventRecord(c.packed, ts));
    VC_HIP(hipStreamWaitEvent(c.cstream, c.packed, 0));
    hipLaunchKernelGGL(live_ckpt_copy_kernel, dim3(CKPT_D2H_BLOCKS), dim3(CKPT_COPY_THREADS), 0, c.cstream, (const char*)c.d_stage, c.hd_blob, (const CkptInfo*)c.d_info, c.hd_info);
    VC_HIP(hipGetLastError());
    VC_HIP(hipEventRecord(c.copied, c.cstream));
    c.in_flight = true;
    return VC_OK;
}

static int ckpt_end(vc_live* l, void* buf, size_t cap, size_t* size) {
    LiveCkpt& c = *l->ck;
    VC_HIP(hipSetDevice(l->e->cfg.device));
    VC_HIP(hipEventSynchronize(c.copied));                                // the copy event only
    const CkptInfo info = *c.h_info;
    if (info.overflow) {
        c.in_flight = false;
        VC_CHECK(false, VC_ERR_CAPACITY, "the checkpoint needs %llu bytes, vc_live_checkpoint_enable reserved %zu", info.total, c.max_bytes);
    }
    *size = (size_t)info.total;
    if (!buf) return VC_OK;                                               // size query: the checkpoint stays ready
    VC_CHECK(cap >= info.total, VC_ERR_CAPACITY, "the checkpoint needs %llu bytes", info.total);
    memcpy(buf, c.h_blob, (size_t)info.total);
    c.in_flight = false;
    return VC_OK;
}

// host's copy of one tracker's list (engine idle)
static int download_list(vc_engine* e, int tracker, std::vector<int>& list) {
    tc::TrackerHdr h;
    VC_HIP(hipMemcpy(&h, e->d_hdrs + tracker, sizeof(h), hipMemcpyDeviceToHost));
    list.resize(std::max(0, std::min(h.n_tracks, e->list_cap)));
    if (!list.empty()) VC_HIP(hipMemcpy(list.data(), e->d_lists + (size_t)tracker * e->list_cap, list.size() * sizeof(int), hipMemcpyDeviceToHost));
    return VC_OK;
}

static int ckpt_restore(vc_live* l, const void* buf, size_t size, const int* cam_map) {
    vc_engine* e = l->e;
    const char* b = (const char*)buf;
    // a batch that is enqueued but not collected would, at its collect, write its own track counts over what the restore sets
    bool outstanding = !e->jobs.empty();
    for (const TrackStage& s : e->tstage) outstanding = outstanding || s.busy;
    VC_CHECK(!outstanding, VC_ERR_STATE, "vc_live_restore: batches are outstanding on this engine: collect their rows first");
    // ---- every refusal first: nothing below this block fails for a reason the blob or the counter's configuration gives ----
    CkptDims d{};
    const int bad = ckpt_validate(buf, size, &d);
    VC_CHECK(bad == CK_OK, VC_ERR_ARG, "not a live checkpoint: %s", ckpt_error_name(bad));
    VC_CHECK(d.n_labels == l->n_labels, VC_ERR_ARG, "the checkpoint holds %d labels per camera, the counter %d", d.n_labels, l->n_labels);
    VC_CHECK(cam_map || d.n_cam <= l->n_cam, VC_ERR_ARG, "the checkpoint holds %d cameras, the counter %d (cam_map picks some)", d.n_cam, l->n_cam);
    std::vector<int> cmap(d.n_cam), trk_map((size_t)d.n_cam * d.n_labels, -1);
    int n_mapped = 0;
    for (int c = 0; c < d.n_cam; ++c) {
        cmap[c] = cam_map ? cam_map[c] : c;
        if (cmap[c] == -1) continue;                                      // this camera of the blob is not restored
        ++n_mapped;
        VC_CHECK(cmap[c] >= 0 && cmap[c] < l->n_cam, VC_ERR_ARG, "cam_map[%d] = %d outside the counter's %d cameras", c, cmap[c], l->n_cam);
        for (int k = 0; k < c; ++k) VC_CHECK(cmap[k] != cmap[c], VC_ERR_ARG, "cam_map names camera %d twice", cmap[c]);
        const CkptCamera cam = ckpt_load<CkptCamera>(b + ckpt_camera_off(c, d.max_dir, d.n_labels));
        const int m = cmap[c];
        VC_CHECK(cam.poly_n == l->poly_n[m] && cam.n_dir == l->n_dir[m] &&
                 memcmp(cam.polygon, l->h_poly.data() + (size_t)m * cc::CC_MAX_POINTS * 2, sizeof(cam.polygon)) == 0 &&
                 memcmp(cam.dir_lines, l->h_dirs.data() + (size_t)m * cc::CC_MAX_DIRS * 4, sizeof(cam.dir_lines)) == 0,
                 VC_ERR_ARG, "the zone of checkpoint camera %d differs from the zone of the counter's camera %d", c, m);
        for (int lb = 0; lb < d.n_labels; ++lb) trk_map[(size_t)c * d.n_labels + lb] = l->trackers[(size_t)m * l->n_labels + lb];
    }
    VC_CHECK(n_mapped >= 1, VC_ERR_ARG, "cam_map restores no camera");
    std::vector<CkptTracker> trk(trk_map.size());
    std::vector<int> rows;                                                // of every track of the blob, restored or not
    size_t n_new = 0;                                                     // tracks of the cameras that are restored
    for (size_t t = 0; t < trk.size(); ++t) {
        trk[t] = ckpt_load<CkptTracker>(b + ckpt_tracker_off((int)t, d.n_cam, d.max_dir, d.n_labels));
        if (trk_map[t] < 0) continue;
        n_new += (size_t)trk[t].n_tracks;
        VC_CHECK(trk[t].nn_budget <= e->cfg.nn_budget_cap, VC_ERR_CAPACITY, "checkpoint nn_budget %d exceeds nn_budget_cap %d", trk[t].nn_budget, e->cfg.nn_budget_cap);
        VC_CHECK(trk[t].n_tracks <= e->list_cap, VC_ERR_CAPACITY, "the checkpoint holds %d tracks of one tracker, tracks_per_tracker is %d", trk[t].n_tracks, e->list_cap);
    }
    {                                                                     // per-track rows, in blob order (the walk ckpt_validate has checked)
        uint64_t o = ckpt_tracks_off(d.n_cam, d.max_dir, d.n_labels);
        for (const CkptTracker& k : trk)
            for (int i = 0; i < k.n_tracks; ++i) {
                const int r = ckpt_load<CkptRec>(b + o).gal_count;
                rows.push_back(r);
                o += ckpt_track_bytes(r);
            }
    }
    std::vector<uint64_t> off(rows.size() + 1);
    const uint64_t total = ckpt_track_offsets(rows.data(), (int)rows.size(), d.n_cam, d.max_dir, d.n_labels, off.data());
    VC_CHECK(total == size, VC_ERR_ARG, "not a live checkpoint: %s", ckpt_error_name(CK_E_SIZE));
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));                                            // restore is rare: drain first (blocking paths leave nothing to collect)
    VC_HIP(hipStreamSynchronize(e->stream));
    std::vector<int> old;
    for (int t : trk_map) { if (t < 0) continue; std::vector<int> li; VC_TRY(download_list(e, t, li)); old.insert(old.end(), li.begin(), li.end()); }
    int ctl[2];
    VC_HIP(hipMemcpy(ctl, e->d_free, sizeof(ctl), hipMemcpyDeviceToHost));
    VC_CHECK((size_t)ctl[0] + old.size() >= n_new, VC_ERR_CAPACITY, "track pool too small: the checkpoint brings %zu tracks, %zu slots are free (max_tracks = %d)",
             n_new, (size_t)ctl[0] + old.size(), e->cfg.max_tracks);
    // device memory of the restore itself, before anything is changed
    DevScratch mem;
    char* d_blob = nullptr; CkptUnpackRef* d_table = nullptr; int *d_trk_map = nullptr, *d_cam_map = nullptr, *d_close = nullptr;
    VC_TRY(mem.upload(&d_blob, buf, size));
    VC_TRY(mem.alloc(&d_table, (n_new + 1) * sizeof(CkptUnpackRef)));
    VC_TRY(mem.alloc(&d_trk_map, trk_map.size() * sizeof(int)));
    VC_TRY(mem.alloc(&d_cam_map, cmap.size() * sizeof(int)));
    VC_TRY(mem.alloc(&d_close, (old.size() + 1) * sizeof(int)));
    // ---- from here on the counter changes --------------------------------------------------------------------------------------
    VC_TRY(host_give_slots(e, old));
    std::vector<int> slots;
    VC_TRY(host_take_slots(e, (int)n_new, slots));
    std::vector<CkptUnpackRef> table;
    table.reserve(n_new + 1);
    size_t n = 0;
    for (size_t t = 0; t < trk.size(); ++t)
        for (int i = 0; i < trk[t].n_tracks; ++i, ++n)
            if (trk_map[t] >= 0) table.push_back(CkptUnpackRef{off[n], slots[table.size()], rows[n], trk_map[t], i, cmap[t / d.n_labels], 0});
    if (table.empty()) table.push_back(CkptUnpackRef{});
    std::vector<int> close;
    {
        std::vector<int> taken(slots);
        std::sort(taken.begin(), taken.end());
        for (int s : old) if (s >= 0 && s < e->pool.max_tracks && !std::binary_search(taken.begin(), taken.end(), s)) close.push_back(s);
    }
    VC_HIP(hipMemcpy(d_table, table.data(), table.size() * sizeof(CkptUnpackRef), hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(d_trk_map, trk_map.data(), trk_map.size() * sizeof(int), hipMemcpyHostToDevice));
    VC_HIP(hipMemcpy(d_cam_map, cmap.data(), cmap.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!close.empty()) VC_HIP(hipMemcpy(d_close, close.data(), close.size() * sizeof(int), hipMemcpyHostToDevice));
    const int whole = n_mapped == d.n_cam && n_mapped == l->n_cam;
    CkptUnpackMisc m{d_trk_map, d_cam_map, d_close, (int)close.size(), d.n_cam, d.max_dir, (int)n_new, whole};
    const int blocks = (int)std::min(n_new + 1, (size_t)CKPT_PACK_BLOCKS);
    hipLaunchKernelGGL(live_ckpt_unpack_kernel, dim3(blocks), dim3(CKPT_COPY_THREADS), 0, e->stream, ckpt_view(l), (const char*)d_blob, (const CkptUnpackRef*)d_table, m);
    VC_HIP(hipGetLastError());
    VC_HIP(hipStreamSynchronize(e->stream));
    for (int c = 0; c < d.n_cam; ++c) if (cmap[c] >= 0) l->frames_done[cmap[c]] = ckpt_load<CkptCamera>(b + ckpt_camera_off(c, d.max_dir, d.n_labels)).frames_done;
    for (size_t t = 0; t < trk.size(); ++t) {
        if (trk_map[t] < 0) continue;
        Tracker& tk = *e->trackers[trk_map[t]];
        const CkptTracker& k = trk[t];
        tk.p.max_dist = k.max_dist; tk.p.min_confidence = k.min_confidence; tk.p.nms_max_overlap = k.nms_max_overlap;
        tk.p.max_iou_distance = k.max_iou_distance; tk.p.max_age = k.max_age; tk.p.n_init = k.n_init; tk.p.nn_budget = k.nn_budget;
        tk.known_tracks = k.n_tracks; tk.pending_dets = 0;
    }
    return VC_OK;
}

}  // namespace vc

using namespace vc;

extern "C" {

int vc_live_checkpoint_enable(vc_live* l, size_t max_bytes) {
    VC_CHECK(l, VC_ERR_ARG, "null argument");
    VC_CHECK(!l->ck, VC_ERR_STATE, "vc_live_checkpoint_enable: enabled already");
    VC_HIP(hipSetDevice(l->e->cfg.device));
    const int rc = ckpt_enable(l, max_bytes);
    if (rc != VC_OK && l->ck) live_ckpt_free(l);
    return rc;
}

int vc_live_checkpoint_begin(vc_live* l) {
    VC_CHECK(l, VC_ERR_ARG, "null argument");
    VC_CHECK(l->ck, VC_ERR_STATE, "vc_live_checkpoint_begin: vc_live_checkpoint_enable first");
    VC_CHECK(!l->ck->in_flight, VC_ERR_STATE, "vc_live_checkpoint_begin: a checkpoint is in flight (vc_live_checkpoint_end first)");
    return ckpt_begin(l);
}

int vc_live_checkpoint_end(vc_live* l, void* buf, size_t cap, size_t* size) {
    VC_CHECK(l && size, VC_ERR_ARG, "null argument");
    VC_CHECK(l->ck && l->ck->in_flight, VC_ERR_STATE, "vc_live_checkpoint_end: no checkpoint in flight (vc_live_checkpoint_begin first)");
    return ckpt_end(l, buf, cap, size);
}

int vc_live_checkpoint(vc_live* l, void* buf, size_t cap, size_t* size) {
    VC_CHECK(l && size, VC_ERR_ARG, "null argument");
    VC_CHECK(l->ck, VC_ERR_STATE, "vc_live_checkpoint: vc_live_checkpoint_enable first");
    if (!l->ck->in_flight) VC_TRY(ckpt_begin(l));                         // after a size query the checkpoint it measured is still ready
    return ckpt_end(l, buf, cap, size);
}

int vc_live_restore(vc_live* l, const void* buf, size_t size, const int* cam_map) {
    VC_CHECK(l && buf, VC_ERR_ARG, "null argument");
    return ckpt_restore(l, buf, size, cam_map);
}

int vc_live_ckpt_validate_host(const void* buf, size_t size) {
    const int bad = ckpt_validate(buf, size, nullptr);
    VC_CHECK(bad == CK_OK, VC_ERR_ARG, "not a live checkpoint: %s", ckpt_error_name(bad));
    return VC_OK;
}

}  // extern "C"
