// The checkpoint of a live counter (live_ckpt.hip: vc_live_checkpoint* / vc_live_restore): ONE self-contained blob that holds everything
// the counter's trackers and the counter itself read from now on, so that a restore onto another counter -- another engine, process or
// GPU -- continues the stream with identical rows, ids, counts and overlay lists.  Written once for the pack / unpack kernels, for the
// host side of vc_live_restore and for the host build the CPU tests compile (tests/native/live_ckpt_host.cpp).  No HIP, no allocation.
//
// Format: little-endian, packed, every section on a 16-byte boundary, all padding zero.  No pool slot number, no pointer, no tracker
// handle, nothing that depends on the engine's configuration (max_tracks, nn_budget_cap, tracks_per_tracker):
//
//   CkptHeader                                   64 B   magic, version, feat_dim, n_cam, n_labels, max_dir, tracks in all, total size
//   n_cam x [CkptCamera | base[max_dir][n_labels] int32 | pad]      frames_done, the zone as the counter holds it (padded arrays), base
//   CkptStats                                    16 B   stats[1]: tracks folded into base so far
//   n_cam * n_labels x CkptTracker               64 B   (camera, label) order: parameters and next_id as vc_tracker_snapshot keeps them, n_tracks, err
//   per tracker, per track IN LIST ORDER (lists[tracker][i] = the reference's self.tracks order, which matching depends on):
//     CkptTrack                                 704 B   the TrackRecD fields, mean[8], cov[64] (fp64, bit for bit), the track's LiveSlot
//                                                       (all zero unless open)
//     rows x 2048 B                                     the gallery ring's PHYSICAL rows [0, min(gal_count, nn_budget)), with gal_head
//                                                       in the record: exactly what vc_tracker_snapshot keeps
//
// Sizes and offsets have one definition, the functions below: the plan kernel scans ckpt_track_bytes into the offset table, the host
// does the same through ckpt_track_offsets.  ckpt_validate checks a whole blob before anything is touched and never reads past `size`.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "count_core.h"

namespace vc {
namespace ck {

enum { CK_VERSION = 1, CK_FEAT_DIM = 512, CK_ROW_BYTES = CK_FEAT_DIM * 4, CK_ALIGN = 16 };
enum { CK_MAX_CAM = 4096, CK_MAX_LABELS = 4096, CK_MAX_TRACKS = 1 << 20 };       // what a blob may claim (per tracker: CK_MAX_TRACKS)
enum { CK_TENTATIVE = 1, CK_CONFIRMED = 2, CK_TERR_LAST = 5 };                     // track_core.h: tc::TENTATIVE / tc::CONFIRMED / tc::TERR_TABLE

// what ckpt_validate answers (0 = a well-formed blob)
enum { CK_OK = 0, CK_E_TRUNCATED, CK_E_MAGIC, CK_E_VERSION, CK_E_FEAT_DIM, CK_E_DIMS, CK_E_SIZE, CK_E_CAMERA, CK_E_STATS, CK_E_PARAMS,
       CK_E_NTRACKS, CK_E_TRACK, CK_E_RING, CK_E_SLOT, CK_E_BOUNDS };

struct CkptHeader {
    char magic[8];
    int32_t version, feat_dim, n_cam, n_labels, max_dir, n_tracks;
    uint64_t total_size;
    uint64_t pad[3];
};                                                                                // 64 B
struct CkptCamera {
    int64_t frames_done;
    int32_t poly_n, n_dir;
    double polygon[cc::CC_MAX_POINTS * 2];
    double dir_lines[cc::CC_MAX_DIRS * 4];
};                                                                                // 1552 B, then base[max_dir][n_labels] and padding
struct CkptStats { int32_t retired, pad[3]; };                                    // 16 B
struct CkptTracker {
    int64_t next_id;
    double max_dist, min_confidence, nms_max_overlap, max_iou_distance;
    int32_t max_age, n_init, nn_budget, n_tracks;
    int32_t err, pad;                                                             // err: tc::TERR_* -- a tracker a capacity error has stopped stays stopped
};                                                                                // 64 B
struct CkptRec { int64_t id; int32_t state, hits, age, tsu, gal_count, gal_head; };   // = tc::TrackRecD, 32 B
struct CkptTrack {
    CkptRec rec;
    double mean[8];
    double cov[64];
    cc::LiveSlot slot;
    int64_t pad;
};                                                                                // 704 B
// the device-resident tracker header (= tc::TrackerHdr, 48 B) and the two parameters only the host's detection filter reads
struct CkptHdr { double max_dist, max_iou_distance; int64_t next_id; int32_t max_age, n_init, nn_budget, n_tracks, err, pad; };
struct CkptHostParams { double min_confidence, nms_max_overlap; };

static_assert(sizeof(CkptHeader) == 64 && sizeof(CkptCamera) == 1552 && sizeof(CkptStats) == 16 && sizeof(CkptTracker) == 64, "checkpoint sections");
static_assert(sizeof(CkptRec) == 32 && sizeof(CkptTrack) == 704 && sizeof(cc::LiveSlot) == 88 && sizeof(CkptHdr) == 48, "checkpoint records");
static_assert(offsetof(CkptTrack, mean) == 32 && offsetof(CkptTrack, cov) == 96 && offsetof(CkptTrack, slot) == 608, "checkpoint track layout");

// ---- sizes and offsets ---------------------------------------------------------------------------------------------------------
VC_CC_HD uint64_t ckpt_align(uint64_t x) { return (x + (CK_ALIGN - 1)) & ~(uint64_t)(CK_ALIGN - 1); }
VC_CC_HD uint64_t ckpt_camera_bytes(int max_dir, int n_labels) { return ckpt_align(sizeof(CkptCamera) + (uint64_t)max_dir * n_labels * 4); }
VC_CC_HD uint64_t ckpt_camera_off(int cam, int max_dir, int n_labels) { return sizeof(CkptHeader) + (uint64_t)cam * ckpt_camera_bytes(max_dir, n_labels); }
VC_CC_HD uint64_t ckpt_stats_off(int n_cam, int max_dir, int n_labels) { return ckpt_camera_off(n_cam, max_dir, n_labels); }
VC_CC_HD uint64_t ckpt_tracker_off(int t, int n_cam, int max_dir, int n_labels) {
    return ckpt_stats_off(n_cam, max_dir, n_labels) + sizeof(CkptStats) + (uint64_t)t * sizeof(CkptTracker);
}
VC_CC_HD uint64_t ckpt_tracks_off(int n_cam, int max_dir, int n_labels) { return ckpt_tracker_off(n_cam * n_labels, n_cam, max_dir, n_labels); }
// gallery rows a track brings, and the bytes of its section
VC_CC_HD int ckpt_track_rows(int gal_count, int nn_budget) { return gal_count < 0 ? 0 : (gal_count < nn_budget ? gal_count : nn_budget); }
VC_CC_HD uint64_t ckpt_track_bytes(int rows) { return sizeof(CkptTrack) + (uint64_t)rows * CK_ROW_BYTES; }
// per-track row counts (all trackers, list order) -> per-track offsets; returns the total size of the blob
VC_CC_HD uint64_t ckpt_track_offsets(const int* rows, int n, int n_cam, int max_dir, int n_labels, uint64_t* off) {
    uint64_t o = ckpt_tracks_off(n_cam, max_dir, n_labels);
    for (int i = 0; i < n; ++i) { off[i] = o; o += ckpt_track_bytes(rows[i]); }
    return o;
}
// bytes of a blob with no track at all: what the plan kernel always writes
VC_CC_HD uint64_t ckpt_fixed_bytes(int n_cam, int max_dir, int n_labels) { return ckpt_tracks_off(n_cam, max_dir, n_labels); }

// ---- unaligned-safe access (a blob handed to vc_live_restore may start anywhere) ------------------------------------------------
template <class T> VC_CC_HD T ckpt_load(const void* p) { T v; __builtin_memcpy(&v, p, sizeof(T)); return v; }
template <class T> VC_CC_HD void ckpt_store(void* p, const T& v) { __builtin_memcpy(p, &v, sizeof(T)); }
VC_CC_HD void ckpt_magic(char* m) { const char k[8] = {'V', 'C', 'L', 'I', 'V', 'E', '0', '1'}; for (int i = 0; i < 8; ++i) m[i] = k[i]; }

// ---- what a checkpoint reads from and a restore writes into, by pointer (device memory in the kernels, host arrays in the tests) ----
struct CkptView {
    // the tracker pool (TrackBatchArgs)
    CkptHdr* hdrs; int* lists; int list_cap; CkptRec* recs; double* mean; double* cov; float* gallery; int budget_cap, max_tracks;
    // the counter (LiveCountArgs)
    cc::LiveSlot* slots; int* base; int* stats; const double* polygons; const int* poly_n; const double* dir_lines; const int* n_dir;
    int n_cam, n_labels, max_dir;
    const int* trackers;                 // [n_cam * n_labels] index into hdrs / lists
    const CkptHostParams* params;        // [n_cam * n_labels]
    const long long* frames_done;        // [n_cam]
};

// ---- pack: one item each, so that the kernels split them over threads and the host walks them in a loop ----------------------------
VC_CC_HD void ckpt_put_header(char* blob, const CkptView& v, int n_tracks, uint64_t total) {
    CkptHeader h{};
    ckpt_magic(h.magic);
    h.version = CK_VERSION; h.feat_dim = CK_FEAT_DIM; h.n_cam = v.n_cam; h.n_labels = v.n_labels; h.max_dir = v.max_dir; h.n_tracks = n_tracks;
    h.total_size = total;
    ckpt_store(blob, h);
}
VC_CC_HD void ckpt_put_camera(char* blob, const CkptView& v, int c) {
    char* o = blob + ckpt_camera_off(c, v.max_dir, v.n_labels);
    CkptCamera cam{};
    cam.frames_done = v.frames_done[c]; cam.poly_n = v.poly_n[c]; cam.n_dir = v.n_dir[c];
    for (int i = 0; i < cc::CC_MAX_POINTS * 2; ++i) cam.polygon[i] = v.polygons[(size_t)c * cc::CC_MAX_POINTS * 2 + i];
    for (int i = 0; i < cc::CC_MAX_DIRS * 4; ++i) cam.dir_lines[i] = v.dir_lines[(size_t)c * cc::CC_MAX_DIRS * 4 + i];
    ckpt_store(o, cam);
    const int nb = v.max_dir * v.n_labels;
    for (int i = 0; i < nb; ++i) ckpt_store<int32_t>(o + sizeof(CkptCamera) + (size_t)i * 4, v.base[(size_t)c * nb + i]);
    for (uint64_t i = sizeof(CkptCamera) + (uint64_t)nb * 4; i < ckpt_camera_bytes(v.max_dir, v.n_labels); ++i) o[i] = 0;
}
VC_CC_HD void ckpt_put_stats(char* blob, const CkptView& v) {
    CkptStats s{};
    s.retired = v.stats[1];
    ckpt_store(blob + ckpt_stats_off(v.n_cam, v.max_dir, v.n_labels), s);
}
VC_CC_HD void ckpt_put_tracker(char* blob, const CkptView& v, int t) {
    const CkptHdr& h = v.hdrs[v.trackers[t]];
    CkptTracker k{};
    k.next_id = h.next_id; k.max_dist = h.max_dist; k.min_confidence = v.params[t].min_confidence; k.nms_max_overlap = v.params[t].nms_max_overlap;
    k.max_iou_distance = h.max_iou_distance; k.max_age = h.max_age; k.n_init = h.n_init; k.nn_budget = h.nn_budget; k.n_tracks = h.n_tracks; k.err = h.err;
    ckpt_store(blob + ckpt_tracker_off(t, v.n_cam, v.max_dir, v.n_labels), k);
}
// the record and the LiveSlot of a track section (mean, cov and the gallery rows are plain copies the caller makes)
VC_CC_HD void ckpt_put_track_head(char* dst, const CkptRec& rec, const cc::LiveSlot& s) {
    ckpt_store(dst, rec);
    cc::LiveSlot z{};
    if (s.open) z = s;
    ckpt_store(dst + offsetof(CkptTrack, slot), z);
    ckpt_store<int64_t>(dst + offsetof(CkptTrack, pad), 0);
}

// The whole pack, serially (the CPU tests; the kernels do the same items in parallel).  rows / off: scratch of at least the number of
// tracks.  Returns the total size; nothing past the fixed part is written if it exceeds cap (the kernels' overflow rule).
inline uint64_t ckpt_pack_serial(char* blob, uint64_t cap, const CkptView& v, int* rows, uint64_t* off, int* overflow) {
    const int n_trk = v.n_cam * v.n_labels;
    int n = 0;
    for (int t = 0; t < n_trk; ++t) {
        const CkptHdr& h = v.hdrs[v.trackers[t]];
        for (int i = 0; i < h.n_tracks; ++i) rows[n++] = ckpt_track_rows(v.recs[v.lists[(size_t)v.trackers[t] * v.list_cap + i]].gal_count, h.nn_budget);
    }
    const uint64_t total = ckpt_track_offsets(rows, n, v.n_cam, v.max_dir, v.n_labels, off);
    *overflow = total > cap;
    if (ckpt_fixed_bytes(v.n_cam, v.max_dir, v.n_labels) > cap) return total;
    ckpt_put_header(blob, v, n, total);
    if (*overflow) return total;
    for (int c = 0; c < v.n_cam; ++c) ckpt_put_camera(blob, v, c);
    ckpt_put_stats(blob, v);
    n = 0;
    for (int t = 0; t < n_trk; ++t) {
        ckpt_put_tracker(blob, v, t);
        const CkptHdr& h = v.hdrs[v.trackers[t]];
        for (int i = 0; i < h.n_tracks; ++i, ++n) {
            const int slot = v.lists[(size_t)v.trackers[t] * v.list_cap + i];
            char* o = blob + off[n];
            ckpt_put_track_head(o, v.recs[slot], v.slots[slot]);
            __builtin_memcpy(o + offsetof(CkptTrack, mean), v.mean + (size_t)slot * 8, 64);
            __builtin_memcpy(o + offsetof(CkptTrack, cov), v.cov + (size_t)slot * 64, 512);
            __builtin_memcpy(o + sizeof(CkptTrack), v.gallery + (size_t)slot * v.budget_cap * CK_FEAT_DIM, (size_t)rows[n] * CK_ROW_BYTES);
        }
    }
    return total;
}

// ---- unpack: driven by a slot table the host builds from a VALIDATED blob -----------------------------------------------------------
struct CkptUnpackRef { uint64_t off; int32_t slot, rows, tracker, pos, cam, pad; };   // one per track: where it lies, where it goes; cam = the counter's camera
// the record and the LiveSlot of one track into the pool and the counter (mean, cov, gallery rows: plain copies the caller makes)
VC_CC_HD void ckpt_get_track_head(const char* src, const CkptUnpackRef& r, const CkptView& v) {
    v.recs[r.slot] = ckpt_load<CkptRec>(src);
    cc::LiveSlot s = ckpt_load<cc::LiveSlot>(src + offsetof(CkptTrack, slot));
    if (s.open) s.cam = r.cam;
    v.slots[r.slot] = s;
    v.lists[(size_t)r.tracker * v.list_cap + r.pos] = r.slot;
}
// tracker section t of the blob -> the device header of tracker `tracker` (engine side)
VC_CC_HD void ckpt_get_tracker(const char* blob, int t, int n_cam, int max_dir, int n_labels, CkptHdr& h) {
    const CkptTracker k = ckpt_load<CkptTracker>(blob + ckpt_tracker_off(t, n_cam, max_dir, n_labels));
    h.max_dist = k.max_dist; h.max_iou_distance = k.max_iou_distance; h.next_id = k.next_id;
    h.max_age = k.max_age; h.n_init = k.n_init; h.nn_budget = k.nn_budget; h.n_tracks = k.n_tracks; h.err = k.err; h.pad = 0;
}
// base of blob camera c (blob dims) -> the counter's base of camera `cam`; directions the blob does not have are zero
VC_CC_HD void ckpt_get_base(const char* blob, int c, int b_max_dir, int n_labels, int cam, const CkptView& v) {
    const char* o = blob + ckpt_camera_off(c, b_max_dir, n_labels) + sizeof(CkptCamera);
    for (int d = 0; d < v.max_dir; ++d)
        for (int l = 0; l < n_labels; ++l)
            v.base[((size_t)cam * v.max_dir + d) * n_labels + l] = d < b_max_dir ? ckpt_load<int32_t>(o + ((size_t)d * n_labels + l) * 4) : 0;
}

// ---- validation ----------------------------------------------------------------------------------------------------------------
struct CkptDims { int n_cam, n_labels, max_dir, n_tracks; };

// A whole blob, before anything is touched: 0, or the first CK_E_* met.  Every read is bounds-checked against `size` first.
inline int ckpt_validate(const void* buf, uint64_t size, CkptDims* dims) {
    const char* b = (const char*)buf;
    if (!b || size < sizeof(CkptHeader)) return CK_E_TRUNCATED;
    const CkptHeader h = ckpt_load<CkptHeader>(b);
    char magic[8];
    ckpt_magic(magic);
    for (int i = 0; i < 8; ++i) if (h.magic[i] != magic[i]) return CK_E_MAGIC;
    if (h.version != CK_VERSION) return CK_E_VERSION;
    if (h.feat_dim != CK_FEAT_DIM) return CK_E_FEAT_DIM;
    if (h.n_cam < 1 || h.n_cam > CK_MAX_CAM || h.n_labels < 1 || h.n_labels > CK_MAX_LABELS || h.max_dir < 1 || h.max_dir > cc::CC_MAX_DIRS) return CK_E_DIMS;
    if (h.n_tracks < 0 || h.pad[0] || h.pad[1] || h.pad[2]) return CK_E_DIMS;
    if (h.total_size != size) return CK_E_SIZE;
    const uint64_t tracks_off = ckpt_tracks_off(h.n_cam, h.max_dir, h.n_labels);
    if (tracks_off > size) return CK_E_BOUNDS;
    for (int c = 0; c < h.n_cam; ++c) {
        const char* o = b + ckpt_camera_off(c, h.max_dir, h.n_labels);
        const CkptCamera cam = ckpt_load<CkptCamera>(o);
        if (cam.frames_done < 0 || cam.poly_n < 1 || cam.poly_n > cc::CC_MAX_POINTS || cam.n_dir < 1 || cam.n_dir > h.max_dir) return CK_E_CAMERA;
        for (uint64_t i = sizeof(CkptCamera) + (uint64_t)h.max_dir * h.n_labels * 4; i < ckpt_camera_bytes(h.max_dir, h.n_labels); ++i) if (o[i]) return CK_E_CAMERA;
    }
    const CkptStats st = ckpt_load<CkptStats>(b + ckpt_stats_off(h.n_cam, h.max_dir, h.n_labels));
    if (st.retired < 0 || st.pad[0] || st.pad[1] || st.pad[2]) return CK_E_STATS;
    uint64_t o = tracks_off;
    long long n_all = 0;
    for (int t = 0; t < h.n_cam * h.n_labels; ++t) {
        const CkptTracker k = ckpt_load<CkptTracker>(b + ckpt_tracker_off(t, h.n_cam, h.max_dir, h.n_labels));
        if (k.nn_budget < 1 || k.max_age < 1 || k.n_init < 1 || k.next_id < 1 || k.err < 0 || k.err > CK_TERR_LAST || k.pad) return CK_E_PARAMS;
        if (k.n_tracks < 0 || k.n_tracks > CK_MAX_TRACKS) return CK_E_NTRACKS;
        n_all += k.n_tracks;
        if (n_all > h.n_tracks) return CK_E_NTRACKS;
        for (int i = 0; i < k.n_tracks; ++i) {
            if (size - o < sizeof(CkptTrack)) return CK_E_BOUNDS;             // o <= size holds throughout
            const CkptTrack tr = ckpt_load<CkptTrack>(b + o);
            if (tr.rec.state != CK_TENTATIVE && tr.rec.state != CK_CONFIRMED) return CK_E_TRACK;
            if (tr.rec.hits < 0 || tr.rec.age < 0 || tr.rec.tsu < 0 || tr.rec.id < 1 || tr.rec.id >= k.next_id || tr.pad) return CK_E_TRACK;
            if (tr.rec.gal_count < 0 || tr.rec.gal_count > k.nn_budget || tr.rec.gal_head < 0 || tr.rec.gal_head >= k.nn_budget) return CK_E_RING;
            const cc::LiveSlot& s = tr.slot;
            if (s.open != 0 && s.open != 1) return CK_E_SLOT;
            if (s.open && (s.cam != t / h.n_labels || s.label < 0 || s.label >= h.n_labels || s.at_last < 1)) return CK_E_SLOT;
            if (!s.open) {
                if (s.cam || s.label || s.at_last || s.last_frame) return CK_E_SLOT;
                for (int q = 0; q < 4; ++q) if (s.first[q] || s.last[q]) return CK_E_SLOT;
            }
            o += sizeof(CkptTrack);
            const uint64_t g = (uint64_t)tr.rec.gal_count * CK_ROW_BYTES;
            if (size - o < g) return CK_E_BOUNDS;
            o += g;
        }
    }
    if (n_all != h.n_tracks) return CK_E_NTRACKS;
    if (o != size) return CK_E_SIZE;
    if (dims) { dims->n_cam = h.n_cam; dims->n_labels = h.n_labels; dims->max_dir = h.max_dir; dims->n_tracks = h.n_tracks; }
    return CK_OK;
}

inline const char* ckpt_error_name(int code) {
    static const char* const names[] = {"ok", "truncated", "wrong magic", "unknown version", "feature width", "camera / label / direction counts",
                                        "total size", "camera section", "stats section", "tracker parameters", "track counts", "track record",
                                        "gallery ring", "live slot", "section out of bounds"};
    return code >= 0 && code < (int)(sizeof(names) / sizeof(names[0])) ? names[code] : "?";
}

}  // namespace ck
}  // namespace vc
