// Engine internals shared between engine.hip / engine_plan.hip / engine_run.hip (networks), tracker.hip (DeepSORT) and stream.hip (fused path),
// and the engine routines that the host-array entry points (host_*.hip, on the staging harness of host_stage.h) share with the engine.
#pragma once
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"
#include "track_batch_plan.h"   // TrackTaskHost, TrackBatchPlan: what track_enqueue decides about a batch, which needs no engine either
#include "det_prep.h"     // FrameDets, Prepared, FramePrepared: the detection hand-over that needs no engine
#include "host_stage.h"   // dev_alloc, and DevScratch for the entry points that stage host arrays beside their kernels (yuv_ingest.hip, yuv_egress.hip)

namespace vc {

struct ConvParam {
    std::string name;
    int O = 0, I = 0, kh = 0, kw = 0;
    bool set = false;
    bool pair_stem = false;          // YOLO stem in bf16: two 4-channel pixels form one 16-byte chunk
    int fuse_a = -1, fuse_b = -1;    // >= 0: internal parameter = rows of params[fuse_a] then params[fuse_b] (same input, 1x1)
    int obj_of = -1;                 // >= 0: internal parameter = the three objectness rows (a * (5 + nc) + 4) of Detect head params[obj_of], padded to 8
    bool hidden = false;             // internal (fused) parameters are not enumerated to the caller
    std::vector<float> w, b;         // host copies (OIHW, BN folded) until finalize()
    void* d_w = nullptr;             // packed [Cout_pad][Kp]
    float* d_scale = nullptr;        // fp8: [Cout_pad] weight scale x activation scale
    int prec = 0;                    // precision the parameter was packed in (the detector's fp8 mode keeps its stem in bf16)
    float* d_b = nullptr;            // [Cout_pad]
    int cin_eff = 0, K = 0, Kp = 0, cout_pad = 0;
};

struct Op {
    enum Kind { CONV, SPPF, UPSAMPLE, MAXPOOL, TO_FP8, HEAD_COMPACT } kind;
    int level = 0;                   // HEAD_COMPACT: detection level
    int sole_reader_next = 0;        // CONV: the next op is the only reader of this op's output (it may stay on chip)
    double flops_override = -1, bytes_override = -1;   // CONV: algorithmic work to report instead of the launch's own (fixed part)
    // CONV with a device-side row count (sparse Detect head): the EXECUTED work is flops_override + rows x flops_per_row (bytes alike),
    // rows = the count the compaction left on the device, read back after the pass; dense_* = what the dense head this launch replaces
    // would have done -- reported separately (vc_profile_read_dense), never mixed into the executed figures (VERDICT r03 / ADVICE r03)
    int rows_level = -1;
    double flops_per_row = 0, bytes_per_row = 0, dense_flops = -1, dense_bytes = -1;
    ConvP conv{};
    View a{}, b{};
    int C = 0;
    int cout_logical = 0;            // > 0: the launch covers zero-padded output channels, FLOPs count this many
    int param = -1;                  // index into Net::params for CONV
    int tuned = -2;                  // CONV: tile configuration resolved at the first launch of this (cached) op; -2 = not yet
    int side = 0;                    // 1: off the detector's critical path -- launched on the engine's head stream, joined before the decode
};

// The op list of one network pass is a pure function of its shape: built once per (batch, tensor size, head variant) / (crop count)
// and replayed -- at batch 1 (the reference's own loop, vc_detect + vc_videotracker_run per frame) rebuilding 70 ops with their
// string-keyed parameter look-ups and autotune keys cost more host time than launching them.
struct YoloPlan { std::vector<Op> ops; View layer_view[24]; bool sparse = false; };
struct ReidPlan { std::vector<Op> ops; View out{}; };

struct LaunchRecorder;              // engine_record.hip

struct Net {
    std::vector<ConvParam> params;
    std::map<std::string, int> index;
    int add(const std::string& name, int O, int I, int kh, int kw) {
        ConvParam p;
        p.name = name; p.O = O; p.I = I; p.kh = kh; p.kw = kw;
        index[name] = (int)params.size();
        params.push_back(p);
        return (int)params.size() - 1;
    }
};

struct ProfCat {
    double ms = 0, flops = 0, bytes = 0;
    double flops_dense = 0, bytes_dense = 0;     // the same launches with the sparse Detect head credited as the dense head it replaces
    int64_t launches = 0;
};

// host-side view of one tracker (tracker.hip): parameters the host needs to prepare detections, and bounds on its size
struct Tracker {
    vc_tracker_params p;
    int known_tracks = 0;            // live tracks reported by the last completed batch
    int pending_dets = 0;            // detections of batches still in flight (each may start a track)
    bool released = false;           // vc_tracker_destroy: the slot is free for the next vc_tracker_create
    int gen = 0;                     // generation of the slot: part of the handle the caller holds
    vc_live* live = nullptr;         // the live counter this tracker is attached to (live_count.hip), and its camera there
    int live_cam = -1;
};
// A tracker HANDLE (what vc_tracker_create returns and every entry point takes) = slot | generation << 16: a handle kept past
// vc_tracker_destroy never addresses the tracker that reuses its slot (the next video's), it is refused.  Inside the library
// (FrameClassDets::tracker, task tables, device arrays) trackers are addressed by slot.
inline bool tracker_ok(const std::vector<std::unique_ptr<Tracker>>& v, int slot) { return slot >= 0 && slot < (int)v.size() && !v[slot]->released; }
inline int tracker_slot(const std::vector<std::unique_ptr<Tracker>>& v, int handle) {
    const int s = handle & 0xffff, g = (int)((unsigned)handle >> 16);
    return handle >= 0 && tracker_ok(v, s) && v[s]->gen == g ? s : -1;
}

// Staging of one tracker batch: inputs (tasks, plans, detections) in one pinned block mirrored on the device by a single copy;
// outputs (rows, per-task counts, status) written by the kernel straight into pinned host memory.
struct TrackStage {
    char* h_in = nullptr; char* d_in = nullptr; size_t in_cap = 0;
    char* h_out = nullptr; char* hd_out = nullptr; size_t out_cap = 0;
    int* d_cursor = nullptr;                 // [0] row cursor
    hipEvent_t done = nullptr;
    bool busy = false;
    TrackBatchPlan plan;                     // the current batch: tasks, sizes and the layout of both blocks (track_batch_plan.h)
    std::vector<int> frame_trk;              // per frame of it the slot of a tracker of the frame's camera, -1 none (filled while a live counter exists)
    int* d_row_slot = nullptr; size_t row_slot_cap = 0;   // TrackBatchArgs::row_slot of this stage, allocated once a live counter is attached
};

// A validated vc_yuv_desc with the zeros resolved (yuv_ingest.hip: yuv_resolve); all byte quantities.  Shared by the ingest
// conversion (yuv_ingest.hip), the egress conversion (yuv_egress.hip) and the render path (render.hip).
// The source formats in the kernels' own numbering (fmt below; VC_PIX_* has a gap between 1 and 16).  Egress writes the first two only.
enum { PF_NV12 = 0, PF_I420, PF_P016, PF_I010, PF_I422, PF_I444, PF_COUNT };
struct YuvGeom {
    int nv12, h, w, pitch_y, pitch_c;
    int fmt;                                            // PF_*; nv12 = (fmt == PF_NV12)
    size_t off_c, off_v, frame_stride, frame_end;      // frame_end: one past the last byte any plane of a frame occupies
    int yoff, cy, cvr, cvg, cug, cub;                   // decode: y = max(0, Y - yoff) * cy: full range is yoff = 0, cy = 1 << 20
    int matrix, full_range;                             // as the descriptor named them (the egress kernel picks its own constants)
};

}  // namespace vc

struct vc_render;

struct vc_engine {
    vc_engine_config cfg{};
    int prec = 0;                    // precision of the detector's convolutions (VC_PREC_*)
    int aux_prec = 0;                // precision of everything else (= prec, or bf16 when prec is fp8)
    float act_scale = 1.0f;          // fp8: real value = stored value x act_scale, one scale for all activations (e4m3 is a floating format)
    hipStream_t stream = nullptr;    // ReID + tracker
    hipStream_t dstream = nullptr;   // detector (runs ahead of the tracker on the next batch)
    hipStream_t rstream = nullptr;   // ReID of the next batch (stream path), concurrent with detector and tracker
    hipStream_t hstream = nullptr;   // Detect-head ops of the P3 / P4 levels, beside the neck layers that follow them (Op::side)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Tile counters of the fused persistent kernels (vc_common.h: tile_claim): a ring of {next, done} pairs, one per 64-byte line, zeroed once
    // here; the kernels leave a pair zero.  A launch takes the next pair (tile_ctr_next).  Launches of one stream run one after the other, so a
    // pair could only be shared by two running kernels if one stream fell a whole ring of such launches behind another: 1 024 pairs, five
    // launches per detector pass today, and the host waits for a batch's rows before it submits the next but one.
    static constexpr unsigned kTileCtrPairs = 1024;
    static constexpr int kDynTilesKept = 7;   // default of option "dyn_tiles_mask": the conversions that are kept (1 front_fused, 2 c3_fused, 4 bneck_fused kernels)
    unsigned* d_tile_ctr = nullptr;
    unsigned tile_ctr_seq = 0;
    unsigned tile_ctr_ring = kTileCtrPairs;   // pairs in use (option "dyn_tiles_ring", tests: 1 = every launch gets the pair the one before it left)
    int conv_slots = 0;              // VC_CONV_SLOTS at creation (tests): grid of front_fused_kernel and c3_fused_kernel, ConvP::slots
    void* d_zero = nullptr; size_t zero_bytes = 0; bool want_hc_count = false;   // per-pass counters cleared by one memset (engine_plan.hip)
    hipEvent_t ev_det[2] = {nullptr, nullptr};
    hipEvent_t ev_reid[3] = {nullptr, nullptr, nullptr};
    bool finalized = false;
    // kernel-selection switches: read from the environment ONCE at engine creation (VC_C3_FUSED, VC_BNECK_FUSED, VC_FRONT_FUSED,
    // VC_CROP_PER_PIXEL, VC_DOT_ARENA_MB), changed afterwards only through vc_engine_set_option -- nothing on the launch path calls getenv per launch
    struct Options { int c3_fused = 1, bneck_fused = 1, bneck_cv3 = 1, front_fused = 1, crop_per_pixel = 0, sparse_head = 1, ff_ablate = 0, c3_ablate = 0, reid_block_fused = 1, dyn_tiles = 1, dyn_tiles_mask = kDynTilesKept, head_side = 1, fuse_upsample = 1, sppf_sep = 1, fuse_s2_pw = 1, stem_direct = 1, embed_kept_only = 1; } opt;
    std::vector<void*> allocs;       // everything hipMalloc'ed, freed on destroy
    std::vector<void*> host_allocs;  // hipHostMalloc'ed

    // ---- detector --------------------------------------------------------------------------------
    vc::Net yolo;
    int ch[5] = {0, 0, 0, 0, 0}, rep[4] = {0, 0, 0, 0};
    std::map<std::string, vc::View> ybuf;        // named activation buffers (max shape)
    const vc::YoloPlan* last_plan = nullptr;     // plan of the last detector pass (a node of yolo_plans): layer views for vc_detect_debug_layer
    std::vector<vc::ConvP> s2pw_folded;                          // stride-2 convs whose output the last pass kept on chip (conv3x3s2_halo_kernel<..., F2>)
    std::vector<std::pair<vc::View, vc::View>> up_folded;        // UPSAMPLE ops (source, destination) the last detector pass folded into their consumers
    std::map<std::vector<int>, vc::YoloPlan> yolo_plans;          // key: B, nh, nw, sparse head?
    std::map<std::pair<int, int>, vc::ReidPlan> reid_plans;   // key: first crop, crop count
    uint8_t* d_frames = nullptr;                 // staging for host images / stream frames
    size_t d_frames_bytes = 0;
    float* d_logits[3] = {nullptr, nullptr, nullptr};
    // sparse Detect head (bf16 engines, detect_post.hip): objectness planes, gathered pixel lists / feature rows / logits, counts
    void* d_obj[3] = {nullptr, nullptr, nullptr};
    int* d_hc_list[3] = {nullptr, nullptr, nullptr};
    void* d_hc_x[3] = {nullptr, nullptr, nullptr};
    void* d_hc_logits[3] = {nullptr, nullptr, nullptr};
    int hc_cap[3] = {0, 0, 0};
    int* d_hc_count = nullptr;                   // [4]
    int* h_hc_ring = nullptr;                    // pinned [HC_RING][4]: the gathered-row counts of the last HC_RING detector passes (profiling)
    static constexpr int HC_RING = 16384;
    unsigned hc_ring_seq = 0; int hc_ring_cur = 0;
    float anchors[3][6];                         // Detect anchors in pixels (default: the COCO set of yolov5{s,m,l}.yaml)
    vc::DetectPostBuffers post{};
    float* d_geom = nullptr;                     // [max_batch][5] gain, padw, padh, src_w, src_h
    float* d_pred_debug = nullptr;
    bool want_pred_debug = false;
    // class filter and label map (class_filter.hip): empty = no map, and yolo_forward launches what it always did; the pinned and the
    // device table are allocated by the first vc_engine_set_class_map
    std::vector<int> class_map;                  // [num_classes] label of each class, -1 = dropped
    int n_labels = 0;
    int* h_class_map = nullptr;
    int* d_class_map = nullptr;
    int last_B = 0, last_nh = 0, last_nw = 0, last_ntotal = 0;
    // letterbox folded into the stem (stem_direct.hip, U8): source of the running / last detector pass; the letterboxed tensor
    // ybuf["in"] is then only produced on demand (vc_detect_debug_layer(-1))
    const uint8_t* stem_src = nullptr;
    vc::LetterboxGeom stem_geom{};
    bool in_stale = false;
    bool l0_stale = false;                       // the last pass ran front_fused_kernel: layer 0 stayed in LDS, ybuf["l0"] holds an older pass
    float* h_det = nullptr;                      // pinned [max_batch][max_det][6]
    int* h_det_count = nullptr;                  // pinned [max_batch]
    float* h_det2[2] = {nullptr, nullptr};       // pinned detector outputs of the (up to) two submissions in flight
    int* h_det_count2[2] = {nullptr, nullptr};
    float* h_geom = nullptr;                     // pinned [2][max_batch][5]
    unsigned geom_seq = 0, submit_seq = 0;
    // host-frame ingest (vc_stream_submit_host): copy stream + four device staging slots
    hipStream_t cstream = nullptr;
    uint8_t* d_ingest[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_ingest[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned ingest_seq = 0;
    bool ingest_staged[4] = {false, false, false, false};   // copied (or being copied) by vc_stream_stage_host, not yet submitted
    // YUV ingest (yuv_ingest.hip): raw 4:2:0 bytes of vc_stream_stage_yuv_host, one buffer per ingest slot, allocated by its first call
    uint8_t* d_yuv_raw[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t yuv_raw_bytes[4] = {0, 0, 0, 0};
    // frame-table ingest (yuv_ingest.hip: vc_stream_stage_frames[_sized]): per slot a pinned table and its device mirror, allocated by the
    // first call -- max_batch frame entries followed, for a sized batch, by its cells; and the dims of the sized batch the slot holds
    // (empty: a uniform batch)
    void* h_frame_tab[4] = {nullptr, nullptr, nullptr, nullptr};
    void* d_frame_tab[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<vc_frame_dims> ingest_dims[4];
    // ... their letterbox table (engine_run.hip: run_detector_dev_sized): two pinned slots like h_geom, one device table (detector stream order)
    vc::LetterboxFrame* h_lb_tab = nullptr;      // pinned [2][max_batch]
    vc::LetterboxFrame* d_lb_tab = nullptr;      // [max_batch]
    // ... and their per-frame crop tables, one per feature / crop buffer
    vc::CropFrame* h_crop_ftab[3] = {nullptr, nullptr, nullptr};
    vc::CropFrame* d_crop_ftab[3] = {nullptr, nullptr, nullptr};
    // stream path: three feature / crop buffers -- the batch being tracked (tracker stream), the batch
    // whose ReID is running, and the one after it
    float* d_feat2[3] = {nullptr, nullptr, nullptr};
    int* d_crops2[3] = {nullptr, nullptr, nullptr};
    int* h_crops2[3] = {nullptr, nullptr, nullptr};
    unsigned reid_seq = 0;
    std::vector<int> crop_scratch;               // crop list of the batch being validated (stream.hip::issue_reid)
    // DeepSort.update's own detection filter (deep_sort.py:31-37): the two tracker parameters prepare_dets reads.  `stream_flt` is the
    // one every tracker of the most recent vc_stream_run_async* call agreed on (valid = false: no such call yet, or they disagreed)
    struct EmbedFilter { bool valid = false; double min_confidence = 0, nms_max_overlap = 0; };
    EmbedFilter stream_flt;
    long long boxes_detected = 0, crops_embedded = 0;   // running totals of the stream and blocking paths (vc_stream_crop_stats)
    struct Pending {
        const void* frames; int b, h, w, slot;
        std::vector<vc_frame_dims> dims; // a sized batch: every frame's own size (h, w above: the largest), frame f at frames + f * cell; empty: a uniform batch
        size_t cell = 0;
        vc_frame_dims frame_dims(int f) const { return dims.empty() ? vc_frame_dims{h, w} : dims[f]; }   // the size of frame f
        int stage = 0;                   // 0: detector enqueued, 1: ReID enqueued as well
        bool embed_refused = false;      // a look-ahead attempt to embed this batch failed; the call that consumes it reports why (stream.hip)
        int fslot = 0;                   // feature / crop buffer of this batch
        std::vector<vc::FrameDets> fd;   // per frame, as VideoTracker.run sees them
        std::vector<int> row0;           // first feature row of each frame when every box is embedded
        // embed_kept_only: the batch was embedded under `flt` -- only the boxes prepare_dets keeps own a feature row, and prep[f] holds
        // frame f's prepare_frame results (det_prep.h), feat_rows indexing those compact rows (stream.hip::issue_reid)
        bool filtered = false;
        EmbedFilter flt;
        std::vector<vc::FramePrepared> prep;
        std::vector<float> inj_det; std::vector<int> inj_cnt; int inj_b = 0, inj_n = 0;   // detection injection captured at submit time
    };
    std::vector<Pending> pending;
    // asynchronous tracking (vc_stream_run_async / vc_stream_collect): a batch's tracker work is one kernel on the tracker stream;
    // the job remembers which staging slot its rows will land in
    struct AsyncJob { int stage = 0, b = 0, cap = 0; std::vector<int> ndet; const void* frames = nullptr; };
    std::deque<AsyncJob> jobs;                   // submission order; front = next to collect

    // ---- ReID ---------------------------------------------------------------------------------------
    vc::Net reid;
    std::map<std::string, vc::View> rbuf;
    int* d_crops = nullptr;                      // [max_crops][5]
    int* h_crops = nullptr;
    float* d_feat = nullptr;                     // [max_crops][512]
    float* h_feat = nullptr;
    float* d_reid_in_nchw = nullptr;

    // ---- tracker (device-resident, tracker.hip / track_kernels.hip) --------------------------------------------
    vc::TrackPool pool{};
    vc::tc::TrackerHdr* d_hdrs = nullptr;         // [max_trackers]
    int* d_lists = nullptr;                      // [max_trackers][list_cap]
    vc::tc::TrackRecD* d_recs = nullptr;          // [max_tracks]
    int* d_free = nullptr;                       // [0] free_top, [1] freed_count
    int* d_free_stack = nullptr; int* d_freed = nullptr;
    int max_trackers = 0, list_cap = 0;
    std::vector<std::unique_ptr<vc::Tracker>> trackers;
    vc::TrackStage tstage[4];                    // 0..2: batches of the stream path in flight, 3: the blocking entry points
    unsigned tstage_seq = 0;
    double* d_track_scratch = nullptr; size_t track_scratch_bytes = 0;
    // appearance dots hoisted out of the sequential loop (TrackDotPlan, kernels.h)
    vc::TrackDotPlan* d_dot_plans = nullptr; size_t dot_plans_cap = 0;
    float* d_dot_arena = nullptr; size_t dot_arena_floats = 0;     // grown on demand by track_enqueue up to dot_arena_max_floats
    size_t dot_arena_max_floats = 0;
    int* d_row_src = nullptr; int row_src_cap = 0;
    int* d_gal_row = nullptr; int* d_dot_ctl = nullptr;
    float* d_nfeat = nullptr; float* d_det_ss = nullptr; size_t nfeat_cap = 0;
    float* d_feat_in = nullptr;                  // features handed in from the host (vc_tracker_step)
    int det_cap = 0;
    std::vector<vc_live*> lives;                 // live counters (live_count.hip); vc_engine_destroy destroys what is left

    // ---- count all-gather (counting.hip): RCCL communicator of the engine's process group ----------------------
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    void* d_comm_buf = nullptr; size_t comm_buf_bytes = 0;
    // vc_allgather_rows (frame-sharded front end): padded send / receive blocks, the compacted embeddings, pinned rows
    void* d_gather_send = nullptr; size_t gather_send_bytes = 0;
    void* d_gather_recv = nullptr; size_t gather_recv_bytes = 0;
    void* d_gather_feat = nullptr; size_t gather_feat_bytes = 0;
    void* h_gather = nullptr; size_t h_gather_bytes = 0;
    void* d_overlay = nullptr; size_t overlay_bytes = 0;      // primitive lists of vc_overlay (overlay.hip)
    std::vector<vc_render*> renders;                          // live render contexts (render.hip); vc_engine_destroy destroys what is left

    // ---- measurement ----------------------------------------------------------------------------------
    bool profiling = false;
    // in-flight conv profiling (vc_profile_enable(e, 2)): event pairs recorded on the launch stream WITHOUT synchronising, so the
    // timed steps keep their three overlapping streams; resolved by vc_profile_read.  Only the thread that issues convs uses it.
    bool prof_async = false;
    struct ProfPair {
        hipEvent_t a, b; double flops, bytes;
        const int* rows = nullptr; double flops_per_row = 0, bytes_per_row = 0;   // + *rows x per-row work (pinned copy of the device row count)
        double flops_dense = 0, bytes_dense = 0;
    };
    std::vector<ProfPair> prof_pairs;
    size_t prof_used = 0;
    double prof_conv_union_ms = 0, prof_conv_span_ms = 0;     // set when the in-flight pairs are resolved (vc_profile_read)
    vc::ProfCat prof[VC_PROF_NCAT];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::map<std::string, int> tuned;            // conv autotune cache: shape signature -> tile config (engine_run.hip::tune_key)
    bool tuned_dirty = false;
    std::string op_log;                          // per-launch lines "name M N K tile ms" while profiling
    double last_ms = 0;
    // launch recorder (engine_record.hip, diagnostics): null until a pass is recorded; rec_armed = 1 + the net whose next pass is (0: none)
    vc::LaunchRecorder* rec = nullptr;
    int rec_armed = 0;

    // ---- stream injection -----------------------------------------------------------------------------
    std::vector<float> inject_det;
    std::vector<int> inject_count;
    int inject_b = 0, inject_n = 0;
};

// A live counter (live_count.hip) and, once vc_live_overlay_enable has run, its overlay list builder (live_overlay.hip)
namespace vc { struct LiveOverlay; struct LiveCkpt; }
struct vc_live {
    vc_engine* e = nullptr;
    int n_cam = 0, n_labels = 0, max_dir = 0;
    std::vector<int> trackers;               // [n_cam * n_labels] tracker slots
    std::vector<long long> frames_done;      // [n_cam] frames handed to the tracker so far
    vc::LiveCountArgs dev{};                 // the counter part; the batch part is filled per launch
    std::vector<void*> allocs;               // device memory of this counter
    int32_t* h_out = nullptr;                // pinned: counts + stats
    std::vector<int> n_dir;                  // [n_cam]
    vc::LiveOverlay* ov = nullptr;           // null until vc_live_overlay_enable: then every uniform tracker launch builds its lists
    std::vector<double> h_poly, h_dirs;      // the zones as the device holds them (padded): what vc_live_restore compares a blob's zones with
    std::vector<int> poly_n;                 // [n_cam]
    vc::LiveCkpt* ck = nullptr;              // null until vc_live_checkpoint_enable (live_ckpt.hip)
};

namespace vc {
// engine.hip
int pack_and_upload(std::vector<void*>& allocs, ConvParam& p, int prec, float act_scale = 1.0f);   // p.w / p.b -> packed device weights, bias, fp8 scales
inline int dev_alloc(vc_engine* e, void** p, size_t bytes) { return dev_alloc(e->allocs, p, bytes); }
// the counter pair of the next fused launch of the kernel with this bit of option "dyn_tiles_mask" (1 front, 2 C3, 4 Bottleneck); null (its bit
// clear, or option "dyn_tiles" 0, which switches every kernel back whatever the mask) = the fixed stride
inline unsigned* tile_ctr_next(vc_engine* e, int bit) {
    if (!e->d_tile_ctr || !e->opt.dyn_tiles || !(e->opt.dyn_tiles_mask & bit)) return nullptr;
    return e->d_tile_ctr + (size_t)(e->tile_ctr_seq++ % e->tile_ctr_ring) * 16;
}
int dev_realloc(vc_engine* e, void** p, size_t bytes);            // frees *p (if it belongs to the engine) and allocates anew
int host_alloc(vc_engine* e, void** p, size_t bytes);
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// engine_plan.hip: the two networks and their op plans
extern const float kAnchors[3][6];
void yolo_define(vc_engine* e);
int yolo_alloc(vc_engine* e);
int yolo_build_ops(vc_engine* e, int B, int Hn, int Wn, bool sparse, YoloPlan& plan);
void reid_define(vc_engine* e);
int reid_alloc(vc_engine* e);
int reid_build_ops(vc_engine* e, int k0, int k, ReidPlan& plan);
int reid_cpad(int prec);                                          // channels of the ReID input buffer
View mkview(const View& buf, int B, int H, int W, int C, int co);
// The one place a ConvP is filled from a packed parameter: the plans (PlanBuilder::conv) and the entry points that launch one convolution
// or a fused block on host arrays (host_conv.hip) both go through it, so a test launches what the engine would launch.  in / out: channel
// slices of NHWC buffers; B x H x W: the logical input (a pair_stem parameter reads it as H x W/2 pixels of 8 channels).  Everything else
// (residual, second destination, out_f32 / out_bf16, m_dev, in_up, cfg / ablate / slots) is the caller's to set on the result.
struct ConvSlice { void* ptr; int cs, co; };
ConvP conv_params(const ConvParam& p, ConvSlice in, ConvSlice out, int B, int H, int W, int kh, int kw, int stride, int pad, int act,
                  float act_scale, float inv_act_scale);
// engine_run.hip: running them
void tune_cache_load(vc_engine* e);
void tune_cache_save(vc_engine* e);
void tune_cache_publish(vc_engine* e);
void plans_retune(vc_engine* e);
void autoshape_net_size(const int* h, const int* w, int n, int size, int& nh, int& nw);
LetterboxGeom letterbox_geom(int h0, int w0, int nh, int nw, bool swap_rb);
int yolo_forward(vc_engine* e, int B, int nh, int nw);
int reid_forward(vc_engine* e, int k, hipStream_t rs, float* feat_out);
int run_detector_dev(vc_engine* e, const uint8_t* d_frames, int B, int h, int w, bool swap_rb);   // frames same size, on device
// a sized batch: frame f (dims[f]) at d_frames + f * cell, every frame's own network shape nh x nw; one letterbox launch, the unfused stem
int run_detector_dev_sized(vc_engine* e, const uint8_t* d_frames, int B, const vc_frame_dims* dims, size_t cell, int nh, int nw, bool swap_rb);
int run_reid_dev(vc_engine* e, const uint8_t* d_frames, int H, int W, int k);                      // crops in e->d_crops -> e->d_feat
int run_reid_on(vc_engine* e, const uint8_t* d_frames, int H, int W, int k, const int* d_crops, float* feat_out, hipStream_t rs,
                const CropFrame* d_ftab = nullptr);     // d_ftab: per-frame {offset, pitch} of a sized batch (device)
// engine_record.hip: *out = the recorder if the next pass of `net` (this one, over `ops`) is armed, else null; the copies around one launch
// of op[0 .. n_ops) on its stream (cp: this pass's copy of op[0].conv, null for the other kinds); what vc_engine_destroy calls
int record_begin(vc_engine* e, int net, const std::vector<Op>& ops, LaunchRecorder** out);
int record_before(LaunchRecorder* r, vc_engine* e, const Op* op, int n_ops, int cfg, const ConvP* cp, bool u8_src, bool side, hipStream_t s);
int record_after(LaunchRecorder* r, hipStream_t s);
void record_free(vc_engine* e);
// stream.hip: the slot rules of vc_stream_stage_host (shared with the YUV staging calls): checks, creates the copy stream and the four
// slots on first use, and hands out the next slot round-robin.  The caller enqueues its work on e->cstream, then calls ingest_publish.
int ingest_take_slot(vc_engine* e, int b, int h, int w, int* slot);
size_t ingest_slot_bytes(const vc_engine* e);
int ingest_publish(vc_engine* e, int slot, void** frames_dev_out);
inline bool nms_capacity_ok(int max_cand, int max_det) { return max_cand % 64 == 0 && max_cand >= 64 && max_cand <= 8192 && max_det >= 1; }   // launch_nms's sizes
// yuv_ingest.hip / yuv_egress.hip: descriptor validation (pure host code) and the two conversions, both enqueued on `s`
int yuv_resolve(const vc_yuv_desc* d, int b, int h, int w, YuvGeom& g);
// yuv_resolve for a destination: the ingest-only formats (VC_PIX_P016 .. VC_PIX_I444) are refused first, by name
int yuv_resolve_out(const vc_yuv_desc* d, int b, int h, int w, YuvGeom& g);
// The rules of a sized batch (pure host code): every size in 1 .. 1 << 15, every frame's own network shape at img_size that of frame 0;
// the cell (the largest frame, rounded up to 16 bytes) and the largest height and width.  Capacities are the caller's to check.
struct SizedDims { size_t cell = 0; int net_h = 0, net_w = 0, max_h = 0, max_w = 0; };
int sized_dims_resolve(const vc_frame_dims* dims, int b, int img_size, SizedDims& out);
size_t yuv_batch_bytes(const YuvGeom& g, int b);
int launch_yuv_to_bgr(const YuvGeom& g, const uint8_t* src, uint8_t* dst, int b, hipStream_t s);
int launch_bgr_to_yuv(const YuvGeom& g, const uint8_t* src_bgr, uint8_t* dst_yuv, int b, hipStream_t s);
// class_filter.hip: the rules of a class map (pure host code): n entries in [-1, n), at least one >= 0; n_labels = largest label + 1
int class_map_check(const int* label_of_class, int n, int* n_labels, int* n_kept);
// overlay.hip: the checks of vc_overlay on the host lists, and overlay_kernel over device-resident lists on `s` (no host wait)
int overlay_check_lists(int b, const int32_t* prims12, const int32_t* frame_first);
int launch_overlay(uint8_t* frames_dev, int b, int h, int w, const void* d_prims, const int* d_first, hipStream_t s);
// render.hip
void render_destroy_all(vc_engine* e);
struct ProfScope {
    vc_engine* e; int cat; double flops, bytes;
    hipStream_t s;
    ProfScope(vc_engine* e_, int cat_, double flops_ = 0, double bytes_ = 0, hipStream_t s_ = nullptr);
    ~ProfScope();
};
// tracker.hip
int tracker_init_pool(vc_engine* e);
// Build + enqueue one tracker batch on the tracker stream (after `wait`, if given, has fired on the GPU).  frame_groups[f] lists
// (class label, tracker id, prepared detections) of frame f in class order.  Rows land in stage `st`; track_collect waits for them.
struct FrameClassDets { int label, tracker; Prepared dets; };
// frame_dims (a sized batch, else nullptr): the tasks of frame f clamp their rows to frame_dims[f] instead of W x H.
// frame_tracker (else nullptr): per frame the slot of one tracker of the frame's camera -- a frame without tasks still advances the frame
// number of its camera's live counter; without it the camera is that of the frame's first task.
int track_enqueue(vc_engine* e, int st, const std::vector<std::vector<FrameClassDets>>& frames, const float* d_feat, int W, int H,
                  int rows_cap, hipEvent_t wait, const vc_frame_dims* frame_dims = nullptr, const int* frame_tracker = nullptr);
// live_count.hip: the counters that own one of batch_trackers (slots), ready for launch_track_batch; the next frame number of a tracker's
// camera (0: not attached); what vc_engine_destroy calls.  counting.hip: the all-gather of a counter's device tensor.
void live_batch_args(vc_engine* e, const std::vector<int>& batch_trackers, const long long* d_frame_no, std::vector<LiveCountArgs>& out);
long long live_next_frame(vc_engine* e, int tracker_slot);
void live_destroy_all(vc_engine* e);
int live_allgather(vc_engine* e, const LiveCountArgs& a, int32_t* out);
// live_overlay.hip: the overlay lists a tracker launch builds for the counters whose overlay is enabled.
//   live_overlay_room    what a run call asks first: VC_ERR_STATE if a counter of one of these tracker HANDLES has no free list buffer
//   live_overlay_begin   in front of the batch's apply launch, before the batch's frames are numbered: the counters of the batch's frames
//                        (frame_trk[f]: slot of a tracker of frame f's camera, -1 none) with an enabled overlay; enqueues their counts read
//   live_overlay_finish  behind the apply launch: the build launches into a free list buffer, and the event behind them.  a: the tracker
//                        launch's arguments, null for a batch without a task
//   live_overlay_take    the oldest unconsumed lists in device memory for a render context (render.hip), released by live_overlay_release
struct LiveOverlayPlan { vc_live* live; std::vector<int> text_cam; };
int live_overlay_room(vc_engine* e, const int* tracker_handles, int n);
int live_overlay_begin(vc_engine* e, const std::vector<int>& frame_trk, hipStream_t s, std::vector<LiveOverlayPlan>& plans);
int live_overlay_finish(vc_engine* e, std::vector<LiveOverlayPlan>& plans, const std::vector<int>& frame_trk, const long long* frame_no,
                        const TrackBatchArgs* a, int n_tasks, int b, int h, int w, hipStream_t s);
int live_overlay_take(vc_live* l, int b, int h, int w, const void** d_prims, const int** d_first, hipEvent_t* built, int* token);
int live_overlay_release(vc_live* l, int token);      // VC_ERR_CAPACITY if a frame of that batch did not fit its arena
void live_overlay_free(vc_live* l);
// live_ckpt.hip: waits for a checkpoint in flight and frees what vc_live_checkpoint_enable allocated
void live_ckpt_free(vc_live* l);
// tracker.hip: the free-slot stack from the host (engine idle): take n slots / give slots back
int host_take_slots(vc_engine* e, int n, std::vector<int>& out);
int host_give_slots(vc_engine* e, const std::vector<int>& slots);
// render.hip: before a counter's lists are freed -- waits for the contexts that read them and drops their references
void render_forget_live(vc_engine* e, vc_live* l);
// rows6 per frame: out_rows6[f * cap_rows_per_frame * 6 ...], out_m[f]
int track_collect(vc_engine* e, int st, int64_t* out_rows6, int cap_rows_per_frame, int* out_m);
int track_idle(vc_engine* e);              // wait until no tracker batch is in flight (stream path included)
int async_wait_all(vc_engine* e);          // stream.hip: the same, named as the blocking entry points call it
// det_prep.h's prepare_frame under each in-range class's own tracker parameters (handle trackers[c]), and a prepared frame -> its tasks
void prepare_for_trackers(vc_engine* e, const int* trackers, int num_classes, const FrameDets& d, int row_base, PrepScratch& scratch, FramePrepared& out);
int frame_tasks(vc_engine* e, const int* trackers, int num_classes, FramePrepared& prep, std::vector<FrameClassDets>& out);
// one frame already on the device, blocking: the boxes of label c (all in [0, num_classes)) go to the tracker with handle trackers[c]
int frame_track(vc_engine* e, const uint8_t* d_frame_base, int frame_index, int H, int W, const int* trackers, int num_classes, const FrameDets& d,
                std::vector<int64_t>& rows6);
}  // namespace vc
