/* libvcount_hip.so -- C ABI of the MI355X-native detect + track hot path of kaylode/vehicle-counting.
 *
 * The reference is pure Python and has no FFI layer; its seam is the duck-typed stage API that
 * modules/__init__.py:54-84 (CountingPipeline.run) calls.  Each group of entry points below is what a
 * ctypes binding of one of those Python operators would call (see INTEGRATION.md for the stubs):
 *
 *   vc_detect*            <- modules/detect.py:30-60 ImageDetect.run -> networks/detector.py:36-38
 *                            -> networks/yolo.py:68-99 YoloBackbone.detect (AutoShape forward: letterbox, YOLOv5
 *                            v6.0 conv stack, Detect decode, NMS, scale_coords)
 *   vc_embed              <- networks/deepsort/deep/feature_extractor.py:42-47 Extractor.__call__ on the crops
 *                            cut by networks/deepsort/deep_sort.py:119-129 DeepSort._get_features
 *   vc_tracker_* / vc_deepsort_update
 *                         <- networks/deepsort/deep_sort.py:25-59 DeepSort.update
 *                            (sort/tracker.py:50-91 Tracker.predict/update and everything below it)
 *   vc_videotracker_run   <- modules/track.py:30-70 VideoTracker.run (one DeepSORT per class)
 *   vc_stream_*           <- the per-frame body of modules/__init__.py:54-84 for device-resident frames
 *   vc_*_host             <- single-function entry points used by the parity tests (one reference function each)
 *
 * Conventions: every function returns an int status (VC_OK == 0); vc_last_error() gives the message for
 * the calling thread.  Handles are opaque, thread-compatible (not thread-safe), own their device memory
 * and HIP streams, and never call back into the caller.  All array arguments are caller-owned plain
 * host pointers unless the name says `_dev`; outputs are caller-allocated.  No torch types anywhere.
 */
#ifndef VCOUNT_HIP_H
#define VCOUNT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC_OK 0
#define VC_ERR_ARG 1       /* bad argument / shape */
#define VC_ERR_HIP 2       /* HIP runtime error (no device, OOM, launch failure) */
#define VC_ERR_STATE 3     /* call order (e.g. run before finalize) */
#define VC_ERR_CAPACITY 4  /* a configured capacity (tracks, candidates, crops) was exceeded */
#define VC_ERR_NOTFOUND 5  /* unknown parameter name / handle id */

#define VC_PREC_BF16 0     /* bf16 activations/weights, fp32 accumulate (throughput mode) */
#define VC_PREC_F32 1      /* fp32 everywhere (tight-parity mode) */
#define VC_PREC_FP8 2      /* detector convs on the MX-scaled fp8 MFMA (OCP e4m3fn activations, per-channel-scaled e4m3fn weights,
                              fp32 accumulate); the 3-channel stem, the Detect logits and the ReID net stay bf16 */

#define VC_FEAT_DIM 512    /* networks/deepsort/deep/model.py: embedding width */
#define VC_REID_SIZE 50    /* feature_extractor.py:18 */

int vc_version(void);
const char* vc_last_error(void);
int vc_device_count(int* n);

/* ------------------------------------------------------------------------------------------------
 * Engine: one per process / GPU.  Holds the detector, the ReID net, the tracker pool and the streams.
 * ---------------------------------------------------------------------------------------------- */
typedef struct vc_engine vc_engine;

typedef struct vc_engine_config {
    int device;            /* HIP device ordinal */
    int precision;         /* VC_PREC_* */
    int yolo_variant;      /* 0 = yolov5s, 1 = yolov5m, 2 = yolov5l, 3 = yolov5x (bf16 / fp32 only)  (configs/configs.yaml: model_name) */
    int num_classes;       /* detector classes == tracker fan-out (modules/__init__.py:33) */
    int img_size;          /* AutoShape `size`, 640 in the reference (quirk Q8) */
    int max_batch;         /* frames per detect launch */
    int max_frame_h, max_frame_w; /* largest source frame */
    float conf_thres;      /* configs/configs.yaml: min_conf 0.25 */
    float iou_thres;       /* configs/configs.yaml: min_iou 0.45 */
    int max_det;           /* configs/configs.yaml: max_det 300 */
    int max_candidates;    /* per-frame cap on boxes entering NMS (upstream max_nms = 30000) */
    int max_crops;         /* ReID crops per launch */
    int max_tracks;        /* live tracks over all trackers */
    int nn_budget_cap;     /* largest NN_BUDGET any tracker will ask for */
    int with_detector;     /* 0: skip building the YOLO plan (track-only users) */
    int with_reid;         /* 0: skip building the ReID plan */
    int max_trackers;      /* (camera, class) trackers the engine can hold (device-resident headers + track lists) */
    int tracks_per_tracker;/* live tracks one tracker may hold (<= 512: the device step keeps its work arrays in LDS) */
} vc_engine_config;

int vc_engine_config_default(vc_engine_config* cfg);
int vc_engine_create(const vc_engine_config* cfg, vc_engine** out);
int vc_engine_destroy(vc_engine* e);

/* Parameters: conv layers addressed by the checkpoint's own names ("model.0.conv", "layer2.0.conv1", ...);
 * weights OIHW fp32 with BatchNorm already folded (vehicle-counting_amd/weights.py: fold_bn). */
#define VC_NET_YOLO 0
#define VC_NET_REID 1
int vc_engine_param_count(const vc_engine* e, int net, int* n);
int vc_engine_param_info(const vc_engine* e, int net, int index, char* name, int name_cap, int dims[4] /* O,I,kh,kw */);
int vc_engine_set_param(vc_engine* e, int net, const char* name, const float* w_oihw, const float* bias);
/* Detect anchors in pixels, 3 levels x 3 anchors x (w, h) = `model.24.anchors * stride` of an ultralytics checkpoint (custom
 * weights loaded by /root/reference/networks/yolo.py:58 may carry autoanchor values).  Default: the COCO set of yolov5{s,m,l,x}.yaml. */
int vc_engine_set_anchors(vc_engine* e, const float* anchors18);
int vc_engine_finalize(vc_engine* e); /* packs + uploads weights; detector/ReID calls are valid afterwards */
/* Kernel-selection switches of a live engine (defaults come from the environment at vc_engine_create: VC_C3_FUSED, VC_BNECK_FUSED,
 * VC_FRONT_FUSED, VC_CROP_PER_PIXEL, VC_DOT_ARENA_MB).  Names: "c3_fused", "bneck_fused", "bneck_cv3" (0 / 1), "front_fused" (0 off, 1 stream path,
 * 2 always), "crop_per_pixel", "sparse_head", "reid_block_fused", "fuse_upsample", "sppf_sep", "fuse_s2_pw", "stem_direct", "head_side" (0 / 1; stem_direct: 0 sends
 * the bf16 detector stem through the implicit GEMM like any other layer, for every variant; head_side: the P3 / P4 Detect-head ops on their own stream
 * beside the neck layers that follow them), "dot_arena_mb" (largest appearance-table arena the tracker may allocate or, once
 * it is allocated, use: lowering it on a live engine bounds the tables of the next launch; 0 = compute the appearance rows inside
 * the walk).  The parity tests use it to compare a fused kernel with the launches it replaces.
 * "embed_kept_only" (default 1, environment VC_EMBED_KEPT_ONLY): crop and embed only the boxes DeepSort.update's own filter keeps
 * (conf > min_confidence, then DeepSORT's NMS per class, deep_sort.py:31-37).  The reference embeds every box first and drops the rest
 * afterwards; a dropped box never becomes a Detection, so its feature is never read and the rows are the same.  0 embeds every box. */
int vc_engine_set_option(vc_engine* e, const char* name, int value);
/* Class filter and label map of the detector.  networks/yolo.py:20,64: get_model hands the keys of args.mapping_dict to
 * YoloBackbone as filter_classes -> model.classes, which non_max_suppression applies behind the conf tests and in front of the max_nms trim,
 * the NMS and the max_det cut; modules/detect.py:41-46: ImageDetect.run relabels what is left.  label_of_class[c] = -1
 * drops every detection whose best class over ALL classes is c (nothing is reassigned), l >= 0 is the label the detection leaves the engine
 * with, on every detect path (vc_detect, the stream path, vc_stream_embed).  Labels need not be dense (n_labels = largest + 1) and classes
 * may share one; the NMS separates ORIGINAL classes, so overlapping boxes of two classes with one label both survive, as they do in the
 * reference's relabel after the NMS.  max_candidates is judged on the unfiltered candidates; vc_stream_inject rows are taken as given;
 * vc_detect_debug_pred / _layer are unchanged.  NULL clears the map.  n != num_classes, an entry outside [-1, n) or no entry >= 0:
 * VC_ERR_ARG before any device call; an engine without a (finalized) detector, or a stream path that holds a pending submission or an
 * outstanding batch: VC_ERR_STATE.  The table is copied on the detector stream from a pinned copy the engine owns. */
int vc_engine_set_class_map(vc_engine* e, const int* label_of_class, int n);
/* The map in force -- model.classes (networks/yolo.py:64) and the relabel (modules/detect.py:41-46) as one table; the identity and
 * n_labels = num_classes when none is set.  n must be num_classes. */
int vc_engine_class_map(const vc_engine* e, int* label_of_class, int n, int* n_labels);
/* The rules of such a table alone (what vc_engine_set_class_map checks of filter_classes, networks/yolo.py:20), pure host code:
 * n_labels = largest label + 1, n_kept = classes with a label (both nullable). */
int vc_class_map_check_host(const int* label_of_class, int n, int* n_labels, int* n_kept);

/* ---- detect: ImageDetect.run ------------------------------------------------------------------ */
/* rgb[i]: H[i] x W[i] x 3 uint8 RGB.  out_det: n * max_det * 6 floats [x1,y1,x2,y2,conf,cls] in source pixels
 * (what AutoShape returns in results.xyxy); out_count[i] = detections of image i.  All images of one call
 * share the AutoShape inference shape (models/common.py v6.0). */
int vc_detect(vc_engine* e, const uint8_t* const* rgb, const int* h, const int* w, int n, float* out_det, int* out_count);
/* Diagnostics for tensor-level parity: the network tensor the detector saw, raw head, candidates. */
int vc_detect_debug_shape(const vc_engine* e, int* net_h, int* net_w, int* n_candidates);
int vc_detect_debug_layer(vc_engine* e, int layer /* 0..23, or -1 = preprocessed input */, float* out_nhwc, size_t cap_floats,
                          int dims[4] /* B,H,W,C */);
int vc_detect_debug_pred(vc_engine* e, float* out /* B * n_candidates * (5+nc) */, size_t cap_floats);

/* Launch recorder (diagnostics): vc_record_arm makes the NEXT pass of `net` (VC_NET_YOLO: vc_detect, a stream submission; VC_NET_REID:
 * vc_embed, vc_embed_tensor, the stream path's ReID) keep, for every launch of its op plan, the ops the launch covered with every
 * launch-view field, the bytes of every buffer it reads (copied just before the launch) and of every buffer it writes (copied before
 * and after), on the launch's own stream.  A launch made while the conv autotuner still times candidates sees their stores in its
 * before-copy: run the shape once before arming.  vc_record_list returns the records as JSON text (buf == NULL: only the size);
 * vc_record_read copies the arena the records' "before" / "after" offsets point into, after waiting for the engine's streams.
 * Unarmed, a pass tests one pointer per launch; the arena is allocated by an armed pass and freed with the engine. */
int vc_record_arm(vc_engine* e, int net);
int vc_record_list(vc_engine* e, char* buf, size_t cap, size_t* size);
int vc_record_read(vc_engine* e, void* out, size_t cap_bytes);

/* ---- embed: Extractor.__call__ over DeepSort._get_features crops -------------------------------- */
/* bgr: H x W x 3 uint8 (the `ori_img` the reference crops from).  boxes_cxcywh: k x 4 float64 centre boxes
 * (deep_sort.py:28 bbox_xywh).  out_feat: k x 512 float32, unit L2 norm. */
int vc_embed(vc_engine* e, const uint8_t* bgr, int h, int w, const double* boxes_cxcywh, int k, float* out_feat);
/* Diagnostics: the k x 50 x 50 x 3 network input the last vc_embed built (Extractor._preprocess: resize, /255, Normalize), as float32. */
int vc_embed_debug_input(vc_engine* e, int k, float* out_nhwc, size_t cap_floats, int dims[4] /* k,50,50,3 */);
int vc_embed_tensor(vc_engine* e, const float* x_nchw /* k x 3 x 50 x 50 */, int k, float* out_feat);

/* ---- tracker: sort/tracker.py + deep_sort.py ------------------------------------------------------ */
typedef struct vc_tracker_params {
    double max_dist;          /* MAX_DIST          (cosine matching threshold) */
    double min_confidence;    /* MIN_CONFIDENCE */
    double nms_max_overlap;   /* NMS_MAX_OVERLAP */
    double max_iou_distance;  /* MAX_IOU_DISTANCE */
    int max_age;              /* MAX_AGE */
    int n_init;               /* N_INIT */
    int nn_budget;            /* NN_BUDGET (<= engine nn_budget_cap) */
} vc_tracker_params;

/* tracker_id is an opaque handle (slot | generation << 16): every entry point that takes one refuses (VC_ERR_NOTFOUND / VC_ERR_ARG) a handle
 * whose tracker has been destroyed, also after its slot has been handed to a later vc_tracker_create. */
int vc_tracker_create(vc_engine* e, const vc_tracker_params* p, int* tracker_id);
/* Drops every track (their pool slots return) and clears the error of a stopped tracker.  A tracker stops at its first capacity
 * error -- more tracks + detections in a step than tracks_per_tracker (that step changes nothing), an exhausted track pool, more rows
 * than the caller's room: the launch returns VC_ERR_CAPACITY naming it, the other trackers of the launch step as usual, and every later
 * step asked of the stopped tracker is refused with the same error until this call. */
int vc_tracker_reset(vc_engine* e, int tracker_id);
/* Gives the tracker's tracks and its slot back.  The reference drops its VideoTracker after every video (modules/__init__.py:32-36); the
 * drop-in's DeepSort calls this when it is closed. */
int vc_tracker_destroy(vc_engine* e, int tracker_id);
/* Tracker.predict() + Tracker.update(detections) for detections already filtered/NMS'ed by the caller.
 * tlwh: k x 4 f64, conf: k f64, feat: k x 512 f32 (host). */
int vc_tracker_step(vc_engine* e, int tracker_id, const double* tlwh, const double* conf, const float* feat, int k);
/* Snapshot of the live tracks in list order (sort/tracker.py: self.tracks). Any pointer may be NULL. */
int vc_tracker_count(vc_engine* e, int tracker_id, int* n);
int vc_tracker_state(vc_engine* e, int tracker_id, int cap, int64_t* ids, int* state, int* hits, int* age, int* tsu,
                     double* mean8, double* cov64, int* gallery_count);
/* Cost matrices of the last blocking step that stepped exactly ONE tracker (vc_tracker_step, vc_deepsort_update), as the tracker
 * kernel computed them: app[t*D + d] = gated min-cosine cost (sort/nn_matching.py:160-177 + linear_assignment.py:148-192) of list
 * position t, valid for the tracks that were confirmed when the step began; iou[t*D + d] = 1 - IoU (sort/iou_matching.py:40-81), valid
 * for the IoU candidates.  T = live tracks before the step, D = detections of the step.  Parity tests read the HOT kernel's numbers. */
int vc_tracker_debug_costs(vc_engine* e, int cap_entries, double* app, double* iou, int* T, int* D);
/* Tracker state for stream migration (the reference keeps it in Python objects, sort/tracker.py:40-60 and
 * sort/track.py:64-80, and cannot move a stream): parameters, id counter, per track the FSM counters, fp64 Kalman mean and
 * covariance and the valid gallery rows.  vc_tracker_snapshot with buf == NULL only reports the size.  vc_tracker_restore
 * replaces the state (and parameters) of an existing tracker of any engine whose nn_budget_cap >= the snapshot's nn_budget. */
int vc_tracker_snapshot(vc_engine* e, int tracker_id, void* buf, size_t cap, size_t* size);
int vc_tracker_restore(vc_engine* e, int tracker_id, const void* buf, size_t size);
/* DeepSort.update: boxes xyxy (k x 4 f64) + confidences on a BGR frame -> rows [x1,y1,x2,y2,track_id,-1,0].
 * Both blocking calls run the update's detection filter (deep_sort.py:31-37) before the crops are cut and, with the option
 * "embed_kept_only", embed only the boxes it keeps; max_crops and the empty-crop refusal still count every box. */
int vc_deepsort_update(vc_engine* e, int tracker_id, const uint8_t* bgr, int h, int w, const double* bbox_xyxy,
                       const double* conf, int k, int64_t* out_rows7, int cap_rows, int* out_m);
/* VideoTracker.run: trackers[c] is the tracker id of class c.  boxes xywh (top-left), labels, scores as
 * ImageDetect.run returns them.  Output rows [x1,y1,x2,y2,track_id,label]. */
int vc_videotracker_run(vc_engine* e, const int* trackers, int num_classes, const uint8_t* bgr, int h, int w,
                        const double* boxes_xywh, const int64_t* labels, const double* scores, int n,
                        int64_t* out_rows6, int cap_rows, int* out_m);

/* ---- fused stream path: the per-frame body of CountingPipeline.run on device-resident frames -------- */
/* frames_dev: device pointer to B x H x W x 3 uint8 *BGR* frames (cv2.VideoCapture order; the RGB view
 * the detector needs is taken on the fly).  Results per frame: rows [x1,y1,x2,y2,track_id,label]. */
/* vc_stream_submit enqueues the detector for a batch and returns at once (at most two outstanding); vc_stream_run consumes
 * submissions in order (submitting itself when none is pending), so `submit(i+1); run(i)` overlaps detect(i+1) with track(i). */
int vc_stream_submit(vc_engine* e, const void* frames_dev, int b, int h, int w);
/* Frames in (pinned) HOST memory, as the reference's loader delivers them (modules/datasets.py:47-61).  vc_stream_stage_host copies the
 * batch to one of four device staging slots on the engine's copy stream and returns at once; *frames_dev_out is the device address to
 * hand to vc_stream_submit and then vc_stream_run / vc_stream_run_async for this batch (valid until its rows have been collected; at
 * most four host batches may be alive).  vc_stream_submit of a staged address enqueues the detector behind the copy.  Staging one
 * batch further ahead than submitting -- stage(i+2); submit(i+1); run(i); collect(i-1) -- puts the PCIe copy under the detector of the
 * batch before.  vc_stream_submit_host = stage + submit in one call (the copy then sits in front of its own detector). */
int vc_stream_stage_host(vc_engine* e, const uint8_t* frames_host, int b, int h, int w, void** frames_dev_out);
int vc_stream_submit_host(vc_engine* e, const uint8_t* frames_host, int b, int h, int w, void** frames_dev_out);
int vc_stream_run(vc_engine* e, const int* trackers, int num_classes, const void* frames_dev, int b, int h, int w,
                  int64_t* out_rows6, int cap_rows_per_frame, int* out_m /* b */, int* out_ndet /* b, may be NULL */);

/* ---- 4:2:0 YUV ingest: what a video decoder hands out (the reference gets BGR because cv2.VideoCapture converts on the CPU,
 * modules/datasets.py:47-61) -------------------------------------------------------------------------------------------- */
#define VC_PIX_NV12 0      /* Y plane, then one plane of interleaved U,V at half resolution (hardware decoder surfaces) */
#define VC_PIX_I420 1      /* Y, U and V planes (software decoders) */
/* Ingest only (every source descriptor takes them; egress and the render path's out_desc refuse them with VC_ERR_ARG).  Ids 2..15 and
 * >= 20 are unknown formats. */
#define VC_PIX_P016 16     /* NV12's planes with little-endian 16-bit samples, significant bits at the TOP: HEVC Main10 / AV1 10-bit decoder
                              surfaces.  P010 and P012 surfaces are passed as this format. */
#define VC_PIX_I010 17     /* I420's planes with little-endian 16-bit samples, 10 significant bits at the BOTTOM (yuv420p10le) */
#define VC_PIX_I422 18     /* Y, U and V planes, 8-bit, chroma at half width and FULL height (MJPEG cameras) */
#define VC_PIX_I444 19     /* Y, U and V planes, 8-bit, chroma at full resolution (H.264 High 4:4:4, screen sources) */
#define VC_YUV_BT601 0
#define VC_YUV_BT709 1
/* Geometry in BYTES from the start of a frame; 0 = tightly packed (pitch_y = w; pitch_c = w for NV12, w / 2 for I420; offset_c =
 * pitch_y * h; offset_v = offset_c + pitch_c * h / 2; frame_stride = end of the last plane).  A decoder surface gives the explicit
 * form, e.g. pitch 1536 for a 1280-wide frame with the chroma plane at pitch x aligned height.  offset_v is ignored for NV12.
 * Per format (everything stays in bytes, the rule for the zeros is the same: offset_c = pitch_y * h, offset_v = offset_c + pitch_c *
 * chroma rows; offset_v is ignored for P016 too; no evenness rule for pitches, offsets or addresses):
 *              luma row bytes   chroma row bytes   chroma rows   chroma of pixel (x, y)   size rule            bytes read / px
 *   NV12       w                w                  h / 2         (x >> 1, y >> 1)         h, w even            1.5
 *   I420       w                w / 2              h / 2         (x >> 1, y >> 1)         h, w even            1.5
 *   P016       2 w              2 w                h / 2         (x >> 1, y >> 1)         h, w even            3
 *   I010       2 w              w                  h / 2         (x >> 1, y >> 1)         h, w even            3
 *   I422       w                w / 2              h             (x >> 1, y)              w even, h >= 1       2
 *   I444       w                w                  h             (x, y)                   h, w >= 1            3                     */
typedef struct vc_yuv_desc {
    int format;            /* VC_PIX_* */
    int matrix;            /* VC_YUV_BT601 / VC_YUV_BT709 */
    int full_range;        /* 0: limited (Y 16..235), 1: full (0..255) */
    int pitch_y, pitch_c;
    size_t offset_c, offset_v, frame_stride;
} vc_yuv_desc;
int vc_yuv_desc_default(vc_yuv_desc* d);   /* NV12, BT.601, limited range, tightly packed */
/* Arithmetic (integer, 32-bit signed): u = U - 128, v = V - 128, chroma replicated over its 2 x 2 luma block,
 *   R = clamp((y + (1 << 19) + CVR * v) >> 20), G = clamp((y + (1 << 19) + CVG * v + CUG * u) >> 20), B = clamp((y + (1 << 19) + CUB * u) >> 20)
 * with y = max(0, Y - 16) * CY (limited) or Y << 20 (full) and constants int(literal * 2^20): OpenCV's COLOR_YUV2BGR_NV12 for
 * BT.601 limited.  The wider formats extend this arithmetic, they do not add a second one: every sample of every plane is first reduced
 * to 8 bits -- P016: s8 = min(255, (s16 + 128) >> 8); I010: s8 = min(255, ((s16 & 1023) + 2) >> 2); 8-bit formats: s8 = s -- then the
 * arithmetic above is applied verbatim with the chroma sample the table names, replicated, never interpolated.  A 4:2:0 frame whose
 * samples are s8 << 8 (P016) or s8 << 2 (I010) therefore converts to the bytes NV12 / I420 of the s8 planes give.  10-bit input is
 * treated as SDR under BT.601 / BT.709.  Parity with cv2 / swscale is UNPINNED for every format.
 * h and w must be even where the table says so.  Bad geometry (a size the format refuses, unknown format / matrix, a pitch below the
 * row bytes, overlapping planes, a frame_stride below the frame, offsets out of range) is VC_ERR_ARG before any HIP call.
 * vc_stream_stage_yuv_host / _dev fill one of the four ingest slots of vc_stream_stage_host with the CONVERTED frames (same slot
 * rules, same VC_ERR_STATE refusals; BGR and YUV staging may be mixed): *frames_dev_out is an ordinary B x H x W x 3 BGR buffer
 * for vc_stream_submit / vc_stream_run*.  _host copies the raw YUV (1.5 B per pixel over PCIe; pinned memory for the copy to
 * overlap) into a per-slot raw buffer on the engine's copy stream and converts from there; _dev converts straight from the
 * caller's device surfaces, which must stay valid until the vc_stream_run / vc_stream_run_async call of that batch has returned. */
int vc_stream_stage_yuv_host(vc_engine* e, const vc_yuv_desc* d, const uint8_t* yuv_host, int b, int h, int w, void** frames_dev_out);
int vc_stream_stage_yuv_dev(vc_engine* e, const vc_yuv_desc* d, const void* yuv_dev, int b, int h, int w, void** frames_dev_out);
/* The same conversion outside the stream path, on the caller's own device buffers (frames for vc_overlay, measurement): enqueued on
 * the NULL stream, returns without waiting for it.  bgr_dev: b x h x w x 3 bytes. */
int vc_yuv_to_bgr_dev(const vc_yuv_desc* d, const void* yuv_dev, int b, int h, int w, void* bgr_dev);

/* Asynchronous form of vc_stream_run: the batch's tracker work is ONE kernel enqueued on the engine's tracker stream (no host
 * thread); the call returns as soon as the batch's ReID and tracker kernel are enqueued.  At most two batches may be outstanding.
 * vc_stream_collect returns the rows of the OLDEST outstanding batch (same layout as vc_stream_run) and blocks until they are
 * ready.  Calls that touch tracker state (vc_tracker_*, vc_deepsort_update, vc_videotracker_run) first wait for outstanding batches.
 * A submission that cannot be embedded (more than max_candidates boxes passed conf_thres, more boxes than max_crops, an empty crop)
 * is reported ONCE by the call that finds it and dropped; vc_stream_reset abandons everything in flight.
 * With the option "embed_kept_only" a batch is embedded under the filter (min_confidence, nms_max_overlap) that all trackers of the
 * most recent vc_stream_run_async* call share -- batches are embedded ahead of the call that names their trackers -- and only the boxes
 * DeepSort.update would turn into Detections (deep_sort.py:31-37) get a crop and a feature row.  If the trackers a batch is then run
 * with have other parameters, or disagree among themselves, the batch is embedded again in full before it is tracked: rows never depend
 * on the option.  max_crops, the empty-crop refusal and out_ndet count every box the detector returned. */
int vc_stream_run_async(vc_engine* e, const int* trackers, int num_classes, const void* frames_dev, int b, int h, int w,
                        int cap_rows_per_frame);
int vc_stream_collect(vc_engine* e, int64_t* out_rows6, int cap_rows_per_frame, int* out_m, int* out_ndet, int b);
/* The same for a batch that interleaves S cameras (the reference builds a new VideoTracker per video, modules/__init__.py:29-36; one
 * engine then serves S videos): frame f belongs to camera cam_of_frame[f] in [0, n_cam) and is stepped on trackers[cam * num_classes +
 * label]; the frames of one camera must appear in stream order inside the batch and across batches.  Rows come back per frame exactly
 * as from vc_stream_run_async (vc_stream_collect).  Per-camera latency is b / n_cam frames, and the tracker kernel walks
 * n_cam x num_classes trackers in parallel, b / n_cam steps each. */
int vc_stream_run_async_multi(vc_engine* e, const int* trackers /* n_cam x num_classes */, int n_cam, int num_classes, const int* cam_of_frame /* b */,
                              const void* frames_dev, int b, int h, int w, int cap_rows_per_frame);
int vc_stream_reset(vc_engine* e);
/* Running 64-bit totals over the stream path and the blocking tracker calls since the engine was created or vc_stream_reset was
 * called: boxes that reached the ReID stage, and crops the ReID net was run on (a batch embedded twice counts twice). */
int vc_stream_crop_stats(vc_engine* e, int64_t* boxes_detected, int64_t* crops_embedded);

/* ---- one stream on several GPUs: frame-sharded front end (ordering contract of modules/__init__.py:54-84) -------- */
/* Front half of the fused path for the OLDEST submission (vc_stream_submit): detections marshalled like networks/yolo.py:72-97 +
 * crops + ReID for EVERY box (deep_sort.py:119-129; the caller owns the tracking, so nothing is filtered, and a batch the look-ahead of
 * an earlier vc_stream_run_async* call embedded under its filter is embedded again in full).  out_rows7: n x [frame index in the batch, x1, y1, x2, y2, conf, label] float64 --
 * the boxes VideoTracker.run works on; frames without boxes contribute nothing (Q1).  *out_feat_dev: DEVICE address of the matching
 * n x 512 float32 embeddings, valid until the third following vc_stream_embed / vc_stream_run* call. */
int vc_stream_embed(vc_engine* e, const void* frames_dev, int b, int h, int w, double* out_rows7, int cap_rows, int* out_n, const float** out_feat_dev);
/* Variable-length all-gather of such rows + embeddings over RCCL / xGMI on the engine's stream (vc_comm_init first): rows of all ranks,
 * rank-major, counts per rank, and the DEVICE address of the gathered embeddings (valid until the next call). */
int vc_allgather_rows(vc_engine* e, const double* rows7, const float* feat_dev, int n, double* out_rows7, int cap_rows, int* out_counts /* world */,
                      const float** out_feat_dev);
/* VideoTracker.run (modules/track.py:30-70) for a run of frames whose detections and embeddings are supplied: rows7 sorted by frame key
 * (column 0, ascending integers), row i's embedding at feat_dev[i] (device).  One tracker kernel launch for the whole run.  Per distinct
 * key j, ascending: out_keys[j], out_m[j] rows [x1, y1, x2, y2, track_id, label] at out_rows6 + j * cap_rows_per_frame * 6. */
int vc_videotracker_run_features(vc_engine* e, const int* trackers, int num_classes, const double* rows7, const float* feat_dev, int n, int h, int w,
                                 int64_t* out_rows6, int cap_rows_per_frame, int* out_m, int64_t* out_keys, int cap_frames, int* out_n_frames);
/* Detection injection for throughput studies: replaces the detector's NMS output of the batches SUBMITTED from now on
 * (vc_stream_submit / vc_stream_submit_host capture it) with caller boxes after the conv stack has run. NULL clears. */
int vc_stream_inject(vc_engine* e, const float* det6 /* b x n x 6 */, const int* count, int b, int n);

/* ---- counting: VideoCounting.run + count_frame_directions, and the one collective of the multi-GPU design -------------------- */
/* modules/track.py:81-137 (zone filter: any box corner inside the polygon; per (label, track) first / last box; direction =
 * utilities/counting/utils.py:139-152 find_best_match_direction) and utilities/counting/utils.py:276-297 (count[direction][label] += 1
 * at each track's last frame).  dir_lines: n_dir x (x0, y0, x1, y1) in the order of the zone file's direction shapes. */
typedef struct vc_counter vc_counter;
int vc_counter_create(const double* polygon_xy, int n_points, const double* dir_lines, int n_dir, int num_classes, vc_counter** out);
int vc_counter_destroy(vc_counter* c);
int vc_counter_add(vc_counter* c, const int64_t* frames, const int64_t* track_ids, const int64_t* labels, const int64_t* boxes_xyxy, int n);
int vc_counter_tracks(const vc_counter* c, int* n);
int vc_counts(const vc_counter* c, int32_t* out /* n_dir x num_classes */);
/* utilities/counting/utils.py:154-198 save_tracking_to_csv as columns (colour excluded, Q10): one row per (track, frame) that passed
 * the zone filter, ordered by label, then by the track's first appearance, then by arrival.  direction = index of the direction line. */
int vc_counter_rows_count(const vc_counter* c, int64_t* n);
int vc_counter_rows(const vc_counter* c, int64_t cap, int64_t* track_id, int64_t* frame_id, int64_t* box4, int64_t* label, int32_t* direction,
                    double* fpoint2, double* lpoint2, int64_t* fframe, int64_t* lframe);
/* One all-gather of the per-camera count tensors over RCCL / xGMI on the engine's stream.  Rank 0 creates the 128-byte
 * id (vc_comm_unique_id) and hands it to the other ranks by any side channel (the Python shim broadcasts it with torch.distributed);
 * every rank then calls vc_comm_init.  out receives world x n values, rank-major. */
int vc_comm_unique_id(void* out128);
int vc_comm_init(vc_engine* e, int rank, int world, const void* id128);
int vc_comm_destroy(vc_engine* e);
int vc_allgather_counts(vc_engine* e, const int32_t* local, int n, int32_t* out);

/* ---- live counts: the same counts while the stream runs, kept on the device beside the tracker (csrc/live_count.hip) --------------
 * The rule: the counts read at any moment equal vc_counts of a vc_counter that was fed exactly the rows of all batches enqueued so far
 * (per camera, frame = the camera's 1-based frame number) -- utilities/counting/utils.py:276-297 for the video cut at that point, with
 * utilities/counting/utils.py:139-152 (Q11) and utilities/counting/bb_polygon.py:96-114 (Q12) as above, integer for integer.  No row is
 * kept: the state is one 88-byte record per tracker pool slot (vc_engine_config.max_tracks) and one int32 tensor per counter.
 *
 * vc_live_create attaches the counter to n_cam x n_labels trackers of the engine, trackers[cam * n_labels + label] (handles of
 * vc_tracker_create).  polygons: the cameras' zone polygons one after the other, poly_n[cam] points (x, y) each; dir_lines: their
 * direction lines one after the other, n_dir[cam] lines (x0, y0, x1, y1) each.  More than 64 points or 16 directions for a camera is
 * VC_ERR_CAPACITY; a tracker that is attached already (or named twice) VC_ERR_STATE; a bad handle VC_ERR_NOTFOUND.  From then on
 * EVERY tracker launch of the engine that steps one of these trackers -- the stream path, vc_videotracker_run*, vc_deepsort_update,
 * vc_tracker_step -- advances the counter on the tracker stream; rows, vc_stream_collect and every other result are what they are
 * without a counter.  While attached, vc_tracker_reset / vc_tracker_destroy / vc_tracker_restore of such a tracker are VC_ERR_STATE
 * (vc_live_destroy first); vc_stream_reset leaves the counter as the batches that ran left it.
 * Counts are int32 [n_cam][max_dir][n_labels], max_dir = the largest n_dir; rows d >= n_dir[cam] are zero. */
typedef struct vc_live vc_live;
int vc_live_create(vc_engine* e, int n_cam, int n_labels, const int* trackers, const double* polygons, const int* poly_n,
                   const double* dir_lines, const int* n_dir, vc_live** out);
int vc_live_destroy(vc_live* live);
/* waits for the batches enqueued so far; frames_done (optional): per camera, the frames handed to the tracker so far */
int vc_live_counts(vc_live* live, int32_t* out, int64_t* frames_done);
/* the same tensor in device memory, valid until the next tracker launch or vc_live_* call of this engine */
int vc_live_counts_dev(vc_live* live, const int32_t** dev_ptr);
/* open_tracks: slots that hold a track seen in its zone which can still produce rows; retired_tracks: tracks folded into the totals */
int vc_live_stats(vc_live* live, int* open_tracks, int* retired_tracks);
/* ncclAllGather straight from the device tensor on the stream vc_allgather_counts uses (vc_comm_init first): out receives world x
 * n_cam x max_dir x n_labels values, rank-major; every rank's counter must have the same shape. */
int vc_live_allgather(vc_engine* e, vc_live* live, int32_t* out);
/* ---- live checkpoint: device-packed snapshot and resume of a counter and its trackers (csrc/live_ckpt.hip, format csrc/live_ckpt.h) ----
 * One self-contained little-endian blob holds everything the counter and its n_cam x n_labels trackers read from now on: frames_done,
 * zones and base per camera, the retired count, and per tracker its parameters, id counter and every track in list order with Kalman
 * state (fp64, bit for bit), its 88-byte counter record and the valid gallery rows.  No pool slot, handle or engine setting is in it:
 * restored onto another counter -- another engine, process or GPU -- and fed the same frames, the stream continues with identical
 * rows, ids, counts and overlay lists.
 *
 * vc_live_checkpoint_enable allocates, once, a device staging buffer and a pinned host buffer of max_bytes, the offset table, two events
 * and a copy stream (a second call: VC_ERR_STATE; max_bytes below the fixed sections: VC_ERR_CAPACITY).  Without it nothing about a
 * tracker launch changes, and with it nothing does either: only vc_live_checkpoint_begin enqueues work.
 * vc_live_checkpoint_begin enqueues, BEHIND everything enqueued so far on the tracker stream, a plan and a pack kernel that write the
 * blob into the staging buffer, and on the copy stream, behind an event, its copy to pinned memory.  frames_done is taken as of this
 * call.  It makes no synchronising call and does not touch batches in flight: their rows are collected as usual, before or after
 * vc_live_checkpoint_end.  A second begin before end: VC_ERR_STATE.
 * vc_live_checkpoint_end waits for the copy only.  buf == NULL reports *size and leaves the checkpoint ready; cap < *size is
 * VC_ERR_CAPACITY and leaves it ready too.  A state larger than max_bytes is VC_ERR_CAPACITY (the message names the size needed) and
 * drops the checkpoint; the stream itself is unaffected.  Without begin: VC_ERR_STATE.
 * vc_live_checkpoint = begin (unless a size query left a checkpoint ready) + end.
 * Every camera of the counter is in the blob; one camera migrates through cam_map of vc_live_restore.
 *
 * vc_live_restore replaces the state of the counter's cameras cam_map[i] (i = camera of the blob; -1: that camera is not restored;
 * NULL: identity) and of their trackers.  The blob may hold fewer cameras than the counter, or more if cam_map picks some.  The whole blob is validated first; a malformed blob, n_labels other
 * than the counter's, a bad cam_map, or a zone that is not bit-equal to the mapped camera's zone: VC_ERR_ARG; nn_budget above
 * nn_budget_cap, more tracks of a tracker than tracks_per_tracker, too few free pool slots: VC_ERR_CAPACITY.  ANY refusal leaves the
 * counter and its trackers untouched.  Batches that are enqueued but not collected: VC_ERR_STATE (vc_stream_collect them first: their
 * collect would write the track counts of the state they ran on over the restored ones).  A tracker an error had stopped stays stopped.
 * The retired count is kept per counter: it becomes the blob's when the whole blob restores the whole counter, and is left as it is by a
 * partial restore.  vc_live_ckpt_validate_host: the validation alone, pure host code. */
int vc_live_checkpoint_enable(vc_live* live, size_t max_bytes);
int vc_live_checkpoint_begin(vc_live* live);
int vc_live_checkpoint_end(vc_live* live, void* buf, size_t cap, size_t* size);
int vc_live_checkpoint(vc_live* live, void* buf, size_t cap, size_t* size);
int vc_live_restore(vc_live* live, const void* buf, size_t size, const int* cam_map);
int vc_live_ckpt_validate_host(const void* buf, size_t size);
/* One launch of live_count_apply_kernel and one of live_count_read_kernel on host arrays (parity tests): zones as for vc_live_create;
 * tracker_cam[n_trackers] = camera of a tracker, -1 = not attached; slots88 = max_tracks records of 88 bytes {int32 open, cam, label,
 * at_last; int64 last_frame, first[4], last[4]}, base and stats2 = {open, retired} as the previous batch left them (in / out); the batch:
 * rows6 [n_rows][6] as the tracker emits them with the pool slot of each in row_slot, tasks5 [n_tasks][5] = {tracker, index into
 * frame_no, label, first row, rows} with each tracker's tasks contiguous and in frame order, frame_no[n_frames] the camera's 1-based
 * frame numbers, freed[n_freed] the slots the batch freed.  counts (out) = base + the open slots.  Everything written lies between
 * guard blocks: a write outside is VC_ERR_HIP. */
int vc_live_count_host(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir,
                       int n_trackers, const int* tracker_cam, int max_tracks, const int64_t* rows6, const int* row_slot, int n_rows,
                       const int* tasks5, int n_tasks, const int64_t* frame_no, int n_frames, const int* freed, int n_freed,
                       void* slots88, int32_t* base, int32_t* stats2, int32_t* counts);

/* ---- live overlay: the lists vc_overlay paints, built on the device per batch (csrc/live_overlay.hip) --------------------------------
 * The picture of a stream that never ends: no CSV, no second pass.  The definition is overlay.py::LiveVisualizer; per
 * frame, in order: the zone annotation; for every row with a box corner in the zone, in the order vc_stream_collect returns the rows,
 * an arrow from the centre of its track's first in-zone box to its own centre and its box with "id: <id> || cls: <label>"; the count
 * text as it stood BEFORE the batch (none before a camera's first frame); the camera's 1-based frame number.
 *
 * vc_live_overlay_enable: dir_keys = the cameras' direction names as numbers (a zone file's "direction01" -> 1; 0..99, drawn with two
 * digits), n_dir[cam] per camera, concatenated.  max_batch (<= 1024) frames per batch and max_rows_per_frame rows size the arena of
 * each of the `depth` (1..4) list buffers; more than 256 labels is VC_ERR_CAPACITY, a second call VC_ERR_STATE.  Without this call
 * nothing below exists and every tracker launch is what it was: no extra kernel, copy or allocation.  From then on every UNIFORM
 * tracker launch that advances the counter -- the stream path, vc_videotracker_run*, vc_deepsort_update, vc_tracker_step -- also
 * builds its batch's lists into a free list buffer (two launches on the tracker stream behind the counter's); a sized batch
 * (vc_stream_run_async_multi_sized) builds none.  If all `depth` buffers hold lists nobody has consumed, such a call is VC_ERR_STATE
 * before anything of it is enqueued.  A frame that does not fit the arena owns nothing, nor do the frames after it: the call that
 * looks next (vc_live_overlay_lists, or vc_render_collect of that batch) is VC_ERR_CAPACITY.  vc_live_destroy frees the overlay. */
int vc_live_overlay_enable(vc_live* live, const int* dir_keys, int max_batch, int max_rows_per_frame, int depth);
/* Waits for the OLDEST unconsumed batch, copies its lists to the host and consumes the buffer (tests, host consumers).  frame_first
 * has room for cap_frames + 1 entries; *b frames and *n_prims primitives come back.  Nothing unconsumed, or the overlay not enabled:
 * VC_ERR_STATE; too little room: VC_ERR_ARG, nothing consumed. */
int vc_live_overlay_lists(vc_live* live, int32_t* prims12, int cap_prims, int32_t* frame_first, int cap_frames, int* b, int* n_prims);
/* One launch of the two build kernels on host arrays (parity tests), like vc_live_count_host: zones and the batch as there, dir_keys
 * as for vc_live_overlay_enable, slots88 the records AFTER the batch's apply launch, counts_before [n_cam][max_dir][n_labels] or NULL
 * for "no text", cam_of_frame[b] the camera of every frame (-1: none, the frame owns nothing); a frame has one task per camera and
 * label.  prims12 receives the WHOLE arena, cap_prims x 12 (what no frame owns keeps the byte 0xA5), frame_first b + 1 entries.  A
 * frame that does not fit: VC_ERR_CAPACITY, the arrays are still written.  Everything written lies between guard blocks: a write
 * outside is VC_ERR_HIP. */
int vc_live_overlay_host(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir,
                         const int* dir_keys, int n_trackers, const int* tracker_cam, int max_tracks, const void* slots88,
                         const int32_t* counts_before, const int64_t* rows6, const int* row_slot, int n_rows, const int* tasks5, int n_tasks,
                         const int64_t* frame_no, const int* cam_of_frame, int b, int h, int w, int32_t* prims12, int cap_prims,
                         int32_t* frame_first);
/* The same arithmetic (csrc/overlay_build.h) compiled for the host: no HIP call.  prims12 beyond frame_first[b] is not touched. */
int vc_overlay_build_host(int n_cam, int n_labels, const double* polygons, const int* poly_n, const double* dir_lines, const int* n_dir,
                          const int* dir_keys, int n_trackers, const int* tracker_cam, int max_tracks, const void* slots88,
                          const int32_t* counts_before, const int64_t* rows6, const int* row_slot, int n_rows, const int* tasks5, int n_tasks,
                          const int64_t* frame_no, const int* cam_of_frame, int b, int h, int w, int32_t* prims12, int cap_prims,
                          int32_t* frame_first);
/* the 35-bit bitmap the builders draw character ch with (bit 5 * row + column; lower case as capitals, unknown as '?') */
int vc_glyph_bits_host(int ch, uint64_t* bits);

/* ---- visualisation egress (off the hot path) --------------------------------------------------------- */
/* utilities/counting/utils.py:299-331 visualize_merged: draws the annotation overlay into b BGR u8 frames (h x w x 3) in device
 * memory.  prims12: n x 12 int32 [type, x0, y0, x1, y1, t, colour (B | G << 8 | R << 16), glyph bits lo, glyph bits hi, 0, 0, 0] with
 * type 0 line (thickness t), 1 disc (radius t), 2 rectangle outline (thickness t), 3 filled box, 4 glyph (5 x 7 bitmap, scale t);
 * frame f owns prims [frame_first[f], frame_first[f + 1]) and paints them in order.  The host side (overlay.py) builds the lists
 * the way the reference's draw_* helpers are called.  Pixel parity with OpenCV's rasteriser / fonts is not claimed. */
int vc_overlay(vc_engine* e, void* frames_dev, int b, int h, int w, const int32_t* prims12, const int32_t* frame_first);

/* ---- annotated video out: BGR -> 4:2:0 YUV egress and the asynchronous render path ----------------------------------------------
 * The reference's second artefact (VideoWriter.write_full_to_video -> visualize_merged, modules/datasets.py:132-145) leaves through
 * an encoder, and an encoder takes 4:2:0 YUV.  bgr_to_yuv_kernel is the inverse of the ingest conversion, laid out by the same
 * vc_yuv_desc under the same rules (bad geometry is VC_ERR_ARG before any HIP call).  Arithmetic (integer, 32-bit signed):
 *   Y = clamp((KYR*R + KYG*G + KYB*B + (1 << 19) + (YOFF << 20)) >> 20)  per pixel, YOFF = 16 (limited) or 0 (full range);
 *   U = clamp((KUR*Rm + KUG*Gm + KUB*Bm + (1 << 19) + (128 << 20)) >> 20), V alike with KV*, per 2 x 2 block, where
 *   Rm, Gm, Bm = (sum over the block + 2) >> 2; constants int(round(literal * 2^20)).
 * Bytes of the destination that belong to no plane (pitch padding, gaps between planes and frames) are NOT written.
 * vc_bgr_to_yuv_dev runs on the caller's device buffers (bgr_dev: b x h x w x 3 bytes), enqueued on the NULL stream, and returns
 * without waiting for it. */
int vc_bgr_to_yuv_dev(const vc_yuv_desc* d, const void* bgr_dev, int b, int h, int w, void* yuv_dev);

/* Render context: per batch  source -> BGR work buffer -> overlay (the vc_overlay lists) -> bgr_to_yuv -> the caller's surface, all
 * enqueued, nothing waited for.  It belongs to an engine (device; vc_engine_destroy destroys the contexts that are left) but is
 * independent of the detector -- an engine with with_detector = 0, with_reid = 0 serves -- and of the stream path: it uses neither
 * the four ingest slots nor the pending submissions.  It owns two streams (in, out) and, per batch in flight (`depth`, 1..4), a
 * raw-input buffer, a BGR work buffer and a YUV output buffer, each allocated on its first use. */
typedef struct vc_render vc_render;
#define VC_SRC_BGR_HOST 0  /* b x h x w x 3 BGR in (pinned) host memory */
#define VC_SRC_BGR_DEV 1   /* the same in device memory: copied into the work buffer, the caller's frames are never painted */
#define VC_SRC_YUV_HOST 2  /* YUV frames laid out as `desc` (any VC_PIX_* format) in (pinned) host memory: 1.5 B per pixel over PCIe for 8-bit
                              4:2:0, 2 for I422, 3 for P016 / I010 / I444; converted on the device */
#define VC_SRC_YUV_DEV 3   /* decoder surfaces in device memory */
typedef struct vc_render_src {
    int kind;              /* VC_SRC_* */
    const void* data;
    vc_yuv_desc desc;      /* VC_SRC_YUV_* only */
} vc_render_src;
int vc_render_create(vc_engine* e, int max_batch, int max_h, int max_w, int depth, vc_render** out);
int vc_render_destroy(vc_render* r);
/* Enqueues one batch and returns at once.  prims12 / frame_first: the lists of vc_overlay, both NULL = no overlay; they are COPIED
 * by this call and may be reused when it returns.  out: a device surface (out_is_dev = 1) or (pinned) host memory that receives the
 * plane bytes only, laid out as out_desc.  The source frames and `out` must stay valid until the batch has been collected.
 * Refusals, all before anything is enqueued: bad geometry of either descriptor or bad lists VC_ERR_ARG; a batch or frame larger
 * than the context VC_ERR_CAPACITY; `depth` batches already outstanding VC_ERR_STATE. */
int vc_render_submit(vc_render* r, const vc_render_src* src, int b, int h, int w, const int32_t* prims12, const int32_t* frame_first,
                     const vc_yuv_desc* out_desc, void* out, int out_is_dev);
/* Blocks until the OLDEST outstanding batch is complete in its `out`; VC_ERR_STATE with nothing outstanding. */
int vc_render_collect(vc_render* r);
/* vc_render_submit with the lists taken IN DEVICE MEMORY from the counter's oldest unconsumed list buffer (vc_live_overlay_enable): the
 * context's in-stream waits on the event recorded behind the build launches on the tracker stream -- no host wait, no list copy.  The
 * counter and the context belong to one engine.  b, h, w must be that batch's own, else VC_ERR_ARG; nothing unconsumed (or, after a
 * sized batch, no list of that batch) is VC_ERR_STATE; the other refusals are vc_render_submit's, and all leave the lists unconsumed.
 * The list buffer counts as consumed when vc_render_collect has returned for this batch.  The source is any VC_SRC_* kind -- typically
 * the decoder surfaces the batch came from, or the BGR slot vc_stream_stage_* returned for it: such a slot must not be restaged
 * before the collect. */
int vc_render_submit_live(vc_render* r, vc_live* live, const vc_render_src* src, int b, int h, int w, const vc_yuv_desc* out_desc, void* out,
                          int out_is_dev);

/* ---- multi-camera ingest: one batch from per-frame sources of mixed formats ------------------------------------------------------
 * A batch that interleaves S cameras has S decoders behind it: every frame has its own address and possibly its own pitch, format,
 * colour matrix and memory space.  The per-frame source is the render path's struct (kind VC_SRC_*, data, desc for the YUV kinds);
 * all frames of a batch share h x w (vc_stream_stage_frames_sized below lifts that), BGR frames are tight h * w * 3 bytes, a YUV frame is ONE frame laid out as its desc
 * (frame_stride is not used).  Per frame the arithmetic is that of yuv_to_bgr_kernel (above); a BGR frame is a byte copy. */
typedef vc_render_src vc_frame_src;
/* Fills one of the four ingest slots of vc_stream_stage_host with the b frames as packed BGR (same slot rules, same VC_ERR_STATE /
 * VC_ERR_CAPACITY refusals; may be mixed freely with the other staging calls): *frames_dev_out goes to vc_stream_submit, which waits
 * for the slot's event, and then to vc_stream_run*.  Enqueued on the engine's copy stream: one copy per host frame (BGR straight
 * into its place in the slot, YUV into the slot's raw buffer at its vc_frames_layout_host offset; pinned memory for the copies to
 * overlap), one copy of the frame table, at most ONE frames_to_bgr_kernel launch whatever b and whatever the mix (none when every
 * frame is VC_SRC_BGR_HOST), the slot's event.  Device sources must stay valid until the vc_stream_run* call of the batch has
 * returned, host sources until its rows are collected.  Every refusal comes before a slot is taken or anything is enqueued: b < 1,
 * a null data, an unknown kind, bad geometry in any frame, an h or w that a YUV frame's format refuses (the table above vc_yuv_desc:
 * odd sizes for NV12 / I420 / P016 / I010, an odd w for I422, none for I444) are VC_ERR_ARG, and the message
 * names the frame ("frame 3: pitch_y ..."). */
int vc_stream_stage_frames(vc_engine* e, const vc_frame_src* frames /* b */, int b, int h, int w, void** frames_dev_out);
/* The validation of vc_stream_stage_frames and the packing of its raw buffer.  Pure host function (no GPU), like vc_gather_offsets:
 * the CPU tests drive it directly.  raw_off[f]: for a VC_SRC_YUV_HOST frame the byte offset of its copy in the raw buffer -- a
 * multiple of 16, ascending with f, the ranges [raw_off[f], raw_off[f] + bytes of that one frame) disjoint -- and -1 for every other
 * kind; *raw_bytes: the end of the last range, 0 when there is none. */
int vc_frames_layout_host(const vc_frame_src* frames, int b, int h, int w, int64_t* raw_off /* b */, size_t* raw_bytes);
/* The same kernel outside the stream path, on the caller's own device buffers (measurement; the counterpart of vc_yuv_to_bgr_dev):
 * frames of the DEVICE kinds only, bgr_dev: b x h x w x 3 bytes, table_dev: b * VC_FRAME_ENTRY_BYTES bytes of device memory for the
 * frame table.  With `frames` the table is built and copied there (a blocking copy) before the launch; with frames == NULL the
 * table is launched as the last such call left it -- repeated launches of one batch cost the kernel alone.  Enqueued on the NULL
 * stream, returns without waiting for it. */
#define VC_FRAME_ENTRY_BYTES 64
int vc_frames_to_bgr_dev(const vc_frame_src* frames /* device kinds only, or NULL */, int b, int h, int w, void* bgr_dev, void* table_dev);

/* ---- sized batches: cameras of different frame sizes in one detector batch ----------------------------------------------------------
 * Under AutoShape a frame's network tensor depends only on its aspect ratio after the stride-32 rounding (Q8): at size 640, 1920x1080,
 * 1280x720, 640x360, 320x180 and 640x362 all run at 384x640.  A SIZED batch is b frames with their own (h, w) whose own network shapes
 * -- vc_autoshape_net_size of each frame alone, what the reference gives that camera at batch size 1 -- are all equal: one ingest slot,
 * one detector pass, one ReID pass, one tracker launch, and every frame gets exactly the result of a batch of its own size.  Frames are
 * never letterboxed to a batch-wide maximum (AutoShape's rule for a mixed list would change each camera's result).
 * Layout in device memory: b CELLS of `cell` bytes, cell = the largest h * w * 3 of the batch rounded up to 16; frame f is tight BGR
 * (row pitch w_f * 3) at f * cell; the rest of a cell is never read and never written.
 * Refusals, all pure host logic before any HIP call: frames whose network shapes differ are VC_ERR_ARG, the message names the first
 * frame that differs and both shapes ("frame 3: 480x640 runs at 480x640, frame 0 at 384x640"); a YUV frame needs the even h and / or w its format asks for (BGR
 * and I444 frames may be odd, I422 frames in h); h_f > max_frame_h, w_f > max_frame_w, b > max_batch or b * cell beyond an ingest slot are VC_ERR_CAPACITY (a slot
 * holds max_batch frames of the configured maximum in cells).  Opt-in: every other entry point runs a uniform batch as before. */
typedef struct vc_frame_dims { int h, w; } vc_frame_dims;
/* The network shape AutoShape gives ONE h x w image at `img_size` (models/common.py v6.0).  Pure host function. */
int vc_autoshape_net_size(int h, int w, int img_size, int* net_h, int* net_w);
/* Counterpart of vc_frames_layout_host for a sized batch: all of its validation with every frame's own size, the packing of the
 * VC_SRC_YUV_HOST frames into the raw buffer (raw_off, raw_bytes as there), the cell size and the shared network shape.  Pure host. */
int vc_frames_layout_sized_host(const vc_frame_src* frames, const vc_frame_dims* dims, int b, int img_size,
                                int64_t* raw_off /* b */, size_t* raw_bytes, size_t* cell, int* net_h, int* net_w);
/* vc_stream_stage_frames for a sized batch: every slot rule and refusal of that call (no slot is taken on a refusal; mixes freely with
 * the other staging calls); one copy per host frame, one table copy, at most ONE kernel launch, the slot's event.  *frames_dev_out
 * addresses the cells. */
int vc_stream_stage_frames_sized(vc_engine* e, const vc_frame_src* frames, const vc_frame_dims* dims, int b, void** frames_dev_out);
/* vc_stream_submit / vc_stream_run_async_multi for a sized batch (a staged one, or the caller's own device buffer laid out in cells).
 * The dims handed to submit and to run must equal those of the staged / submitted batch (VC_ERR_ARG otherwise).  All frames of one
 * camera within a batch have one size (VC_ERR_ARG otherwise): it is the size that camera's track boxes are clamped to.  The detector
 * runs the unfused stem behind ONE letterbox launch for the batch.  Rows are picked up with vc_stream_collect. */
int vc_stream_submit_sized(vc_engine* e, const void* frames_dev, const vc_frame_dims* dims, int b);
int vc_stream_run_async_multi_sized(vc_engine* e, const int* trackers /* n_cam x num_classes */, int n_cam, int num_classes, const int* cam_of_frame /* b */,
                                    const void* frames_dev, const vc_frame_dims* dims, int b, int cap_rows_per_frame);

/* Host half of vc_allgather_rows: RCCL gathers equal-sized blocks, so every rank contributes `max_rows` rows (its own counts[r] rows
 * followed by padding) and the receive buffer is rank-major [world][max_rows][row_bytes].  This compacts such a padded buffer into
 * the first sum(counts) rows of `out` in rank-major order -- for frame chunks dealt round-robin to the ranks that is frame order
 * (the ordering contract of /root/reference/modules/__init__.py:54-84).  Pure host function (no GPU): it is the logic a world of
 * 2 / 3 / 8 ranks exercises and a single-GPU box cannot, so the CPU tests drive it directly.  vc_allgather_rows calls it for the rows
 * and uses vc_gather_offsets for the device-side copies of the embeddings.  Returns the row count through *out_total. */
int vc_gather_compact_host(const void* padded, int world, int max_rows, size_t row_bytes, const int* counts, void* out, size_t out_cap_rows,
                           int64_t* out_total);
/* src_off[r] / dst_off[r]: first row of rank r's block in the padded buffer / in the compacted output (rows, not bytes). */
int vc_gather_offsets(int world, int max_rows, const int* counts, int64_t* src_off, int64_t* dst_off, int64_t* out_total);

/* Conv autotune choices of this engine as text ("<shape key> <tile config>\n" per line, the VC_TUNE_CACHE file format), and their
 * import into another engine (keys already present are overwritten; call before the first launch of those shapes).  Multi-GPU
 * launches tune on rank 0 and broadcast the text (parallel.share_tune_cache): N ranks then neither time the candidates N times nor
 * disagree on the member of a near-tie (bf16 results are identical across tile configurations of one kernel family only). */
int vc_tune_export(vc_engine* e, char* buf, size_t cap, size_t* size);   /* buf may be NULL: *size receives the bytes needed (incl. NUL) */
int vc_tune_import(vc_engine* e, const char* text);

/* ---- measurement ---------------------------------------------------------------------------------- */
#define VC_PROF_CONV 0       /* all implicit-GEMM conv launches */
#define VC_PROF_DETECT_AUX 1 /* letterbox, pools, upsample, decode, NMS */
#define VC_PROF_REID_AUX 2   /* crop/resize, pools, L2 norm */
#define VC_PROF_TRACK 3      /* Kalman, cost matrices */
#define VC_PROF_NCAT 4
int vc_profile_enable(vc_engine* e, int on);   /* 0 off; 1 blocking events around every launch (serialises the streams);
                                                  2 in-flight event pairs around conv launches only, resolved by vc_profile_read */   /* brackets every launch with hipEvents on its own stream; disables graphs */
int vc_profile_read(vc_engine* e, int category, double* total_ms, int64_t* launches, double* flops, double* bytes);
/* After vc_profile_read(VC_PROF_CONV) resolved an in-flight (mode 2) region: milliseconds during which at least one conv kernel was
 * running, and the window from the first conv start to the last conv stop. */
int vc_profile_conv_busy(vc_engine* e, double* union_ms, double* span_ms);
/* vc_profile_read reports the work the launches EXECUTE (the sparse Detect head: the gathered rows only).  This returns the same
 * category with the sparse head credited as the dense Detect.m[i] it replaces -- the reference's algorithmic work -- as a separate
 * figure (bench.py: roofline.algorithmic_dense_*).  Call vc_profile_read first. */
int vc_profile_read_dense(vc_engine* e, int category, double* flops_dense, double* bytes_dense);
int vc_profile_reset(vc_engine* e);
int vc_profile_ops(vc_engine* e, char* buf, size_t cap);   /* per-conv-launch lines "conv M= N= K= ... ms= tflops=" recorded while profiling */
int vc_engine_sync(vc_engine* e);

/* ---- single-function entry points (parity tests; each runs the device kernel on host arrays) ------- */
typedef struct vc_conv_desc {
    int b, h, w, cin, cout, kh, kw, stride, pad;
    int act;         /* 0 none, 1 SiLU, 2 ReLU */
    int res_mode;    /* 0 none, 1 add after act, 2 add before act */
    int precision;   /* VC_PREC_* */
} vc_conv_desc;
/* x NHWC f32, w OIHW f32, bias f32[cout], res NHWC f32 or NULL, y NHWC f32 (bf16 mode rounds x, w, res, y). */
int vc_conv2d_host(const vc_conv_desc* d, const float* x, const float* w, const float* bias, const float* res, float* y);
/* The launch views of a convolution (what the engine's ConvP carries besides the plain problem), on whole host buffers at full channel
 * stride.  Element type E = d->precision; a channel slice is (cs, co) as below. */
typedef struct vc_conv_view {
    int in_cs, in_co;                /* input channels [in_co, in_co + cin) of x */
    int out_cs, out_co;              /* the concat-slice store into y */
    int res_cs, res_co;              /* the residual as a slice of res (res != NULL) */
    int split, out2_cs, out2_co;     /* split > 0: output channels >= split go to y2 at out2_co + (channel - split) */
    int out_f32;                     /* bf16 arithmetic, f32 store */
    int out_bf16;                    /* fp8 arithmetic, bf16 store */
    int m_valid;                     /* -1: none; otherwise the number of valid output pixels, put in device memory (ConvP::m_dev) */
    int up_c, up_cs, up_co;          /* up_c > 0: input channels [0, up_c) are the 2 x nearest upsampling of channels [up_co, up_co + up_c) of x_up */
} vc_conv_view;
/* vc_conv2d_host's launch with these views: the same launch_conv call, the same environment (VC_CONV_CFG, VC_CONV_SLOTS, VC_CONV_STRICT).
 * x [b][h][w][in_cs], x_up [b][h/2][w/2][up_cs] (up_c > 0), res [b][ho][wo][res_cs] (or NULL): converted element by element to E, NaN
 * stays NaN.  y [b][ho][wo][out_cs] and y2 [b][ho][wo][out2_cs] (split > 0) are in AND out: uploaded as the store type (f32 / bf16 / e4m3),
 * launched into between guard blocks and read back whole, so elements no launch may touch can be compared by value.  d->cin must be a
 * multiple of the chunk (8 bf16, 4 f32, 16 fp8).  A refused launch is VC_ERR_ARG and leaves y / y2 as they were. */
int vc_conv2d_view_host(const vc_conv_desc* d, const vc_conv_view* v, const float* x, const float* x_up, const float* w, const float* bias,
                        const float* res, float* y, float* y2);
/* launch_s2halo_pw on host arrays (bf16): the 3x3 / s2 / p1 convolution d (SiLU, cout 128, weights w, bias) over channels [in_co, in_co + cin)
 * of x [b][h][w][in_cs], and on the tile the pointwise 128 -> 128 conv (SiLU, w_pw, bias_pw) that alone reads it, stored through v's
 * out_cs / out_co / split / out2_*: y, y2 as above.  The 3x3's own output is never written and not returned. */
int vc_conv_s2_pw_host(const vc_conv_desc* d, const vc_conv_view* v, const float* x, const float* w, const float* bias, const float* w_pw,
                       const float* bias_pw, float* y, float* y2);
/* The fused block kernels (c3_fused_kernel, bneck_fused_kernel<false / true>, reid_block_fused_kernel; bf16) as ONE launch on host arrays,
 * without an engine.  Each entry point builds the ConvP chain the engine's plan builds for the block and calls the block's launcher, so
 * the launcher's own applicability function decides; its quiet refusal comes back as VC_ERR_ARG with an empty message and leaves every
 * array as passed.  A channel slice is (cs, co) as above; arrays are whole buffers at full channel stride, converted element by element
 * to bf16 (NaN stays NaN), in AND out: x too is launched on between guard blocks and read back, so that elements no launch may touch
 * can be compared by value.  Tensors the fused kernel keeps on chip (C3: y1, b1, [m | y2]; Bottleneck: b1, and m under cv3; ReID: t)
 * live in buffers of the entry point's own; a fused launch that writes one of them, or a guard block, is VC_ERR_HIP. */
typedef struct vc_fused_view {
    int in_cs, in_co;                /* the block's input: channels [in_co, in_co + 64) of x */
    int out_cs, out_co;              /* C3: out; ReID: y; Bottleneck: m -- under cv3 y is the concat buffer [m | y2]: m is NOT written
                                        and channels [out_co + 64, out_co + 128) hold y2 */
    int z_cs, z_co;                  /* Bottleneck under cv3: cv3's output, channels [z_co, z_co + 128) of z */
    int out_buf;                     /* 0: y is a buffer of its own; 1: the (out_cs = in_cs, out_co) slice lies in x's buffer, y is not used */
    int z_buf;                       /* 0: z is a buffer of its own; 1: cv3 stores into x's buffer, 2: into y's (z_cs = that buffer's stride) */
    int res;                         /* Bottleneck: with the shortcut */
    int cv3;                         /* Bottleneck: the CV3 instance (w3 [128][128], b3, z) */
    int split;                       /* C3: the channel split of the cv1 | cv2 launch; 0 = 32, what the block has (anything else breaks the chain) */
    int unfused;                     /* 1: the SAME chain through launch_conv, one launch per convolution (VC_CONV_CFG, VC_CONV_STRICT as for
                                        vc_conv2d_host); the intermediates are then written, m under cv3 included */
    int grid;                        /* > 0: at most this many workgroups, which then walk all tiles or crops; 0 = the product's grid */
} vc_fused_view;
/* C3(64 -> 64, n = 1, shortcut): x [b][h][w][in_cs], w12 [64][64] = cv1 over cv2, wm1 [32][32], wm2 [32][32][3][3], w3 [64][64], y [b][h][w][out_cs] */
int vc_c3_fused_host(int b, int h, int w, const vc_fused_view* v, float* x, const float* w12, const float* b12, const float* wm1, const float* bm1,
                     const float* wm2, const float* bm2, const float* w3, const float* b3, float* y);
/* Bottleneck(64 -> 64, e = 1): w1 [64][64], w2 [64][64][3][3]; w3 / b3 / z may be NULL without cv3 */
int vc_bneck_fused_host(int b, int h, int w, const vc_fused_view* v, float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, float* y, float* z);
/* ReID BasicBlock(64 -> 64) on k maps of h x w (the kernel takes 25 x 25): w1, w2 [64][64][3][3] */
int vc_reid_block_fused_host(int k, int h, int w, const vc_fused_view* v, float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y);
/* The kernels that open a detector pass (bf16) as ONE launch on host arrays, without an engine: the direct stem (stem_direct_kernel<CT>,
 * stem_direct_wide_kernel<5>; 6x6 / s2 / p2 + SiLU, cout = 16 CT) and layers 0 + 1 in one kernel (front_fused_kernel; stem to 32 channels, then
 * 3x3 / s2 / p1 + SiLU to 64).  The network input is EITHER x, the letterboxed tensor [b][net_h][net_w][3] as floats (rounded to bf16 into
 * the 4-channel pair view the plan builds; frames NULL), OR frames, b packed u8 frames [h][w][3] whose letterbox into net_h x net_w (the
 * engine's own geometry) the kernel folds in (x NULL).  net_w is even.  The ConvPs are filled as the plan fills them; inputs and outputs lie
 * between guard blocks, the frames' base is 4-byte aligned; a launch that writes an input, a guard block or -- direct launches -- the
 * letterboxed tensor or layer 0 is VC_ERR_HIP.  A launcher's own refusal is VC_ERR_ARG and leaves every array as passed. */
typedef struct vc_front_view {
    int out_cs, out_co;              /* the output: channels [out_co, out_co + cout) of y */
    int q_cs, q_co;                  /* stem, q8 != NULL: the e4m3 copy of the output the fp8 engine's stem writes, bytes [q_co, q_co + cout) of q8 */
    float inv_scale;                 /* ... of value x inv_scale */
    int swap_rb;                     /* frames: channels 0 and 2 exchanged inside the image */
    int mode;                        /* 1: the direct launcher (launch_stem_direct / launch_stem_direct_u8 / launch_front_fused; the tensor input
                                        gives front_fused_kernel<false>); 0: the same ConvPs through launch_conv (VC_CONV_CFG, VC_CONV_STRICT as for
                                        vc_conv2d_host), behind launch_letterbox for frames, followed by the bf16 -> fp8 launch under q8 */
    int grid_cap;                    /* mode 1, > 0: at most this many workgroups, which then walk all tiles; 0 = the product's grid */
} vc_front_view;
/* w0 [cout][3][6][6], b0 [cout]; y [b][net_h / 2][net_w / 2][out_cs] and q8 [b][net_h / 2][net_w / 2][q_cs] (nullable) are in AND out */
int vc_stem_host(int b, int net_h, int net_w, int cout, const vc_front_view* v, const float* x, const uint8_t* frames, int h, int w, const float* w0,
                 const float* b0, float* y, uint8_t* q8);
/* w0 [32][3][6][6], w1 [cout1][32][3][3] (the kernel takes cout1 = 64); y [b][h1][w1][out_cs], h1 = (net_h / 2 - 1) / 2 + 1, in AND out */
int vc_front_fused_host(int b, int net_h, int net_w, int cout1, const vc_front_view* v, const float* x, const uint8_t* frames, int h, int w, const float* w0,
                        const float* b0, const float* w1, const float* b1, float* y);
int vc_kalman_initiate_host(const double* xyah, int n, double* mean8, double* cov64);
int vc_kalman_predict_host(double* mean8, double* cov64, int n);
int vc_kalman_update_host(double* mean8, double* cov64, const double* z4, int n);
int vc_kalman_gating_host(const double* mean8, const double* cov64, const double* z4, int n_meas, double* out);
int vc_iou_cost_host(const double* track_tlwh, int t, const double* det_tlwh, int d, double* out_iou);
int vc_cosine_cost_host(const float* gallery, const int* gal_count, int t, int s_cap, const float* feat, int d, double* out);
int vc_dsort_nms_host(const double* tlwh, const double* scores, int n, double max_overlap, int* keep, int* n_keep);
int vc_lap_host(const double* cost, int nr, int nc, int* row4col_rows, int* cols, int* n_assigned);
int vc_letterbox_host(const uint8_t* rgb, int h, int w, int net_h, int net_w, int precision, float* out_nhwc3);
/* yuv_to_bgr_kernel (the stream path's ingest conversion) on host arrays: b frames laid out as `d` says -> packed BGR b x h x w x 3 */
int vc_yuv_to_bgr_host(const vc_yuv_desc* d, const uint8_t* yuv, int b, int h, int w, uint8_t* bgr_out);
/* frames_to_bgr_kernel (vc_stream_stage_frames) on host arrays: b frames of the HOST kinds, each at its own address -> packed BGR
 * b x h x w x 3.  Each frame is uploaded to a device address congruent to its host pointer mod 16, so where the caller puts a frame
 * decides whether it takes the kernel's 16-byte path or the generic one.  Validation first: bad input is VC_ERR_ARG without a GPU too. */
int vc_frames_to_bgr_host(const vc_frame_src* frames /* host kinds only */, int b, int h, int w, uint8_t* bgr_out);
/* The three per-frame-size kernels of a sized batch on host arrays.
 * vc_frames_to_bgr_sized_host: the sized ingest kernel; frames as for vc_frames_to_bgr_host, `cells` holds b cells (cell size as
 * vc_frames_layout_sized_host reports it), is uploaded, converted into and read back: bytes of a cell beyond its frame keep the caller's values.
 * vc_letterbox_frames_host: letterbox_frames_kernel, ONE launch for b frames of their own sizes (frames[f]: h_f x w_f x 3 u8) into
 * b x net_h x net_w x 3 floats; swap_rb exchanges channels 0 and 2 inside the image.
 * vc_crop_resize_frames_host: the ReID crop kernel (fp32 instance) with the per-frame table: box i is cut from frame frame_of_box[i]
 * and clamped to that frame's own size (deep_sort.py:89-95); out k x 50 x 50 x 3, the network input vc_embed_debug_input shows. */
int vc_frames_to_bgr_sized_host(const vc_frame_src* frames /* host kinds only */, const vc_frame_dims* dims, int b, uint8_t* cells /* b * cell */);
int vc_letterbox_frames_host(const uint8_t* const* frames, const vc_frame_dims* dims, int b, int net_h, int net_w, int swap_rb, int precision,
                             float* out_nhwc3);
int vc_crop_resize_frames_host(const uint8_t* const* bgr, const vc_frame_dims* dims, int b, const int* frame_of_box, const double* boxes_cxcywh, int k,
                               float* out_nhwc);
/* The letterbox kernels on the caller's own device buffers (measurement, like vc_frames_to_bgr_dev): frames_dev = b packed h x w x 3 frames,
 * out_dev = b x net_h x net_w x 4 elements of `precision`.  mode 0: the kernels a uniform batch runs; mode 1: builds the per-frame table of
 * these uniform frames in table_dev (b * 64 bytes of device memory, a blocking copy) and runs letterbox_frames_kernel; mode 2: that kernel
 * with the table as the last mode-1 call left it.  Enqueued on the NULL stream, returns without waiting for it. */
int vc_letterbox_dev(const void* frames_dev, int b, int h, int w, int net_h, int net_w, int swap_rb, int precision, void* out_dev, void* table_dev, int mode);
/* bgr_to_yuv_kernel (the render path's egress conversion) on host arrays: packed BGR b x h x w x 3 -> b frames laid out as `d` says.
 * Only plane bytes of yuv_out change. */
int vc_bgr_to_yuv_host(const vc_yuv_desc* d, const uint8_t* bgr, int b, int h, int w, uint8_t* yuv_out);
/* VideoCounting.run zone filter (modules/track.py:102-104): inside[i] = any corner of boxes[i] in the polygon. Host only. */
int vc_zone_filter_host(const double* polygon_xy, int n_points, const int64_t* boxes_xyxy, int n, uint8_t* inside);
/* candidates (already conf-filtered, in the reference's candidate order): boxes xyxy, conf, class -> kept rows */
int vc_nms_host(const float* boxes4, const float* conf, const int* cls, int n, float iou, int max_det, int max_cand,
                float* out6, int* out_n);
/* The same three kernels on a batch: frame f has counts[f] <= max_cand candidates at boxes4 / conf / cls + f * max_cand (candidate
 * order = position, as above) and its own scale_coords geometry geom4[f] = {net_h, net_w, src_h, src_w} (the engine's scale_geom_host;
 * geom4 == NULL or net_h <= 0: network pixels, no rescale and no clamp, like vc_nms_host).  out6: [b][max_det][6], out_n: [b]. */
int vc_nms_batch_host(const float* boxes4, const float* conf, const int* cls, const int* counts, int b, float iou, int max_det, int max_cand,
                      const int* geom4, float* out6, int* out_n);
/* vc_nms_batch_host with the class filter in front and the relabel behind, the order of non_max_suppression(classes=...) under
 * networks/yolo.py:64 and of modules/detect.py:41-46 (vc_engine_set_class_map: cand_class_filter_kernel, the three
 * NMS kernels on the ORIGINAL classes, det_relabel_kernel), on the same device buffers; validated before any device call.  The class column
 * of out6 holds labels.  kept_count[f] = candidates of frame f the filter kept, kept_idx + f * max_cand (nullable) their positions in
 * ascending order (the filter is stable).  Rows and positions lie between guard blocks: a write outside them is VC_ERR_HIP. */
int vc_class_filter_nms_host(const float* boxes4, const float* conf, const int* cls, const int* counts, int b, const int* label_of_class,
                             int n_classes, float iou, int max_det, int max_cand, const int* geom4, float* out6, int* out_n, int* kept_count,
                             int* kept_idx /* b * max_cand, nullable */);
/* The detector's tail on explicit logits, without an engine or a network: decode_kernel<f32 | bf16>, or head_compact_kernel +
 * decode_sparse_kernel wired as the bf16 engine wires them (objectness plane = channels a * (nc + 5) + 4 of the logits, the head conv's
 * input rows = the dense logits themselves, cap = every pixel of the batch).  The bf16 and the sparse mode round the logits to bf16. */
typedef struct vc_decode_desc {
    int b, nc;
    int mode;            /* 0 dense f32, 1 dense bf16, 2 sparse (bf16) */
    int ny[3], nx[3];
    float stride[3];
    float anchors[18];   /* [level][anchor][w, h] in pixels */
    float conf;
    int max_cand;
} vc_decode_desc;
/* logits[i]: float32 [b][ny[i]][nx[i]][round_up(3 * (nc + 5), 8)].  Candidates of frame f (slot order is arbitrary; idx = position in
 * the reference's flattened prediction) at cand_* + f * max_cand, min(cand_count[f], max_cand) of them; overflow[f] = 1 when more than
 * max_cand passed.  Sparse mode, when hc_count is given: hc_count[i] pixels of level i gathered, their indices (frame-major) in hc_list[i]
 * (room for b * ny[i] * nx[i] each).  out6 != NULL chains the NMS over the SAME device buffers (iou, max_det, geom4 as in
 * vc_nms_batch_host): out_n[f] = -1 for a frame whose overflow flag is set. */
int vc_decode_host(const vc_decode_desc* d, const float* const* logits, int* cand_count, int* overflow, float* cand_box, float* cand_conf,
                   int* cand_cls, int* cand_idx, int* hc_count, int* const* hc_list, float iou, int max_det, const int* geom4, float* out6,
                   int* out_n);
/* The pool, resample, layout and cast kernels between the convolutions, each through the launch function the engine calls, on host
 * float arrays.  Values are converted to `precision` on the way in and back to float on the way out; a caller that passes values the
 * element type represents gets the kernel's own bits.  A channel slice is (cs, co): channel c of a pixel at cs * pixel + co + c.
 * Everything a kernel writes lies between guard blocks: a write outside the buffer is VC_ERR_HIP, not a plausible result. */
#define VC_SPPF_RAN_SEP 1    /* sppf_pool_sep_kernel: the register form */
#define VC_SPPF_RAN_WIDE 2   /* sppf_pool_wide_kernel: the plane in LDS */
#define VC_SPPF_RAN_PLAIN 3  /* sppf_pool_kernel: every output reads its 13 x 13 window (f32 / bf16) */
#define VC_SPPF_RAN_FP8 4    /* sppf_pool_fp8_kernel: the same for e4m3 planes */
/* buf [b][h][w][cs], in and out: SPPF of channels [co, co + c) into [co + c, co + 4c); form as the engine's sppf_sep option.
 * ran_kernel / ran_ws (nullable): the kernel that ran (VC_SPPF_RAN_*) and its slice width in 32-bit words. */
int vc_sppf_pool_host(float* buf, int b, int h, int w, int cs, int co, int c, int precision, int form, int* ran_kernel, int* ran_ws);
/* src [b][h][w][c] -> channels [co, co + c) of dst [b][2h][2w][cs] (in and out); f32, bf16, fp8 */
int vc_upsample2x_host(const float* src, int b, int h, int w, int c, float* dst, int cs, int co, int precision);
/* MaxPool2d(3, 2, 1): src [b][h][w][c] -> channels [co, co + c) of dst [b][(h - 1) / 2 + 1][(w - 1) / 2 + 1][cs] (in and out); f32, bf16 */
int vc_maxpool3s2_host(const float* src, int b, int h, int w, int c, float* dst, int cs, int co, int precision);
/* AvgPool over the whole h x w map + L2 normalisation: x [k][h][w][512] -> out [k][512] (always f32); f32, bf16 */
int vc_avgpool_l2norm_host(const float* x, int k, int h, int w, int precision, float* out);
/* x [k][c][h][w] -> out [k][h][w][cpad], channels >= c zero; cpad must be the ReID input buffer's (4 in f32, 8 in bf16) */
int vc_nchw_to_nhwc_pad_host(const float* x, int k, int c, int h, int w, int cpad, int precision, float* out);
/* bf16 -> e4m3fn of value x inv_scale: channels [src_co, src_co + c) of src [npix][src_cs] (floats, rounded to bf16) into bytes
 * [dst_co, dst_co + c) of dst [npix][dst_cs] (in and out) */
int vc_bf16_to_fp8_host(const float* src, int npix, int c, int src_cs, int src_co, float inv_scale, uint8_t* dst, int dst_cs, int dst_co);
/* The ReID stem in one kernel (bf16): conv3x3(3 -> 64) + bias + ReLU + MaxPool2d(3, 2, 1).  crops [k][50][50][3], w [64][3][3][3],
 * bias [64] -> out [k][25][25][64] */
int vc_reid_stem_pool_host(const float* crops, int k, const float* w, const float* bias, float* out);

#ifdef __cplusplus
}
#endif
#endif /* VCOUNT_HIP_H */
