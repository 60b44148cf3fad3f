"""Engine: owns one `vc_engine` (one GPU) and exposes its entry points with numpy in / numpy out."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .weights import fold_reid

YOLO_VARIANT_ID = {"yolov5s": 0, "yolov5m": 1, "yolov5l": 2, "yolov5x": 3}


class Engine:
    """One per process/GPU.  `yolo_sd`: {name+'.weight'/'.bias': ndarray} (BN folded); `reid_sd`: un-fused ReID state_dict."""

    def __init__(self, yolo_sd=None, reid_sd=None, *, device=0, precision="bf16", model_name="yolov5s", num_classes=80,
                 img_size=640, max_batch=16, max_frame_hw=(720, 1280), conf_thres=0.25, iou_thres=0.45, max_det=300,
                 max_candidates=4096, max_crops=1024, max_tracks=4096, nn_budget_cap=100, max_trackers=256, tracks_per_tracker=0):
        lib = L.lib()
        cfg = L.EngineConfig()
        L.check(lib.vc_engine_config_default(C.byref(cfg)))
        cfg.device = device
        cfg.precision = L.PREC_ID[precision]
        cfg.yolo_variant = YOLO_VARIANT_ID[model_name]
        cfg.num_classes, cfg.img_size, cfg.max_batch = num_classes, img_size, max_batch
        cfg.max_frame_h, cfg.max_frame_w = max_frame_hw
        cfg.conf_thres, cfg.iou_thres, cfg.max_det, cfg.max_candidates = conf_thres, iou_thres, max_det, max_candidates
        cfg.max_crops, cfg.max_tracks, cfg.nn_budget_cap = max_crops, max_tracks, nn_budget_cap
        cfg.max_trackers = max_trackers
        cfg.tracks_per_tracker = tracks_per_tracker      # live tracks + detections one tracker step may hold; 0: 512, the most the kernel takes
        cfg.with_detector = 1 if yolo_sd is not None else 0
        cfg.with_reid = 1 if reid_sd is not None else 0
        self.cfg = cfg
        self.precision = precision
        self._h = C.c_void_p()
        self._deferred_destroy = []          # tracker handles queued by finalisers (tracker_destroy_later)
        L.check(lib.vc_engine_create(C.byref(cfg), C.byref(self._h)))
        if yolo_sd is not None:
            self._upload(L.NET_YOLO, lambda n: (yolo_sd[n + ".weight"], yolo_sd[n + ".bias"]))
            if "model.24.anchors_px" in yolo_sd:             # checkpoint.load_yolov5_checkpoint: Detect anchors x stride (pixels)
                a = L.f32(yolo_sd["model.24.anchors_px"]).reshape(18)
                L.check(lib.vc_engine_set_anchors(self._h, L.ptr(a, C.c_float)))
        if reid_sd is not None:
            folded = fold_reid(reid_sd)
            self._upload(L.NET_REID, lambda n: folded[n])
        L.check(lib.vc_engine_finalize(self._h))

    # ---------------------------------------------------------------- lifecycle
    def _upload(self, net, getter):
        lib = L.lib()
        n = C.c_int()
        L.check(lib.vc_engine_param_count(self._h, net, C.byref(n)))
        for i in range(n.value):
            name = C.create_string_buffer(128)
            dims = (C.c_int * 4)()
            L.check(lib.vc_engine_param_info(self._h, net, i, name, 128, dims))
            w, b = getter(name.value.decode())
            w, b = L.f32(w), L.f32(b)
            if tuple(w.shape) != tuple(dims):
                raise ValueError(f"{name.value.decode()}: expected weight shape {tuple(dims)}, got {w.shape}")
            L.check(lib.vc_engine_set_param(self._h, net, name.value, L.ptr(w, C.c_float), L.ptr(b, C.c_float)))

    def close(self):
        if self._h:
            for r in list(getattr(self, "_renderers", ())):      # their contexts die with the engine: close them first
                r.close()
            for l in list(getattr(self, "_lives", ())):          # live counters too
                l.close()
            L.lib().vc_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        L.check(L.lib().vc_engine_sync(self._h))

    def set_option(self, name, value):
        """Kernel-selection switch of the live engine ("c3_fused", "bneck_fused", "bneck_cv3", "front_fused", "sparse_head", "reid_block_fused", "stem_direct", "crop_per_pixel", "dot_arena_mb", "dyn_tiles" (1: the fused persistent kernels claim their tiles from a per-launch counter, 0: they walk them by fixed stride; same results), "dyn_tiles_mask" (which of them claim while "dyn_tiles" is on: 1 front_fused_kernel, 2 c3_fused_kernel, 4 bneck_fused_kernel); diagnostics: "ff_ablate", "c3_ablate", "dyn_tiles_ring" (counter pairs in use, 1 .. 1024: the tests make them come round again)), or "embed_kept_only" (1: crop and embed only the boxes DeepSort.update's own filter keeps; 0: every box)."""
        L.check(L.lib().vc_engine_set_option(self._h, name.encode(), int(value)))

    def stream_reset(self):
        """Abandon everything in flight on the stream path (after an error, or to replay a clip)."""
        L.check(L.lib().vc_stream_reset(self._h))
        self._async_shapes = []

    def stream_crop_stats(self):
        """(boxes that reached the ReID stage, crops the ReID net was run on): running totals of the stream path and the blocking
        tracker calls since the engine was created or `stream_reset` was called."""
        boxes, crops = C.c_int64(), C.c_int64()
        L.check(L.lib().vc_stream_crop_stats(self._h, C.byref(boxes), C.byref(crops)))
        return boxes.value, crops.value

    # ---------------------------------------------------------------- class filter and label map
    def set_class_map(self, classes):
        """Restrict the detector to some classes and relabel them, on every detect path (`vc_engine_set_class_map`: the filter runs on
        the device in front of the NMS, where upstream's `classes` argument applies; the relabel behind it).  `classes`: a list of
        class ids (list order gives labels 0..), a dict {class: label} (labels may repeat and need not be dense), or None to clear."""
        if classes is None:
            L.check(L.lib().vc_engine_set_class_map(self._h, None, 0))
            return
        t = class_table(self.cfg.num_classes, classes)
        L.check(L.lib().vc_engine_set_class_map(self._h, L.ptr(t, C.c_int), len(t)))

    def _class_map(self):
        nc = self.cfg.num_classes
        t, n = np.zeros(nc, np.int32), C.c_int()
        L.check(L.lib().vc_engine_class_map(self._h, L.ptr(t, C.c_int), nc, C.byref(n)))
        return t, n.value

    @property
    def class_map(self):
        """label_of_class [num_classes] int32 (-1 = dropped); the identity when no map is set."""
        return self._class_map()[0]

    @property
    def num_labels(self):
        """Labels a detection can leave the engine with (largest label + 1; num_classes when no map is set): the tracker fan-out."""
        return self._class_map()[1]

    # ---------------------------------------------------------------- detect (AutoShape forward)
    def detect(self, imgs_rgb):
        """list of HxWx3 uint8 RGB -> list of (n,6) float32 [x1,y1,x2,y2,conf,cls] in source pixels."""
        n = len(imgs_rgb)
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs_rgb]
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        hs = (C.c_int * n)(*[im.shape[0] for im in imgs])
        ws = (C.c_int * n)(*[im.shape[1] for im in imgs])
        md = self.cfg.max_det
        out = np.zeros((n, md, 6), np.float32)
        cnt = np.zeros(n, np.int32)
        L.check(L.lib().vc_detect(self._h, ptrs, hs, ws, n, L.ptr(out, C.c_float), L.ptr(cnt, C.c_int)))
        return [out[i, :cnt[i]].copy() for i in range(n)]

    def debug_layer(self, layer, batch=1):
        dims = (C.c_int * 4)()
        cap = batch * max(640, int(self.cfg.img_size)) ** 2 * 32     # largest layer: (size/2)^2 x 64..128 channels
        buf = np.zeros(cap, np.float32)
        L.check(L.lib().vc_detect_debug_layer(self._h, layer, L.ptr(buf, C.c_float), cap, dims))
        b, h, w, c = dims
        return buf[: b * h * w * c].reshape(b, h, w, c).copy()

    def debug_pred(self, arm=False):
        if arm:
            L.check(L.lib().vc_detect_debug_pred(self._h, None, 0))
            return None
        nh, nw, nt = C.c_int(), C.c_int(), C.c_int()
        L.check(L.lib().vc_detect_debug_shape(self._h, C.byref(nh), C.byref(nw), C.byref(nt)))
        no = self.cfg.num_classes + 5
        buf = np.zeros(self.cfg.max_batch * nt.value * no, np.float32)
        L.check(L.lib().vc_detect_debug_pred(self._h, L.ptr(buf, C.c_float), buf.size))
        return buf.reshape(self.cfg.max_batch, nt.value, no)

    # ---------------------------------------------------------------- launch recorder (diagnostics)
    def record_arm(self, net="yolo"):
        """Record every launch of the next detector ("yolo") or ReID ("reid") pass (`vc_record_arm`)."""
        L.check(L.lib().vc_record_arm(self._h, L.NET_YOLO if net == "yolo" else L.NET_REID))

    def record_read(self):
        """(records, arena) of the recorded pass: the parsed JSON of `vc_record_list` and the uint8 array its offsets point into."""
        import json
        size = C.c_size_t()
        L.check(L.lib().vc_record_list(self._h, None, 0, C.byref(size)))
        text = C.create_string_buffer(size.value)
        L.check(L.lib().vc_record_list(self._h, text, size.value, C.byref(size)))
        rec = json.loads(text.value.decode())
        arena = np.zeros(max(rec["arena_bytes"], 1), np.uint8)
        L.check(L.lib().vc_record_read(self._h, arena.ctypes.data_as(C.c_void_p), arena.size))
        return rec["launches"], arena

    # ---------------------------------------------------------------- embed (Extractor)
    def embed(self, bgr, boxes_cxcywh):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        boxes = L.f64(boxes_cxcywh).reshape(-1, 4)
        out = np.zeros((len(boxes), L.FEAT_DIM), np.float32)
        L.check(L.lib().vc_embed(self._h, L.ptr(bgr, C.c_uint8), bgr.shape[0], bgr.shape[1], L.ptr(boxes, C.c_double),
                                 len(boxes), L.ptr(out, C.c_float)))
        return out

    def embed_input(self, k):
        """The k x 50 x 50 x 3 network input the last embed() built (diagnostics)."""
        buf = np.empty((k, 50, 50, 3), np.float32)
        dims = (C.c_int * 4)()
        L.check(L.lib().vc_embed_debug_input(self._h, k, L.ptr(buf, C.c_float), buf.size, dims))
        return buf

    def embed_tensor(self, x_nchw):
        x = L.f32(x_nchw)
        out = np.zeros((len(x), L.FEAT_DIM), np.float32)
        L.check(L.lib().vc_embed_tensor(self._h, L.ptr(x, C.c_float), len(x), L.ptr(out, C.c_float)))
        return out

    def pretune(self, crop_counts=(32, 64, 128, 256, 512, 1024)):
        """Run the ReID net once per problem-size bucket so the conv autotuner (engine_run.hip::tuned_cfg) has picked its tile
        configurations before any timed work; the detector's convs are tuned by the first (warm-up) batch."""
        for k in crop_counts:
            if k <= self.cfg.max_crops and self.cfg.with_reid:
                self.embed_tensor(np.zeros((k, 3, 50, 50), np.float32))

    # ---------------------------------------------------------------- tracker
    def tracker_create(self, max_dist=0.2, min_confidence=0.3, nms_max_overlap=1.0, max_iou_distance=0.7, max_age=70,
                       n_init=3, nn_budget=100):
        while self._deferred_destroy:                      # handles queued by DeepSort.__del__
            L.check(L.lib().vc_tracker_destroy(self._h, self._deferred_destroy.pop()))
        p = L.TrackerParams(max_dist, min_confidence, nms_max_overlap, max_iou_distance, max_age, n_init, nn_budget)
        tid = C.c_int()
        L.check(L.lib().vc_tracker_create(self._h, C.byref(p), C.byref(tid)))
        return tid.value

    def tracker_destroy(self, tid):
        if self._h:
            L.check(L.lib().vc_tracker_destroy(self._h, tid))

    def tracker_destroy_later(self, tid):
        """From a finaliser: the handle is given back at the next tracker_create (vc_tracker_destroy waits for the batches in flight)."""
        self._deferred_destroy.append(tid)

    def tracker_reset(self, tid):
        L.check(L.lib().vc_tracker_reset(self._h, tid))

    def tracker_step(self, tid, tlwh, conf, feat):
        tlwh, conf, feat = L.f64(tlwh).reshape(-1, 4), L.f64(conf).reshape(-1), L.f32(feat).reshape(-1, L.FEAT_DIM)
        L.check(L.lib().vc_tracker_step(self._h, tid, L.ptr(tlwh, C.c_double), L.ptr(conf, C.c_double),
                                        L.ptr(feat, C.c_float), len(conf)))

    def tracker_state(self, tid, with_cov=True):
        n = C.c_int()
        L.check(L.lib().vc_tracker_count(self._h, tid, C.byref(n)))
        n = n.value
        ids = np.zeros(n, np.int64)
        st, hits, age, tsu, gal = (np.zeros(n, np.int32) for _ in range(5))
        mean = np.zeros((n, 8))
        cov = np.zeros((n, 8, 8)) if with_cov else None
        L.check(L.lib().vc_tracker_state(self._h, tid, max(n, 1), L.ptr(ids, C.c_int64), L.ptr(st, C.c_int), L.ptr(hits, C.c_int),
                                         L.ptr(age, C.c_int), L.ptr(tsu, C.c_int), L.ptr(mean, C.c_double),
                                         L.ptr(cov, C.c_double), L.ptr(gal, C.c_int)))
        return {"ids": ids, "state": st, "hits": hits, "age": age, "tsu": tsu, "mean": mean, "cov": cov, "gallery": gal}

    def tracker_debug_costs(self, cap=1 << 18):
        """(appearance [T, D], iou [T, D]) cost matrices of the last blocking single-tracker step, as the tracker kernel computed
        them (rows are only meaningful for the tracks that took part: confirmed tracks / IoU candidates)."""
        app, iou = np.zeros(cap), np.zeros(cap)
        t, d = C.c_int(), C.c_int()
        L.check(L.lib().vc_tracker_debug_costs(self._h, cap, L.ptr(app, C.c_double), L.ptr(iou, C.c_double), C.byref(t), C.byref(d)))
        n = t.value * d.value
        return app[:n].reshape(t.value, d.value).copy(), iou[:n].reshape(t.value, d.value).copy()

    def tracker_snapshot(self, tid) -> bytes:
        """Serialised tracker state (parameters, id counter, Kalman state, galleries) for stream migration."""
        n = C.c_size_t()
        L.check(L.lib().vc_tracker_snapshot(self._h, tid, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        L.check(L.lib().vc_tracker_snapshot(self._h, tid, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def tracker_restore(self, tid, blob: bytes):
        """Replace tracker `tid`'s state and parameters with a snapshot (possibly taken on another engine / GPU)."""
        buf = C.create_string_buffer(bytes(blob), len(blob))
        L.check(L.lib().vc_tracker_restore(self._h, tid, buf, len(blob)))

    def deepsort_update(self, tid, bbox_xyxy, confidences, ori_img):
        img = np.ascontiguousarray(ori_img, dtype=np.uint8)
        b, c = L.f64(bbox_xyxy).reshape(-1, 4), L.f64(confidences).reshape(-1)
        cap = self.cfg.max_tracks
        rows = np.zeros((cap, 7), np.int64)
        m = C.c_int()
        L.check(L.lib().vc_deepsort_update(self._h, tid, L.ptr(img, C.c_uint8), img.shape[0], img.shape[1], L.ptr(b, C.c_double),
                                           L.ptr(c, C.c_double), len(c), L.ptr(rows, C.c_int64), cap, C.byref(m)))
        return rows[: m.value].copy()

    def videotracker_run(self, tracker_ids, image, boxes_xywh, labels, scores):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        b, s = L.f64(boxes_xywh).reshape(-1, 4), L.f64(scores).reshape(-1)
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        cap = self.cfg.max_tracks
        rows = np.zeros((cap, 6), np.int64)
        m = C.c_int()
        L.check(L.lib().vc_videotracker_run(self._h, L.ptr(tr, C.c_int), len(tr), L.ptr(img, C.c_uint8), img.shape[0], img.shape[1],
                                            L.ptr(b, C.c_double), L.ptr(lab, C.c_int64), L.ptr(s, C.c_double), len(s),
                                            L.ptr(rows, C.c_int64), cap, C.byref(m)))
        return rows[: m.value].copy()

    # ---------------------------------------------------------------- fused stream path
    def _stream_call(self, tracker_ids, frames_dev_ptr, b, h, w, cap_rows):
        key = (b, cap_rows)
        bufs = self._stream_bufs.get(key) if hasattr(self, "_stream_bufs") else None
        if bufs is None:                                  # output buffers are reused across calls (1.5 MB at b = 64)
            if not hasattr(self, "_stream_bufs"):
                self._stream_bufs = {}
            bufs = self._stream_bufs[key] = (np.empty((b, cap_rows, 6), np.int64), np.zeros(b, np.int32), np.zeros(b, np.int32))
        rows, m, nd = bufs
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        L.check(L.lib().vc_stream_run(self._h, L.ptr(tr, C.c_int), len(tr), C.c_void_p(frames_dev_ptr), b, h, w,
                                      L.ptr(rows, C.c_int64), cap_rows, L.ptr(m, C.c_int), L.ptr(nd, C.c_int)))
        return rows, m, nd

    def stream_run(self, tracker_ids, frames_dev_ptr, b, h, w, cap_rows=512):
        """frames_dev_ptr: integer device address of B x H x W x 3 uint8 BGR frames (e.g. torch_tensor.data_ptr()).
        Returns (per-frame row arrays [m_i, 6] = x1,y1,x2,y2,track id,label; detections per frame)."""
        rows, m, nd = self._stream_call(tracker_ids, frames_dev_ptr, b, h, w, cap_rows)
        return [rows[i, : m[i]].copy() for i in range(b)], nd.copy()

    def stream_run_packed(self, tracker_ids, frames_dev_ptr, b, h, w, cap_rows=512):
        """Same step, rows of all frames packed: (rows [sum m, 6], frame index of each row [sum m], detections per frame)."""
        rows, m, nd = self._stream_call(tracker_ids, frames_dev_ptr, b, h, w, cap_rows)
        keep = np.arange(cap_rows)[None, :] < m[:, None]
        return rows[keep], np.repeat(np.arange(b), m), nd.copy()

    def stream_run_async(self, tracker_ids, frames_dev_ptr, b, h, w, cap_rows=512):
        """Enqueue the batch's ReID and its tracker kernel (one launch on the engine's tracker stream, no host thread) and return;
        `stream_collect` picks the rows up (in order)."""
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        L.check(L.lib().vc_stream_run_async(self._h, L.ptr(tr, C.c_int), len(tr), C.c_void_p(frames_dev_ptr), b, h, w, cap_rows))
        self._async_shapes = getattr(self, "_async_shapes", [])
        self._async_shapes.append((b, cap_rows))

    def stream_run_async_multi(self, tracker_ids, cam_of_frame, frames_dev_ptr, b, h, w, cap_rows=512):
        """Multi-camera batch: tracker_ids [n_cam][num_classes], cam_of_frame [b] (each camera's frames in stream order); rows are
        collected with `stream_collect` per frame of the batch, as for one camera."""
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        assert tr.ndim == 2, "tracker_ids must be [n_cam][num_classes]"
        cams = np.ascontiguousarray(cam_of_frame, dtype=np.int32).reshape(-1)
        assert len(cams) == b
        L.check(L.lib().vc_stream_run_async_multi(self._h, L.ptr(tr, C.c_int), tr.shape[0], tr.shape[1], L.ptr(cams, C.c_int),
                                                  C.c_void_p(frames_dev_ptr), b, h, w, cap_rows))
        self._async_shapes = getattr(self, "_async_shapes", [])
        self._async_shapes.append((b, cap_rows))

    def stream_collect(self):
        """Rows of the oldest asynchronous batch, packed like `stream_run_packed` (blocks until its tracker loop is done)."""
        if not getattr(self, "_async_shapes", None):
            raise L.VcError(3, "stream_collect: no asynchronous batch is in flight (stream_run_async first)")
        b, cap_rows = self._async_shapes.pop(0)
        rows, m, nd = np.empty((b, cap_rows, 6), np.int64), np.zeros(b, np.int32), np.zeros(b, np.int32)
        L.check(L.lib().vc_stream_collect(self._h, L.ptr(rows, C.c_int64), cap_rows, L.ptr(m, C.c_int), L.ptr(nd, C.c_int), b))
        keep = np.arange(cap_rows)[None, :] < m[:, None]
        return rows[keep], np.repeat(np.arange(b), m), nd

    def stream_submit(self, frames_dev_ptr, b, h, w):
        """Enqueue the detector for a batch (returns immediately); the matching stream_run consumes it."""
        L.check(L.lib().vc_stream_submit(self._h, C.c_void_p(frames_dev_ptr), b, h, w))

    def stream_stage_host(self, frames_host_ptr, b, h, w):
        """Enqueue ONLY the host-to-device copy of a batch of (pinned) host frames; returns the device address to pass to stream_submit
        (which starts the detector behind the copy) and then stream_run / stream_run_async.  Stage batch i + 2 before submitting
        batch i + 1 and the copy runs under the detector of the batch before it."""
        out = C.c_void_p()
        L.check(L.lib().vc_stream_stage_host(self._h, C.c_void_p(frames_host_ptr), b, h, w, C.byref(out)))
        return out.value

    def stream_submit_host(self, frames_host_ptr, b, h, w):
        """Enqueue the host-to-device copy of a batch of (pinned) host frames and the detector behind it; returns the device
        address to pass to stream_run / stream_run_async for this batch."""
        out = C.c_void_p()
        L.check(L.lib().vc_stream_submit_host(self._h, C.c_void_p(frames_host_ptr), b, h, w, C.byref(out)))
        return out.value

    def stream_stage_yuv_host(self, yuv_host_ptr, b, h, w, desc=None):
        """Like stream_stage_host for a batch of YUV frames in (pinned) host memory laid out as `desc` (`yuv_desc(...)`, any of its
        formats; None: tight NV12, BT.601 limited): the raw bytes cross PCIe (1.5 B per pixel for 8-bit 4:2:0, 2 for i422, 3 for p016 /
        i010 / i444) and are converted on the engine's copy stream;
        returns the device address of the BGR batch for stream_submit / stream_run*."""
        out = C.c_void_p()
        d = desc if desc is not None else yuv_desc()
        L.check(L.lib().vc_stream_stage_yuv_host(self._h, C.byref(d), C.c_void_p(yuv_host_ptr), b, h, w, C.byref(out)))
        return out.value

    def stream_stage_yuv_dev(self, yuv_dev_ptr, b, h, w, desc=None):
        """The same for YUV surfaces already in device memory (a hardware decoder's output): converted in place of the copy.  The
        surfaces must stay valid until the batch's stream_run / stream_run_async call has returned."""
        out = C.c_void_p()
        d = desc if desc is not None else yuv_desc()
        L.check(L.lib().vc_stream_stage_yuv_dev(self._h, C.byref(d), C.c_void_p(yuv_dev_ptr), b, h, w, C.byref(out)))
        return out.value

    def stream_stage_frames(self, frames, h, w):
        """One batch from per-frame sources (`frame_src(...)` each: its own address, kind and, for YUV, descriptor -- the surfaces of
        several decoders interleaved): host frames are copied, YUV frames converted and device BGR frames copied by ONE kernel launch
        on the engine's copy stream, into an ingest slot under the rules of stream_stage_host.  All frames share h x w.  Returns the
        device address of the BGR batch for stream_submit / stream_run*."""
        out = C.c_void_p()
        arr = _frame_array(frames)
        L.check(L.lib().vc_stream_stage_frames(self._h, arr, len(frames), h, w, C.byref(out)))
        return out.value

    # ---------------------------------------------------------------- sized batches: cameras of different frame sizes in one batch
    def stream_stage_frames_sized(self, frames, dims):
        """`stream_stage_frames` for a sized batch: frame f has its own size dims[f] = (h, w); all frames must run at one network
        shape (`autoshape_net_size` of each alone).  Frame f lands as tight BGR in cell f of an ingest slot (`frames_layout_sized`
        gives the cell size).  Returns the device address of the cells for stream_submit_sized / stream_run_async_multi_sized."""
        out = C.c_void_p()
        L.check(L.lib().vc_stream_stage_frames_sized(self._h, _frame_array(frames), _dims_array(dims), len(frames), C.byref(out)))
        return out.value

    def stream_submit_sized(self, frames_dev_ptr, dims):
        """Enqueue the detector for a sized batch (a staged one or the caller's own device buffer laid out in cells)."""
        L.check(L.lib().vc_stream_submit_sized(self._h, C.c_void_p(frames_dev_ptr), _dims_array(dims), len(dims)))

    def stream_run_async_multi_sized(self, tracker_ids, cam_of_frame, frames_dev_ptr, dims, cap_rows=512):
        """`stream_run_async_multi` for a sized batch; within the batch all frames of one camera have one size (the size that
        camera's track boxes are clamped to).  Rows are collected with `stream_collect`."""
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        assert tr.ndim == 2, "tracker_ids must be [n_cam][num_classes]"
        b = len(dims)
        cams = np.ascontiguousarray(cam_of_frame, dtype=np.int32).reshape(-1)
        assert len(cams) == b
        L.check(L.lib().vc_stream_run_async_multi_sized(self._h, L.ptr(tr, C.c_int), tr.shape[0], tr.shape[1], L.ptr(cams, C.c_int),
                                                        C.c_void_p(frames_dev_ptr), _dims_array(dims), b, cap_rows))
        self._async_shapes = getattr(self, "_async_shapes", [])
        self._async_shapes.append((b, cap_rows))

    # ---------------------------------------------------------------- frame-sharded front end (one stream on several GPUs)
    def stream_embed(self, frames_dev_ptr, b, h, w):
        """Front half of the fused path for the oldest submission: (rows [n, 7] float64 = frame index in the batch, x1, y1, x2, y2,
        conf, label -- the boxes VideoTracker.run works on -- and the DEVICE address of the matching [n, 512] float32 embeddings)."""
        cap = b * self.cfg.max_det
        rows = np.zeros((cap, 7), np.float64)
        n, feat = C.c_int(), C.c_void_p()
        L.check(L.lib().vc_stream_embed(self._h, C.c_void_p(frames_dev_ptr), b, h, w, L.ptr(rows, C.c_double), cap, C.byref(n), C.byref(feat)))
        return rows[: n.value].copy(), feat.value or 0

    def allgather_rows(self, rows7, feat_dev_ptr, world):
        """RCCL all-gather (C ABI, vc_comm_init first) of every rank's rows + embeddings: (rows of all ranks, rank-major; device
        address of the gathered embeddings in the same order; rows per rank)."""
        rows = L.f64(rows7).reshape(-1, 7)
        cap = world * self.cfg.max_batch * self.cfg.max_det
        out = np.zeros((cap, 7), np.float64)
        counts = np.zeros(world, np.int32)
        feat = C.c_void_p()
        L.check(L.lib().vc_allgather_rows(self._h, L.ptr(rows, C.c_double), C.c_void_p(feat_dev_ptr or None), len(rows), L.ptr(out, C.c_double), cap,
                                          L.ptr(counts, C.c_int), C.byref(feat)))
        return out[: int(counts.sum())].copy(), feat.value or 0, counts

    def videotracker_run_features(self, tracker_ids, rows7, feat_dev_ptr, h, w, cap_rows=512):
        """VideoTracker.run for a run of frames with supplied detections (rows7 sorted by frame key) and device-resident embeddings:
        [(frame key, rows [m, 6] = x1, y1, x2, y2, track id, label)] per distinct key, ascending; one tracker kernel launch."""
        rows = L.f64(rows7).reshape(-1, 7)
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        nf_cap = max(len(np.unique(rows[:, 0])), 1)
        out = np.empty((nf_cap, cap_rows, 6), np.int64)
        m, keys, nf = np.zeros(nf_cap, np.int32), np.zeros(nf_cap, np.int64), C.c_int()
        L.check(L.lib().vc_videotracker_run_features(self._h, L.ptr(tr, C.c_int), len(tr), L.ptr(rows, C.c_double), C.c_void_p(feat_dev_ptr or None),
                                                     len(rows), h, w, L.ptr(out, C.c_int64), cap_rows, L.ptr(m, C.c_int), L.ptr(keys, C.c_int64),
                                                     nf_cap, C.byref(nf)))
        return [(int(keys[j]), out[j, : m[j]].copy()) for j in range(nf.value)]

    def stream_inject(self, det6=None, counts=None):
        if det6 is None:
            L.check(L.lib().vc_stream_inject(self._h, None, None, 0, 0))
            return
        d = L.f32(det6)
        c = np.ascontiguousarray(counts, dtype=np.int32)
        L.check(L.lib().vc_stream_inject(self._h, L.ptr(d, C.c_float), L.ptr(c, C.c_int), d.shape[0], d.shape[1]))

    # ---------------------------------------------------------------- measurement
    def profile(self, on):
        """False/0 off; True/1 blocking per-launch events for every stage (serialises the streams); 2 in-flight event pairs
        around the conv launches only (no host waits: usable inside a timed region), resolved by profile_read(PROF_CONV)."""
        L.check(L.lib().vc_profile_enable(self._h, 2 if on == 2 else (1 if on else 0)))

    def profile_reset(self):
        L.check(L.lib().vc_profile_reset(self._h))

    def profile_ops(self):
        buf = C.create_string_buffer(1 << 20)
        L.check(L.lib().vc_profile_ops(self._h, buf, len(buf)))
        return buf.value.decode()

    def profile_conv_busy(self):
        """(union_ms, span_ms) of the conv launches of the last resolved in-flight profiling region."""
        u, sp = C.c_double(), C.c_double()
        L.check(L.lib().vc_profile_conv_busy(self._h, C.byref(u), C.byref(sp)))
        return u.value, sp.value

    def profile_read_dense(self, cat):
        """(flops, bytes) of the category with the sparse Detect head credited as the dense head it replaces (after profile_read)."""
        fl, by = C.c_double(), C.c_double()
        L.check(L.lib().vc_profile_read_dense(self._h, cat, C.byref(fl), C.byref(by)))
        return fl.value, by.value

    def tune_export(self) -> str:
        """Conv autotune choices of this engine as text (the VC_TUNE_CACHE file format)."""
        n = C.c_size_t()
        L.check(L.lib().vc_tune_export(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        L.check(L.lib().vc_tune_export(self._h, buf, n.value, C.byref(n)))
        return buf.value.decode()

    def tune_import(self, text: str):
        """Adopt another engine's autotune choices (before the first launch of those shapes)."""
        L.check(L.lib().vc_tune_import(self._h, text.encode()))

    def profile_read(self, cat):
        ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        L.check(L.lib().vc_profile_read(self._h, cat, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}


# ---- single-function entry points (used by the parity tests) -------------------------------------------------------
# one record of the live counter's per-slot state (csrc/count_core.h: cc::LiveSlot, 88 bytes)
LIVE_SLOT_DTYPE = np.dtype([("open", np.int32), ("cam", np.int32), ("label", np.int32), ("at_last", np.int32), ("last_frame", np.int64),
                            ("first", np.int64, 4), ("last", np.int64, 4)])


def _live_zones(polygons, dir_lines):
    """Per-camera polygons [(n, 2)] and direction lines [(d, 4)] -> the concatenated arrays and counts of vc_live_create."""
    polys = [np.asarray(p, np.float64).reshape(-1, 2) for p in polygons]
    dirs = [np.asarray(d, np.float64).reshape(-1, 4) for d in dir_lines]
    if len(polys) != len(dirs) or not polys:
        raise ValueError("one polygon and one list of direction lines per camera")
    poly_n = np.array([len(p) for p in polys], np.int32)
    n_dir = np.array([len(d) for d in dirs], np.int32)
    return np.ascontiguousarray(np.concatenate(polys, 0)), poly_n, np.ascontiguousarray(np.concatenate(dirs, 0)), n_dir


class LiveCounter:
    """Running per-camera counts on the device (vc_live_*): attached to the engine's trackers tracker_ids [n_cam][n_labels], advanced by
    every tracker launch that steps one of them.  `counts()` at any moment = `NativeCounter.counts()` of each camera over the rows of
    all batches enqueued so far, as int32 (n_cam, max_dir, n_labels) -- rows d >= the camera's own number of directions are zero.
    polygons: per camera (n, 2); dir_lines: per camera (n_dir, 4) = x0, y0, x1, y1 in the order of the zone file's direction shapes.
    While it lives its trackers cannot be reset, destroyed or restored: `close()` first."""

    def __init__(self, engine, tracker_ids, polygons, dir_lines):
        tr = np.ascontiguousarray(tracker_ids, dtype=np.int32)
        if tr.ndim != 2:
            raise ValueError("tracker_ids must be [n_cam][n_labels]")
        poly, poly_n, dirs, n_dir = _live_zones(polygons, dir_lines)
        if len(poly_n) != tr.shape[0]:
            raise ValueError(f"{tr.shape[0]} cameras of trackers, {len(poly_n)} zones")
        self.engine, self.n_cam, self.n_labels, self.n_dir = engine, tr.shape[0], tr.shape[1], n_dir.copy()
        self.max_dir = int(n_dir.max())
        self._h = C.c_void_p()
        L.check(L.lib().vc_live_create(engine._h, self.n_cam, self.n_labels, L.ptr(tr.reshape(-1), C.c_int), L.ptr(poly, C.c_double),
                                       L.ptr(poly_n, C.c_int), L.ptr(dirs, C.c_double), L.ptr(n_dir, C.c_int), C.byref(self._h)))
        engine._lives = getattr(engine, "_lives", [])
        engine._lives.append(self)

    @property
    def shape(self):
        return (self.n_cam, self.max_dir, self.n_labels)

    def counts(self, with_frames=False):
        """The counts after every batch enqueued so far (waits for them); with_frames: also the frames handed in per camera."""
        out = np.zeros(self.shape, np.int32)
        fd = np.zeros(self.n_cam, np.int64)
        L.check(L.lib().vc_live_counts(self._h, L.ptr(out.reshape(-1), C.c_int), L.ptr(fd, C.c_int64)))
        return (out, fd) if with_frames else out

    def counts_dev(self):
        """Device address of the same int32 tensor (valid until the engine's next tracker launch or live-counter call)."""
        p = C.c_void_p()
        L.check(L.lib().vc_live_counts_dev(self._h, C.byref(p)))
        return p.value

    def stats(self):
        """(open_tracks, retired_tracks): tracks seen in their zone that can still produce rows / that were folded into the totals."""
        a, b = C.c_int(), C.c_int()
        L.check(L.lib().vc_live_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def allgather(self):
        """The count tensors of all ranks, (world, n_cam, max_dir, n_labels) rank-major: ncclAllGather from the device tensor."""
        from . import parallel
        _, world = parallel.ensure_comm(self.engine)
        out = np.zeros((world,) + self.shape, np.int32)
        L.check(L.lib().vc_live_allgather(self.engine._h, self._h, L.ptr(out.reshape(-1), C.c_int)))
        return out

    def enable_overlay(self, dir_keys, max_batch, max_rows_per_frame=64, depth=2):
        """From now on every uniform tracker launch that advances the counter also builds its batch's overlay lists on the device
        (vc_live_overlay_enable; the definition is overlay.LiveVisualizer).  dir_keys: per camera the names of its directions in the
        order of dir_lines, as the zone file spells them ("01") or as numbers.  depth: list buffers (1..4) -- a run call with all of
        them unconsumed raises VcError (VC_ERR_STATE)."""
        keys = [int(k) for cam in dir_keys for k in cam]
        if [len(cam) for cam in dir_keys] != self.n_dir.tolist():
            raise ValueError(f"direction keys per camera {[len(c) for c in dir_keys]}, direction lines {self.n_dir.tolist()}")
        k = np.array(keys, np.int32)
        L.check(L.lib().vc_live_overlay_enable(self._h, L.ptr(k, C.c_int), int(max_batch), int(max_rows_per_frame), int(depth)))
        self.overlay_depth, self._ov_cap = int(depth), None

    def overlay_lists(self, cap_prims=1 << 16, cap_frames=1024):
        """(prims12 (n, 12) int32, frame_first (b + 1) int32) of the OLDEST unconsumed batch, copied to the host (waits for it); the
        list buffer is consumed.  For tests and host consumers: the render path takes the lists on the device (Renderer.submit_live)."""
        prims = np.zeros((cap_prims, 12), np.int32)
        first = np.zeros(cap_frames + 1, np.int32)
        b, n = C.c_int(), C.c_int()
        L.check(L.lib().vc_live_overlay_lists(self._h, L.ptr(prims.reshape(-1), C.c_int), cap_prims, L.ptr(first, C.c_int), cap_frames, C.byref(b), C.byref(n)))
        return prims[:n.value].copy(), first[:b.value + 1].copy()

    # ---- checkpoint (vc_live_checkpoint* / vc_live_restore; DESIGN.md 5 "Live checkpoint") ----
    def enable_checkpoint(self, max_bytes):
        """Reserve the staging buffers of a checkpoint of at most max_bytes, once.  Nothing about a tracker launch changes."""
        L.check(L.lib().vc_live_checkpoint_enable(self._h, int(max_bytes)))

    def checkpoint_begin(self):
        """Enqueue the device pack of this counter and its trackers behind every batch enqueued so far, and its copy to pinned memory on
        a stream of its own.  Does not wait and does not touch the batches in flight; VcError (VC_ERR_STATE) if one is in flight already."""
        L.check(L.lib().vc_live_checkpoint_begin(self._h))

    def _checkpoint_out(self, fn) -> bytes:
        n = C.c_size_t()
        L.check(fn(self._h, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.uint8)
        L.check(fn(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out[:n.value].tobytes()

    def checkpoint_end(self) -> bytes:
        """The blob of the last `checkpoint_begin` (waits for its copy only).  VcError (VC_ERR_CAPACITY) if the state outgrew max_bytes."""
        return self._checkpoint_out(L.lib().vc_live_checkpoint_end)

    def checkpoint(self) -> bytes:
        """`checkpoint_begin` + `checkpoint_end`."""
        return self._checkpoint_out(L.lib().vc_live_checkpoint)

    def restore(self, blob: bytes, cam_map=None):
        """Replace the state of this counter's cameras cam_map[i] (i = camera of the blob; -1: that camera is not restored; None: identity) and of their
        trackers by the blob's, possibly taken on another engine / GPU.  Any refusal (VcError) leaves the counter and its trackers untouched."""
        buf = C.create_string_buffer(bytes(blob), max(len(blob), 1))
        cm = None if cam_map is None else np.ascontiguousarray(cam_map, dtype=np.int32).reshape(-1)
        if cm is not None and len(blob) >= CKPT_HEADER_BYTES and bytes(blob[:8]) == b"VCLIVE01" and len(cm) != checkpoint_dims(blob)[0]:
            raise ValueError(f"cam_map has {len(cm)} entries, the checkpoint {checkpoint_dims(blob)[0]} cameras")   # the library reads one per camera of the blob
        L.check(L.lib().vc_live_restore(self._h, buf, len(blob), L.ptr(cm, C.c_int)))

    def close(self):
        if self._h and self.engine._h:
            L.check(L.lib().vc_live_destroy(self._h))
        self._h = None
        if self in getattr(self.engine, "_lives", []):
            self.engine._lives.remove(self)


CKPT_HEADER_BYTES, CKPT_CAMERA_BYTES = 64, 1552          # sizeof(ck::CkptHeader), sizeof(ck::CkptCamera) of csrc/live_ckpt.h (tests/test_live_ckpt_host.py)


def checkpoint_dims(blob):
    """(n_cam, n_labels, max_dir) from the header of a live checkpoint"""
    import struct
    if len(blob) < CKPT_HEADER_BYTES or bytes(blob[:8]) != b"VCLIVE01":
        raise ValueError("not a live checkpoint")
    return struct.unpack_from("<3i", blob, 16)


def checkpoint_frames_done(blob):
    """frames_done per camera of a live checkpoint (header, then one section per camera), as of its `checkpoint_begin`"""
    import struct
    n_cam, n_labels, max_dir = checkpoint_dims(blob)
    cam_bytes = (CKPT_CAMERA_BYTES + 4 * max_dir * n_labels + 15) // 16 * 16
    if len(blob) < CKPT_HEADER_BYTES + n_cam * cam_bytes:
        raise ValueError("not a live checkpoint")
    return np.array([struct.unpack_from("<q", blob, CKPT_HEADER_BYTES + c * cam_bytes)[0] for c in range(n_cam)], np.int64)


def live_count(polygons, dir_lines, n_labels, tracker_cam, rows6, row_slot, tasks5, frame_no, freed, slots, base, stats):
    """vc_live_count_host: one launch of live_count_apply_kernel and live_count_read_kernel on host arrays.  slots (LIVE_SLOT_DTYPE
    [max_tracks]), base (n_cam, max_dir, n_labels) and stats [2] are the state before the batch; returns (slots, base, stats, counts) after."""
    poly, poly_n, dirs, n_dir = _live_zones(polygons, dir_lines)
    n_cam, max_dir = len(poly_n), int(n_dir.max())
    cam = np.ascontiguousarray(tracker_cam, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(rows6, dtype=np.int64).reshape(-1, 6)
    rs = np.ascontiguousarray(row_slot, dtype=np.int32).reshape(-1)
    tk = np.ascontiguousarray(tasks5, dtype=np.int32).reshape(-1, 5)
    fno = np.ascontiguousarray(frame_no, dtype=np.int64).reshape(-1)
    fr = np.ascontiguousarray(freed, dtype=np.int32).reshape(-1)
    slots = np.ascontiguousarray(slots, dtype=LIVE_SLOT_DTYPE).copy()
    base = np.ascontiguousarray(base, dtype=np.int32).reshape(n_cam, max_dir, n_labels).copy()
    stats = np.ascontiguousarray(stats, dtype=np.int32).reshape(2).copy()
    counts = np.zeros_like(base)
    assert len(rs) == len(rows)
    L.check(L.lib().vc_live_count_host(n_cam, n_labels, L.ptr(poly, C.c_double), L.ptr(poly_n, C.c_int), L.ptr(dirs, C.c_double), L.ptr(n_dir, C.c_int),
                                       len(cam), L.ptr(cam, C.c_int), len(slots), L.ptr(rows, C.c_int64), L.ptr(rs, C.c_int), len(rows),
                                       L.ptr(tk, C.c_int), len(tk), L.ptr(fno, C.c_int64), len(fno), L.ptr(fr, C.c_int), len(fr),
                                       C.c_void_p(slots.ctypes.data), L.ptr(base.reshape(-1), C.c_int), L.ptr(stats, C.c_int), L.ptr(counts.reshape(-1), C.c_int)))
    return slots, base, stats, counts


OVERLAY_UNWRITTEN = np.frombuffer(b"\xa5" * 4, np.int32)[0]          # what an arena word no frame owns holds after vc_live_overlay_host


def live_overlay(polygons, dir_lines, dir_keys, n_labels, tracker_cam, slots, counts_before, rows6, row_slot, tasks5, frame_no, cam_of_frame, hw,
                 cap_prims, *, host=False, allow_overflow=False):
    """vc_live_overlay_host: one launch of the two overlay build kernels on host arrays (host=True: vc_overlay_build_host, the same
    arithmetic on the CPU, no GPU needed).  slots: LIVE_SLOT_DTYPE records AFTER the batch's apply launch; counts_before
    (n_cam, max_dir, n_labels) or None for "no text".  Returns (arena (cap_prims, 12) int32, frame_first (b + 1) int32, overflow): frame
    f owns arena[frame_first[f]:frame_first[f + 1]].  A frame that does not fit raises VcError (VC_ERR_CAPACITY) unless allow_overflow."""
    poly, poly_n, dirs, n_dir = _live_zones(polygons, dir_lines)
    n_cam, max_dir = len(poly_n), int(n_dir.max())
    keys = np.array([int(k) for cam in dir_keys for k in cam], np.int32)
    assert [len(c) for c in dir_keys] == n_dir.tolist()
    cam = np.ascontiguousarray(tracker_cam, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(rows6, dtype=np.int64).reshape(-1, 6)
    rs = np.ascontiguousarray(row_slot, dtype=np.int32).reshape(-1)
    tk = np.ascontiguousarray(tasks5, dtype=np.int32).reshape(-1, 5)
    fno = np.ascontiguousarray(frame_no, dtype=np.int64).reshape(-1)
    cof = np.ascontiguousarray(cam_of_frame, dtype=np.int32).reshape(-1)
    slots = np.ascontiguousarray(slots, dtype=LIVE_SLOT_DTYPE)
    cb = None if counts_before is None else np.ascontiguousarray(counts_before, dtype=np.int32).reshape(n_cam, max_dir, n_labels)
    assert len(rs) == len(rows) and len(cof) == len(fno)
    arena = np.full((cap_prims, 12), OVERLAY_UNWRITTEN, np.int32)
    first = np.zeros(len(fno) + 1, np.int32)
    fn = L.lib().vc_overlay_build_host if host else L.lib().vc_live_overlay_host
    rc = fn(n_cam, n_labels, L.ptr(poly, C.c_double), L.ptr(poly_n, C.c_int), L.ptr(dirs, C.c_double), L.ptr(n_dir, C.c_int), L.ptr(keys, C.c_int),
            len(cam), L.ptr(cam, C.c_int), len(slots), C.c_void_p(slots.ctypes.data), L.ptr(None if cb is None else cb.reshape(-1), C.c_int),
            L.ptr(rows, C.c_int64), L.ptr(rs, C.c_int), len(rows), L.ptr(tk, C.c_int), len(tk), L.ptr(fno, C.c_int64), L.ptr(cof, C.c_int), len(fno),
            int(hw[0]), int(hw[1]), L.ptr(arena.reshape(-1), C.c_int), cap_prims, L.ptr(first, C.c_int))
    overflow = rc == 4                                      # VC_ERR_CAPACITY
    if not (allow_overflow and overflow):
        L.check(rc)
    return arena, first, overflow


def conv2d(x_nhwc, w_oihw, bias, *, stride=1, pad=0, act=0, res=None, res_mode=0, precision="bf16"):
    x, w, b = L.f32(x_nhwc), L.f32(w_oihw), L.f32(bias)
    B, H, W, Ci = x.shape
    Co, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    d = L.ConvDesc(B, H, W, Ci, Co, kh, kw, stride, pad, act, res_mode, L.PREC_ID[precision])
    y = np.zeros((B, Ho, Wo, Co), np.float32)
    r = L.f32(res) if res is not None else None
    L.check(L.lib().vc_conv2d_host(C.byref(d), L.ptr(x, C.c_float), L.ptr(w, C.c_float), L.ptr(b, C.c_float),
                                   L.ptr(r, C.c_float), L.ptr(y, C.c_float)))
    return y


def _conv_view(view, *, in_cs, out_cs):
    v = L.ConvView(in_cs=in_cs, in_co=0, out_cs=out_cs, out_co=0, m_valid=-1)
    for k, val in view.items():
        if not hasattr(v, k):
            raise KeyError(k)
        setattr(v, k, int(val))
    return v


def conv2d_view(x, w_oihw, bias, y, *, view, x_up=None, res=None, y2=None, stride=1, pad=0, act=0, res_mode=0, precision="bf16"):
    """launch_conv under the views of `view` (a dict of vc_conv_view fields) on WHOLE buffers: x (B, H, W, in_cs), x_up (B, H/2, W/2, up_cs),
    res (B, Ho, Wo, res_cs); y (B, Ho, Wo, out_cs) and y2 (B, Ho, Wo, out2_cs) are uploaded, launched into and returned as copies.
    The input channel count is the weights'.  Returns y, or (y, y2) under a split."""
    x, w, b = L.f32(x), L.f32(w_oihw), L.f32(bias)
    B, H, W, in_cs = x.shape
    Co, Ci, kh, kw = w.shape
    y = L.f32(y).copy()
    v = _conv_view(view, in_cs=in_cs, out_cs=y.shape[3])
    d = L.ConvDesc(B, H, W, Ci, Co, kh, kw, stride, pad, act, res_mode if res is not None else 0, L.PREC_ID[precision])
    xu = L.f32(x_up) if x_up is not None else None
    r = L.f32(res) if res is not None else None
    y2 = L.f32(y2).copy() if y2 is not None else None
    if xu is not None:
        assert xu.shape == (B, H // 2, W // 2, v.up_cs)
    if r is not None:
        assert r.shape == y.shape[:3] + (v.res_cs,)
    if y2 is not None:
        assert y2.shape == y.shape[:3] + (v.out2_cs,)
    try:
        L.check(L.lib().vc_conv2d_view_host(C.byref(d), C.byref(v), L.ptr(x, C.c_float), L.ptr(xu, C.c_float), L.ptr(w, C.c_float), L.ptr(b, C.c_float),
                                            L.ptr(r, C.c_float), L.ptr(y, C.c_float), L.ptr(y2, C.c_float)))
    except L.VcError as err:
        err.outputs = (y, y2)              # what the refused call left in the output arrays
        raise
    return y if y2 is None else (y, y2)


def conv_s2_pw(x, w3, b3, w1, b1, y, *, view, y2=None):
    """launch_s2halo_pw on whole buffers (bf16): 3x3 / s2 / p1 + SiLU to 128 channels over the slice (in_cs, in_co) of x, then on the tile the
    pointwise 128 -> 128 + SiLU, stored through view's out_* / split / out2_*.  Returns y, or (y, y2) under a split."""
    x, w3, b3, w1, b1 = L.f32(x), L.f32(w3), L.f32(b3), L.f32(w1), L.f32(b1)
    B, H, W, in_cs = x.shape
    Co, Ci, kh, kw = w3.shape
    y = L.f32(y).copy()
    v = _conv_view(view, in_cs=in_cs, out_cs=y.shape[3])
    d = L.ConvDesc(B, H, W, Ci, Co, kh, kw, 2, 1, 1, 0, L.PREC_BF16)
    y2 = L.f32(y2).copy() if y2 is not None else None
    if y2 is not None:
        assert y2.shape == y.shape[:3] + (v.out2_cs,)
    L.check(L.lib().vc_conv_s2_pw_host(C.byref(d), C.byref(v), L.ptr(x, C.c_float), L.ptr(w3, C.c_float), L.ptr(b3, C.c_float), L.ptr(w1, C.c_float),
                                       L.ptr(b1, C.c_float), L.ptr(y, C.c_float), L.ptr(y2, C.c_float)))
    return y if y2 is None else (y, y2)


def fused_block(kind, x, weights, *, view, y=None, z=None):
    """One launch of a fused block kernel on WHOLE buffers (bf16): kind "c3" (vc_c3_fused_host, weights = w12, b12, wm1, bm1, wm2, bm2, w3,
    b3), "bneck" (vc_bneck_fused_host: w1, b1, w2, b2 and, with view["cv3"], w3, b3) or "reid" (vc_reid_block_fused_host: w1, b1, w2, b2).
    x (B, H, W, in_cs), y (B, H, W, out_cs) and z (B, H, W, z_cs) are uploaded, launched on and returned as copies (x, y, z); y is None when
    view["out_buf"] is 1, z when there is no cv3 or view["z_buf"] is not 0.  `view`: the other vc_fused_view fields.  A refusal raises VcError
    with the arrays as the call left them in err.outputs."""
    x = L.f32(x).copy()
    B, H, W, in_cs = x.shape
    y = L.f32(y).copy() if y is not None else None
    z = L.f32(z).copy() if z is not None else None
    v = L.FusedView(in_cs=in_cs, out_cs=y.shape[3] if y is not None else 0, z_cs=z.shape[3] if z is not None else 0)
    for k, val in view.items():
        if not hasattr(v, k):
            raise KeyError(k)
        setattr(v, k, int(val))
    assert (y is None) == (v.out_buf == 1) and (y is None or y.shape[:3] == x.shape[:3])
    assert (z is None) == (not v.cv3 or v.z_buf != 0) and (z is None or z.shape[:3] == x.shape[:3])
    ws = [L.f32(a) for a in weights]
    assert len(ws) == {"c3": 8, "bneck": 6 if v.cv3 else 4, "reid": 4}[kind]
    pw = [L.ptr(a, C.c_float) for a in ws]
    try:
        if kind == "c3":
            L.check(L.lib().vc_c3_fused_host(B, H, W, C.byref(v), L.ptr(x, C.c_float), *pw, L.ptr(y, C.c_float)))
        elif kind == "bneck":
            pw += [None] * (6 - len(pw))
            L.check(L.lib().vc_bneck_fused_host(B, H, W, C.byref(v), L.ptr(x, C.c_float), *pw, L.ptr(y, C.c_float), L.ptr(z, C.c_float)))
        else:
            L.check(L.lib().vc_reid_block_fused_host(B, H, W, C.byref(v), L.ptr(x, C.c_float), *pw, L.ptr(y, C.c_float)))
    except L.VcError as err:
        err.outputs = (x, y, z)
        raise
    return x, y, z


def _front_call(inp, net, view, y):
    """shared by stem / front_fused: (b, net_h, net_w, x, frames, h, w, vc_front_view, copy of y)"""
    a = np.asarray(inp)
    if a.dtype == np.uint8:
        frames, x = np.ascontiguousarray(a), None
        b, h, w = frames.shape[:3]
        net_h, net_w = net
    else:
        frames, x = None, L.f32(a)
        b, net_h, net_w = x.shape[:3]
        h = w = 0
        assert net is None or tuple(net) == (net_h, net_w)
    assert a.ndim == 4 and a.shape[3] == 3
    y = L.f32(y).copy()
    v = L.FrontView(out_cs=y.shape[3], inv_scale=1.0, mode=1)
    for k, val in view.items():
        if not hasattr(v, k):
            raise KeyError(k)
        setattr(v, k, float(val) if k == "inv_scale" else int(val))
    return b, net_h, net_w, x, frames, h, w, v, y


def stem(inp, w0, b0, y, *, view, net=None, q8=None):
    """One launch of the detector's stem on WHOLE buffers (vc_stem_host, bf16).  inp: the letterboxed tensor (b, net_h, net_w, 3) as floats, or
    uint8 frames (b, h, w, 3) with net = (net_h, net_w).  w0 (cout, 3, 6, 6), b0 (cout,).  y (b, net_h / 2, net_w / 2, out_cs) and q8 (the
    e4m3 view, uint8 (b, net_h / 2, net_w / 2, q_cs), or None) are uploaded, launched into and returned as copies (y, q8).  `view`: the other
    vc_front_view fields.  A refusal raises VcError with the arrays as the call left them in err.outputs."""
    b, net_h, net_w, x, frames, h, w, v, y = _front_call(inp, net, view, y)
    w0, b0 = L.f32(w0), L.f32(b0)
    assert w0.shape[1:] == (3, 6, 6) and b0.shape == (len(w0),) and y.shape[:3] == (b, net_h // 2, net_w // 2)
    if q8 is not None:
        q8 = np.ascontiguousarray(q8, dtype=np.uint8).copy()
        assert q8.shape[:3] == y.shape[:3]
        v.q_cs = q8.shape[3]
    try:
        L.check(L.lib().vc_stem_host(b, net_h, net_w, len(w0), C.byref(v), L.ptr(x, C.c_float), L.ptr(frames, C.c_uint8), h, w, L.ptr(w0, C.c_float),
                                     L.ptr(b0, C.c_float), L.ptr(y, C.c_float), L.ptr(q8, C.c_uint8)))
    except L.VcError as err:
        err.outputs = (y, q8)
        raise
    return y, q8


def front_fused(inp, w0, b0, w1, b1, y, *, view, net=None):
    """One launch of the detector's layers 0 + 1 on WHOLE buffers (vc_front_fused_host, bf16): inp and `view` as for stem, w0 (32, 3, 6, 6),
    w1 (cout1, 32, 3, 3); y (b, h1, w1, out_cs) is uploaded, launched into and returned as a copy."""
    b, net_h, net_w, x, frames, h, w, v, y = _front_call(inp, net, view, y)
    w0, b0, w1, b1 = L.f32(w0), L.f32(b0), L.f32(w1), L.f32(b1)
    assert w0.shape == (32, 3, 6, 6) and w1.shape[1:] == (32, 3, 3) and y.shape[:3] == (b, (net_h // 2 - 1) // 2 + 1, (net_w // 2 - 1) // 2 + 1)
    try:
        L.check(L.lib().vc_front_fused_host(b, net_h, net_w, len(w1), C.byref(v), L.ptr(x, C.c_float), L.ptr(frames, C.c_uint8), h, w, L.ptr(w0, C.c_float),
                                            L.ptr(b0, C.c_float), L.ptr(w1, C.c_float), L.ptr(b1, C.c_float), L.ptr(y, C.c_float)))
    except L.VcError as err:
        err.outputs = (y, None)
        raise
    return y


def kalman_initiate(xyah):
    z = L.f64(xyah).reshape(-1, 4)
    m, c = np.zeros((len(z), 8)), np.zeros((len(z), 8, 8))
    L.check(L.lib().vc_kalman_initiate_host(L.ptr(z, C.c_double), len(z), L.ptr(m, C.c_double), L.ptr(c, C.c_double)))
    return m, c


def kalman_predict(mean, cov):
    m, c = L.f64(mean).reshape(-1, 8).copy(), L.f64(cov).reshape(-1, 8, 8).copy()
    L.check(L.lib().vc_kalman_predict_host(L.ptr(m, C.c_double), L.ptr(c, C.c_double), len(m)))
    return m, c


def kalman_update(mean, cov, z):
    m, c, z = L.f64(mean).reshape(-1, 8).copy(), L.f64(cov).reshape(-1, 8, 8).copy(), L.f64(z).reshape(-1, 4)
    L.check(L.lib().vc_kalman_update_host(L.ptr(m, C.c_double), L.ptr(c, C.c_double), L.ptr(z, C.c_double), len(m)))
    return m, c


def kalman_gating(mean, cov, zs):
    m, c, z = L.f64(mean).reshape(8), L.f64(cov).reshape(8, 8), L.f64(zs).reshape(-1, 4)
    out = np.zeros(len(z))
    L.check(L.lib().vc_kalman_gating_host(L.ptr(m, C.c_double), L.ptr(c, C.c_double), L.ptr(z, C.c_double), len(z), L.ptr(out, C.c_double)))
    return out


def iou_matrix(track_tlwh, det_tlwh):
    a, b = L.f64(track_tlwh).reshape(-1, 4), L.f64(det_tlwh).reshape(-1, 4)
    out = np.zeros((len(a), len(b)))
    L.check(L.lib().vc_iou_cost_host(L.ptr(a, C.c_double), len(a), L.ptr(b, C.c_double), len(b), L.ptr(out, C.c_double)))
    return out


def cosine_cost(galleries, feats):
    """galleries: list of (s_i, 512) arrays -> (T, D) min cosine distance."""
    t, s_cap = len(galleries), max(len(g) for g in galleries)
    gal = np.zeros((t, s_cap, L.FEAT_DIM), np.float32)
    cnt = np.zeros(t, np.int32)
    for i, g in enumerate(galleries):
        gal[i, : len(g)] = g
        cnt[i] = len(g)
    f = L.f32(feats).reshape(-1, L.FEAT_DIM)
    out = np.zeros((t, len(f)))
    L.check(L.lib().vc_cosine_cost_host(L.ptr(gal, C.c_float), L.ptr(cnt, C.c_int), t, s_cap, L.ptr(f, C.c_float), len(f), L.ptr(out, C.c_double)))
    return out


def dsort_nms(tlwh, scores, max_overlap):
    b, s = L.f64(tlwh).reshape(-1, 4), L.f64(scores).reshape(-1)
    keep = np.zeros(max(len(s), 1), np.int32)
    n = C.c_int()
    L.check(L.lib().vc_dsort_nms_host(L.ptr(b, C.c_double), L.ptr(s, C.c_double), len(s), float(max_overlap), L.ptr(keep, C.c_int), C.byref(n)))
    return keep[: n.value].tolist()


def lap(cost):
    c = L.f64(cost)
    nr, nc = c.shape
    k = max(min(nr, nc), 1)
    r, q = np.zeros(k, np.int32), np.zeros(k, np.int32)
    n = C.c_int()
    L.check(L.lib().vc_lap_host(L.ptr(c, C.c_double), nr, nc, L.ptr(r, C.c_int), L.ptr(q, C.c_int), C.byref(n)))
    return r[: n.value].copy(), q[: n.value].copy()


def letterbox(rgb, net_h, net_w, precision="f32"):
    im = np.ascontiguousarray(rgb, dtype=np.uint8)
    out = np.zeros((net_h, net_w, 3), np.float32)
    L.check(L.lib().vc_letterbox_host(L.ptr(im, C.c_uint8), im.shape[0], im.shape[1], net_h, net_w,
                                      L.PREC_BF16 if precision == "bf16" else L.PREC_F32, L.ptr(out, C.c_float)))
    return out


def sppf_pool(buf, c, co, precision="bf16", form=1):
    """launch_sppf_pool on a whole concat buffer (B, H, W, cs): channels [co, co + c) pooled into [co + c, co + 4c).
    Returns (buffer after the launch, name of the kernel that ran, its slice width in 32-bit words)."""
    a = L.f32(buf).copy()
    B, H, W, cs = a.shape
    kern, ws = C.c_int(), C.c_int()
    L.check(L.lib().vc_sppf_pool_host(L.ptr(a, C.c_float), B, H, W, cs, co, c, L.PREC_ID[precision], form, C.byref(kern), C.byref(ws)))
    return a, L.SPPF_RAN[kern.value], ws.value


def upsample2x(src, dst, co, precision="bf16"):
    """upsample2x_kernel: src (B, H, W, c) into channels [co, co + c) of a copy of dst (B, 2H, 2W, cs)."""
    s, d = L.f32(src), L.f32(dst).copy()
    B, H, W, c = s.shape
    assert d.shape[:3] == (B, 2 * H, 2 * W)
    L.check(L.lib().vc_upsample2x_host(L.ptr(s, C.c_float), B, H, W, c, L.ptr(d, C.c_float), d.shape[3], co, L.PREC_ID[precision]))
    return d


def maxpool3s2(src, dst, co, precision="bf16"):
    """maxpool3s2_kernel (MaxPool2d(3, 2, 1)): src (B, H, W, c) into channels [co, co + c) of a copy of dst (B, Ho, Wo, cs)."""
    s, d = L.f32(src), L.f32(dst).copy()
    B, H, W, c = s.shape
    assert d.shape[:3] == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    L.check(L.lib().vc_maxpool3s2_host(L.ptr(s, C.c_float), B, H, W, c, L.ptr(d, C.c_float), d.shape[3], co, L.PREC_ID[precision]))
    return d


def avgpool_l2norm(x, precision="f32"):
    """avgpool_l2norm_kernel: (k, h, w, 512) -> (k, 512) float32."""
    a = L.f32(x)
    k, h, w, c = a.shape
    assert c == L.FEAT_DIM
    out = np.zeros((k, L.FEAT_DIM), np.float32)
    L.check(L.lib().vc_avgpool_l2norm_host(L.ptr(a, C.c_float), k, h, w, L.PREC_ID[precision], L.ptr(out, C.c_float)))
    return out


def nchw_to_nhwc_pad(x, precision="f32"):
    """nchw_to_nhwc_pad_kernel: (k, C, H, W) -> (k, H, W, cpad) with the ReID input buffer's cpad (4 in f32, 8 in bf16)."""
    a = L.f32(x)
    k, c, h, w = a.shape
    cpad = 4 if precision == "f32" else 8
    out = np.full((k, h, w, cpad), np.nan, np.float32)
    L.check(L.lib().vc_nchw_to_nhwc_pad_host(L.ptr(a, C.c_float), k, c, h, w, cpad, L.PREC_ID[precision], L.ptr(out, C.c_float)))
    return out


def bf16_to_fp8(src, c, src_co, inv_scale, dst, dst_co):
    """bf16_to_fp8_kernel: channels [src_co, src_co + c) of src (npix, src_cs) float -> e4m3fn bytes [dst_co, dst_co + c) of a copy of
    dst (npix, dst_cs) uint8."""
    s, d = L.f32(src), np.ascontiguousarray(dst, dtype=np.uint8).copy()
    assert s.ndim == 2 and d.ndim == 2 and len(s) == len(d)
    L.check(L.lib().vc_bf16_to_fp8_host(L.ptr(s, C.c_float), len(s), c, s.shape[1], src_co, float(inv_scale), L.ptr(d, C.c_uint8), d.shape[1], dst_co))
    return d


def reid_stem_pool(crops, w_oihw, bias):
    """reid_stem_pool_kernel (bf16): crops (k, 50, 50, 3), weights (64, 3, 3, 3), bias (64,) -> (k, 25, 25, 64)."""
    x, w, b = L.f32(crops), L.f32(w_oihw), L.f32(bias)
    assert x.shape[1:] == (50, 50, 3) and w.shape == (64, 3, 3, 3) and b.shape == (64,)
    out = np.zeros((len(x), 25, 25, 64), np.float32)
    L.check(L.lib().vc_reid_stem_pool_host(L.ptr(x, C.c_float), len(x), L.ptr(w, C.c_float), L.ptr(b, C.c_float), L.ptr(out, C.c_float)))
    return out


def yuv_desc(fmt="nv12", matrix="bt601", full_range=False, pitch_y=0, pitch_c=0, offset_c=0, offset_v=0, frame_stride=0):
    """vc_yuv_desc: layout of YUV frames in bytes (0 = tightly packed; include/vcount_hip.h).  fmt: "nv12" / "i420" (8-bit 4:2:0), or for
    ingest only "p016" (16-bit NV12 layout, significant bits at the top: P010 / P012 surfaces are passed as "p016"), "i010" (yuv420p10le),
    "i422", "i444"."""
    if fmt not in L.PIX_ID and fmt not in L.PIX_WIDE_ID:
        raise ValueError(f"unknown pixel format {fmt!r}: one of {sorted(L.PIX_ID) + sorted(L.PIX_WIDE_ID)}")
    if matrix not in L.YUV_MATRIX_ID:
        raise ValueError(f"unknown colour matrix {matrix!r}: one of {sorted(L.YUV_MATRIX_ID)}")
    return L.YuvDesc(L.PIX_ID[fmt] if fmt in L.PIX_ID else L.PIX_WIDE_ID[fmt], L.YUV_MATRIX_ID[matrix], 1 if full_range else 0, int(pitch_y), int(pitch_c),
                     int(offset_c), int(offset_v), int(frame_stride))


def yuv_format_rows(format_id, h, w):
    """What a pixel format id (PIX_ID / PIX_WIDE_ID) makes of an h x w frame: (luma row bytes, chroma row bytes, chroma rows, U and V
    share a plane, the size is one the format takes); None for an unknown id."""
    #        sample bytes, interleaved, chroma at half height, chroma at half width
    table = {0: (1, True, True, True), 1: (1, False, True, True), 16: (2, True, True, True), 17: (2, False, True, True),
             18: (1, False, False, True), 19: (1, False, False, False)}
    if format_id not in table:
        return None
    ss, semi, vsub, hsub = table[format_id]
    size_ok = h >= (2 if vsub else 1) and w >= (2 if hsub else 1) and not (vsub and h % 2) and not (hsub and w % 2)
    return w * ss, (w if semi or not hsub else w // 2) * ss, (h // 2 if vsub else h), semi, size_ok


def yuv_to_bgr(yuv, b, h, w, fmt="nv12", matrix="bt601", full_range=False, *, desc=None, **geometry):
    """yuv_to_bgr_kernel on a host array: `yuv` = uint8 bytes of b frames laid out as the descriptor says -> (b, h, w, 3) BGR.  For the
    16-bit formats ("p016": P010 / P012 / P016 surfaces, "i010") a uint16 array is taken as its bytes."""
    d = desc if desc is not None else yuv_desc(fmt, matrix, full_range, **geometry)
    yuv = np.asarray(yuv)
    if yuv.dtype == np.uint16 and d.format in (L.PIX_WIDE_ID["p016"], L.PIX_WIDE_ID["i010"]):
        yuv = np.ascontiguousarray(yuv).astype("<u2", copy=False).view(np.uint8)
    src = np.ascontiguousarray(yuv, dtype=np.uint8).reshape(-1)
    out = np.zeros((b, h, w, 3), np.uint8)
    rows = yuv_format_rows(d.format, h, w)
    if b >= 1 and rows is not None and rows[4]:      # the library refuses anything else; the length check needs a valid geometry
        need = yuv_batch_bytes(d, b, h, w)
        if need is not None and src.size < need:
            raise ValueError(f"yuv holds {src.size} bytes, the descriptor needs {need}")
    L.check(L.lib().vc_yuv_to_bgr_host(C.byref(d), L.ptr(src, C.c_uint8), b, h, w, L.ptr(out, C.c_uint8)))
    return out


def frame_src(kind, ptr, desc=None):
    """vc_frame_src: ONE frame of a batch for `Engine.stream_stage_frames` / `frames_to_bgr`.  kind: "bgr_host", "bgr_dev", "yuv_host"
    or "yuv_dev"; ptr: integer address of the frame; desc (`yuv_desc(...)`, YUV kinds; None: tight NV12, BT.601 limited): the layout of
    that one frame (frame_stride is not used).  BGR frames are tight h * w * 3 bytes."""
    if kind not in L.RENDER_SRC_ID:
        raise ValueError(f"unknown frame source kind {kind!r}: one of {sorted(L.RENDER_SRC_ID)}")
    return L.FrameSrc(L.RENDER_SRC_ID[kind], ptr, desc if desc is not None else yuv_desc())


def _frame_array(frames):
    return (L.FrameSrc * max(len(frames), 1))(*frames)


def frames_layout(frames, h, w):
    """vc_frames_layout_host: validates a frame list like `Engine.stream_stage_frames` does (no GPU needed) and returns (raw_off, raw_bytes):
    the byte offset of every "yuv_host" frame in the staging call's raw buffer (-1 for the other kinds) and the buffer's size."""
    off, total = np.full(max(len(frames), 1), -2, np.int64), C.c_size_t(0)
    L.check(L.lib().vc_frames_layout_host(_frame_array(frames), len(frames), h, w, L.ptr(off, C.c_int64), C.byref(total)))
    return off[:len(frames)], total.value


def frames_to_bgr(frames, h, w, out=None):
    """frames_to_bgr_kernel on host arrays: `frames` = `frame_src("bgr_host" | "yuv_host", address, desc)` each -> (b, h, w, 3) BGR.  A frame
    whose host address is a multiple of 16 (and whose geometry is) takes the kernel's 16-byte path, any other the generic one.  `out`: a
    C-contiguous uint8 array of b * h * w * 3 elements to write into instead of a new one."""
    b = len(frames)
    if out is None:
        out = np.zeros((max(b, 0), h, w, 3), np.uint8)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= b * h * w * 3
    dst = C.cast(out.ctypes.data, C.POINTER(C.c_uint8))
    L.check(L.lib().vc_frames_to_bgr_host(_frame_array(frames), b, h, w, dst))
    return out


def _dims_array(dims):
    return (L.FrameDims * max(len(dims), 1))(*[L.FrameDims(int(h), int(w)) for h, w in dims])


def autoshape_net_size(h, w, img_size=640):
    """vc_autoshape_net_size: the (net_h, net_w) AutoShape gives ONE h x w image at `img_size` -- frames of a sized batch must agree on it."""
    nh, nw = C.c_int(), C.c_int()
    L.check(L.lib().vc_autoshape_net_size(int(h), int(w), int(img_size), C.byref(nh), C.byref(nw)))
    return nh.value, nw.value


def frames_layout_sized(frames, dims, img_size=640):
    """vc_frames_layout_sized_host: validates a sized frame list like `Engine.stream_stage_frames_sized` does (no GPU needed) and returns
    (raw_off, raw_bytes, cell, (net_h, net_w))."""
    b = len(frames)
    off, total, cell, nh, nw = np.full(max(b, 1), -2, np.int64), C.c_size_t(0), C.c_size_t(0), C.c_int(), C.c_int()
    L.check(L.lib().vc_frames_layout_sized_host(_frame_array(frames), _dims_array(dims), b, int(img_size), L.ptr(off, C.c_int64), C.byref(total),
                                                C.byref(cell), C.byref(nh), C.byref(nw)))
    return off[:b], total.value, cell.value, (nh.value, nw.value)


def frames_to_bgr_sized(frames, dims, cells):
    """The sized ingest kernel on host arrays: `cells` (uint8, b * cell bytes, C-contiguous) is converted into IN PLACE -- frame f tight at
    f * cell, every other byte as the caller left it."""
    assert cells.dtype == np.uint8 and cells.flags["C_CONTIGUOUS"]
    L.check(L.lib().vc_frames_to_bgr_sized_host(_frame_array(frames), _dims_array(dims), len(frames), C.cast(cells.ctypes.data, C.POINTER(C.c_uint8))))
    return cells


def letterbox_frames(frames, net_h, net_w, swap_rb=False, precision="f32"):
    """letterbox_frames_kernel on host arrays: ONE launch for frames (h_f, w_f, 3) uint8 of different sizes -> (b, net_h, net_w, 3) float32."""
    ims = [np.ascontiguousarray(im, dtype=np.uint8) for im in frames]
    ptrs = (C.c_void_p * len(ims))(*[im.ctypes.data for im in ims])
    out = np.zeros((len(ims), net_h, net_w, 3), np.float32)
    L.check(L.lib().vc_letterbox_frames_host(ptrs, _dims_array([im.shape[:2] for im in ims]), len(ims), net_h, net_w, 1 if swap_rb else 0,
                                             L.PREC_BF16 if precision == "bf16" else L.PREC_F32, L.ptr(out, C.c_float)))
    return out


def letterbox_dev(frames_dev_ptr, b, h, w, net_h, net_w, out_dev_ptr, *, swap_rb=True, precision="bf16", table_dev_ptr=None, mode=0):
    """The letterbox kernels on the caller's device buffers (integer addresses), enqueued on the null stream; returns without waiting.
    mode 0: the kernels a uniform batch runs; 1: build the per-frame table in table_dev_ptr (b * 64 bytes) and run letterbox_frames_kernel;
    2: that kernel with the table as mode 1 left it (the kernel alone, for measurement)."""
    L.check(L.lib().vc_letterbox_dev(C.c_void_p(frames_dev_ptr), b, h, w, net_h, net_w, 1 if swap_rb else 0, L.PREC_BF16 if precision == "bf16" else L.PREC_F32,
                                     C.c_void_p(out_dev_ptr), C.c_void_p(table_dev_ptr) if table_dev_ptr else None, mode))


def crop_resize_frames(frames, frame_of_box, boxes_cxcywh):
    """The ReID crop kernel with the per-frame table on host arrays: box i is cut from frames[frame_of_box[i]] (BGR uint8, own size) ->
    (k, 50, 50, 3) float32, the network input `Engine.embed_input` shows for that frame alone."""
    ims = [np.ascontiguousarray(im, dtype=np.uint8) for im in frames]
    ptrs = (C.c_void_p * len(ims))(*[im.ctypes.data for im in ims])
    fob = np.ascontiguousarray(frame_of_box, dtype=np.int32).reshape(-1)
    boxes = L.f64(boxes_cxcywh).reshape(-1, 4)
    assert len(fob) == len(boxes)
    out = np.zeros((len(boxes), 50, 50, 3), np.float32)
    L.check(L.lib().vc_crop_resize_frames_host(ptrs, _dims_array([im.shape[:2] for im in ims]), len(ims), L.ptr(fob, C.c_int), L.ptr(boxes, C.c_double),
                                               len(boxes), L.ptr(out, C.c_float)))
    return out


def frames_to_bgr_dev(frames, b, h, w, bgr_dev_ptr, table_dev_ptr):
    """frames_to_bgr_kernel on the caller's device buffers (integer addresses), enqueued on the null stream; returns without waiting.
    frames: `frame_src("bgr_dev" | "yuv_dev", ...)` each; table_dev_ptr: b * FRAME_ENTRY_BYTES bytes of device memory that receive the
    frame table.  frames=None launches the table of the last call again (the kernel alone, for measurement)."""
    L.check(L.lib().vc_frames_to_bgr_dev(_frame_array(frames) if frames is not None else None, b, h, w, C.c_void_p(bgr_dev_ptr), C.c_void_p(table_dev_ptr)))


def yuv_to_bgr_dev(yuv_dev_ptr, b, h, w, bgr_dev_ptr, desc=None):
    """The conversion on the caller's device buffers (integer addresses), enqueued on the null stream; returns without waiting."""
    d = desc if desc is not None else yuv_desc()
    L.check(L.lib().vc_yuv_to_bgr_dev(C.byref(d), C.c_void_p(yuv_dev_ptr), b, h, w, C.c_void_p(bgr_dev_ptr)))


def yuv_batch_bytes(d, b, h, w):
    """Bytes that b frames of h x w occupy under descriptor d (the zeros resolved like the library does); None if a pitch is too small
    (or the format id is unknown)."""
    rows = yuv_format_rows(d.format, h, w)
    if rows is None:
        return None
    rowb, crow, hc, semi, _ = rows
    py, pc = d.pitch_y or rowb, d.pitch_c or crow
    if py < rowb or pc < crow:
        return None
    off_c = d.offset_c or py * h
    end = off_c + pc * (hc - 1) + crow
    if not semi:
        off_v = d.offset_v or off_c + pc * hc
        end = max(end, off_v + pc * (hc - 1) + crow)
    return (b - 1) * (d.frame_stride or end) + end


def bgr_to_yuv(bgr, fmt="nv12", matrix="bt601", full_range=False, *, desc=None, **geometry):
    """bgr_to_yuv_kernel on a host array: (b, h, w, 3) uint8 BGR -> flat uint8 bytes of b frames laid out as the descriptor says
    (`yuv_batch_bytes` of them).  Bytes that belong to no plane come back as the zero fill.  Egress writes "nv12" / "i420" only."""
    if desc is None and fmt in L.PIX_WIDE_ID:
        raise ValueError(f"pixel format {fmt!r} is ingest only: egress writes one of {sorted(L.PIX_ID)}")
    d = desc if desc is not None else yuv_desc(fmt, matrix, full_range, **geometry)
    src = np.ascontiguousarray(bgr, dtype=np.uint8)
    if src.ndim != 4 or src.shape[3] != 3:
        raise ValueError(f"bgr must be (b, h, w, 3), got {src.shape}")
    b, h, w, _ = src.shape
    need = yuv_batch_bytes(d, b, h, w) if b >= 1 and h >= 2 and w >= 2 else None      # the library refuses what has no size
    out = np.zeros(need if need is not None else 16, np.uint8)
    L.check(L.lib().vc_bgr_to_yuv_host(C.byref(d), L.ptr(src.reshape(-1), C.c_uint8), b, h, w, L.ptr(out, C.c_uint8)))
    return out


def bgr_to_yuv_dev(bgr_dev_ptr, b, h, w, yuv_dev_ptr, desc=None):
    """The conversion on the caller's device buffers (integer addresses), enqueued on the null stream; returns without waiting."""
    d = desc if desc is not None else yuv_desc()
    L.check(L.lib().vc_bgr_to_yuv_dev(C.byref(d), C.c_void_p(bgr_dev_ptr), b, h, w, C.c_void_p(yuv_dev_ptr)))


class Renderer:
    """A render context of `engine` (vc_render): per batch  source -> overlay -> 4:2:0 YUV -> the caller's surface, asynchronous,
    `depth` batches in flight.  `submit` enqueues and returns; `collect` waits for the oldest batch.  Usable as a context manager."""

    def __init__(self, engine, max_batch=16, max_hw=(720, 1280), depth=2):
        self._h = C.c_void_p()
        self.engine, self.depth = engine, depth
        L.check(L.lib().vc_render_create(engine._h, max_batch, max_hw[0], max_hw[1], depth, C.byref(self._h)))
        engine._renderers = getattr(engine, "_renderers", [])
        engine._renderers.append(self)
        self._alive = []                                   # per outstanding batch: the arrays its addresses point into

    @staticmethod
    def _addr(x):
        return (x.ctypes.data, x) if isinstance(x, np.ndarray) else (int(x), None)

    def submit(self, src, b, h, w, out, *, kind="bgr_host", src_desc=None, prims=None, first=None, out_desc=None, out_is_dev=False):
        """src / out: integer addresses (torch `data_ptr()`) or C-contiguous uint8 arrays for host memory; kind: "bgr_host",
        "bgr_dev", "yuv_host" or "yuv_dev" (the YUV kinds with `src_desc`); prims / first: the lists of `overlay.overlay`
        (None = no overlay; copied by the call); out_desc: layout of `out` (None: tight NV12, BT.601 limited).  Source and
        destination must stay valid until the batch has been collected."""
        sa, sk = self._addr(src)
        oa, ok = self._addr(out)
        rs = L.RenderSrc(L.RENDER_SRC_ID[kind], sa, src_desc if src_desc is not None else yuv_desc())
        od = out_desc if out_desc is not None else yuv_desc()
        p = f = None
        if prims is not None:
            p = np.ascontiguousarray(prims, dtype=np.int32).reshape(-1)
            f = np.ascontiguousarray(first, dtype=np.int32)
        L.check(L.lib().vc_render_submit(self._h, C.byref(rs), b, h, w, L.ptr(p, C.c_int), L.ptr(f, C.c_int), C.byref(od), C.c_void_p(oa),
                                         1 if out_is_dev else 0))
        self._alive.append((sk, ok))

    def submit_live(self, live, src, b, h, w, out, *, kind="bgr_host", src_desc=None, out_desc=None, out_is_dev=False):
        """`submit` with the overlay lists taken in device memory from `live` (a LiveCounter after enable_overlay): its oldest
        unconsumed batch, which must be this one (b, h, w).  No list crosses to the host; the list buffer is free again when
        `collect` has returned for this batch.  A BGR slot of the stream path given as `src` must not be restaged before that."""
        sa, sk = self._addr(src)
        oa, ok = self._addr(out)
        rs = L.RenderSrc(L.RENDER_SRC_ID[kind], sa, src_desc if src_desc is not None else yuv_desc())
        od = out_desc if out_desc is not None else yuv_desc()
        L.check(L.lib().vc_render_submit_live(self._h, live._h, C.byref(rs), b, h, w, C.byref(od), C.c_void_p(oa), 1 if out_is_dev else 0))
        self._alive.append((sk, ok))

    def collect(self):
        """Block until the oldest outstanding batch is complete in its destination."""
        try:
            L.check(L.lib().vc_render_collect(self._h))
        finally:                                           # the batch has left the context even where the call reports its overlay's overflow
            if self._alive:
                self._alive.pop(0)

    @property
    def outstanding(self):
        return len(self._alive)

    def close(self):
        if self._h:
            L.lib().vc_render_destroy(self._h)
            self._h = C.c_void_p()
            self._alive = []
            if self in getattr(self.engine, "_renderers", ()):
                self.engine._renderers.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nms(boxes, conf, cls, iou=0.45, max_det=300, max_cand=4096):
    b, c = L.f32(boxes).reshape(-1, 4), L.f32(conf).reshape(-1)
    k = np.ascontiguousarray(cls, dtype=np.int32).reshape(-1)
    out = np.zeros((max_det, 6), np.float32)
    n = C.c_int()
    L.check(L.lib().vc_nms_host(L.ptr(b, C.c_float), L.ptr(c, C.c_float), L.ptr(k, C.c_int), len(c), iou, max_det, max_cand,
                                L.ptr(out, C.c_float), C.byref(n)))
    return out[: n.value].copy()


def _geom_array(geoms, b):
    if geoms is None:
        return None
    g = np.ascontiguousarray(geoms, dtype=np.int32).reshape(-1, 4)
    assert len(g) == b, "one (net_h, net_w, src_h, src_w) per frame"
    return g


def nms_batch(boxes, conf, cls, counts, iou=0.45, max_det=300, max_cand=4096, geoms=None):
    """vc_nms_batch_host: rank_sort + nms_mask + nms_scan on a batch of explicit candidate lists.  boxes / conf / cls: one array per frame
    (candidate order = position) or padded [b][max_cand] arrays with `counts`; geoms: per frame (net_h, net_w, src_h, src_w) for
    scale_coords, a row of zeros or None = network pixels.  Returns ([b][max_det][6] rows, [b] counts)."""
    b = len(counts)
    bx, cf, cl = np.zeros((b, max_cand, 4), np.float32), np.zeros((b, max_cand), np.float32), np.zeros((b, max_cand), np.int32)
    for f, n in enumerate(counts):
        bx[f, :n], cf[f, :n], cl[f, :n] = np.reshape(boxes[f], (-1, 4))[:n], np.reshape(conf[f], -1)[:n], np.reshape(cls[f], -1)[:n]
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    g = _geom_array(geoms, b)
    out, n_out = np.zeros((b, max_det, 6), np.float32), np.zeros(b, np.int32)
    L.check(L.lib().vc_nms_batch_host(L.ptr(bx, C.c_float), L.ptr(cf, C.c_float), L.ptr(cl, C.c_int), L.ptr(cnt, C.c_int), b, iou, max_det, max_cand,
                                      L.ptr(g, C.c_int), L.ptr(out, C.c_float), L.ptr(n_out, C.c_int)))
    return out, n_out


def class_table(nc, classes):
    """label_of_class [nc] int32 for `vc_engine_set_class_map`: -1 = dropped.  `classes`: a list of class ids (list order gives labels
    0, 1, ...) or a dict {class: label}.  A class outside [0, nc), a class named twice, a label outside [0, nc) or an empty selection
    raises ValueError."""
    pairs = list(classes.items()) if isinstance(classes, dict) else [(c, l) for l, c in enumerate(classes)]
    t = np.full(int(nc), -1, np.int32)
    for c, l in pairs:
        if isinstance(c, bool) or isinstance(l, bool) or int(c) != c or int(l) != l:
            raise ValueError(f"class map: class {c!r} -> label {l!r}: ids must be integers")
        c, l = int(c), int(l)
        if not 0 <= c < nc:
            raise ValueError(f"class map: class {c} outside [0, {nc})")
        if not 0 <= l < nc:
            raise ValueError(f"class map: label {l} of class {c} outside [0, {nc})")
        if t[c] >= 0:
            raise ValueError(f"class map: class {c} named twice")
        t[c] = l
    if not len(pairs):
        raise ValueError("class map: no class selected (None clears the map)")
    return t


def class_map_check(table):
    """vc_class_map_check_host: (n_labels, n_kept) of a label_of_class table, VcError(VC_ERR_ARG) for a bad one.  Pure host code."""
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
    nl, nk = C.c_int(), C.c_int()
    L.check(L.lib().vc_class_map_check_host(L.ptr(t, C.c_int), len(t), C.byref(nl), C.byref(nk)))
    return nl.value, nk.value


def class_filter_nms(boxes, conf, cls, counts, table, iou=0.45, max_det=300, max_cand=4096, geoms=None):
    """vc_class_filter_nms_host: `nms_batch` with cand_class_filter_kernel in front and det_relabel_kernel behind, `table` = label_of_class.
    Returns ([b][max_det][6] rows with labels in the class column, [b] counts, [b] kept candidates, [b][max_cand] their positions)."""
    b = len(counts)
    bx, cf, cl = np.zeros((b, max_cand, 4), np.float32), np.zeros((b, max_cand), np.float32), np.zeros((b, max_cand), np.int32)
    for f, n in enumerate(counts):
        bx[f, :n], cf[f, :n], cl[f, :n] = np.reshape(boxes[f], (-1, 4))[:n], np.reshape(conf[f], -1)[:n], np.reshape(cls[f], -1)[:n]
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
    g = _geom_array(geoms, b)
    out, n_out = np.zeros((b, max_det, 6), np.float32), np.zeros(b, np.int32)
    kept, kept_idx = np.zeros(b, np.int32), np.zeros((b, max_cand), np.int32)
    L.check(L.lib().vc_class_filter_nms_host(L.ptr(bx, C.c_float), L.ptr(cf, C.c_float), L.ptr(cl, C.c_int), L.ptr(cnt, C.c_int), b, L.ptr(t, C.c_int), len(t),
                                             iou, max_det, max_cand, L.ptr(g, C.c_int), L.ptr(out, C.c_float), L.ptr(n_out, C.c_int), L.ptr(kept, C.c_int),
                                             L.ptr(kept_idx, C.c_int)))
    return out, n_out, kept, kept_idx


def decode(logits, nc, strides, anchors, conf=0.25, max_cand=4096, mode="f32", nms=None):
    """vc_decode_host: the Detect decode + candidate filter on explicit logits.  logits: three float32 arrays [b][ny][nx][round_up(3 * (nc + 5), 8)];
    mode "f32" / "bf16" (decode_kernel) or "sparse" (head_compact_kernel + decode_sparse_kernel).  Returns a dict: cand_count, overflow ([b]),
    box / conf / cls / idx ([b][max_cand], the first min(cand_count, max_cand) rows of a frame valid, in arbitrary order), in sparse mode
    hc_lists (three arrays of gathered pixel indices); with nms = dict(iou=, max_det=, geoms=) the NMS runs on the same device buffers and
    det ([b][max_det][6]) / det_count ([b], -1 = the frame's overflow flag) are added."""
    lg = [L.f32(x) for x in logits]
    b = lg[0].shape[0]
    lcs = (3 * (nc + 5) + 7) // 8 * 8
    d = L.DecodeDesc(b=b, nc=nc, mode=L.DECODE_MODE_ID[mode], conf=conf, max_cand=max_cand)
    for i, x in enumerate(lg):
        assert x.ndim == 4 and x.shape[0] == b and x.shape[3] == lcs, (x.shape, lcs)
        d.ny[i], d.nx[i], d.stride[i] = x.shape[1], x.shape[2], float(strides[i])
    d.anchors[:] = [float(v) for v in np.reshape(anchors, -1)]
    lp = (C.POINTER(C.c_float) * 3)(*[L.ptr(x, C.c_float) for x in lg])
    r = {"cand_count": np.zeros(b, np.int32), "overflow": np.zeros(b, np.int32), "box": np.zeros((b, max_cand, 4), np.float32),
         "conf": np.zeros((b, max_cand), np.float32), "cls": np.zeros((b, max_cand), np.int32), "idx": np.zeros((b, max_cand), np.int32)}
    hc_count, lists, hl = None, None, None
    if mode == "sparse":
        hc_count = np.zeros(3, np.int32)
        lists = [np.zeros(x.shape[0] * x.shape[1] * x.shape[2], np.int32) for x in lg]
        hl = (C.POINTER(C.c_int) * 3)(*[L.ptr(x, C.c_int) for x in lists])
    iou, max_det, g, det, det_n = 0.0, 0, None, None, None
    if nms is not None:
        iou, max_det, g = nms.get("iou", 0.45), nms.get("max_det", 300), _geom_array(nms.get("geoms"), b)
        det, det_n = np.zeros((b, max_det, 6), np.float32), np.zeros(b, np.int32)
    L.check(L.lib().vc_decode_host(C.byref(d), lp, L.ptr(r["cand_count"], C.c_int), L.ptr(r["overflow"], C.c_int), L.ptr(r["box"], C.c_float),
                                   L.ptr(r["conf"], C.c_float), L.ptr(r["cls"], C.c_int), L.ptr(r["idx"], C.c_int), L.ptr(hc_count, C.c_int), hl,
                                   iou, max_det, L.ptr(g, C.c_int), L.ptr(det, C.c_float), L.ptr(det_n, C.c_int)))
    if mode == "sparse":
        r["hc_lists"] = [x[:n] for x, n in zip(lists, hc_count)]
    if nms is not None:
        r["det"], r["det_count"] = det, det_n
    return r
