"""CountingPipeline: the per-video driver of /root/reference/modules/__init__.py:7-100 behind the same stage objects.

Video decode/encode (cv2.VideoCapture / VideoWriter, modules/datasets.py) is out of scope: frames come from a
`FrameSource` over an in-memory BGR array (or any iterable of such batches) that honours the reference's input contract
-- RGB frame for the detector, BGR original for the tracker, 1-based frame ids (modules/datasets.py:47-76).

Drivers with identical results:
  run()                the reference's loop, one frame at a time through ImageDetect.run / VideoTracker.run (host frames);
  run_pipelined()      the same loop over the same loader (any iterable of the reference's batch dicts, batch_size 1 included), but the
                       stage calls are asynchronous: the detector of batch n+1 runs behind the ReID net and the tracker of batch n;
  run_stream()         frames resident in HBM, B frames per `vc_stream_run` call (detect batched, trackers stepped in order);
  run_frame_sharded()  ONE stream on several GPUs: detect + ReID shard by frame chunk over the ranks, the
                       per-detection payloads are gathered in frame order, rank 0 runs the sequential tracker.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np

from .counting import count_directions, csv_records
from .detect import ImageDetect
from .track import VideoCounting, VideoTracker


class FrameSource:
    """In-memory video: (T, H, W, 3) uint8 BGR, like cv2.VideoCapture.read() delivers frames."""

    def __init__(self, frames_bgr, name="cam_04.mp4", fps=10):
        self.frames = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        t, h, w, _ = self.frames.shape
        self.video_info = {"name": name, "width": w, "height": h, "fps": fps, "num_frames": t}

    def __len__(self):
        return len(self.frames)

    def __iter__(self):
        for i, f in enumerate(self.frames):
            yield {"imgs": [f[:, :, ::-1]], "ori_imgs": [f], "frames": [i + 1]}       # BGR->RGB view, 1-based id


def _yuv_geometry(h, w, fmt, matrix, full_range, pitch, pitch_c, offset_c, offset_v, frame_stride):
    """(vc_yuv_desc, bytes from one frame to the next) of a clip of YUV frames.  Unless given, the chroma pitch follows the luma pitch
    (`pitch` where a chroma row has the bytes of a luma row: nv12, p016, i444; `pitch // 2` for i420, i010, i422), the planes follow each
    other without a gap, and a frame ends with the last whole row of its last plane."""
    from .engine import yuv_batch_bytes, yuv_desc, yuv_format_rows
    h, w, pitch, pitch_c = int(h), int(w), int(pitch), int(pitch_c)
    d = yuv_desc(fmt, matrix, full_range)                   # the name first: an unknown one has no size rule
    rowb, crow, hc, semi, size_ok = yuv_format_rows(d.format, h, w)
    if not size_ok:
        if fmt in ("i422", "i444"):
            raise ValueError(f"{fmt} frames need {'an even width' if fmt == 'i422' else 'a height and width of at least 1'}, got {h}x{w}")
        raise ValueError(f"4:2:0 frames need an even height and width, got {h}x{w}")
    if pitch and not pitch_c:
        if crow != rowb and pitch % 2:
            raise ValueError(f"an odd luma pitch needs an explicit pitch_c for {fmt}")
        pitch_c = pitch if crow == rowb else pitch // 2
    d = yuv_desc(fmt, matrix, full_range, pitch, pitch_c, offset_c, offset_v, frame_stride)
    frame_bytes = yuv_batch_bytes(d, 1, h, w)
    if frame_bytes is None:
        raise ValueError(f"pitch {pitch} / {pitch_c} is below the row width of a {w}-wide {fmt} frame")
    pc = d.pitch_c or crow                                  # default stride: whole rows of the last plane (= the frame's bytes when tight)
    off_c = d.offset_c or (d.pitch_y or rowb) * h
    whole = off_c + pc * hc if semi else max(off_c + pc * hc, (d.offset_v or off_c + pc * hc) + pc * hc)
    stride = int(frame_stride) or whole
    if stride < frame_bytes:
        raise ValueError(f"frame_stride {stride} is below the frame's {frame_bytes} bytes")
    return d, stride


class YuvFrameSource:
    """In-memory video as a decoder delivers it: T frames of YUV, `data` = uint8 array whose first axis is the frame (or a flat buffer
    of T whole frames).  `fmt`: "nv12" or "i420" (8-bit 4:2:0); "p016" (the NV12 layout with 16-bit samples, significant bits at the top:
    P010 / P012 surfaces are passed as "p016") or "i010" (yuv420p10le), for which `data` may also be a uint16 array, taken as its bytes;
    "i422" (any height) or "i444" (any height and width), 8-bit planar.  Geometry in bytes, 0 = tightly packed (include/vcount_hip.h:
    vc_yuv_desc): `pitch` is the luma pitch; unless given, the chroma pitch follows it (`pitch` for nv12, p016 and i444, `pitch // 2`
    for i420, i010 and i422), the planes follow each other without a gap and a frame ends with the last whole row of its last plane.
    `CountingPipeline.run_stream` takes it, and so does `run_streams` (one per camera, mixed freely with BGR `FrameSource`s and with
    YUV sources of other formats and pitches); `render` reads it as well.  The conversion to BGR runs on the device."""

    def __init__(self, data, h, w, fmt="nv12", matrix="bt601", full_range=False, pitch=0, pitch_c=0, offset_c=0, offset_v=0,
                 frame_stride=0, name="cam_04.mp4", fps=10):
        h, w = int(h), int(w)
        self.desc, stride = _yuv_geometry(h, w, fmt, matrix, full_range, pitch, pitch_c, offset_c, offset_v, frame_stride)
        data = np.asarray(data)
        if data.dtype == np.uint16 and fmt in ("p016", "i010"):                # 16-bit samples: little-endian bytes, the frame axis kept
            data = np.ascontiguousarray(data).astype("<u2", copy=False)
            data = data.view(np.uint8).reshape(data.shape[:-1] + (-1,)) if data.ndim > 1 else data.view(np.uint8)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.ndim == 1:
            if data.size == 0 or data.size % stride:
                raise ValueError(f"{data.size} bytes are not a whole number of {stride}-byte frames")
            data = data.reshape(-1, stride)
        else:
            data = data.reshape(len(data), -1)
        if data.shape[1] != stride:
            raise ValueError(f"a {h}x{w} {fmt} frame of this geometry has {stride} bytes, got {data.shape[1]}")
        self.desc.frame_stride = stride
        self.data, self.h, self.w, self.fmt = data, h, w, fmt
        self.video_info = {"name": name, "width": w, "height": h, "fps": fps, "num_frames": len(data)}

    def __len__(self):
        return len(self.data)


class YuvFrameSink:
    """Where a rendered clip lands: `n_frames` 4:2:0 frames (`fmt` "nv12" or "i420") of the geometry YuvFrameSource describes, as an
    encoder takes them.  By default the sink owns host memory for the whole clip (pinned when a GPU is present, zero-filled, so the
    bytes that belong to no plane stay zero): `data` is the (n_frames, frame_stride) uint8 array, `frame(i)` one frame's bytes.  With
    `device_ptr` the clip is a caller's device surface of `nbytes` bytes instead; `data` is then None."""

    def __init__(self, h, w, fmt="nv12", matrix="bt601", full_range=False, pitch=0, pitch_c=0, offset_c=0, offset_v=0, frame_stride=0,
                 n_frames=1, device_ptr=None):
        h, w, n_frames = int(h), int(w), int(n_frames)
        if n_frames < 1:
            raise ValueError(f"a sink needs at least one frame, got {n_frames}")
        from ._lib import PIX_ID
        if fmt not in PIX_ID:
            raise ValueError(f"unknown egress pixel format {fmt!r}: a sink takes one of {sorted(PIX_ID)} (the wider formats are ingest only)")
        self.desc, stride = _yuv_geometry(h, w, fmt, matrix, full_range, pitch, pitch_c, offset_c, offset_v, frame_stride)
        self.desc.frame_stride = stride
        self.h, self.w, self.fmt, self.n_frames, self.frame_stride = h, w, fmt, n_frames, stride
        self.nbytes = n_frames * stride
        self.device_ptr = int(device_ptr) if device_ptr is not None else None
        self.data = self._keep = None
        if self.device_ptr is None:
            import torch
            self._keep = torch.zeros((n_frames, stride), dtype=torch.uint8)
            if torch.cuda.is_available():
                self._keep = self._keep.pin_memory()
            self.data = self._keep.numpy()

    @property
    def is_device(self):
        return self.device_ptr is not None

    def __len__(self):
        return self.n_frames

    def address(self, i=0):
        """Address of frame i (host or device)."""
        if not 0 <= i < self.n_frames:
            raise IndexError(i)
        return (self.device_ptr if self.is_device else self.data.ctypes.data) + i * self.frame_stride

    def frame(self, i):
        if self.is_device:
            raise ValueError("a device sink has no host data")
        return self.data[i]


class PipelineLive:
    """The live counter of a group of cameras, opened by `CountingPipeline.open_live` and handed to `run_stream` / `run_streams` as
    `live=`: the call attaches it to the trackers it creates (`engine.LiveCounter`), calls `on_counts(batch_index, counts)` after every
    collect -- counts int32 (n_cam, max_dir, n_labels) over the rows of batches 0..batch_index, the batches enqueued by then -- and
    detaches it before the trackers are given back; `counts()` then keeps returning the final tensor.  `direction_keys[c]` names the
    rows of camera c ('01', ...); rows past them are zero.
    resume (a blob of `checkpoint_end`, possibly of another engine, process or GPU): the counter and its trackers are restored from it
    right after the counter is attached, once; `frame_base[c]` is then the number of frames camera c had had, and the run numbers its
    rows from `frame_base[c] + 1`.  on_checkpoint(batch_index, blob, frames_done): called by a run with `checkpoint_every=k` with the
    checkpoint taken behind every k-th batch (`engine.LiveCounter.checkpoint_begin` / `checkpoint_end`; checkpoint_bytes = the largest
    blob, reserved once on the device and in pinned memory)."""

    def __init__(self, engine, cam_names, zone_paths, n_labels, on_counts=None, resume=None, on_checkpoint=None, checkpoint_bytes=256 << 20):
        from .counting import load_zone_anno
        self.engine, self.cam_names, self.n_labels, self.on_counts = engine, list(cam_names), n_labels, on_counts
        self.resume, self.on_checkpoint, self.checkpoint_bytes = resume, on_checkpoint, checkpoint_bytes
        self.frame_base = np.zeros(len(self.cam_names), np.int64)
        self._ckpt_batch = None
        zones = [load_zone_anno(z) for z in zone_paths]
        self.polygons = [np.asarray(p, np.float64).reshape(-1, 2) for p, _ in zones]
        self.direction_keys = [list(d.keys()) for _, d in zones]
        self.dir_lines = [np.asarray([d[k] for k in d], np.float64).reshape(-1, 4) for _, d in zones]
        self.counter, self.last, self.last_stats = None, None, (0, 0)

    def attach(self, tracker_ids, annotate=None):
        """annotate: None, or the keyword arguments of `LiveCounter.enable_overlay` (max_batch, max_rows_per_frame, depth) -- every
        batch then also leaves its overlay lists on the device for `Renderer.submit_live`."""
        from .engine import LiveCounter, checkpoint_frames_done
        if self.counter is not None:
            raise RuntimeError("the live counter is attached already")
        self.counter = LiveCounter(self.engine, tracker_ids, self.polygons, self.dir_lines)
        self.frame_base[:] = 0
        self._ckpt_batch = None
        try:
            if annotate is not None:
                self.counter.enable_overlay(self.direction_keys, **annotate)
            if self.on_checkpoint is not None:
                self.counter.enable_checkpoint(self.checkpoint_bytes)
            if self.resume is not None:
                self.counter.restore(self.resume)
                self.frame_base[:] = checkpoint_frames_done(self.resume)
                self.resume = None
        except BaseException:
            self.counter.close()
            self.counter = None
            raise

    def checkpoint_begin(self, batch_index):
        """Behind the run of batch `batch_index`: the device pack is enqueued, nothing waits.  A checkpoint whose batch has not been
        collected yet (checkpoint_every=1: batch n + 1 runs before batch n is collected) is handed out first -- one is in flight at a time."""
        self._hand_out()
        self.counter.checkpoint_begin()
        self._ckpt_batch = batch_index

    def checkpoint_end(self, collected):
        """Behind the collect of batch `collected`: once the rows of the checkpointed batch itself are in -- its tracker launch is over
        then, the pack behind it all but certainly too, and nothing waits -- the blob of the last `checkpoint_begin` goes to on_checkpoint."""
        if self._ckpt_batch is not None and collected >= self._ckpt_batch:
            self._hand_out()

    def _hand_out(self):
        from .engine import checkpoint_frames_done
        if self._ckpt_batch is None:
            return
        n, self._ckpt_batch = self._ckpt_batch, None
        blob = self.counter.checkpoint_end()
        self.on_checkpoint(n, blob, checkpoint_frames_done(blob))

    def counts(self):
        return self.counter.counts() if self.counter is not None else self.last

    def stats(self):
        return self.counter.stats() if self.counter is not None else self.last_stats

    def allgather(self):
        return self.counter.allgather()

    def counts_of(self, cam):
        """Camera `cam` (index or name) in the form `run_stream` returns its counts: {direction key: [per label]}."""
        c = self.cam_names.index(cam) if isinstance(cam, str) else cam
        t = self.counts()
        return {k: t[c, i].tolist() for i, k in enumerate(self.direction_keys[c])}

    def notify(self, batch_index):
        if self.on_counts is not None:
            self.on_counts(batch_index, self.counts())

    def detach(self):
        if self.counter is not None:
            try:
                self.last, self.last_stats = self.counter.counts(), self.counter.stats()
            finally:
                self.counter.close()
                self.counter = None

    close = detach


class CountingPipeline:
    def __init__(self, args, config, cam_config, engine=None, class_names=None, synthetic=False, classes=None):
        """classes: the detector's class filter and label map (`Engine.set_class_map`: a list of class ids, labelled 0.. in list order,
        or a dict {class: label}).  Every driver then runs one tracker per LABEL and counts per label; `class_names` becomes one name
        per label, that of the lowest class mapped to it."""
        # the ReID checkpoint of the reference's cam_configs.yaml (`checkpoint: .../ckpt.t7`, handed to every DeepSort at
        # modules/__init__.py:36) becomes the engine's ReID parameters -- one engine owns both networks
        ck = cam_config.get("checkpoint") if isinstance(cam_config, dict) else getattr(cam_config, "checkpoint", None)
        self.detector = ImageDetect(args, config, engine=engine, class_names=class_names, synthetic=synthetic, reid_checkpoint=ck)
        self.engine = self.detector.engine
        self.class_names = self.detector.class_names
        if classes is not None:
            self.engine.set_class_map(classes)
            table, n_labels = self.engine.class_map, self.engine.num_labels
            names = [f"label{l}" for l in range(n_labels)]                # a label no class maps to keeps a placeholder: it never occurs
            for c in range(len(table) - 1, -1, -1):
                if table[c] >= 0:
                    names[table[c]] = self.class_names[c]
            self.class_names = names
        self.saved_path = getattr(args, "output_path", None)
        self.cam_config = cam_config
        self.config = config

    def _stages(self, cam_name, video_info, zone_path):
        cam = self.cam_config["cam"][cam_name] if isinstance(self.cam_config, dict) else self.cam_config.cam[cam_name]
        tracker = VideoTracker(len(self.class_names), cam, video_info, engine=self.engine)
        counter = VideoCounting(class_names=self.class_names, zone_path=zone_path)
        return tracker, counter

    @contextlib.contextmanager
    def _video(self, *trackers):
        """One video's stage objects: whatever happens inside, the engine-side trackers are given back (the reference drops the video's
        VideoTracker, modules/__init__.py:32-36), and after an exception the submissions still in flight are abandoned so that the
        next video starts on an idle engine."""
        try:
            yield
        except BaseException:
            try:
                self.engine.stream_reset()
            except Exception:
                pass
            raise
        finally:
            for t in trackers:
                if t is not None:
                    t.close()

    def open_live(self, cam_names, zone_paths, on_counts=None, resume=None, on_checkpoint=None, checkpoint_bytes=256 << 20):
        """A live counter for these cameras (one tracker per camera and label, as every driver creates them): hand it to `run_stream`
        (one camera) or `run_streams` as `live=`.  Its counts after any batch are the counts the call would return for the video cut
        there; nothing of the stream is kept for them.
        resume=blob (a live checkpoint, DESIGN.md 5 "Live checkpoint"): the run restores the counter and its trackers from it right after
        attaching them and goes on where the checkpointed stream stood -- rows of camera c are numbered from frames_done[c] + 1, with the
        ids, boxes and counts the uninterrupted stream would give.  The (rows, counts) pair the run returns then covers ONLY the resumed
        part (its CSV columns direction / fpoint / fframe are computed over those rows alone); `live.counts()` is the WHOLE stream's
        counts.  on_checkpoint / checkpoint_bytes: see PipelineLive; used by a run with `checkpoint_every=k`."""
        return PipelineLive(self.engine, cam_names, zone_paths, len(self.class_names), on_counts, resume, on_checkpoint, checkpoint_bytes)

    @staticmethod
    def _checkpoint_every(live, checkpoint_every):
        """(after_run(n), after_collect(n)) of a run: begin behind the run of every k-th batch, end behind that batch's own collect; both
        no-ops without k"""
        if not checkpoint_every:
            return (lambda n: None), (lambda n: None)
        if live is None or live.on_checkpoint is None:
            raise ValueError("checkpoint_every= needs live= opened with on_checkpoint=")
        k = int(checkpoint_every)
        return (lambda n: live.checkpoint_begin(n) if (n + 1) % k == 0 else None), live.checkpoint_end

    @contextlib.contextmanager
    def _live(self, live, trackers, annotate=None):
        """Attach `live` (or nothing) to these VideoTrackers for the length of a run; detached -- with its final counts kept -- before
        `_video` gives the trackers back, which the engine refuses while a counter is attached."""
        if live is None:
            yield
            return
        live.attach(np.array([t.tracker_ids for t in trackers], np.int32), annotate=annotate)
        try:
            yield
        finally:
            live.detach()

    @contextlib.contextmanager
    def _annotator(self, live, sink, n_frames, batch, h, w, mixed_sizes=False, depth=2, rows_per_frame=64):
        """The render side of run_stream / run_streams(annotate=sink): a Renderer of `depth` batches, and paint(n_frames_done, src, b) that
        renders one tracked batch through `Renderer.submit_live` into the sink's next b frames.  before_run() is called in front of every
        run call and before an ingest slot is restaged: it collects until fewer than `depth` batches are in flight, so a list buffer is
        free for the run and the slot's last reader is done.  Yields (overlay arguments for PipelineLive.attach, before_run, paint,
        drain)."""
        if sink is None:
            yield None, (lambda: None), None, (lambda: None)
            return
        if live is None:
            raise ValueError("annotate= needs live=: the overlay lists are built beside the live counter")
        if mixed_sizes:
            raise ValueError("annotate= with mixed_sizes=True: overlay lists are built for uniform batches only")
        if (sink.h, sink.w) != (h, w) or len(sink) < n_frames:
            raise ValueError(f"the sink holds {len(sink)} frames of {sink.h}x{sink.w}, the stream has {n_frames} of {h}x{w}")
        from .engine import Renderer
        with Renderer(self.engine, max_batch=batch, max_hw=(h, w), depth=depth) as rnd:
            def before_run():
                while rnd.outstanding >= depth:
                    rnd.collect()

            def paint(f0, src, b):
                rnd.submit_live(live.counter, src, b, h, w, sink.address(f0), kind="bgr_dev", out_desc=sink.desc, out_is_dev=sink.is_device)

            def drain():                                    # while the counter is still attached: its lists are what the batches read
                while rnd.outstanding:
                    rnd.collect()

            yield dict(max_batch=batch, max_rows_per_frame=rows_per_frame, depth=depth), before_run, paint, drain

    def _finish(self, counter, obj, cam_name):
        out = os.path.join(self.saved_path, cam_name + ".csv") if self.saved_path else None
        td = counter.run(frames=obj["frames"], tracks=obj["tracks"], labels=obj["labels"], boxes=obj["boxes"], output_path=out)
        rows = csv_records(td)
        counts = count_directions(rows, list(counter.directions.keys()), len(self.class_names))
        return rows, counts

    def run(self, source, cam_name, zone_path):
        """modules/__init__.py:28-100 for one video."""
        tracker, counter = self._stages(cam_name, source.video_info, zone_path)
        obj = {"frames": [], "tracks": [], "labels": [], "boxes": []}
        with self._video(tracker):
            for batch in source:
                if batch is None:
                    continue
                preds = self.detector.run(batch)
                for i in range(len(batch["ori_imgs"])):
                    boxes, labels, scores = preds["boxes"][i], preds["labels"][i], preds["scores"][i]
                    if len(boxes) == 0:                         # :68-69 (Q1)
                        continue
                    res = tracker.run(batch["ori_imgs"][i], boxes, labels, scores)
                    for j in range(len(res["boxes"])):
                        obj["frames"].append(batch["frames"][i])
                        obj["tracks"].append(res["tracks"][j])
                        obj["labels"].append(res["labels"][j])
                        obj["boxes"].append(res["boxes"][j])
        return self._finish(counter, obj, cam_name)

    def run_pipelined(self, source, cam_name, zone_path):
        """modules/__init__.py:28-100 for one video with the per-frame body software-pipelined over the engine's streams.

        Same input as run(): an iterable of the reference's loader batches ({'imgs', 'ori_imgs', 'frames'}, modules/datasets.py:47-76;
        batch_size = 1 at :93), host frames.  Same results (rows in the same order, Q1 skip included): what changes is WHEN a batch's
        stage work is issued -- batch n+2 is copied to the device and batch n+1's detector pass is enqueued before batch n's detections are
        marshalled, embedded and tracked (`vc_stream_stage_host` / `vc_stream_submit` / `vc_stream_run_async` / `vc_stream_collect`), so
        the ~60 dependent launches of a batch-1 detector pass overlap with the ReID net and the tracker walk of the frame before instead
        of following them.  ImageDetect.run / VideoTracker.run stay blocking calls for callers that use the stage objects directly;
        this driver is the drop-in for CountingPipeline.run itself."""
        import collections
        tracker, counter = self._stages(cam_name, source.video_info, zone_path)
        obj = {"frames": [], "tracks": [], "labels": [], "boxes": []}
        it = (b for b in source if b is not None)
        staged = collections.deque()        # (frame ids, host array, device address, b, h, w): copied, detector not yet enqueued
        submitted = collections.deque()     # detector enqueued, not yet handed to ReID + tracker
        running = collections.deque()       # tracker enqueued, rows not yet collected

        def stage():
            batch = next(it, None)
            if batch is None:
                return
            arr = np.ascontiguousarray(np.stack([np.asarray(f) for f in batch["ori_imgs"]]), dtype=np.uint8)   # (b, h, w, 3) BGR as the loader delivers it
            b, h, w, _ = arr.shape
            ptr = self.engine.stream_stage_host(arr.ctypes.data, b, h, w)
            staged.append((np.asarray(batch["frames"], dtype=np.int64), arr, ptr, b, h, w))

        def submit():
            if staged:
                ids, arr, ptr, b, h, w = staged.popleft()
                self.engine.stream_submit(ptr, b, h, w)
                submitted.append((ids, arr, ptr, b, h, w))

        def collect():
            ids, _arr = running.popleft()
            rows, fidx = self.engine.stream_collect()[:2]
            obj["frames"].extend(ids[fidx].tolist())
            obj["tracks"].extend(rows[:, 4].tolist())
            obj["labels"].extend(rows[:, 5].tolist())
            obj["boxes"].extend(list(rows[:, :4].copy()))

        with self._video(tracker):
            stage(); stage()                                 # staging order = batch order (four host slots, round-robin)
            submit()
            while submitted:
                stage()                                      # copy batch n+2 under the detector of batch n+1
                submit()                                     # detect batch n+1 while batch n is embedded and tracked
                ids, arr, ptr, b, h, w = submitted.popleft()
                self.engine.stream_run_async(tracker.tracker_ids, ptr, b, h, w)
                running.append((ids, arr))
                if len(running) > 1:
                    collect()
            while running:
                collect()
        return self._finish(counter, obj, cam_name)

    def run_stream(self, source, cam_name, zone_path, batch=16, asynchronous=False, host_frames=False, live=None, annotate=None,
                   checkpoint_every=None):
        """asynchronous=True: the tracker kernel of batch n runs on the engine's tracker stream while batch n+1 is submitted and
        embedded (`stream_run_async` / `stream_collect`); rows are identical, they arrive one batch later.
        host_frames=True: the frames stay in (pinned) host memory, as the reference's loader delivers them, and cross PCIe batch by
        batch -- batch n+2 is staged (`stream_stage_host`) while the detector works on batch n+1, so a video of any length needs four
        batches of device memory; otherwise the whole clip is uploaded once.
        A `YuvFrameSource` takes the same modes: its frames (any of its formats) are converted to BGR on the device as they are staged
        (`stream_stage_yuv_host` from pinned YUV -- half the PCIe bytes of BGR for 8-bit 4:2:0, two thirds for i422, the same for p016 /
        i010 / i444 -- or `stream_stage_yuv_dev` from the uploaded clip).
        live (`open_live([cam_name], [zone_path])`): the running counts of this camera on the device, see PipelineLive.
        annotate (a `YuvFrameSink` of the stream's frame size, with `live`): the live annotated video in ONE pass -- every batch's
        overlay lists are built on the device behind its tracker launch (`overlay.LiveVisualizer` is the definition) and the batch is
        rendered into the sink's next frames through `Renderer.submit_live` while the following batches run, two batches in flight.
        Rows, counts and the CSV are what they are without it.
        checkpoint_every=k (with `live` opened with on_checkpoint=): behind the run of every k-th batch the counter and its trackers are
        packed on the device (`checkpoint_begin`, no wait); behind the collect of that batch's own rows the blob goes to on_checkpoint
        (`checkpoint_end`: the pack lies behind the batch's tracker launch, which is over by then).  The stream is unchanged."""
        import torch
        ck_run, ck_collect = self._checkpoint_every(live, checkpoint_every)
        tracker, counter = self._stages(cam_name, source.video_info, zone_path)
        obj = {"frames": [], "tracks": [], "labels": [], "boxes": []}
        yuv = isinstance(source, YuvFrameSource)
        if yuv:
            frames, t, h, w = source.data, len(source.data), source.h, source.w
        else:
            frames = source.frames
            t, h, w, _ = frames.shape
        starts = list(range(0, t, batch))
        size = lambda n: min(batch, t - starts[n])
        ptr = {}
        if yuv:                                             # every batch goes through an ingest slot: staged two ahead in both modes
            keep = torch.from_numpy(frames).pin_memory() if host_frames else torch.from_numpy(frames).to(f"cuda:{self.engine.cfg.device}")
            convert = self.engine.stream_stage_yuv_host if host_frames else self.engine.stream_stage_yuv_dev
            stage = lambda n: ptr.__setitem__(n, convert(keep[starts[n]:starts[n] + size(n)].data_ptr(), size(n), h, w, source.desc))
        elif host_frames:
            host = torch.from_numpy(frames).pin_memory()
            stage = lambda n: ptr.__setitem__(n, self.engine.stream_stage_host(host[starts[n]:starts[n] + size(n)].data_ptr(), size(n), h, w))
        else:
            dev = torch.from_numpy(frames).to(f"cuda:{self.engine.cfg.device}")      # tensor container only
            stage = lambda n: ptr.__setitem__(n, dev[starts[n]:starts[n] + size(n)].data_ptr())

        def record(f0, rows, fidx):
            obj["frames"].extend((f0 + 1 + fidx + (int(live.frame_base[0]) if live is not None else 0)).tolist())
            obj["tracks"].extend(rows[:, 4].tolist())
            obj["labels"].extend(rows[:, 5].tolist())
            obj["boxes"].extend(list(rows[:, :4].copy()))

        with self._video(tracker), self._annotator(live, annotate, t, batch, h, w) as (ov_args, before_run, paint, drain), \
                self._live(live, [tracker], annotate=ov_args):
            for n in range(min(2, len(starts))):            # staging order = batch order (the engine hands its four host slots out round-robin)
                stage(n)
            if starts:
                self.engine.stream_submit(ptr[0], size(0), h, w)
            for n, f0 in enumerate(starts):
                b = size(n)
                before_run()                                # annotate: a list buffer is free, and batch n - 2 no longer reads the slot staged next
                if n + 2 < len(starts):                     # copy batch n+2 (host frames) under the detector of batch n+1
                    stage(n + 2)
                if n + 1 < len(starts):                     # detect the next batch while this one is tracked
                    self.engine.stream_submit(ptr[n + 1], size(n + 1), h, w)
                if asynchronous:
                    self.engine.stream_run_async(tracker.tracker_ids, ptr[n], b, h, w)
                    ck_run(n)
                    if n > 0:
                        record(starts[n - 1], *self.engine.stream_collect()[:2])
                        ck_collect(n - 1)
                else:
                    record(f0, *self.engine.stream_run_packed(tracker.tracker_ids, ptr[n], b, h, w)[:2])
                    ck_run(n)
                    ck_collect(n)
                if paint is not None:                       # the batch's lists were built behind its tracker launch: rendered from the BGR frames it ran on
                    paint(f0, ptr[n], b)
                if live is not None and (n > 0 or not asynchronous):
                    live.notify(n)                          # batches 0..n are enqueued: their rows are in the counts
                ptr.pop(n - 1, None)
            if asynchronous and starts:
                record(starts[-1], *self.engine.stream_collect()[:2])
                ck_collect(len(starts) - 1)
                if live is not None:
                    live.notify(len(starts) - 1)
            drain()
        return self._finish(counter, obj, cam_name)

    def visualizer(self, rows, zone_path):
        """The MergedVisualizer of one video: the CSV rows that run* returned, read the way the reference reads its CSV back
        (counting/utils.py:299-331: direction as an integer), and the zone file.  The reference colours a track from an unseeded
        RNG (Q10); rows without a colour get `overlay.track_color`, a fixed function of (label, track id)."""
        from .counting import load_zone_anno
        from .overlay import MergedVisualizer, track_color
        polygon, directions = load_zone_anno(zone_path)
        fixed = []
        for r in rows:
            r = dict(r)
            r["direction"] = int(r["direction"])
            if not isinstance(r.get("color"), (tuple, list)) or len(r["color"]) != 3:
                r["color"] = track_color(r["label"], r["track_id"])
            fixed.append(r)
        return MergedVisualizer(fixed, directions, polygon, len(self.class_names))

    def render(self, source, rows, cam_name, zone_path, sink, batch=16, depth=2):
        """The annotated video, the reference's VideoWriter.write_full_to_video (modules/datasets.py:132-145 -> visualize_merged,
        counting/utils.py:299-331): a second pass over `source` (FrameSource or YuvFrameSource) that paints the overlay of the CSV
        `rows` on the device and leaves every frame in `sink` (YuvFrameSink) as 4:2:0 YUV -- no frame exists as BGR on the host when
        the source is YUV.  Frames go `batch` at a time through a Renderer: the primitive lists are built strictly in frame order
        (the visualiser is stateful), batch n + 1 is submitted before batch n is collected.  Frame ids are 1-based.  Returns the sink."""
        import torch

        from .engine import Renderer
        viz = self.visualizer(rows, zone_path)
        yuv = isinstance(source, YuvFrameSource)
        if yuv:
            frames, t, h, w = source.data, len(source.data), source.h, source.w
        else:
            frames = source.frames
            t, h, w, _ = frames.shape
        if (sink.h, sink.w) != (h, w) or len(sink) < t:
            raise ValueError(f"the sink holds {len(sink)} frames of {sink.h}x{sink.w}, the source has {t} of {h}x{w}")
        # the source stays where the sink is: host frames cross PCIe batch by batch, a device sink gets the clip uploaded once
        # (a decoder's surfaces in a real deployment)
        keep = torch.from_numpy(frames)
        keep = keep.to(f"cuda:{self.engine.cfg.device}") if sink.is_device else keep.pin_memory()
        kind = ("yuv" if yuv else "bgr") + ("_dev" if sink.is_device else "_host")
        with Renderer(self.engine, max_batch=batch, max_hw=(h, w), depth=depth) as rnd:
            for f0 in range(0, t, batch):
                b = min(batch, t - f0)
                prims, first = viz.batch_prims(list(range(f0 + 1, f0 + b + 1)), (h, w))
                if rnd.outstanding >= depth:
                    rnd.collect()
                rnd.submit(keep[f0:f0 + b].data_ptr(), b, h, w, sink.address(f0), kind=kind, src_desc=source.desc if yuv else None,
                           prims=prims, first=first, out_desc=sink.desc, out_is_dev=sink.is_device)
            while rnd.outstanding:
                rnd.collect()
        return sink

    def run_streams(self, sources, cam_names, zone_paths, batch=16, host_frames=False, mixed_sizes=False, live=None, annotate=None,
                    checkpoint_every=None):
        """S videos at once on ONE engine (the reference runs them one after another, each with a new VideoTracker,
        modules/__init__.py:28-36): the frames of the cameras are interleaved round-robin into batches of `batch` frames, the
        detector and the ReID net see one batch, every camera's frames are stepped on that camera's own trackers
        (`vc_stream_run_async_multi`).  Per-camera results are identical to S separate `run_stream` calls; per-camera latency is
        batch / S frames.  All sources must share one frame size.  Returns [(rows, counts)] in camera order.
        With BGR `FrameSource`s only and host_frames=False the interleaved clip is built on the host and uploaded once.  With any
        `YuvFrameSource`, or host_frames=True, every camera's clip stays where a deployment has it -- its own pinned host tensor
        (host_frames=True) or its own device tensor -- and each batch is gathered from the cameras' own addresses on the device
        (`stream_stage_frames`, staged two batches ahead as in `run_stream`): no interleaved copy of the clips exists, cameras may
        differ in format, colour matrix, range, pitch and length, and a video of any length needs four batches of device memory
        when its frames stay on the host.
        mixed_sizes=True: the cameras may also differ in frame size, as long as every camera's own AutoShape network shape
        (`engine.autoshape_net_size`) is the same -- at size 640, 1920x1080, 1280x720, 640x360 and 320x180 all run at 384x640.  Each
        batch is a sized batch (`stream_stage_frames_sized`): one detector pass, and every camera still gets the result of running
        alone.  Cameras whose network shapes differ are refused; run each group of equal shapes in a call of its own.
        live (`open_live(cam_names, zone_paths)`): the running counts of all cameras on the device, see PipelineLive.
        annotate (a `YuvFrameSink`, with `live`; not with mixed_sizes): as in `run_stream`, for all cameras into ONE sink in batch
        (interleaved) order; the call then returns (results, [(camera index, 1-based frame number) of every sink frame]).  Each sink
        frame is a self-contained surface: an encoder per camera takes its frames by `sink.address(i)`.
        checkpoint_every=k: as in `run_stream`, one blob for all cameras."""
        import torch
        ck_run, ck_collect = self._checkpoint_every(live, checkpoint_every)
        if annotate is not None and mixed_sizes:
            raise ValueError("annotate= with mixed_sizes=True: overlay lists are built for uniform batches only")
        S = len(sources)
        order = []                                                                       # (camera, frame) round-robin, exhausted cameras drop out
        for t in range(max(len(s) for s in sources)):
            order.extend((c, t) for c in range(S) if t < len(sources[c]))
        cams = np.array([c for c, _ in order], np.int32)
        fidx = np.array([t for _, t in order], np.int64)
        starts = list(range(0, len(order), batch))

        def span(n):
            f0 = starts[n]
            return f0, min(batch, len(order) - f0)

        # the three modes differ in how batch n is staged, submitted and run: stage(n), submit(n), run(n, tids, cams of the batch)
        if mixed_sizes or host_frames or any(isinstance(s, YuvFrameSource) for s in sources):
            stage, submit, run = self._frames_batches(sources, cam_names, host_frames, mixed_sizes, order, span)
        else:
            shapes = {s.frames.shape[1:] for s in sources}
            assert len(shapes) == 1, "run_streams: all cameras must deliver frames of one size"
            h, w, _ = next(iter(shapes))
            dev = torch.from_numpy(np.stack([sources[c].frames[t] for c, t in order])).to(f"cuda:{self.engine.cfg.device}")

            def batch_ptr(n):
                f0, b = span(n)
                return dev[f0:f0 + b].data_ptr(), b

            stage = lambda n: None                                                       # the whole clip is on the device already
            submit = lambda n: self.engine.stream_submit(*batch_ptr(n), h, w)

            def run(n, tids, bcams):                                                     # returns the batch's BGR frames on the device
                self.engine.stream_run_async_multi(tids, bcams, *batch_ptr(n), h, w)
                return batch_ptr(n)[0]
        stages = [self._stages(n, s.video_info, z) for n, s, z in zip(cam_names, sources, zone_paths)]
        tids = np.array([st[0].tracker_ids for st in stages], np.int32)                 # [S][num_classes]
        objs = [{"frames": [], "tracks": [], "labels": [], "boxes": []} for _ in range(S)]

        def record(f0, rows, fb):
            g = f0 + fb                                                                  # global position of each row's frame
            for c in range(S):
                sel = cams[g] == c
                o = objs[c]
                o["frames"].extend((fidx[g[sel]] + 1 + (int(live.frame_base[c]) if live is not None else 0)).tolist())
                o["tracks"].extend(rows[sel, 4].tolist())
                o["labels"].extend(rows[sel, 5].tolist())
                o["boxes"].extend(list(rows[sel, :4].copy()))

        s0 = sources[0]
        h0, w0 = (s0.h, s0.w) if isinstance(s0, YuvFrameSource) else s0.frames.shape[1:3]
        with self._video(*[st[0] for st in stages]), self._annotator(live, annotate, len(order), batch, h0, w0, mixed_sizes) as (ov_args, before_run, paint, drain), \
                self._live(live, [st[0] for st in stages], annotate=ov_args):
            for n in range(min(2, len(starts))):            # staging order = batch order (four slots, round-robin)
                stage(n)
            if starts:
                submit(0)
            for n in range(len(starts)):
                f0, b = span(n)
                before_run()                                # annotate: a list buffer is free, and batch n - 2 no longer reads the slot staged next
                if n + 2 < len(starts):                     # gather batch n+2 under the detector of batch n+1
                    stage(n + 2)
                if n + 1 < len(starts):
                    submit(n + 1)
                frames_dev = run(n, tids, cams[f0:f0 + b])
                ck_run(n)
                if paint is not None:                       # sink frame f0 + i = frame i of the batch: interleaved order
                    paint(f0, frames_dev, b)
                if n > 0:
                    record(starts[n - 1], *self.engine.stream_collect()[:2])
                    ck_collect(n - 1)
                    if live is not None:
                        live.notify(n)                      # batches 0..n are enqueued: their rows are in the counts
            if starts:
                record(starts[-1], *self.engine.stream_collect()[:2])
                ck_collect(len(starts) - 1)
                if live is not None:
                    live.notify(len(starts) - 1)
            drain()
        results = [self._finish(st[1], o, n) for st, o, n in zip(stages, objs, cam_names)]
        if annotate is not None:
            return results, [(int(c), int(t) + 1) for c, t in order]
        return results

    def _frames_batches(self, sources, cam_names, host_frames, mixed_sizes, order, span):
        """run_streams over per-camera clips: camera c frame t is read at base_c + t * stride_c with that camera's descriptor.  Returns
        (stage, submit, run) for the batches of `order` that `span` cuts out; they keep the clips alive."""
        import torch

        from .engine import frame_src
        yuv = [isinstance(s, YuvFrameSource) for s in sources]
        sizes = [(s.h, s.w) if y else tuple(s.frames.shape[1:3]) for s, y in zip(sources, yuv)]
        if mixed_sizes:
            from .engine import autoshape_net_size
            shapes = [autoshape_net_size(h, w, self.engine.cfg.img_size) for h, w in sizes]
            if len(set(shapes)) != 1:
                per_cam = ", ".join(f"{n}: {h}x{w} runs at {nh}x{nw}" for n, (h, w), (nh, nw) in zip(cam_names, sizes, shapes))
                raise ValueError(f"run_streams(mixed_sizes=True): the cameras' network shapes differ ({per_cam}); run each group of equal shapes in its own call")
        elif len(set(sizes)) != 1:
            raise ValueError(f"run_streams: all cameras must deliver frames of one size, got {sizes}")
        h, w = sizes[0]
        # each camera's clip where its decoder would leave it: one tensor per camera, never an interleaved copy
        clips = [torch.from_numpy(s.data if y else s.frames.reshape(len(s.frames), -1)) for s, y in zip(sources, yuv)]
        clips = [c.pin_memory() if host_frames else c.to(f"cuda:{self.engine.cfg.device}") for c in clips]
        stride = [c.shape[1] for c in clips]
        kind = [("yuv" if y else "bgr") + ("_host" if host_frames else "_dev") for y in yuv]
        desc = [s.desc if y else None for s, y in zip(sources, yuv)]
        ptr = {}

        def dims(n):
            f0, b = span(n)
            return [sizes[c] for c, _ in order[f0:f0 + b]]

        def stage(n):
            f0, b = span(n)
            srcs = [frame_src(kind[c], clips[c].data_ptr() + t * stride[c], desc[c]) for c, t in order[f0:f0 + b]]
            ptr[n] = self.engine.stream_stage_frames_sized(srcs, dims(n)) if mixed_sizes else self.engine.stream_stage_frames(srcs, h, w)

        def submit(n):
            if mixed_sizes:
                self.engine.stream_submit_sized(ptr[n], dims(n))
            else:
                self.engine.stream_submit(ptr[n], span(n)[1], h, w)

        def run(n, tids, bcams):                             # returns the batch's BGR slot
            p = ptr.pop(n)
            if mixed_sizes:
                self.engine.stream_run_async_multi_sized(tids, bcams, p, dims(n))
            else:
                self.engine.stream_run_async_multi(tids, bcams, p, span(n)[1], h, w)
            return p

        return stage, submit, run

    def run_frame_sharded(self, source, cam_name, zone_path, chunk=8, device=None):
        """ONE camera stream on several GPUs, on the product's own batched path: the stateless front end shards by
        frame chunk over the ranks (chunk j on rank j % world): every rank submits its chunk to the batched detector
        (`vc_stream_submit`) and takes the marshalled boxes + device-resident embeddings of the whole chunk back
        (`vc_stream_embed`: one detector pass and one ReID pass per chunk); one variable-length RCCL all-gather per round behind the
        C ABI (`vc_allgather_rows`: rows over PCIe-free xGMI, embeddings device to device) brings every round's rows to all ranks in
        frame order; rank 0 steps the sequential tracker on the gathered round with ONE tracker kernel launch
        (`vc_videotracker_run_features`) and runs the counting -- tracker state never shards below a camera.  The ordering contract
        is the reference's (modules/__init__.py:54-84): frames reach the tracker in ascending order, empty frames are skipped (Q1).
        Returns (rows, counts) on rank 0, (None, None) elsewhere."""
        import torch
        import torch.distributed as dist

        from . import parallel
        rank, world = parallel.ensure_comm(self.engine)
        frames = source.frames
        t, h, w, _ = frames.shape
        mine = parallel.shard_frames(t, rank, world, chunk)
        n_rounds = (len(range(0, t, chunk)) + world - 1) // world
        tracker, counter = self._stages(cam_name, source.video_info, zone_path) if rank == 0 else (None, None)
        obj = {"frames": [], "tracks": [], "labels": [], "boxes": []}
        devs = [torch.from_numpy(frames[a:b]).to(f"cuda:{self.engine.cfg.device}") for a, b in mine]     # only this rank's chunks
        with self._video(tracker):
            if mine:
                self.engine.stream_submit(devs[0].data_ptr(), len(devs[0]), h, w)
            for r in range(n_rounds):
                if r + 1 < len(mine):                                                # detector of the next chunk runs behind this round's ReID / gather
                    self.engine.stream_submit(devs[r + 1].data_ptr(), len(devs[r + 1]), h, w)
                if r < len(mine):
                    rows7, feat = self.engine.stream_embed(devs[r].data_ptr(), len(devs[r]), h, w)
                    rows7[:, 0] += mine[r][0] + 1                                     # 1-based global frame id (modules/datasets.py:61)
                else:
                    rows7, feat = np.zeros((0, 7)), 0
                all_rows, all_feat, _ = self.engine.allgather_rows(rows7, feat, world)   # rank-major = frame order within a round
                if rank != 0:
                    continue
                for fid, rows in self.engine.videotracker_run_features(tracker.tracker_ids, all_rows, all_feat, h, w):
                    obj["frames"].extend([fid] * len(rows))
                    obj["tracks"].extend(rows[:, 4].tolist())
                    obj["labels"].extend(rows[:, 5].tolist())
                    obj["boxes"].extend(list(rows[:, :4].copy()))
        if rank != 0:
            return None, None
        return self._finish(counter, obj, cam_name)
