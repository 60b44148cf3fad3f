// Fused stream path: the per-frame body of CountingPipeline.run (/root/reference/modules/__init__.py:54-84) for a
// batch of device-resident frames of one camera: detect (batched) -> marshal like networks/yolo.py:72-97 ->
// skip empty frames (quirk Q1) -> crops + ReID for every box of the batch in one launch -> per frame, in order,
// one batched tracker step over the classes that have boxes (modules/track.py:50-59).
// What is here is the queueing: submissions, staging slots, the three feature buffers, events and error reporting.  The hand-over itself
// (marshal, crop list, grouping by class, DeepSort.update's filter, the embed_kept_only compaction) is det_prep.h.
// (The detect tail on host arrays -- vc_nms_host, vc_decode_host and their kin -- is host_detect.hip.)
#include <chrono>
#include <cstdlib>
#include <thread>

#include "engine.h"

using namespace vc;

namespace {
// host-timeline instrumentation (VC_TIMING=1): where a vc_stream_run call spends its wall time
struct Tm {
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long calls = 0;
    std::chrono::steady_clock::time_point t;
    bool on = getenv("VC_TIMING") != nullptr;
    void start() { if (on) t = std::chrono::steady_clock::now(); }
    void lap(int i) {
        if (!on) return;
        auto n = std::chrono::steady_clock::now();
        acc[i] += std::chrono::duration<double, std::micro>(n - t).count();
        t = n;
    }
    void report() {
        if (!on || ++calls % 10) return;
        fprintf(stderr, "[vc timing, us per call] wait_det+reid_issue %.0f prepare %.0f enqueue %.0f - %.0f %.0f %.0f %.0f %.0f\n",
                acc[0] / 10, acc[1] / 10, acc[2] / 10, acc[3] / 10, acc[4] / 10, acc[5] / 10, acc[6] / 10, acc[7] / 10);
        for (double& a : acc) a = 0;                   // windowed: the last 10 calls
    }
} g_tm;
}  // namespace

namespace vc {

// an ingest slot holds max_batch frames of the configured maximum, also as the 16-byte-aligned cells of a sized batch
size_t ingest_slot_bytes(const vc_engine* e) { return (size_t)e->cfg.max_batch * ((size_t)e->cfg.max_frame_h * e->cfg.max_frame_w * 3 + 16); }

int ingest_take_slot(vc_engine* e, int b, int h, int w, int* slot_out) {
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "engine not finalized");
    VC_CHECK(b >= 1 && b <= e->cfg.max_batch && h >= 1 && w >= 1 && h <= e->cfg.max_frame_h && w <= e->cfg.max_frame_w, VC_ERR_CAPACITY,
             "batch of %d frames %dx%d exceeds max_batch / max_frame_h / max_frame_w", b, h, w);
    VC_HIP(hipSetDevice(e->cfg.device));
    const size_t slot_bytes = ingest_slot_bytes(e);
    if (!e->cstream) {
        VC_HIP(hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking));
        for (int i = 0; i < 4; ++i) {
            VC_TRY(dev_alloc(e, (void**)&e->d_ingest[i], slot_bytes));
            VC_HIP(hipEventCreateWithFlags(&e->ev_ingest[i], hipEventDisableTiming));
        }
    }
    // four slots: one batch staged ahead + <= 2 submissions + the batch whose rows are still to be collected
    const int slot = (int)(e->ingest_seq & 3);
    VC_CHECK(!e->ingest_staged[slot], VC_ERR_STATE, "four host batches are staged and none has been submitted: call vc_stream_submit");
    for (const auto& pd : e->pending)
        VC_CHECK(pd.frames != e->d_ingest[slot], VC_ERR_STATE, "the staging slot's previous batch is still waiting for vc_stream_run: at most four host batches may be alive");
    for (const auto& job : e->jobs)                      // its crops may still be being cut on the ReID stream
        VC_CHECK(job.frames != e->d_ingest[slot], VC_ERR_STATE, "the staging slot's previous batch has not been collected: at most four host batches may be alive");
    ++e->ingest_seq;
    e->ingest_dims[slot].clear();                        // a uniform batch until vc_stream_stage_frames_sized says otherwise
    *slot_out = slot;
    return VC_OK;
}

// the slot's work has been enqueued on the copy stream: vc_stream_submit of the returned address starts the detector behind it
int ingest_publish(vc_engine* e, int slot, void** frames_dev_out) {
    VC_HIP(hipEventRecord(e->ev_ingest[slot], e->cstream));
    e->ingest_staged[slot] = true;
    *frames_dev_out = e->d_ingest[slot];
    return VC_OK;
}

}  // namespace vc

extern "C" {

int vc_stream_inject(vc_engine* e, const float* det6, const int* count, int b, int n) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    if (!det6 || !count || b <= 0) { e->inject_b = 0; e->inject_det.clear(); e->inject_count.clear(); return VC_OK; }
    VC_CHECK(n <= e->cfg.max_det, VC_ERR_CAPACITY, "injected detections per frame exceed max_det");
    e->inject_det.assign(det6, det6 + (size_t)b * n * 6);
    e->inject_count.assign(count, count + b);
    e->inject_b = b; e->inject_n = n;
    return VC_OK;
}

// Enqueue the detector (letterbox .. NMS, results to pinned memory) for a batch on the detector stream and return
// immediately.  At most two submissions may be outstanding; vc_stream_run consumes them in order.
// dims == nullptr: a uniform batch of h x w frames.  Otherwise a sized batch whose dims have been validated (sized_dims_resolve): frame f
// at frames_dev + f * cell, every frame's own network shape nh x nw, h x w the largest frame.
static int submit_batch(vc_engine* e, const void* frames_dev, int b, int h, int w, const vc_frame_dims* dims, size_t cell, int nh, int nw) {
    VC_CHECK(e->finalized && e->cfg.with_detector, VC_ERR_STATE, "engine not finalized");
    VC_CHECK(e->pending.size() < 2, VC_ERR_STATE, "two submissions are already in flight: call vc_stream_run first");
    int staged = -1;                                     // the ingest slot frames_dev was staged into, if it was
    for (int i = 0; i < 4; ++i)
        if (e->d_ingest[i] && frames_dev == e->d_ingest[i] && e->ingest_staged[i]) staged = i;
    if (staged >= 0) {                                   // a staged batch is submitted as what it was staged as
        const std::vector<vc_frame_dims>& sd = e->ingest_dims[staged];
        VC_CHECK(dims || sd.empty(), VC_ERR_ARG, "the batch was staged by vc_stream_stage_frames_sized: submit it with vc_stream_submit_sized");
        VC_CHECK(!dims || ((int)sd.size() == b && memcmp(sd.data(), dims, (size_t)b * sizeof(vc_frame_dims)) == 0), VC_ERR_ARG,
                 "the frame sizes differ from those the batch was staged with");
    }
    VC_HIP(hipSetDevice(e->cfg.device));
    if (staged >= 0) {                                   // the detector starts behind the slot's copy
        VC_HIP(hipStreamWaitEvent(e->dstream, e->ev_ingest[staged], 0));
        e->ingest_staged[staged] = false;
    }
    const int slot = (int)(e->submit_seq++ & 1);
    const int md = e->cfg.max_det;
    if (dims) VC_TRY(run_detector_dev_sized(e, (const uint8_t*)frames_dev, b, dims, cell, nh, nw, /*swap_rb=*/true));
    else VC_TRY(run_detector_dev(e, (const uint8_t*)frames_dev, b, h, w, /*swap_rb=*/true));
    VC_HIP(hipMemcpyAsync(e->h_det2[slot], e->post.det, (size_t)b * md * 6 * sizeof(float), hipMemcpyDeviceToHost, e->dstream));
    VC_HIP(hipMemcpyAsync(e->h_det_count2[slot], e->post.det_count, b * sizeof(int), hipMemcpyDeviceToHost, e->dstream));
    VC_HIP(hipEventRecord(e->ev_det[slot], e->dstream));
    vc_engine::Pending pd{};
    pd.frames = frames_dev; pd.b = b; pd.h = h; pd.w = w; pd.slot = slot;
    if (dims) { pd.dims.assign(dims, dims + b); pd.cell = cell; }
    if (e->inject_b > 0) { pd.inj_det = e->inject_det; pd.inj_cnt = e->inject_count; pd.inj_b = e->inject_b; pd.inj_n = e->inject_n; }   // this batch's own rectangles
    e->pending.push_back(std::move(pd));
    return VC_OK;
}

int vc_stream_submit(vc_engine* e, const void* frames_dev, int b, int h, int w) {
    VC_CHECK(e && frames_dev, VC_ERR_ARG, "null argument");
    return submit_batch(e, frames_dev, b, h, w, nullptr, 0, 0, 0);
}

int vc_stream_submit_sized(vc_engine* e, const void* frames_dev, const vc_frame_dims* dims, int b) {
    VC_CHECK(e && frames_dev && dims, VC_ERR_ARG, "null argument");
    SizedDims sd;
    VC_TRY(sized_dims_resolve(dims, b, e->cfg.img_size, sd));
    VC_CHECK(b <= e->cfg.max_batch && sd.max_h <= e->cfg.max_frame_h && sd.max_w <= e->cfg.max_frame_w, VC_ERR_CAPACITY,
             "batch of %d frames up to %dx%d exceeds max_batch / max_frame_h / max_frame_w", b, sd.max_h, sd.max_w);
    return submit_batch(e, frames_dev, b, sd.max_h, sd.max_w, dims, sd.cell, sd.net_h, sd.net_w);
}

// Ingest from host memory (the reference decodes on the host and hands numpy frames over, modules/datasets.py:47-61):
// vc_stream_stage_host copies the batch into one of four device staging slots on the engine's copy stream and returns; a later
// vc_stream_submit of the returned address enqueues the detector behind the copy.  Staged ONE BATCH FURTHER AHEAD than it is submitted
// (stage i + 2, submit i + 1, run i, collect i - 1) the copy runs under the detector of the batch before it; vc_stream_submit_host
// (stage + submit in one call) leaves the copy in front of its own detector, overlapped only with the ReID of the batch before --
// 157 MB per 128 frames of 640 x 640 is 3 - 5 ms of PCIe in front of a 7 ms step.  *frames_dev_out receives the device address to pass to
// vc_stream_run / vc_stream_run_async for this batch.  `frames_host` should be pinned (hipHostMalloc / hipHostRegister / torch
// pin_memory) for the copy to overlap; it may be reused as soon as the call returns only if it is pinned AND the caller keeps
// it untouched until the batch's rows have been collected -- plain pageable memory is copied synchronously by the runtime.
int vc_stream_stage_host(vc_engine* e, const uint8_t* frames_host, int b, int h, int w, void** frames_dev_out) {
    VC_CHECK(e && frames_host && frames_dev_out, VC_ERR_ARG, "null argument");
    int slot = 0;
    VC_TRY(ingest_take_slot(e, b, h, w, &slot));
    VC_HIP(hipMemcpyAsync(e->d_ingest[slot], frames_host, (size_t)b * h * w * 3, hipMemcpyHostToDevice, e->cstream));
    return ingest_publish(e, slot, frames_dev_out);
}

int vc_stream_submit_host(vc_engine* e, const uint8_t* frames_host, int b, int h, int w, void** frames_dev_out) {
    VC_CHECK(e && e->pending.size() < 2, e ? VC_ERR_STATE : VC_ERR_ARG, "two submissions are already in flight: call vc_stream_run first");
    VC_TRY(vc_stream_stage_host(e, frames_host, b, h, w, frames_dev_out));
    return vc_stream_submit(e, *frames_dev_out, b, h, w);
}

}  // extern "C"

namespace {

// The crop of every box of the batch, in (frame, box) order (deep_sort.py:78-95), with the checks that refuse a batch: more boxes than
// max_crops, an empty crop.  Both count ALL boxes, whatever is embedded afterwards.  pd.row0[f] = first row of frame f in that list.
int all_crops(vc_engine* e, vc_engine::Pending& pd, std::vector<int>& crops) {
    const int b = pd.b;
    crops.clear();
    pd.row0.assign(b, 0);
    for (int f = 0; f < b; ++f) {
        const int k = (int)(crops.size() / 5), n = (int)pd.fd[f].conf.size();
        pd.row0[f] = k;
        VC_CHECK(k + n <= e->cfg.max_crops, VC_ERR_CAPACITY,
                 "the batch has more boxes than max_crops (%d): raise vc_engine_config.max_crops", e->cfg.max_crops);
        const int empty = append_crops_xyxy(f, pd.frame_dims(f).w, pd.frame_dims(f).h, pd.fd[f].xyxy.data(), n, crops);   // the frame's own size
        VC_CHECK(empty < 0, VC_ERR_ARG, "frame %d box %d gives an empty crop (the reference's cv2.resize raises here)", f, empty);
    }
    return VC_OK;
}

// Upload k crops and enqueue the ReID net for them on the ReID stream, into the batch's feature slot; ev_reid marks its end.
int enqueue_reid(vc_engine* e, vc_engine::Pending& pd, const int* crops, int k) {
    int* hc = e->h_crops2[pd.fslot];
    if (k > 0) {
        const CropFrame* ftab = nullptr;
        if (!pd.dims.empty()) {                              // a sized batch: the crop kernels reach frame f through its cell and its own pitch
            if (!e->h_crop_ftab[pd.fslot]) {
                VC_TRY(host_alloc(e, (void**)&e->h_crop_ftab[pd.fslot], (size_t)e->cfg.max_batch * sizeof(CropFrame)));
                VC_TRY(dev_alloc(e, (void**)&e->d_crop_ftab[pd.fslot], (size_t)e->cfg.max_batch * sizeof(CropFrame)));
            }
            CropFrame* hf = e->h_crop_ftab[pd.fslot];
            for (int f = 0; f < pd.b; ++f) hf[f] = CropFrame{(long long)((size_t)f * pd.cell), pd.dims[f].w, 0};
            VC_HIP(hipMemcpyAsync(e->d_crop_ftab[pd.fslot], hf, (size_t)pd.b * sizeof(CropFrame), hipMemcpyHostToDevice, e->rstream));
            ftab = e->d_crop_ftab[pd.fslot];
        }
        memcpy(hc, crops, (size_t)k * 5 * sizeof(int));
        VC_HIP(hipMemcpyAsync(e->d_crops2[pd.fslot], hc, (size_t)k * 5 * sizeof(int), hipMemcpyHostToDevice, e->rstream));
        VC_TRY(run_reid_on(e, (const uint8_t*)pd.frames, pd.h, pd.w, k, e->d_crops2[pd.fslot], e->d_feat2[pd.fslot], e->rstream, ftab));
    }
    VC_HIP(hipEventRecord(e->ev_reid[pd.fslot], e->rstream));
    e->crops_embedded += k;
    return VC_OK;
}

// Second pipeline stage of a submission whose detector has finished: marshal the detections like networks/yolo.py:72-97,
// cut the crops (deep_sort.py:89-95,119-129) and enqueue the ReID net on its own stream.
// The reference embeds every box and only then, inside DeepSort.update, drops the boxes with conf <= min_confidence and those its own
// NMS suppresses (deep_sort.py:31-37, per class): a dropped box never becomes a Detection, so its feature row is never read by the cost
// matrices, the galleries or the output (Q5).  That filter (prepare_dets) reads the boxes, the confidences and two tracker parameters,
// no tracker state -- so with the engine option embed_kept_only and a filter `flt` (the parameters every tracker of the stream agrees
// on) it runs HERE, per (frame, label), and only the kept boxes are cropped and embedded: they get consecutive feature rows in (frame,
// box) order, and the prepare_dets results, their feat_rows pointing at those rows, stay in pd.prep for enqueue_batch_tracking.
int issue_reid(vc_engine* e, vc_engine::Pending& pd, const vc_engine::EmbedFilter& flt) {
    const int md = e->cfg.max_det, b = pd.b;
    const float* h_det = e->h_det2[pd.slot];
    const int* h_cnt = e->h_det_count2[pd.slot];
    pd.fd.assign(b, FrameDets{});
    for (int f = 0; f < b; ++f) {
        VC_CHECK(h_cnt[f] >= 0 || pd.inj_b > 0, VC_ERR_CAPACITY, "frame %d: more than max_candidates (%d) boxes passed conf_thres; raise vc_engine_config.max_candidates", f,
                 e->cfg.max_candidates);
        if (pd.inj_b > 0) {
            const int fi = f % pd.inj_b;
            marshal(pd.inj_det.data() + (size_t)fi * pd.inj_n * 6, pd.inj_cnt[fi], pd.fd[f]);
        } else {
            marshal(h_det + (size_t)f * md * 6, h_cnt[f], pd.fd[f]);
        }
    }
    // every check comes before a feature / crop slot is taken: a refused batch leaves the three-buffer rotation untouched
    std::vector<int>& crops = e->crop_scratch;
    VC_TRY(all_crops(e, pd, crops));
    int k = (int)(crops.size() / 5);
    e->boxes_detected += k;
    pd.filtered = e->opt.embed_kept_only != 0 && flt.valid;
    pd.flt = flt;
    pd.prep.clear();
    if (pd.filtered) {
        // every label that occurs: num_classes is not known at look-ahead time, enqueue_batch_tracking skips the labels outside it
        pd.prep.resize(b);
        PrepScratch scratch;
        const auto one_filter = [&flt](int, double& min_confidence, double& nms_max_overlap) {
            min_confidence = flt.min_confidence; nms_max_overlap = flt.nms_max_overlap;
            return true;
        };
        for (int f = 0; f < b; ++f) prepare_frame(pd.fd[f], pd.row0[f], one_filter, scratch, pd.prep[f]);
        k = compact_kept(crops, pd.prep.data(), b);
    }
    pd.fslot = (int)(e->reid_seq++ % 3);
    VC_TRY(enqueue_reid(e, pd, crops.data(), k));
    pd.stage = 1;
    return VC_OK;
}

// A batch that was embedded under a filter its consumer does not share (other tracker parameters than the remembered ones, or
// vc_stream_embed, which hands out every box's features): embed it again, every box, into the same feature slot.  The ReID stream
// runs it behind the first pass; the wait keeps the first pass's crop upload from reading the pinned list while it is rewritten.
int reembed_unfiltered(vc_engine* e, vc_engine::Pending& pd) {
    VC_HIP(hipEventSynchronize(e->ev_reid[pd.fslot]));
    std::vector<int>& crops = e->crop_scratch;
    VC_TRY(all_crops(e, pd, crops));
    pd.filtered = false;
    pd.prep.clear();
    return enqueue_reid(e, pd, crops.data(), (int)(crops.size() / 5));
}

// A submission whose detections cannot be embedded (candidate overflow, more boxes than max_crops, an empty crop) is DROPPED: the
// error is reported once, by the call that CONSUMES that submission (vc_stream_run* / vc_stream_embed for its frames), and the stream
// continues with the next one (it used to stay at the front of the queue and fail every following call).
int issue_reid_or_drop(vc_engine* e, size_t idx) {
    const int st = issue_reid(e, e->pending[idx], e->stream_flt);
    if (st != VC_OK) e->pending.erase(e->pending.begin() + idx);
    return st;
}

// Look-ahead: if the detector of the next submission has finished, start its ReID now (it then overlaps the tracking in progress).
// Never fails on behalf of the look-ahead submission (a drop of batch n + 1 used to come back as the status of the
// run_async / collect call made for batch n -- whose rows were then lost and whose job stayed queued behind the caller's back).  A
// submission that cannot be embedded stays queued at stage 0 with `embed_refused` set; take_front runs the same checks again when the
// caller asks for THAT batch, reports the error there and drops it.  issue_reid checks everything before it takes a feature / crop
// slot, so the refused attempt leaves no state behind.
// The trackers of the look-ahead batch have not been handed in yet: it is embedded under the filter REMEMBERED from the most recent
// vc_stream_run_async* call (e->stream_flt); enqueue_batch_tracking checks that against the trackers the batch really gets.
void try_issue_next(vc_engine* e) {
    int next = -1;
    int embedded = 0;                                   // batches that own one of the three feature buffers
    for (size_t i = 0; i < e->pending.size(); ++i) {
        if (e->pending[i].stage == 0) { next = (int)i; break; }
        ++embedded;
    }
    if (next < 0 || e->pending[next].embed_refused) return;
    embedded += (int)e->jobs.size();
    if (embedded >= 3) return;
    if (hipEventQuery(e->ev_det[e->pending[next].slot]) != hipSuccess) return;
    if (issue_reid(e, e->pending[next], e->stream_flt) != VC_OK) e->pending[next].embed_refused = true;
}

}  // namespace

extern "C" {

// The tracker work of one batch whose ReID has been enqueued (pd.stage == 1): per frame, in class order, the detections
// VideoTracker.run would hand to that class's DeepSort.update (modules/track.py:50-59; frames without boxes are skipped,
// modules/__init__.py:68-69, Q1), prepared on the host (confidence filter + DeepSORT NMS do not depend on tracker state), then ONE
// kernel on the tracker stream that steps every tracker through the whole batch (track_kernels.hip).  No host round trip per frame.
// Multi-camera batches: frame f of the batch belongs to camera cam_of_frame[f] (nullptr: one camera) and is stepped on that camera's
// trackers, trackers[cam * num_classes + c]; the frames of one camera appear in the batch in stream order.  One engine (one weight
// copy, one detector launch per layer) then serves S cameras with B / S frames of latency each, and the tracker kernel walks
// S x num_classes trackers in parallel, B / S steps each (a new VideoTracker per video, /root/reference/modules/__init__.py:29-36).
static int enqueue_batch_tracking(vc_engine* e, vc_engine::Pending& pd, const int* all_trackers, int num_classes, const int* cam_of_frame, int n_cam,
                                  int stage, int cap_rows_per_frame, std::vector<int>& ndet) {
    const int b = pd.b;
    ndet.assign(b, 0);
    for (int f = 0; f < b; ++f) {
        const int cam = cam_of_frame ? cam_of_frame[f] : 0;
        VC_CHECK(cam >= 0 && cam < n_cam, VC_ERR_ARG, "frame %d: camera index %d outside [0, %d)", f, cam, n_cam);
    }
    if (pd.filtered) {
        // the remembered filter is never trusted: every tracker the batch uses must have the parameters it was embedded under
        bool same = true;
        for (int f = 0; f < b && same; ++f) {
            const int* trackers = all_trackers + (size_t)(cam_of_frame ? cam_of_frame[f] : 0) * num_classes;
            for (const auto& lp : pd.prep[f]) {
                if (lp.first < 0 || lp.first >= num_classes) continue;
                const int ts = tracker_slot(e->trackers, trackers[lp.first]);
                if (ts < 0) continue;                                                    // refused below, as before
                const vc_tracker_params& p = e->trackers[ts]->p;
                if (p.min_confidence != pd.flt.min_confidence || p.nms_max_overlap != pd.flt.nms_max_overlap) { same = false; break; }
            }
        }
        if (!same) VC_TRY(reembed_unfiltered(e, pd));
    }
    std::vector<std::vector<FrameClassDets>> frames(b);
    std::vector<int> cam_tracker(b);                                                  // one tracker of each frame's camera: its live counter counts the frame
    PrepScratch scratch;
    FramePrepared own;
    for (int f = 0; f < b; ++f) {
        const int* trackers = all_trackers + (size_t)(cam_of_frame ? cam_of_frame[f] : 0) * num_classes;
        cam_tracker[f] = tracker_slot(e->trackers, trackers[0]);
        ndet[f] = (int)pd.fd[f].conf.size();                                         // a frame without boxes gives no task: Q1
        // filtered: prepared before the crops were cut (issue_reid); else here, box i of the frame on feature row row0[f] + i
        if (!pd.filtered) prepare_for_trackers(e, trackers, num_classes, pd.fd[f], pd.row0[f], scratch, own);
        VC_TRY(frame_tasks(e, trackers, num_classes, pd.filtered ? pd.prep[f] : own, frames[f]));
    }
    g_tm.lap(1);
    VC_TRY(track_enqueue(e, stage, frames, e->d_feat2[pd.fslot], pd.w, pd.h, b * cap_rows_per_frame, e->ev_reid[pd.fslot], pd.dims.empty() ? nullptr : pd.dims.data(),
                         cam_tracker.data()));
    g_tm.lap(2);
    return VC_OK;
}

// Pop the oldest submission once its detector has finished and its ReID is enqueued.
static int take_front(vc_engine* e, const void* frames_dev, int b, int h, int w, vc_engine::Pending& out, const vc_frame_dims* dims = nullptr) {
    if (e->pending.empty()) VC_TRY(dims ? vc_stream_submit_sized(e, frames_dev, dims, b) : vc_stream_submit(e, frames_dev, b, h, w));
    {
        const vc_engine::Pending& fr = e->pending.front();
        if (dims) {                                          // a sized run: the front must be that sized batch, frame size by frame size
            VC_CHECK(fr.frames == frames_dev && fr.b == b, VC_ERR_STATE, "vc_stream_run must consume submissions in the order they were made");
            VC_CHECK((int)fr.dims.size() == b && memcmp(fr.dims.data(), dims, (size_t)b * sizeof(vc_frame_dims)) == 0, VC_ERR_ARG,
                     "the frame sizes differ from those the batch was submitted with");
        } else {
            VC_CHECK(fr.frames == frames_dev && fr.b == b && fr.h == h && fr.w == w, VC_ERR_STATE,
                     "vc_stream_run must consume submissions in the order they were made");
            VC_CHECK(fr.dims.empty(), VC_ERR_ARG, "the batch was submitted by vc_stream_submit_sized: run it with vc_stream_run_async_multi_sized");
        }
    }
    g_tm.start();
    if (e->pending.front().stage == 0) {
        VC_HIP(hipEventSynchronize(e->ev_det[e->pending.front().slot]));
        VC_TRY(issue_reid_or_drop(e, 0));
    }
    out = std::move(e->pending.front());
    e->pending.erase(e->pending.begin());
    g_tm.lap(0);
    return VC_OK;
}

}  // extern "C" (helpers above have internal linkage)

namespace vc {
// Blocking entry points that touch tracker state wait for every tracker batch in flight (their rows stay in pinned memory until
// vc_stream_collect picks them up).
int async_wait_all(vc_engine* e) { return track_idle(e); }
}  // namespace vc

extern "C" {

// Asynchronous form: the batch's tracker work is enqueued on the tracker stream (it starts on the GPU when the batch's ReID has
// finished) and the call returns; the caller goes on to submit / embed the following batches; rows are picked up in order with
// vc_stream_collect.  At most two batches may be outstanding.
int vc_stream_run_async(vc_engine* e, const int* trackers, int num_classes, const void* frames_dev, int b, int h, int w,
                        int cap_rows_per_frame) {
    return vc_stream_run_async_multi(e, trackers, 1, num_classes, nullptr, frames_dev, b, h, w, cap_rows_per_frame);
}

static int run_async_batch(vc_engine* e, const int* trackers, int n_cam, int num_classes, const int* cam_of_frame, const void* frames_dev, int b, int h,
                           int w, int cap_rows_per_frame, const vc_frame_dims* dims) {
    VC_CHECK(e && trackers && frames_dev && cap_rows_per_frame > 0 && n_cam >= 1 && (n_cam == 1 || cam_of_frame), VC_ERR_ARG, "bad argument");
    VC_CHECK(e->finalized && e->cfg.with_detector && e->cfg.with_reid, VC_ERR_STATE, "engine not finalized");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_CHECK(e->jobs.size() < 2, VC_ERR_STATE, "two asynchronous batches are already outstanding: call vc_stream_collect");
    if (!dims && !e->lives.empty()) VC_TRY(live_overlay_room(e, trackers, n_cam * num_classes));   // a uniform batch builds overlay lists: refused before anything is enqueued
    {
        // the filter of THIS call's trackers: take_front embeds under it when it issues the ReID itself (first batch of a stream), and
        // the look-ahead of the following batches remembers it; valid only if every tracker handed in agrees on both parameters
        vc_engine::EmbedFilter flt;
        for (int i = 0; i < n_cam * num_classes; ++i) {
            const int ts = tracker_slot(e->trackers, trackers[i]);
            if (ts < 0) { flt.valid = false; break; }
            const vc_tracker_params& p = e->trackers[ts]->p;
            if (i == 0) { flt.valid = true; flt.min_confidence = p.min_confidence; flt.nms_max_overlap = p.nms_max_overlap; }
            else if (p.min_confidence != flt.min_confidence || p.nms_max_overlap != flt.nms_max_overlap) { flt.valid = false; break; }
        }
        e->stream_flt = flt;
    }
    vc_engine::Pending pd;
    VC_TRY(take_front(e, frames_dev, b, h, w, pd, dims));
    vc_engine::AsyncJob job;
    job.stage = (int)(e->tstage_seq++ % 3); job.b = b; job.cap = cap_rows_per_frame; job.frames = frames_dev;
    VC_TRY(enqueue_batch_tracking(e, pd, trackers, num_classes, cam_of_frame, n_cam, job.stage, cap_rows_per_frame, job.ndet));
    e->jobs.push_back(std::move(job));
    g_tm.report();
    try_issue_next(e);
    return VC_OK;
}

int vc_stream_run_async_multi(vc_engine* e, const int* trackers, int n_cam, int num_classes, const int* cam_of_frame, const void* frames_dev, int b, int h,
                              int w, int cap_rows_per_frame) {
    return run_async_batch(e, trackers, n_cam, num_classes, cam_of_frame, frames_dev, b, h, w, cap_rows_per_frame, nullptr);
}

// The same for a sized batch.  A camera's track boxes are clamped to ITS frame (track_core.h: emit_rows), so within the batch all frames
// of one camera have one size; refused before the submission is consumed.
int vc_stream_run_async_multi_sized(vc_engine* e, const int* trackers, int n_cam, int num_classes, const int* cam_of_frame, const void* frames_dev,
                                    const vc_frame_dims* dims, int b, int cap_rows_per_frame) {
    VC_CHECK(e && dims && b >= 1 && n_cam >= 1 && (n_cam == 1 || cam_of_frame), VC_ERR_ARG, "bad argument");
    std::vector<int> first((size_t)n_cam, -1);
    for (int f = 0; f < b; ++f) {
        const int cam = cam_of_frame ? cam_of_frame[f] : 0;
        VC_CHECK(cam >= 0 && cam < n_cam, VC_ERR_ARG, "frame %d: camera index %d outside [0, %d)", f, cam, n_cam);
        if (first[cam] < 0) first[cam] = f;
        VC_CHECK(dims[f].h == dims[first[cam]].h && dims[f].w == dims[first[cam]].w, VC_ERR_ARG, "frame %d: camera %d delivers %dx%d here and %dx%d in frame %d", f, cam,
                 dims[f].h, dims[f].w, dims[first[cam]].h, dims[first[cam]].w, first[cam]);
    }
    SizedDims sd;                                            // for the largest frame: what the submission was filed under
    VC_TRY(sized_dims_resolve(dims, b, e->cfg.img_size, sd));
    return run_async_batch(e, trackers, n_cam, num_classes, cam_of_frame, frames_dev, b, sd.max_h, sd.max_w, cap_rows_per_frame, dims);
}

// Results of the oldest asynchronous batch (blocks until its tracker kernel has finished).  While waiting, the ReID of the
// next submission is started as soon as its detector has finished.
int vc_stream_collect(vc_engine* e, int64_t* out_rows6, int cap_rows_per_frame, int* out_m, int* out_ndet, int b) {
    VC_CHECK(e && out_rows6 && out_m, VC_ERR_ARG, "null argument");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_CHECK(!e->jobs.empty(), VC_ERR_STATE, "no asynchronous batch is outstanding");
    const vc_engine::AsyncJob& front = e->jobs.front();
    VC_CHECK(front.b == b && front.cap == cap_rows_per_frame, VC_ERR_ARG, "collect: batch of %d frames x %d rows expected", front.b, front.cap);
    while (hipEventQuery(e->tstage[front.stage].done) == hipErrorNotReady) {
        try_issue_next(e);
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    vc_engine::AsyncJob job = std::move(e->jobs.front());
    e->jobs.pop_front();
    VC_TRY(track_collect(e, job.stage, out_rows6, cap_rows_per_frame, out_m));
    if (out_ndet) memcpy(out_ndet, job.ndet.data(), (size_t)b * sizeof(int));
    try_issue_next(e);
    return VC_OK;
}

int vc_stream_run(vc_engine* e, const int* trackers, int num_classes, const void* frames_dev, int b, int h, int w,
                  int64_t* out_rows6, int cap_rows_per_frame, int* out_m, int* out_ndet) {
    VC_CHECK(e && trackers && frames_dev && out_rows6 && out_m, VC_ERR_ARG, "null argument");
    VC_CHECK(e->jobs.empty(), VC_ERR_STATE, "asynchronous batches are outstanding: vc_stream_collect them first");
    VC_TRY(vc_stream_run_async(e, trackers, num_classes, frames_dev, b, h, w, cap_rows_per_frame));
    return vc_stream_collect(e, out_rows6, cap_rows_per_frame, out_m, out_ndet, b);
}

// ---- one stream on several GPUs: the stateless front end shards by frame chunk over the ranks -----------------------
// Front half of the fused path for the OLDEST submission: wait for its detector, marshal the detections like networks/yolo.py:72-97,
// cut the crops and run the ReID net for EVERY box (deep_sort.py:119-129, Q5: no tracker is known here, so embed_kept_only does not
// apply and the remembered filter is forgotten), and hand back what VideoTracker.run works on: rows
// [frame index in the batch, x1, y1, x2, y2, conf, label] (float64; a frame without boxes contributes nothing, Q1) plus the device
// address of the matching [n][512] float32 embeddings.  The embeddings stay valid until the third following vc_stream_embed /
// vc_stream_run* call (three feature buffers rotate).
int vc_stream_embed(vc_engine* e, const void* frames_dev, int b, int h, int w, double* out_rows7, int cap_rows, int* out_n, const float** out_feat_dev) {
    VC_CHECK(e && frames_dev && out_rows7 && out_n && out_feat_dev, VC_ERR_ARG, "null argument");
    VC_CHECK(e->finalized && e->cfg.with_detector && e->cfg.with_reid, VC_ERR_STATE, "engine not finalized");
    VC_HIP(hipSetDevice(e->cfg.device));
    e->stream_flt = vc_engine::EmbedFilter{};             // this consumer wants every box's features: no filter from here on
    vc_engine::Pending pd;
    VC_TRY(take_front(e, frames_dev, b, h, w, pd));
    if (pd.filtered) VC_TRY(reembed_unfiltered(e, pd));   // the look-ahead of a vc_stream_run_async* call embedded it under that call's filter
    VC_HIP(hipEventSynchronize(e->ev_reid[pd.fslot]));
    int n = 0;
    for (int f = 0; f < b; ++f) n += (int)pd.fd[f].conf.size();
    VC_CHECK(n <= cap_rows, VC_ERR_CAPACITY, "vc_stream_embed: %d rows, room for %d", n, cap_rows);
    double* o = out_rows7;
    for (int f = 0; f < b; ++f) {
        const FrameDets& d = pd.fd[f];
        for (size_t i = 0; i < d.conf.size(); ++i, o += 7) {
            o[0] = (double)f; memcpy(o + 1, &d.xyxy[i * 4], 4 * sizeof(double)); o[5] = d.conf[i]; o[6] = (double)d.label[i];
        }
    }
    *out_n = n;
    *out_feat_dev = e->d_feat2[pd.fslot];
    return VC_OK;
}

// VideoTracker.run (modules/track.py:30-70) for a run of frames whose detections AND embeddings are supplied -- the tracker rank of the
// frame-sharded front end.  rows7 [n][7] = [frame key, x1, y1, x2, y2, conf, label] sorted by frame key (any ascending integer, e.g. the
// 1-based frame id); row i's embedding is feat_dev[i].  One launch of track_batch_kernel steps every (frame, class with boxes) in order.
// Output per distinct frame key, ascending: out_keys[j], out_m[j] rows [x1, y1, x2, y2, track id, label] at out_rows6[j * cap_rows_per_frame].
int vc_videotracker_run_features(vc_engine* e, const int* trackers, int num_classes, const double* rows7, const float* feat_dev, int n, int h, int w,
                                 int64_t* out_rows6, int cap_rows_per_frame, int* out_m, int64_t* out_keys, int cap_frames, int* out_n_frames) {
    VC_CHECK(e && trackers && out_rows6 && out_m && out_keys && out_n_frames && (n == 0 || (rows7 && feat_dev)) && n >= 0, VC_ERR_ARG, "bad argument");
    if (!e->lives.empty()) VC_TRY(live_overlay_room(e, trackers, num_classes));
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_TRY(async_wait_all(e));
    std::vector<std::vector<FrameClassDets>> frames;
    std::vector<int64_t> keys;
    PrepScratch scratch;
    FramePrepared prep;
    FrameDets d;
    for (int i0 = 0; i0 < n;) {
        const double key = rows7[(size_t)i0 * 7];
        VC_CHECK(keys.empty() || (int64_t)key > keys.back(), VC_ERR_ARG, "rows must be sorted by frame key");
        keys.push_back((int64_t)key);
        frames.emplace_back();
        d.xyxy.clear(); d.conf.clear(); d.label.clear();
        int i1 = i0;
        for (; i1 < n && rows7[(size_t)i1 * 7] == key; ++i1) {
            const double* r = rows7 + (size_t)i1 * 7;
            d.xyxy.insert(d.xyxy.end(), r + 1, r + 5); d.conf.push_back(r[5]); d.label.push_back((int)r[6]);
        }
        prepare_for_trackers(e, trackers, num_classes, d, i0, scratch, prep);        // modules/track.py:50-59; row i's embedding is feat_dev[i]
        VC_TRY(frame_tasks(e, trackers, num_classes, prep, frames.back()));
        i0 = i1;
    }
    const int nf = (int)frames.size();
    VC_CHECK(nf <= cap_frames, VC_ERR_CAPACITY, "%d frames, room for %d", nf, cap_frames);
    *out_n_frames = nf;
    for (int j = 0; j < nf; ++j) out_keys[j] = keys[j];
    if (nf == 0) return VC_OK;
    VC_TRY(track_enqueue(e, 3, frames, feat_dev, w, h, nf * cap_rows_per_frame, nullptr));
    return track_collect(e, 3, out_rows6, cap_rows_per_frame, out_m);
}

// Abandon everything in flight on the stream path: waits for the GPU, discards the rows of uncollected batches (their tracker steps
// HAVE run: reset the trackers as well if the clip is to be replayed) and empties the submission queue.  The way out of any error
// state of vc_stream_* without destroying the engine.
int vc_stream_reset(vc_engine* e) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_HIP(hipStreamSynchronize(e->dstream)); VC_HIP(hipStreamSynchronize(e->rstream)); VC_HIP(hipStreamSynchronize(e->stream));
    while (!e->jobs.empty()) {
        const vc_engine::AsyncJob job = std::move(e->jobs.front());
        e->jobs.pop_front();
        std::vector<int64_t> rows((size_t)job.b * job.cap * 6);
        std::vector<int> m(job.b);
        (void)track_collect(e, job.stage, rows.data(), job.cap, m.data());      // bookkeeping (pending_dets, known_tracks); errors are dropped with the rows
    }
    e->pending.clear();
    if (e->cstream) VC_HIP(hipStreamSynchronize(e->cstream));         // staged host batches are abandoned with the rest
    for (bool& st : e->ingest_staged) st = false;
    e->stream_flt = vc_engine::EmbedFilter{};
    e->boxes_detected = e->crops_embedded = 0;
    return VC_OK;
}

// Running totals since engine creation / the last vc_stream_reset, over the stream path and the blocking tracker entry points:
// boxes handed to the ReID stage, and crops the ReID net was really run on (fewer with embed_kept_only; a batch that had to be embedded
// a second time counts twice).
int vc_stream_crop_stats(vc_engine* e, int64_t* boxes_detected, int64_t* crops_embedded) {
    VC_CHECK(e && boxes_detected && crops_embedded, VC_ERR_ARG, "null argument");
    *boxes_detected = e->boxes_detected;
    *crops_embedded = e->crops_embedded;
    return VC_OK;
}

}  // extern "C"
