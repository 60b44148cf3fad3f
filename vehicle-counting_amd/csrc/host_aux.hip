// The pool, resample, layout, cast, letterbox and crop kernels (aux_kernels.hip) on host arrays (include/vcount_hip.h).  Entry points only:
// each stages its arrays (host_stage.h), runs one launcher and reads the guarded result back.  None of them touches a vc_engine.
#include "engine.h"

using namespace vc;

namespace {

bool prec_known(int prec, bool fp8_too) { return prec == PREC_F32 || prec == PREC_BF16 || (fp8_too && prec == PREC_FP8); }

// a dense (b, h, w, c) tensor through `launch` into channels [co, co + c) of the caller's (b, ho, wo, cs) buffer
int resample(const float* src, int b, int h, int w, int c, float* dst, int ho, int wo, int cs, int co, int precision,
             int (*launch)(const View&, const View&, int, hipStream_t), const char* kernel) {
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    const size_t n = (size_t)b * ho * wo * cs;
    VC_TRY(upload_elems(mem, src, (size_t)b * h * w * c, precision, &ds));
    VC_TRY(guarded_elems(mem, dd, dst, n, precision));
    const View a{ds, b, h, w, c, c, 0, elem_size(precision)}, d{dd.out(), b, ho, wo, c, cs, co, elem_size(precision)};
    VC_TRY(launch(a, d, precision, nullptr));
    return read_elems(dd, n, precision, dst, kernel);
}

// ---- sized batches: the letterbox and crop kernels with their per-frame tables -------------------------------------------------------------
// frames of their own sizes uploaded into cells (include/vcount_hip.h) -> *cells_out (device, in mem); *cell_out: the cell size.
// Network shapes are not compared here (img_size 1 gives every frame 32 x 32).
int upload_cells(DevScratch& mem, const uint8_t* const* frames, const vc_frame_dims* dims, int b, uint8_t** cells_out, size_t* cell_out) {
    VC_CHECK(frames, VC_ERR_ARG, "null frame list");
    SizedDims sd;
    VC_TRY(sized_dims_resolve(dims, b, 1, sd));
    for (int f = 0; f < b; ++f) VC_CHECK(frames[f], VC_ERR_ARG, "frame %d: null data", f);
    const size_t cell = sd.cell;
    VC_TRY(mem.alloc(cells_out, (size_t)b * cell));
    VC_HIP(hipMemset(*cells_out, 0xA5, (size_t)b * cell));             // what a kernel that strays outside a frame would pick up
    for (int f = 0; f < b; ++f) VC_HIP(hipMemcpy(*cells_out + (size_t)f * cell, frames[f], (size_t)dims[f].h * dims[f].w * 3, hipMemcpyHostToDevice));
    *cell_out = cell;
    return VC_OK;
}

}  // namespace

extern "C" {

int vc_letterbox_host(const uint8_t* rgb, int h, int w, int net_h, int net_w, int precision, float* out) {
    VC_CHECK(rgb && out, VC_ERR_ARG, "null argument");
    DevScratch mem;
    GuardedOut dd;
    const LetterboxGeom g = letterbox_geom(h, w, net_h, net_w, false);
    void* ds = nullptr;
    const size_t px = (size_t)net_h * net_w;
    VC_TRY(mem.upload(&ds, rgb, (size_t)h * w * 3));
    VC_TRY(dd.alloc(mem, px * 4 * elem_size(precision)));
    VC_TRY(launch_letterbox((const uint8_t*)ds, dd.out(), 1, g, precision, nullptr));
    return read_rgb_of4(dd, px, precision, out, "letterbox");
}

int vc_sppf_pool_host(float* buf, int b, int h, int w, int cs, int co, int c, int precision, int form, int* ran_kernel, int* ran_ws) {
    VC_CHECK(buf && b >= 1 && h >= 1 && w >= 1 && c >= 1 && co >= 0 && cs >= co + 4 * c, VC_ERR_ARG, "sppf: bad shape");
    VC_CHECK(prec_known(precision, true) && (form == 0 || form == 1), VC_ERR_ARG, "sppf: bad precision or form");
    if (ran_kernel) *ran_kernel = 0;
    if (ran_ws) *ran_ws = 0;
    DevScratch mem;
    GuardedOut dd;
    const size_t n = (size_t)b * h * w * cs;
    VC_TRY(guarded_elems(mem, dd, buf, n, precision));
    const View cat{dd.out(), b, h, w, c, cs, co, elem_size(precision)};
    SppfRan ran{0, 0};
    VC_TRY(launch_sppf_pool(cat, c, precision, form, nullptr, &ran));
    VC_TRY(read_elems(dd, n, precision, buf, "the SPPF pool kernel"));
    if (ran_kernel) *ran_kernel = ran.kernel;
    if (ran_ws) *ran_ws = ran.ws;
    return VC_OK;
}

int vc_upsample2x_host(const float* src, int b, int h, int w, int c, float* dst, int cs, int co, int precision) {
    VC_CHECK(src && dst && b >= 1 && h >= 1 && w >= 1 && c >= 1 && co >= 0 && cs >= co + c, VC_ERR_ARG, "upsample: bad shape");
    VC_CHECK(prec_known(precision, true), VC_ERR_ARG, "upsample: bad precision");
    return resample(src, b, h, w, c, dst, 2 * h, 2 * w, cs, co, precision, launch_upsample2x, "upsample2x_kernel");
}

int vc_maxpool3s2_host(const float* src, int b, int h, int w, int c, float* dst, int cs, int co, int precision) {
    VC_CHECK(src && dst && b >= 1 && h >= 1 && w >= 1 && c >= 1 && co >= 0 && cs >= co + c, VC_ERR_ARG, "maxpool: bad shape");
    VC_CHECK(prec_known(precision, false), VC_ERR_ARG, "maxpool: precision must be VC_PREC_BF16 or VC_PREC_F32");
    return resample(src, b, h, w, c, dst, (h - 1) / 2 + 1, (w - 1) / 2 + 1, cs, co, precision, launch_maxpool3s2, "maxpool3s2_kernel");
}

int vc_avgpool_l2norm_host(const float* x, int k, int h, int w, int precision, float* out) {
    VC_CHECK(x && out && k >= 1 && h >= 1 && w >= 1, VC_ERR_ARG, "avgpool: bad shape");
    VC_CHECK(prec_known(precision, false), VC_ERR_ARG, "avgpool: precision must be VC_PREC_BF16 or VC_PREC_F32");
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    VC_TRY(upload_elems(mem, x, (size_t)k * h * w * VC_FEAT_DIM, precision, &ds));
    VC_TRY(dd.alloc(mem, (size_t)k * VC_FEAT_DIM * sizeof(float)));
    const View a{ds, k, h, w, VC_FEAT_DIM, VC_FEAT_DIM, 0, elem_size(precision)};
    VC_TRY(launch_avgpool_l2norm(a, dd.as<float>(), precision, nullptr));
    return dd.read_back(out, "avgpool_l2norm_kernel");
}

int vc_nchw_to_nhwc_pad_host(const float* x, int k, int c, int h, int w, int cpad, int precision, float* out) {
    VC_CHECK(x && out && k >= 1 && c >= 1 && h >= 1 && w >= 1, VC_ERR_ARG, "layout: bad shape");
    VC_CHECK(prec_known(precision, false), VC_ERR_ARG, "layout: precision must be VC_PREC_BF16 or VC_PREC_F32");
    VC_CHECK(cpad == reid_cpad(precision) && c <= cpad, VC_ERR_ARG, "layout: cpad must be %d at this precision", reid_cpad(precision));
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    const size_t n = (size_t)k * h * w * cpad;
    VC_TRY(upload_elems(mem, x, (size_t)k * c * h * w, PREC_F32, &ds));
    VC_TRY(dd.alloc(mem, n * elem_size(precision)));
    VC_TRY(launch_nchw_to_nhwc_pad((const float*)ds, k, c, h, w, dd.out(), cpad, precision, nullptr));
    return read_elems(dd, n, precision, out, "nchw_to_nhwc_pad_kernel");
}

int vc_bf16_to_fp8_host(const float* src, int npix, int c, int src_cs, int src_co, float inv_scale, uint8_t* dst, int dst_cs, int dst_co) {
    VC_CHECK(src && dst && npix >= 1 && c >= 1 && src_co >= 0 && src_cs >= src_co + c && dst_co >= 0 && dst_cs >= dst_co + c, VC_ERR_ARG, "bf16 -> fp8: bad shape");
    DevScratch mem;
    GuardedOut dd;
    void* ds = nullptr;
    VC_TRY(upload_elems(mem, src, (size_t)npix * src_cs, PREC_BF16, &ds));
    VC_TRY(dd.alloc(mem, (size_t)npix * dst_cs, dst));
    const View a{ds, 1, 1, npix, c, src_cs, src_co, 2}, d{dd.out(), 1, 1, npix, c, dst_cs, dst_co, 1};
    VC_TRY(launch_bf16_to_fp8(a, d, inv_scale, nullptr));
    return dd.read_back(dst, "bf16_to_fp8_kernel");
}

int vc_letterbox_frames_host(const uint8_t* const* frames, const vc_frame_dims* dims, int b, int net_h, int net_w, int swap_rb, int precision, float* out) {
    VC_CHECK(out, VC_ERR_ARG, "null argument");
    VC_CHECK(net_h >= 1 && net_w >= 4 && net_w % 4 == 0, VC_ERR_ARG, "network tensor %dx%d (the width must be a multiple of 4)", net_h, net_w);
    VC_CHECK(precision == VC_PREC_BF16 || precision == VC_PREC_F32, VC_ERR_ARG, "precision must be VC_PREC_BF16 or VC_PREC_F32");
    DevScratch mem;
    GuardedOut dd;
    uint8_t* dc = nullptr;
    LetterboxFrame* dt = nullptr;
    size_t cell = 0;
    VC_TRY(upload_cells(mem, frames, dims, b, &dc, &cell));
    const size_t px = (size_t)b * net_h * net_w;
    VC_TRY(dd.alloc(mem, px * 4 * elem_size(precision)));
    std::vector<LetterboxFrame> tab((size_t)b);
    for (int f = 0; f < b; ++f) tab[f] = letterbox_frame((long long)((size_t)f * cell), letterbox_geom(dims[f].h, dims[f].w, net_h, net_w, swap_rb != 0));
    VC_TRY(mem.upload(&dt, tab.data(), (size_t)b * sizeof(LetterboxFrame)));
    VC_TRY(launch_letterbox_frames(dc, dt, dd.out(), b, net_h, net_w, swap_rb ? 1 : 0, precision, nullptr));
    return read_rgb_of4(dd, px, precision, out, "letterbox_frames_kernel");
}

// The letterbox kernels on the caller's own device buffers (measurement; the counterpart of vc_frames_to_bgr_dev): frames_dev = b packed
// h x w x 3 u8 frames, out_dev = b x net_h x net_w x 4 elements of `precision`.  mode 0: launch_letterbox, the kernels a uniform batch
// runs.  mode 1: a table of b entries for these uniform frames is built and copied to table_dev (b * 64 bytes, a blocking copy), then
// letterbox_frames_kernel runs; mode 2: letterbox_frames_kernel with the table as the last mode-1 call left it.  NULL stream, no wait.
int vc_letterbox_dev(const void* frames_dev, int b, int h, int w, int net_h, int net_w, int swap_rb, int precision, void* out_dev, void* table_dev, int mode) {
    VC_CHECK(frames_dev && out_dev && (mode == 0 || table_dev), VC_ERR_ARG, "null argument");
    VC_CHECK(b >= 1 && h >= 1 && w >= 1 && net_h >= 1 && net_w >= 4 && net_w % 4 == 0 && mode >= 0 && mode <= 2, VC_ERR_ARG, "bad argument");
    VC_CHECK(precision == VC_PREC_BF16 || precision == VC_PREC_F32, VC_ERR_ARG, "precision must be VC_PREC_BF16 or VC_PREC_F32");
    static_assert(sizeof(LetterboxFrame) <= 64, "the caller reserves 64 bytes per table entry");
    const LetterboxGeom g = letterbox_geom(h, w, net_h, net_w, swap_rb != 0);
    if (mode == 0) return launch_letterbox((const uint8_t*)frames_dev, out_dev, b, g, precision, nullptr);
    if (mode == 1) {
        std::vector<LetterboxFrame> tab((size_t)b);
        for (int f = 0; f < b; ++f) tab[f] = letterbox_frame((long long)((size_t)f * h * w * 3), g);
        VC_HIP(hipMemcpy(table_dev, tab.data(), (size_t)b * sizeof(LetterboxFrame), hipMemcpyHostToDevice));
    }
    return launch_letterbox_frames((const uint8_t*)frames_dev, (const LetterboxFrame*)table_dev, out_dev, b, net_h, net_w, swap_rb ? 1 : 0, precision, nullptr);
}

int vc_crop_resize_frames_host(const uint8_t* const* bgr, const vc_frame_dims* dims, int b, const int* frame_of_box, const double* boxes, int k, float* out) {
    VC_CHECK(frame_of_box && boxes && out && k >= 1, VC_ERR_ARG, "bad argument");
    std::vector<int> crops;
    for (int i = 0; i < k; ++i) {
        const int f = frame_of_box[i];
        VC_CHECK(dims && f >= 0 && f < b, VC_ERR_ARG, "box %d: frame %d outside [0, %d)", i, f, b);
        const int empty = append_crops_cxcywh(f, dims[f].w, dims[f].h, boxes + (size_t)i * 4, 1, crops);   // the frame's own W - 1, H - 1
        VC_CHECK(empty < 0, VC_ERR_ARG, "box %d gives an empty crop (the reference's cv2.resize raises here)", i);
    }
    DevScratch mem;
    GuardedOut dd;
    uint8_t* dc = nullptr;
    CropFrame* dt = nullptr;
    int* dk = nullptr;
    size_t cell = 0;
    const size_t px = (size_t)k * VC_REID_SIZE * VC_REID_SIZE;
    VC_TRY(upload_cells(mem, bgr, dims, b, &dc, &cell));
    VC_TRY(dd.alloc(mem, px * 4 * sizeof(float)));
    std::vector<CropFrame> tab((size_t)b);
    for (int f = 0; f < b; ++f) tab[f] = CropFrame{(long long)((size_t)f * cell), dims[f].w, 0};
    VC_TRY(mem.upload(&dt, tab.data(), (size_t)b * sizeof(CropFrame)));
    VC_TRY(mem.upload(&dk, crops.data(), crops.size() * sizeof(int)));
    VC_TRY(launch_crop_resize(dc, 0, 0, dk, k, dd.out(), 4, VC_PREC_F32, nullptr, false, dt));
    return read_rgb_of4(dd, px, VC_PREC_F32, out, "crop_resize_kernel");
}

}  // extern "C"
