// The tracker's single-function kernels (track_kernels.hip: the batch kernel's own __device__ functions on caller-supplied state) on host
// arrays (include/vcount_hip.h): Kalman initiate / predict / update, the gate, the IoU and cosine cost matrices and the assignment solver.
// Entry points only, on the harness of host_stage.h: every output lies between guard blocks.  None of them touches a vc_engine.
#include <algorithm>
#include <numeric>

#include "engine.h"

using namespace vc;

namespace {

// a pool of n tracks whose mean / cov start as the caller's arrays (null: the guard fill), no gallery
int guarded_pool(DevScratch& mem, TrackPool& tp, GuardedOut& gm, GuardedOut& gc, int n, const double* mean8, const double* cov64) {
    VC_TRY(gm.alloc(mem, (size_t)n * 8 * sizeof(double), mean8));
    VC_TRY(gc.alloc(mem, (size_t)n * 64 * sizeof(double), cov64));
    tp.max_tracks = n; tp.budget_cap = 1;
    tp.mean = gm.as<double>(); tp.cov = gc.as<double>(); tp.gallery = nullptr;
    return VC_OK;
}

// which: 0 initiate (z -> mean, cov), 1 predict, 2 update (z)
int kalman_kat(double* mean8, double* cov64, const double* z4, int n, int which) {
    VC_CHECK(mean8 && cov64 && n > 0, VC_ERR_ARG, "bad argument");
    DevScratch mem;
    GuardedOut gm, gc;
    TrackPool tp{};
    double* dz = nullptr;
    VC_TRY(guarded_pool(mem, tp, gm, gc, n, which ? mean8 : nullptr, which ? cov64 : nullptr));
    if (z4) VC_TRY(mem.upload(&dz, z4, (size_t)n * 32));
    VC_TRY(launch_kat_kalman(tp, which, dz, n, nullptr));
    VC_TRY(kernel_wait("kat_kalman_kernel"));
    VC_TRY(gm.read_back(mean8, "kat_kalman_kernel (mean)"));
    return gc.read_back(cov64, "kat_kalman_kernel (cov)");
}

}  // namespace

extern "C" {

int vc_kalman_initiate_host(const double* xyah, int n, double* mean8, double* cov64) {
    VC_CHECK(xyah, VC_ERR_ARG, "null measurement");
    return kalman_kat(mean8, cov64, xyah, n, 0);
}
int vc_kalman_predict_host(double* mean8, double* cov64, int n) { return kalman_kat(mean8, cov64, nullptr, n, 1); }
int vc_kalman_update_host(double* mean8, double* cov64, const double* z4, int n) {
    VC_CHECK(z4, VC_ERR_ARG, "null measurement");
    return kalman_kat(mean8, cov64, z4, n, 2);
}

// squared Mahalanobis distances of ONE track against n_meas measurements (the gate's project4 / chol4 / maha4)
int vc_kalman_gating_host(const double* mean8, const double* cov64, const double* z4, int n_meas, double* out) {
    VC_CHECK(mean8 && cov64 && z4 && out && n_meas > 0, VC_ERR_ARG, "bad argument");
    DevScratch mem;
    GuardedOut gm, gc, gout;
    TrackPool tp{};
    double* dz = nullptr;
    VC_TRY(guarded_pool(mem, tp, gm, gc, 1, mean8, cov64));
    VC_TRY(mem.upload(&dz, z4, (size_t)n_meas * 32));
    VC_TRY(gout.alloc(mem, (size_t)n_meas * 8));
    VC_TRY(launch_gating_values(tp, 0, dz, n_meas, gout.as<double>(), nullptr));
    VC_TRY(kernel_wait("kat_gating_kernel"));
    return gout.read_back(out, "kat_gating_kernel");
}

int vc_iou_cost_host(const double* track_tlwh, int t, const double* det_tlwh, int d, double* out_iou) {
    VC_CHECK(track_tlwh && det_tlwh && out_iou && t > 0 && d > 0, VC_ERR_ARG, "bad argument");
    DevScratch mem;
    GuardedOut gout;
    double *da = nullptr, *db = nullptr;
    VC_TRY(mem.upload(&da, track_tlwh, (size_t)t * 32));
    VC_TRY(mem.upload(&db, det_tlwh, (size_t)d * 32));
    VC_TRY(gout.alloc(mem, (size_t)t * d * 8));
    VC_TRY(launch_iou_boxes(da, t, db, d, gout.as<double>(), nullptr));
    VC_TRY(kernel_wait("kat_iou_boxes_kernel"));
    return gout.read_back(out_iou, "kat_iou_boxes_kernel");
}

int vc_cosine_cost_host(const float* gallery, const int* gal_count, int t, int s_cap, const float* feat, int d, double* out) {
    VC_CHECK(gallery && gal_count && feat && out && t > 0 && d > 0 && s_cap > 0, VC_ERR_ARG, "bad argument");
    const size_t gal_bytes = (size_t)t * s_cap * VC_FEAT_DIM * 4;
    // a wide-open gate: identity covariance scaled up, measurement = mean
    std::vector<double> mean((size_t)t * 8, 0.0), cov((size_t)t * 64, 0.0), z((size_t)d * 4, 0.0);
    for (int i = 0; i < t; ++i) { mean[i * 8 + 3] = 100.0; for (int k = 0; k < 8; ++k) cov[(size_t)i * 64 + k * 9] = 1e6; }
    for (int i = 0; i < d; ++i) z[i * 4 + 3] = 100.0;
    std::vector<CostJob> jobs(t);
    std::vector<int> rows(d), sps;
    std::iota(rows.begin(), rows.end(), 0);
    for (int i = 0; i < t; ++i) jobs[i] = CostJob{i, gal_count[i], 0, d, i * d, 1};
    for (int i = 0; i < t; ++i) for (int q = 0; q < gal_count[i]; ++q) { sps.push_back(i); sps.push_back(q); sps.push_back(i * s_cap + q); }
    DevScratch mem;
    GuardedOut gm, gc, gout;
    TrackPool tp{};
    float *dfeat = nullptr, *draw = nullptr; double* dz = nullptr; CostJob* dj = nullptr; int *drow = nullptr, *dsps = nullptr;
    VC_TRY(guarded_pool(mem, tp, gm, gc, t, mean.data(), cov.data()));
    tp.budget_cap = s_cap;
    VC_TRY(mem.alloc(&tp.gallery, gal_bytes));
    VC_TRY(mem.upload(&dfeat, feat, (size_t)d * VC_FEAT_DIM * 4));
    VC_TRY(mem.upload(&dz, z.data(), z.size() * 8));
    VC_TRY(mem.upload(&dj, jobs.data(), jobs.size() * sizeof(CostJob)));
    VC_TRY(mem.upload(&drow, rows.data(), rows.size() * 4));
    VC_TRY(gout.alloc(mem, (size_t)t * d * 8));
    // samples enter the device gallery the way the tracker stores them (normalised rows)
    VC_TRY(mem.upload(&draw, gallery, gal_bytes));
    VC_TRY(mem.upload(&dsps, sps.data(), sps.size() * 4));
    VC_TRY(launch_gallery_write(tp, dsps, (int)sps.size() / 3, draw, nullptr));
    VC_TRY(launch_appearance_cost(tp, dj, t, dfeat, drow, dz, gout.as<double>(), nullptr));
    VC_TRY(kernel_wait("kat_appearance_kernel"));
    return gout.read_back(out, "kat_appearance_kernel");
}

// scipy.optimize.linear_sum_assignment through the tracker kernel's own solver (track_core.h lap_solve, one wave on the device)
int vc_lap_host(const double* cost, int nr, int nc, int* rows, int* cols, int* n_assigned) {
    VC_CHECK(cost && rows && cols && n_assigned && nr >= 0 && nc >= 0, VC_ERR_ARG, "bad argument");
    *n_assigned = 0;
    if (nr == 0 || nc == 0) return VC_OK;
    VC_CHECK(nr <= 512 && nc <= 512, VC_ERR_CAPACITY, "lap: at most 512 rows / columns");
    const int k = std::min(nr, nc);
    DevScratch mem;
    GuardedOut gr, gq, gn;
    double *dc = nullptr, *dt = nullptr;
    VC_TRY(mem.upload(&dc, cost, (size_t)nr * nc * 8));
    VC_TRY(mem.alloc(&dt, (size_t)nr * nc * 8));
    VC_TRY(gr.alloc(mem, (size_t)k * 4));
    VC_TRY(gq.alloc(mem, (size_t)k * 4));
    VC_TRY(gn.alloc(mem, 4));
    VC_TRY(launch_kat_lap(dc, nr, nc, dt, gr.as<int>(), gq.as<int>(), gn.as<int>(), nullptr));
    VC_TRY(kernel_wait("kat_lap_kernel"));
    int n = 0;
    std::vector<int> r(k), q(k);
    VC_TRY(gn.read_back(&n, "kat_lap_kernel (count)"));
    VC_TRY(gr.read_back(r.data(), "kat_lap_kernel (rows)"));
    VC_TRY(gq.read_back(q.data(), "kat_lap_kernel (columns)"));
    VC_CHECK(n >= 0, VC_ERR_ARG, "lap: infeasible cost matrix");
    VC_CHECK(n <= k, VC_ERR_HIP, "kat_lap_kernel reported %d pairs of at most %d", n, k);
    std::copy(r.begin(), r.begin() + n, rows);
    std::copy(q.begin(), q.begin() + n, cols);
    *n_assigned = n;
    return VC_OK;
}

}  // extern "C"
