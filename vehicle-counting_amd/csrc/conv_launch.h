// Host-side pieces the launchers of the convolution kernels share (the conv_*.hip family files, front_fused.hip, c3_fused.hip): the
// device query, the resident-workgroup count of a kernel, and the process-wide A/B and diagnostic switches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vc_common.h"
#include "conv_geom.h"

namespace vc {

// A/B and diagnostic switches of the launchers, read from the environment once per process (at the first conv launch).  The A/B
// switches are on unless set to 0.  (Not here: VC_CONV_STRICT, which the tests set after the library is loaded -- launch_conv reads it at
// the point of the fall-back -- and what vc_conv2d_host reads per call: VC_CONV_CFG, VC_CONV_SLOTS, VC_CONV_ABLATE, VC_CONV_DBG, VC_CONV_TIME.)
struct ConvSwitches {
    bool sk;            // VC_CONV_SK: the split-K tiles
    bool s2halo;        // VC_CONV_S2HALO: conv3x3s2_halo_kernel
    bool direct;        // VC_CONV_DIRECT: conv1x1_direct_kernel
    bool direct8;       // VC_CONV_DIRECT8: conv1x1_direct_fp8_kernel
    bool wreg;          // VC_CONV_WREG: conv1x1_wreg_kernel
    bool halo_v2;       // VC_CONV_HALO_V2: conv3x3_halo_v2_kernel
    bool persist;       // VC_CONV_PERSIST: persistent grids of the implicit GEMM (0: one workgroup per tile)
    bool balanced;      // VC_CONV_BALANCED: persistent_grid's rounds-first rule (0: the old rule)
    bool sk_uncached;   // VC_SK_UNCACHED: the split-K workspace in memory no L2 caches
    bool s2pw_store;    // VC_S2PW_STORE (diagnostics, off unless non-zero): launch_s2halo_pw also stores the 3x3's own output
    int dyn_lds;        // VC_CONV_DYN_LDS (diagnostics, default 0): dynamic LDS bytes of an implicit-GEMM launch, caps workgroups per CU
    // A persistent grid that fills every workgroup slot of the chip leaves no room for the kernels of the other streams (ReID next to the
    // detector, the tracker walk), which then wait for a conv launch to end: 64 slots are left free (round 2, 128-frame steps:
    // 0 / 32 / 64 / 96 / 128 free slots = 14.9 / 15.1 / 15.6 / 15.6 / 15.4 k frames/s; 256 free slots cost 9 % of conv time).
    int reserve;        // VC_CONV_RESERVE
};
inline const ConvSwitches& conv_switches() {
    static const ConvSwitches sw = [] {
        const auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        ConvSwitches c;
        c.sk = num("VC_CONV_SK", 1) != 0;
        c.s2halo = num("VC_CONV_S2HALO", 1) != 0;
        c.direct = num("VC_CONV_DIRECT", 1) != 0;
        c.direct8 = num("VC_CONV_DIRECT8", 1) != 0;
        c.wreg = num("VC_CONV_WREG", 1) != 0;
        c.halo_v2 = num("VC_CONV_HALO_V2", 1) != 0;
        c.persist = num("VC_CONV_PERSIST", 1) != 0;
        c.balanced = num("VC_CONV_BALANCED", 1) != 0;
        c.sk_uncached = num("VC_SK_UNCACHED", 1) != 0;
        c.s2pw_store = num("VC_S2PW_STORE", 0) != 0;
        c.dyn_lds = num("VC_CONV_DYN_LDS", 0);
        c.reserve = num("VC_CONV_RESERVE", 64);
        return c;
    }();
    return sw;
}
inline int conv_slots_reserve() { return conv_switches().reserve; }

// compute units of the current device, queried once
inline int device_cus() {
    static const int n = [] {
        int dev = 0, cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        return cus;
    }();
    return n;
}

// resident workgroups of one kernel instantiation on the whole device (occupancy x CUs); the callers keep the result in a static
template <class K>
static int resident_workgroups(K kernel, int threads = 256) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    return per_cu * device_cus();
}

// Diagnostics of the fused persistent kernels (VC_FF_DBG / VC_C3_DBG / VC_BN_DBG = n): every workgroup stamps wall_clock64() (100 MHz) when it
// starts and when it leaves.  The stamps of n launches collect in device memory with nothing but a memset in the stream -- no allocation,
// no host wait: the launches run inside the pipeline as they always do -- and are read back and printed after the n-th.  n = 1 reports every launch at once.
// Record of a workgroup: `stride` 64-bit words, the start stamp in word w0, the end stamp in word w1.
struct WgStamps {
    const char* name;
    int n = 0, used = 0, stride = 0, w0 = 0, w1 = 0;
    long long* d = nullptr;
    size_t per_launch = 0;                       // words
    std::vector<int> grids, tiles;
    WgStamps(const char* env, const char* kernel, int max_grid, int stride_, int w0_, int w1_) : name(kernel), stride(stride_), w0(w0_), w1(w1_) {
        const char* v = getenv(env);
        n = v ? std::max(1, atoi(v)) : 0;
        per_launch = (size_t)max_grid * stride;
        if (n && hipMalloc((void**)&d, (size_t)n * per_launch * 8) != hipSuccess) { d = nullptr; n = 0; }
    }
    long long* next(int grid, int ntiles, hipStream_t s) {                  // this launch's records, zeroed in stream order; null = off
        if (!d || used >= n || (size_t)grid * stride > per_launch) return nullptr;
        long long* p = d + (size_t)used++ * per_launch;
        hipMemsetAsync(p, 0, (size_t)grid * stride * 8, s);
        grids.push_back(grid); tiles.push_back(ntiles);
        return p;
    }
    template <class F>
    void report(hipStream_t s, F extra) {                                    // after a launch: prints once `n` launches have been collected
        if (!d || used < n) return;
        hipStreamSynchronize(s);
        std::vector<long long> h(per_launch);
        for (int l = 0; l < used; ++l) {
            const int grid = grids[l];
            if (hipMemcpy(h.data(), d + (size_t)l * per_launch, (size_t)grid * stride * 8, hipMemcpyDeviceToHost) != hipSuccess) break;
            std::vector<double> st, du;
            long long lo = INT64_MAX, hi = 0;
            for (int b = 0; b < grid; ++b) { const long long* t = &h[(size_t)b * stride]; if (t[w0] && t[w1]) { lo = std::min(lo, t[w0]); hi = std::max(hi, t[w1]); } }
            int late = 0;
            for (int b = 0; b < grid; ++b) {
                const long long* t = &h[(size_t)b * stride];
                if (!t[w0] || !t[w1]) continue;
                st.push_back((double)(t[w0] - lo) / 100); du.push_back((double)(t[w1] - t[w0]) / 100);
                late += t[w0] - lo > 10000;                                  // more than 0.1 ms after the first
            }
            const size_t m = st.size();
            if (!m) continue;
            std::sort(st.begin(), st.end()); std::sort(du.begin(), du.end());
            fprintf(stderr, "[vc %s dbg] launch %d: %d tiles on %d workgroups; start offsets us p10/p50/p90/max %.1f %.1f %.1f %.1f ; lifetimes us p10/p50/p90/max %.1f %.1f %.1f %.1f ; "
                            "%d workgroups (%.1f %%) start > 100 us late ; first start -> last end %.1f us\n",
                    name, l, tiles[l], grid, st[m / 10], st[m / 2], st[m * 9 / 10], st[m - 1], du[m / 10], du[m / 2], du[m * 9 / 10], du[m - 1], late, 100.0 * late / m,
                    (double)(hi - lo) / 100);
            extra(h.data(), grid, tiles[l]);
        }
        used = 0; grids.clear(); tiles.clear();
    }
};

}  // namespace vc
