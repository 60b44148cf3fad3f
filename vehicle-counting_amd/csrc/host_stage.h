// Staging harness of the stateless host-array entry points (vc_*_host in host_conv.hip, host_aux.hip, host_detect.hip, host_track.hip and the
// YUV files): device scratch that every early return frees, outputs between guard blocks, float arrays as elements of a precision and back,
// and the wait that names the kernel.  None of it touches a vc_engine.
#pragma once
#include <vector>

#include "kernels.h"

namespace vc {

// engine.hip: the one allocation routine: hipMalloc, recorded in `allocs`
int dev_alloc(std::vector<void*>& allocs, void** p, size_t bytes);

// Device scratch memory of an entry point: freed when the owner goes out of scope, so every early VC_TRY / VC_HIP / VC_CHECK return releases it.
struct DevScratch {
    std::vector<void*> allocs;
    DevScratch() = default;
    DevScratch(const DevScratch&) = delete;
    DevScratch& operator=(const DevScratch&) = delete;
    ~DevScratch() { for (void* q : allocs) (void)hipFree(q); }
    template <class T> int alloc(T** p, size_t bytes) { return dev_alloc(allocs, (void**)p, bytes); }
    // a block that starts as the caller's array
    template <class T> int upload(T** p, const void* src, size_t bytes) {
        VC_TRY(alloc(p, bytes));
        if (bytes) VC_HIP(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
        return VC_OK;
    }
};

// wait for the device, and name the kernel if it failed
inline int kernel_wait(const char* kernel) {
    VC_CHECK(hipDeviceSynchronize() == hipSuccess, VC_ERR_HIP, "%s failed: %s", kernel, hipGetErrorString(hipGetLastError()));
    return VC_OK;
}

// The device output of a parity entry point between two guard blocks that read_back checks: a kernel that wrote outside its output is
// reported instead of returning a plausible result.
struct GuardedOut {
    static constexpr size_t kGuard = 256;
    uint8_t* base = nullptr;
    size_t bytes = 0, guard = kGuard;
    uint8_t fill = 0xA5;
    // out_bytes + 2 guard blocks, all 0xA5; with `preload` the output starts as the caller's array.  guard_bytes (a multiple of 256): a
    // caller that knows how far a kernel without its bounds tests would stray (a tile's overhang) asks for blocks that hold all of it.
    // fill_byte: an INPUT between guard blocks takes 0xFF -- a bf16 NaN, the byte 255 -- so that a read outside it shows in the result
    int alloc(DevScratch& mem, size_t out_bytes, const void* preload = nullptr, size_t guard_bytes = kGuard, uint8_t fill_byte = 0xA5) {
        bytes = out_bytes;
        guard = guard_bytes;
        fill = fill_byte;
        VC_TRY(mem.alloc(&base, bytes + 2 * guard));
        VC_HIP(hipMemset(base, fill, bytes + 2 * guard));
        if (preload) VC_HIP(hipMemcpy(out(), preload, bytes, hipMemcpyHostToDevice));
        return VC_OK;
    }
    uint8_t* out() const { return base + guard; }
    template <class T> T* as() const { return (T*)out(); }
    // waits for the null stream; `kernel` names the culprit
    int read_back(void* host_out, const char* kernel) const {
        std::vector<uint8_t> all(bytes + 2 * guard);
        VC_CHECK(hipMemcpy(all.data(), base, all.size(), hipMemcpyDeviceToHost) == hipSuccess, VC_ERR_HIP, "%s failed: %s", kernel, hipGetErrorString(hipGetLastError()));
        memcpy(host_out, all.data() + guard, bytes);
        for (size_t i = 0; i < 2 * guard; ++i) VC_CHECK(all[i < guard ? i : bytes + i] == fill, VC_ERR_HIP, "%s wrote outside its output (guard byte %zu)", kernel, i);
        return VC_OK;
    }
};

// n floats -> elements of `prec` (exact for values the type represents; NaN stays NaN), and one element back
inline std::vector<uint8_t> to_elems(const float* src, size_t n, int prec) {
    const int es = elem_size(prec);
    std::vector<uint8_t> buf(n * es);
    for (size_t i = 0; i < n; ++i) {
        if (es == 4) ((float*)buf.data())[i] = src[i];
        else if (es == 2) ((uint16_t*)buf.data())[i] = f32_to_bf16(src[i]);
        else buf[i] = f32_to_e4m3(src[i]);
    }
    return buf;
}
inline float from_elem(const uint8_t* buf, size_t i, int es) {
    return es == 4 ? ((const float*)buf)[i] : es == 2 ? bf16_to_f32(((const uint16_t*)buf)[i]) : e4m3_to_f32(buf[i]);
}
inline int upload_elems(DevScratch& mem, const float* src, size_t n, int prec, void** dst) {
    const std::vector<uint8_t> buf = to_elems(src, n, prec);
    return mem.upload(dst, buf.data(), buf.size());
}
// the caller's float array as the guarded device buffer a kernel writes into, and back
inline int guarded_elems(DevScratch& mem, GuardedOut& g, const float* init, size_t n, int prec, size_t guard = GuardedOut::kGuard) {
    const std::vector<uint8_t> buf = to_elems(init, n, prec);
    return g.alloc(mem, buf.size(), buf.data(), guard);
}
inline int read_elems(const GuardedOut& g, size_t n, int prec, float* dst, const char* kernel) {
    std::vector<uint8_t> buf(g.bytes);
    VC_TRY(g.read_back(buf.data(), kernel));
    for (size_t i = 0; i < n; ++i) dst[i] = from_elem(buf.data(), i, elem_size(prec));
    return VC_OK;
}
// a guarded [npix][4] tensor of `prec` (the letterbox and crop kernels pad 3 channels to 4) -> the caller's [npix][3] floats
inline int read_rgb_of4(const GuardedOut& g, size_t npix, int prec, float* out, const char* kernel) {
    std::vector<uint8_t> buf(g.bytes);
    VC_TRY(g.read_back(buf.data(), kernel));
    for (size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = from_elem(buf.data(), i * 4 + c, elem_size(prec));
    return VC_OK;
}

}  // namespace vc
