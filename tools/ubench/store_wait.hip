// What does an epilogue pay for a load that sits BEHIND a store?  Stores count on vmcnt and retire in issue order (vmcnt_order.hip), so
// `store; load; s_waitcnt vmcnt(0)` waits for the store's acknowledgement plus the load.  Four forms of one epilogue step, per lane a
// 16-byte store to a streaming output and a 16-byte operand (a bias vector: 512 hot bytes) that the NEXT value depends on:
//   (a) store; global load; s_waitcnt vmcnt(0); use      -- the load behind the store
//   (b) global load; store; s_waitcnt vmcnt(1); use      -- the same load issued first, the wait never names the store
//   (c) store; ds_read_b128; s_waitcnt lgkmcnt(0); use   -- the operand from LDS
//   (d) store; use of a register                         -- no operand fetch at all: the floor of the loop
// One workgroup per CU (96 KB of LDS keep a second one out), eight waves, all CUs, `work` dependent FMAs between two steps (0: back to
// back; 64: roughly one channel tile's SiLU epilogue).  Cycles per step = s_memtime difference / steps, median over the waves.
//   hipcc --offload-arch=gfx950 -O2 -o store_wait store_wait.hip && ./store_wait
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MODE>
__global__ __launch_bounds__(512) void step_kernel(f32x4* out, const f32x4* bias, int steps, int work, unsigned long long* cyc) {
    __shared__ f32x4 pad[6144];                              // 96 KB: one workgroup per CU; the first 512 B hold the bias
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 6144; i += 512) pad[i] = bias[i & 31];
    __syncthreads();
    const unsigned lds_addr = (unsigned)(size_t)(__attribute__((address_space(3))) f32x4*)&pad[lane >> 4];
    const f32x4* bp = bias + (lane >> 4);
    // this wave's slice of the output: `steps` consecutive 1 KB rows, written once each
    f32x4* op = out + ((size_t)(blockIdx.x * 8 + wave) * steps) * 64 + lane;
    f32x4 v = {(float)lane, 1.f, 2.f, 3.f};
    const unsigned long long c0 = __builtin_readcyclecounter();
    for (int i = 0; i < steps; ++i) {
        f32x4 b;
        f32x4* o = op + (size_t)i * 64;
        if (MODE == 0)
            asm volatile("global_store_dwordx4 %1, %2, off\n\tglobal_load_dwordx4 %0, %3, off\n\ts_waitcnt vmcnt(0)" : "=&v"(b) : "v"(o), "v"(v), "v"(bp) : "memory");
        else if (MODE == 1)
            asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_store_dwordx4 %1, %2, off\n\ts_waitcnt vmcnt(1)" : "=&v"(b) : "v"(o), "v"(v), "v"(bp) : "memory");
        else if (MODE == 2)
            asm volatile("global_store_dwordx4 %1, %2, off\n\tds_read_b128 %0, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(b) : "v"(o), "v"(v), "v"(lds_addr) : "memory");
        else {
            asm volatile("global_store_dwordx4 %0, %1, off" : : "v"(o), "v"(v) : "memory");
            b = (f32x4){1.f, 1.f, 1.f, 1.f};
            asm volatile("" : "+v"(b));
        }
        v = v * 0.5f + b;
        for (int w = 0; w < work; ++w) v.x = __builtin_fmaf(v.x, 0.999f, v.y);
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) cyc[blockIdx.x * 8 + wave] = c1 - c0;
}

template <int MODE>
static double run(f32x4* out, const f32x4* bias, unsigned long long* cyc, int grid, int steps, int work) {
    std::vector<unsigned long long> h((size_t)grid * 8);
    std::vector<double> med;
    for (int rep = 0; rep < 4; ++rep) {                      // the first repeat warms up
        hipLaunchKernelGGL(step_kernel<MODE>, dim3(grid), dim3(512), 0, 0, out, bias, steps, work, cyc);
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
        if (hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); exit(1); }
        std::sort(h.begin(), h.end());
        if (rep) med.push_back((double)h[h.size() / 2] / steps);
    }
    std::sort(med.begin(), med.end());
    return med[med.size() / 2];
}

int main(int argc, char** argv) {
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    const int steps = argc > 1 ? atoi(argv[1]) : 512;        // 256 CUs x 8 waves x 512 steps x 1 KB = 1 GiB of output, far beyond L2 + MALL
    const size_t n = (size_t)cus * 8 * steps * 64;
    f32x4 *out, *bias;
    unsigned long long* cyc;
    if (hipMalloc(&out, n * sizeof(f32x4)) != hipSuccess || hipMalloc(&bias, 512) != hipSuccess || hipMalloc(&cyc, (size_t)cus * 8 * 8) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    if (hipMemset(bias, 0, 512) != hipSuccess) return 1;
    printf("%d CUs x 8 waves, %d steps of one 16-byte store per lane; cycles per step (median wave, median of 3 launches)\n", cus, steps);
    printf("%-52s %10s %10s\n", "form", "work = 0", "work = 64");
    const char* names[4] = {"(a) store; load; vmcnt(0); use", "(b) load; store; vmcnt(1); use", "(c) store; ds_read_b128; lgkmcnt(0); use", "(d) store; use (no operand fetch)"};
    double r[4][2];
    for (int wi = 0; wi < 2; ++wi) {
        const int work = wi ? 64 : 0;
        r[0][wi] = run<0>(out, bias, cyc, cus, steps, work);
        r[1][wi] = run<1>(out, bias, cyc, cus, steps, work);
        r[2][wi] = run<2>(out, bias, cyc, cus, steps, work);
        r[3][wi] = run<3>(out, bias, cyc, cus, steps, work);
    }
    for (int m = 0; m < 4; ++m) printf("%-52s %10.1f %10.1f\n", names[m], r[m][0], r[m][1]);
    (void)hipFree(out); (void)hipFree(bias); (void)hipFree(cyc);
    return 0;
}
