// Host build of vehicle-counting_amd/csrc/sppf_keys.h (the order-preserving keys of the max-pool kernels: plain integer functions)
// behind a C interface for tests/test_aux_cases.py.  et: 0 = fp32 words, 1 = bf16 pairs, 2 = fp8 quads.
#include "../../vehicle-counting_amd/csrc/sppf_keys.h"

extern "C" {

void skh_key(int et, const uint32_t* v, uint32_t* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = et == 0 ? vc::word_key<0>(v[i]) : et == 1 ? vc::word_key<1>(v[i]) : vc::word_key<2>(v[i]);
}

void skh_unkey(int et, const uint32_t* k, uint32_t* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = et == 0 ? vc::word_unkey<0>(k[i]) : et == 1 ? vc::word_unkey<1>(k[i]) : vc::word_unkey<2>(k[i]);
}

void skh_max(int et, const uint32_t* a, const uint32_t* b, uint32_t* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = et == 0 ? vc::word_max<0>(a[i], b[i]) : et == 1 ? vc::word_max<1>(a[i], b[i]) : vc::word_max<2>(a[i], b[i]);
}

// the plain per-byte form sppf_pool_fp8_kernel uses
void skh_umax4(const uint32_t* a, const uint32_t* b, uint32_t* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = vc::umax4(a[i], b[i]);
}

}
