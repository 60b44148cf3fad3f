// Order-preserving integer keys of the max-pool kernels (aux_kernels.hip), usable from host and device: the host build is what
// tests/native/sppf_keys_host.cpp compiles and tests/test_aux_cases.py checks exhaustively.
//
// A float's bits compare like unsigned integers once negative values have all bits flipped and non-negative ones the sign bit set.
// bf16 pairs are keyed per half and fp8 (e4m3fn: sign-magnitude -> biased unsigned) quads per byte, so a word of a plane is keyed,
// compared and turned back as one 32-bit value.  Key 0 is the key of no non-NaN value and lies below all of them: the padding of
// MaxPool2d.  -0 keys below +0.  NaNs are outside the kernels' contract.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VC_KEY_FN __host__ __device__ __forceinline__
#else
#define VC_KEY_FN inline
#endif

namespace vc {

VC_KEY_FN uint32_t fp8_key4(uint32_t v) {                             // per byte: b ^ (b & 0x80 ? 0xff : 0x80)
    const uint32_t neg = (v >> 7) & 0x01010101u;
    return v ^ (0x80808080u | (neg * 0x7fu));
}
VC_KEY_FN uint32_t fp8_unkey4(uint32_t k) {                           // inverse: key >= 0x80 was a positive byte (k ^ 0x80), else negative (k ^ 0xff)
    const uint32_t pos = (k >> 7) & 0x01010101u;
    return k ^ (0xffffffffu ^ (pos * 0x7fu));
}
VC_KEY_FN uint32_t umax4(uint32_t a, uint32_t b) {                    // per byte, plain form
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) { const uint32_t x = (a >> (8 * i)) & 0xff, y = (b >> (8 * i)) & 0xff; r |= (x > y ? x : y) << (8 * i); }
    return r;
}
VC_KEY_FN uint32_t umax2(uint32_t a, uint32_t b) {                    // per half, plain form
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al : bl) | ((ah > bh ? ah : bh) << 16);
}
template <bool F32>
VC_KEY_FN uint32_t to_key(uint32_t v) {
    if (F32) return v ^ ((uint32_t)((int32_t)v >> 31) | 0x80000000u);
    const uint32_t neg = (v >> 15) & 0x00010001u;                     // sign of each half
    return v ^ ((neg * 0x7fffu) | 0x80008000u);                        // negative: flip all 16 bits, else flip the sign bit
}
template <bool F32>
VC_KEY_FN uint32_t from_key(uint32_t k) {
    if (F32) return k ^ ((uint32_t)(~((int32_t)k >> 31)) | 0x80000000u);
    const uint32_t pos = (k >> 15) & 0x00010001u;                     // key has its top bit set <=> the value was non-negative
    return k ^ (((pos ^ 0x00010001u) * 0x7fffu) | 0x80008000u);
}
template <bool F32>
VC_KEY_FN uint32_t kmax(uint32_t a, uint32_t b) {
    if (F32) return a > b ? a : b;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));   // one v_pk_max_u16
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
#else
    return umax2(a, b);
#endif
}

// element type of the plane: 0 = fp32, 1 = bf16 pairs, 2 = fp8 (e4m3fn) quads
template <int ET> VC_KEY_FN uint32_t word_key(uint32_t v) { return ET == 2 ? fp8_key4(v) : to_key<ET == 0>(v); }
template <int ET> VC_KEY_FN uint32_t word_unkey(uint32_t k) { return ET == 2 ? fp8_unkey4(k) : from_key<ET == 0>(k); }
template <int ET> VC_KEY_FN uint32_t word_max(uint32_t a, uint32_t b) {
    if (ET == 2) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef unsigned char u8x4 __attribute__((ext_vector_type(4)));
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u8x4, a), __builtin_bit_cast(u8x4, b)));
#else
        return umax4(a, b);
#endif
    }
    return kmax<ET == 0>(a, b);
}

}  // namespace vc
