// Element traits of the layout passes (csrc/layout.hip, csrc/patch.hip): an fp32 or bf16 element as a 32-bit word in an LDS tile.
#pragma once
#include <hip/hip_runtime.h>

template <typename T> struct LayoutElem;
template <> struct LayoutElem<float> {
    static __device__ __forceinline__ unsigned bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(unsigned b) { return __uint_as_float(b); }
    static __device__ __forceinline__ unsigned round(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float from(unsigned b) { return __uint_as_float(b); }
};
template <> struct LayoutElem<unsigned short> {     // bf16
    static __device__ __forceinline__ unsigned bits(unsigned short v) { return v; }
    static __device__ __forceinline__ unsigned short from(unsigned b) { return (unsigned short)b; }
    static __device__ __forceinline__ float value(unsigned b) { return __uint_as_float(b << 16); }
    static __device__ __forceinline__ unsigned round(float v) {     // to nearest even; NaN stays NaN
        const unsigned u = __float_as_uint(v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
};

// word k of a 16-byte vector of T: one fp32, or the k-th of eight bf16
template <typename T> __device__ __forceinline__ unsigned vec_word(const uint4& v, int k) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (sizeof(T) == 4) return w[k];
    else return (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
}

// the 16-byte vector of T whose words are w[0 ... 16 / sizeof(T) - 1]
template <typename T> __device__ __forceinline__ uint4 vec_pack(const unsigned* w) {
    if constexpr (sizeof(T) == 4) return make_uint4(w[0], w[1], w[2], w[3]);
    else return make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
}
