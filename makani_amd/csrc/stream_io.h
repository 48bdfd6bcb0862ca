// Device helpers of the HBM streaming kernels (metrics.hip, lploss.hip, preproc.hip, pointwise.hip; zenith.hip takes
// head_points only): rows of fp32 or bf16 points walked as a scalar head up to a 16-byte boundary, a body of 16-byte
// accesses and a scalar tail, and the fixed-order finish of their slab sums.
//
// Only helpers live here, never the body of a kernel: a helper is shared when every kernel that uses it comes out of the
// compiler with the same instructions as with its own copy.  Nothing here is a file's tuning knob:
// the files keep their own kT / kE, the vector width below has a name of its own.  The 64-lane __shfl_down fold is not
// here: as a function it changed the schedule of every kernel that folds more than one sum, so each kernel spells it out.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

namespace mk {
namespace sio {

constexpr int kVec = 8;          // points per lane per step of the vector body: one or two 16-byte accesses

// kVec points at p (16-byte aligned) <-> kVec floats, one point at p <-> one float
template <typename T> struct IO;
template <> struct IO<float> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[kVec]) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[kVec]) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
    static __device__ __forceinline__ float ld1(const float* p) { return *p; }
    static __device__ __forceinline__ void st1(float* p, float v) { *p = v; }
};
template <> struct IO<__hip_bfloat16> {
    static __device__ __forceinline__ void load(const __hip_bfloat16* p, float (&v)[kVec]) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void store(__hip_bfloat16* p, const float (&v)[kVec]) {
        __hip_bfloat16 h[kVec];
#pragma unroll
        for (int i = 0; i < kVec; ++i) h[i] = __float2bfloat16(v[i]);  // round to nearest even, NaN safe
        *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(h);
    }
    static __device__ __forceinline__ float ld1(const __hip_bfloat16* p) { return __bfloat162float(*p); }
    static __device__ __forceinline__ void st1(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }
};

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// scalar points before the 16-byte boundary of a row that starts at p (at most W)
template <typename T>
__device__ __forceinline__ int head_points(const T* p, int W) {
    const int head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
    return head > W ? W : head;
}

}  // namespace sio
}  // namespace mk

namespace {

// sums[i] = sum over slabs of part[slab][i], i in [0, n), one wave per i in a fixed order: lane q adds slabs q, q + 64,
// ... in order, then the lanes fold by the same shuffle tree every time (a single thread per i would wait on nslab dependent loads).  Launch with
// THREADS threads and ceil(n / (THREADS / 64)) workgroups.  A template in an anonymous namespace: each translation unit
// that launches it gets a kernel of its own, the others none.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void slab_finalize_kernel(const double* __restrict__ part, double* __restrict__ sums,
                                                                int nslab, long long n) {
    const long long i = (long long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wave-uniform
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int q = lane; q < nslab; q += 64) v += part[(long long)q * n + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sums[i] = v;
}

}  // namespace
