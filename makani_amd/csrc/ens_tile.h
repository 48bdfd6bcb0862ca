// Device helpers of the ensemble kernels (ens.hip, ens_products.hip): the decomposition's constants, the staging of a tile of
// E member streams through LDS and its mirror image, and the in-register bitonic sort of a point's members.
//
// Only helpers live here, never the body of a kernel (the rule of stream_io.h and DESIGN section 23): the kernels of ens.hip
// come out of the compiler with the same instructions as with their own copies.
#pragma once
#include "stream_io.h"

namespace {

constexpr int kRows = 8;           // latitude rows per workgroup (721 x 1440: 91 slabs of 45 tiles of 256 points)
constexpr int kV = mk::sio::kVec;  // points per 16-byte step of a stream's body (fp32: two accesses)
constexpr int kMaxE = 64;

using mk::sio::head_points;
using mk::sio::IO;

// threads per workgroup = points per tile: [E + 1][TP] fp32 of LDS stay below 34 KB for every P
template <int P> constexpr int tile_points() { return P <= 32 ? 256 : 128; }

// n points of `nstreams` streams (stream s starts at src + s * sstride) -> dst [nstreams][TP] fp32.  Every stream finds its
// own 16-byte boundary: items (stream, body vector) and (stream, head or tail point) are dealt over the TP threads.
template <typename S, int TP>
__device__ __forceinline__ void stage(const S* __restrict__ src, long long sstride, int nstreams, float* __restrict__ dst, int n,
                                      int tid) {
    constexpr int VPS = TP / kV;              // body vectors of a stream, at most
    constexpr int NS = 2 * (kV - 1);          // scalar slots of a stream: kV - 1 head points, kV - 1 tail points
    for (int i = tid; i < nstreams * VPS; i += TP) {
        const int s = i / VPS, j = i - s * VPS;
        const S* p = src + s * sstride;
        const int head = head_points(p, n);
        if (j < (n - head) / kV) {
            float v[kV];
            IO<S>::load(p + head + j * kV, v);
            float* d = dst + s * TP + head + j * kV;
#pragma unroll
            for (int k = 0; k < kV; ++k) d[k] = v[k];
        }
    }
    for (int i = tid; i < nstreams * NS; i += TP) {
        const int s = i / NS, q = i - s * NS;
        const S* p = src + s * sstride;
        const int head = head_points(p, n);
        const int tail0 = head + (n - head) / kV * kV;       // scalar points: [0, head) and [tail0, n)
        const int idx = q < kV - 1 ? q : tail0 + (q - (kV - 1));
        if (q < kV - 1 ? q < head : idx < n) dst[s * TP + idx] = IO<S>::ld1(p + idx);
    }
}

// ascending bitonic network on P registers (P a power of two); every index is a compile-time constant after unrolling
template <int P>
__device__ __forceinline__ void sort_ascending(float (&x)[P]) {
    static_assert(P >= 2 && (P & (P - 1)) == 0, "a power of two");
#pragma unroll
    for (int lk = 1; (1 << lk) <= P; ++lk) {
        const int k = 1 << lk;
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) {
            const int j = 1 << lj;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float lo = fminf(x[i], x[l]), hi = fmaxf(x[i], x[l]);
                    const bool up = (i & k) == 0;
                    x[i] = up ? lo : hi;
                    x[l] = up ? hi : lo;
                }
            }
        }
    }
}

// The mirror image of `stage`: n points of `nstreams` rows of src [nstreams][TP] fp32 -> stream s at dst + s * dstride, each
// stream from ITS OWN 16-byte boundary: a scalar head, 16-byte stores, a scalar tail.  Nothing outside the n points is written.
template <typename S, int TP>
__device__ __forceinline__ void unstage(const float* __restrict__ src, S* __restrict__ dst, long long dstride, int nstreams, int n,
                                        int tid) {
    constexpr int VPS = TP / kV;
    constexpr int NS = 2 * (kV - 1);
    for (int i = tid; i < nstreams * VPS; i += TP) {
        const int s = i / VPS, j = i - s * VPS;
        S* p = dst + s * dstride;
        const int head = head_points(p, n);
        if (j < (n - head) / kV) {
            float v[kV];
            const float* d = src + s * TP + head + j * kV;
#pragma unroll
            for (int k = 0; k < kV; ++k) v[k] = d[k];
            IO<S>::store(p + head + j * kV, v);
        }
    }
    for (int i = tid; i < nstreams * NS; i += TP) {
        const int s = i / NS, q = i - s * NS;
        S* p = dst + s * dstride;
        const int head = head_points(p, n);
        const int tail0 = head + (n - head) / kV * kV;
        const int idx = q < kV - 1 ? q : tail0 + (q - (kV - 1));
        if (q < kV - 1 ? q < head : idx < n) IO<S>::st1(p + idx, src[s * TP + idx]);
    }
}

}  // namespace
