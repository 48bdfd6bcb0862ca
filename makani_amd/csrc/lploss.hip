// Training losses of the trainer's Lp family (makani/utils/losses.py:174-271, GeometricLpLoss): every spelling --
// relative or absolute, with or without the root, any channel weights and reduction -- is a function of two
// latitude-weighted integrals per (sample, channel),
//   s0 = sum w |p - t|^P,   s1 = sum w |t|^P,   P in {1, 2},   w = wrow[h]
// (the quadrature weights depend on the latitude only).  The integrals add up across spatial shards, so a sharded run
// all-reduces these sums instead of gathering the fields.  The ratio, the root, the channel weights and the reduction
// are [B, C] arithmetic and stay with the caller.
//
// Forward (geo_lp_sums_kernel): the decomposition of metrics.hip.  Workgroup (slab, c) takes kRows latitude rows of
// channel c for ALL samples; each wave walks whole rows, a lane 8 consecutive points per step.  Row sums are fp32 per
// lane, folded into fp64 with the row's weight at the end of the row.  Each workgroup writes its 2 * B fp64 partials
// to a workspace slot of its own; the finalize kernel adds the slabs in a fixed order.  No atomics: the result is bitwise
// repeatable.  Both sums are always formed: s1 costs two VALU operations per point of a pass that waits on memory, and
// a switch would double the instantiations.
//
// Backward (geo_lp_bwd_kernel): gp = g[b][c] * wrow[h] * (P == 2 ? 2 (p - t) : sign(p - t)), sign(0) = 0, one wave per
// row, written in the prediction's dtype.  s1 does not depend on the prediction.
//
// Any W: a row is walked as a scalar head up to the 16-byte boundary of the prediction, an 8-wide vector body
// (16-byte accesses) and a scalar tail; when the streams of a row disagree on their alignment the row runs scalar.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cstdint>

namespace {

constexpr int kT = 256;          // threads per workgroup (4 waves)
constexpr int kE = mk::sio::kVec;  // points per lane per step (the width of IO<T>)
constexpr int kRows = 16;        // latitude rows per forward workgroup
constexpr int kK = 2;            // sums per (sample, channel)
constexpr int kBwdGrid = 8192;   // backward: at most this many workgroups, waves stride over the rows

using mk::sio::al16;
using mk::sio::head_points;
using mk::sio::IO;

template <int P>
__device__ __forceinline__ void accum(float (&s)[kK], float p, float t) {
    const float d = p - t;
    if (P == 2) {
        s[0] = fmaf(d, d, s[0]);
        s[1] = fmaf(t, t, s[1]);
    } else {
        s[0] += fabsf(d);
        s[1] += fabsf(t);
    }
}

// k d(|d|^P)/dd, up to the factor 2 of P == 2 that the caller folds into k
template <int P>
__device__ __forceinline__ float dnorm(float k, float p, float t) {
    const float d = p - t;
    if (P == 2) return k * d;
    return d > 0.f ? k : (d < 0.f ? -k : 0.f);
}

// partials [nslab][B][C][2]: slab s = blockIdx.x, channel c = blockIdx.y
template <typename T, int NB, int P>
__global__ __launch_bounds__(kT) void geo_lp_sums_kernel(const T* __restrict__ pred, const float* __restrict__ tar,
                                                         const float* __restrict__ wrow, double* __restrict__ part, int B,
                                                         int C, int H, int W) {
    __shared__ double red[kT / 64][NB * kK];
    const int s = blockIdx.x, c = blockIdx.y;
    const int h0 = s * kRows, h1 = min(H, h0 + kRows);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long HW = (long long)H * W, CHW = (long long)C * HW;
    for (int b0 = 0; b0 < B; b0 += NB) {
        const int nb = min(NB, B - b0);
        double acc[NB][kK];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kK; ++k) acc[b][k] = 0.0;
        for (int h = h0 + wave; h < h1; h += kT / 64) {
            const T* pr = pred + ((long long)b0 * C + c) * HW + (long long)h * W;     // row of sample b0
            const float* tr = tar + ((long long)b0 * C + c) * HW + (long long)h * W;
            float r[NB][kK];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int k = 0; k < kK; ++k) r[b][k] = 0.f;
            // the row is vectorised when every stream of every sample of the pass is 16-byte aligned behind the head
            // (wave-uniform), else walked scalar
            const int head = head_points(pr, W);
            bool vec = true;
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b < nb) vec = vec && al16(pr + b * CHW + head) && al16(tr + b * CHW + head);
            const int nv = vec ? (W - head) / kE : 0;
            const int vend = vec ? head + nv * kE : 0;        // scalar points: [0, head) and [vend, W) (all when !vec)
            for (int j = lane; j < nv; j += 64) {
                const int i = head + j * kE;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b < nb) {
                        float pv[kE], tv[kE];
                        IO<T>::load(pr + b * CHW + i, pv);
                        IO<float>::load(tr + b * CHW + i, tv);
#pragma unroll
                        for (int e = 0; e < kE; ++e) accum<P>(r[b], pv[e], tv[e]);
                    }
                }
            }
            const int nhead = vec ? head : 0;
            const int nscal = nhead + (W - vend);
            for (int q = lane; q < nscal; q += 64) {
                const int i = q < nhead ? q : vend + (q - nhead);
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (b < nb) accum<P>(r[b], IO<T>::ld1(pr + b * CHW + i), tr[b * CHW + i]);
            }
            const double w = (double)wrow[h];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int k = 0; k < kK; ++k) acc[b][k] = fma((double)r[b][k], w, acc[b][k]);
        }
        // fixed-order reduction: lanes by shuffle, then the four waves in order; the fold is spelled out in each kernel,
        // as a shared function it changed the generated code (stream_io.h)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kK; ++k) {
                double v = acc[b][k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
                if (lane == 0) red[wave][b * kK + k] = v;
            }
        __syncthreads();
        if ((int)threadIdx.x < nb * kK) {
            const int b = threadIdx.x / kK, k = threadIdx.x % kK;
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < kT / 64; ++q) v += red[q][threadIdx.x];
            part[(((long long)s * B + b0 + b) * C + c) * kK + k] = v;
        }
        __syncthreads();
    }
}

// rows = B * C * H rows of W points; wave (blockIdx.x, wave) takes rows blockIdx.x * 4 + wave, + 4 gridDim.x, ...
template <typename T, int P>
__global__ __launch_bounds__(kT) void geo_lp_bwd_kernel(const T* __restrict__ pred, const float* __restrict__ tar,
                                                        const float* __restrict__ wrow, const float* __restrict__ g,
                                                        T* __restrict__ gpred, long long rows, int H, int W) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * (kT / 64) + wave; row < rows; row += (long long)gridDim.x * (kT / 64)) {
        const long long bc = row / H;
        const float k = (P == 2 ? 2.f : 1.f) * g[bc] * wrow[row - bc * H];
        const T* pr = pred + row * W;
        const float* tr = tar + row * W;
        T* gr = gpred + row * W;
        const int head = head_points(pr, W);
        const bool vec = al16(pr + head) && al16(tr + head) && al16(gr + head);
        const int nv = vec ? (W - head) / kE : 0;
        const int vend = vec ? head + nv * kE : 0;
        for (int j = lane; j < nv; j += 64) {
            const int i = head + j * kE;
            float pv[kE], tv[kE];
            IO<T>::load(pr + i, pv);
            IO<float>::load(tr + i, tv);
#pragma unroll
            for (int e = 0; e < kE; ++e) pv[e] = dnorm<P>(k, pv[e], tv[e]);
            IO<T>::store(gr + i, pv);
        }
        const int nhead = vec ? head : 0;
        const int nscal = nhead + (W - vend);
        for (int q = lane; q < nscal; q += 64) {
            const int i = q < nhead ? q : vend + (q - nhead);
            IO<T>::st1(gr + i, dnorm<P>(k, IO<T>::ld1(pr + i), tr[i]));
        }
    }
}

template <typename T, int NB>
void launch_sums(const T* pred, const float* tar, const float* wrow, double* part, int p, int B, int C, int H, int W,
                 hipStream_t st) {
    const dim3 grid((unsigned)mk::ceil_div(H, kRows), (unsigned)C);
    if (p == 2)
        hipLaunchKernelGGL((geo_lp_sums_kernel<T, NB, 2>), grid, dim3(kT), 0, st, pred, tar, wrow, part, B, C, H, W);
    else
        hipLaunchKernelGGL((geo_lp_sums_kernel<T, NB, 1>), grid, dim3(kT), 0, st, pred, tar, wrow, part, B, C, H, W);
}

template <typename T>
void launch_nb(const T* pred, const float* tar, const float* wrow, double* part, int p, int B, int C, int H, int W,
               hipStream_t st) {
    if (B == 1) launch_sums<T, 1>(pred, tar, wrow, part, p, B, C, H, W, st);
    else launch_sums<T, 2>(pred, tar, wrow, part, p, B, C, H, W, st);
}

template <typename T>
void launch_bwd(const T* pred, const float* tar, const float* wrow, const float* g, T* gpred, int p, long long rows, int H,
                int W, hipStream_t st) {
    const long long want = mk::ceil_div_ll(rows, kT / 64);
    const dim3 grid((unsigned)(want < kBwdGrid ? want : kBwdGrid));
    if (p == 2)
        hipLaunchKernelGGL((geo_lp_bwd_kernel<T, 2>), grid, dim3(kT), 0, st, pred, tar, wrow, g, gpred, rows, H, W);
    else
        hipLaunchKernelGGL((geo_lp_bwd_kernel<T, 1>), grid, dim3(kT), 0, st, pred, tar, wrow, g, gpred, rows, H, W);
}

}  // namespace

extern "C" long long mk_geo_lp_workspace(int B, int C, int H) {
    if (B < 1 || C < 1 || H < 1) return 0;
    return (long long)mk::ceil_div(H, kRows) * B * C * kK;
}

extern "C" int mk_geo_lp_sums(const void* pred, int dtype, const float* tar, const float* wrow, double* workspace,
                              double* sums, int p, int B, int C, int H, int W, void* stream) {
    MK_REQUIRE(pred && tar && wrow && workspace && sums, "null pointer");
    MK_REQUIRE(p == 1 || p == 2, "p must be 1 or 2");
    MK_REQUIRE(B >= 1 && C >= 1 && C <= 65535 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE((long long)B * C * H * W < (1LL << 40), "field too large");
    MK_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(mk::aligned_to(pred, dtype == 0 ? 4 : 2), "prediction not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(tar, wrow), "fp32 stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(workspace, sums), "fp64 buffer not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        launch_nb<float>((const float*)pred, tar, wrow, workspace, p, B, C, H, W, st);
    else
        launch_nb<__hip_bfloat16>((const __hip_bfloat16*)pred, tar, wrow, workspace, p, B, C, H, W, st);
    MK_LAUNCH_CHECK();
    const long long n = (long long)B * C * kK;
    hipLaunchKernelGGL(slab_finalize_kernel<kT>, dim3((unsigned)mk::ceil_div_ll(n, kT / 64)), dim3(kT), 0, st, workspace, sums,
                       mk::ceil_div(H, kRows), n);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_geo_lp_bwd(const void* pred, int dtype, const float* tar, const float* wrow, const float* g, void* gpred,
                             int p, int B, int C, int H, int W, void* stream) {
    MK_REQUIRE(pred && tar && wrow && g && gpred, "null pointer");
    MK_REQUIRE(p == 1 || p == 2, "p must be 1 or 2");
    MK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE((long long)B * C * H * W < (1LL << 40), "field too large");
    MK_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(mk::aligned_to(pred, dtype == 0 ? 4 : 2) && mk::aligned_to(gpred, dtype == 0 ? 4 : 2),
               "prediction or its gradient not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(tar, wrow, g), "fp32 stream not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * C * H;
    if (dtype == 0)
        launch_bwd<float>((const float*)pred, tar, wrow, g, (float*)gpred, p, rows, H, W, st);
    else
        launch_bwd<__hip_bfloat16>((const __hip_bfloat16*)pred, tar, wrow, g, (__hip_bfloat16*)gpred, p, rows, H, W, st);
    MK_LAUNCH_CHECK();
    return 0;
}
