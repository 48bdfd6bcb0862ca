// Validation metrics of the trainer (makani/utils/metrics/functions.py:20-107 through MetricsHandler.update,
// makani/utils/metric.py:186-204): every metric the handler keeps -- geometric L1, RMSE and the anomaly correlation
// (ACC) -- is a ratio or a root of five latitude-weighted integrals per (sample, channel),
//   s0 = sum w |p - t|,  s1 = sum w (p - t)^2,  s2 = sum w (p - c)(t - c),  s3 = sum w (p - c)^2,  s4 = sum w (t - c)^2,
// with w = wrow[h] (the quadrature weights depend on the latitude only) and c the climatology (0 when absent).  The
// integrals add up across spatial shards, so a sharded run all-reduces these sums instead of gathering the fields.
//
// Decomposition: workgroup (slab, c) takes kRows latitude rows of channel c for ALL samples; each wave walks whole
// rows (one row per wave at a time), a lane 8 consecutive points per step, and the climatology vector it loads serves
// the NB <= 2 samples of one pass (clim is read once per (c, h) row for B <= 2).  Row sums are fp32 per lane, folded into
// fp64 with the row's weight at the end of the row (as wmse_kernel, pointwise.hip).  Each workgroup writes its
// 5 * B fp64 partials to a workspace slot of its own; the finalize kernel adds the slabs in slab order.  No atomics:
// the result is bitwise repeatable.
//
// Any W: a row is walked as a scalar head up to the 16-byte boundary of the prediction, an 8-wide vector body
// (16-byte loads) and a scalar tail; when the streams of a row disagree on their alignment the row runs scalar.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cstdint>

namespace {

constexpr int kT = 256;          // threads per workgroup (4 waves)
constexpr int kE = mk::sio::kVec;  // points per lane per step (the width of IO<T>)
constexpr int kRows = 16;        // latitude rows per workgroup
constexpr int kK = 5;            // sums per (sample, channel)

using mk::sio::al16;
using mk::sio::head_points;
using mk::sio::IO;

__device__ __forceinline__ void accum(float (&s)[kK], float p, float t, float c) {
    const float d = p - t, pa = p - c, ta = t - c;
    s[0] += fabsf(d);
    s[1] = fmaf(d, d, s[1]);
    s[2] = fmaf(pa, ta, s[2]);
    s[3] = fmaf(pa, pa, s[3]);
    s[4] = fmaf(ta, ta, s[4]);
}

// partials [nslab][B][C][5]: slab s = blockIdx.x, channel c = blockIdx.y
template <typename T, int NB, bool CLIM>
__global__ __launch_bounds__(kT) void geo_sums_kernel(const T* __restrict__ pred, const float* __restrict__ tar,
                                                      const float* __restrict__ clim, const float* __restrict__ wrow,
                                                      double* __restrict__ part, int B, int C, int H, int W) {
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
            const float* cr = CLIM ? clim + (long long)c * HW + (long long)h * W : nullptr;
            const T* pr = pred + ((long long)b0 * C + c) * HW + (long long)h * W;     // row of sample b0
            const float* tr = tar + ((long long)b0 * C + c) * HW + (long long)h * W;
            float r[NB][kK];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int k = 0; k < kK; ++k) r[b][k] = 0.f;
            // head: scalar points up to the prediction's 16-byte boundary; the row is vectorised when every stream of
            // every sample of the pass is 16-byte aligned there (wave-uniform), else walked scalar
            const int head = head_points(pr, W);
            bool vec = !CLIM || al16(cr + head);
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b < nb) vec = vec && al16(pr + b * CHW + head) && al16(tr + b * CHW + head);
            const int nv = vec ? (W - head) / kE : 0;
            const int vend = vec ? head + nv * kE : 0;        // scalar points: [0, head) and [vend, W) (all when !vec)
            for (int j = lane; j < nv; j += 64) {
                const int i = head + j * kE;
                float cv[kE];
                if (CLIM) IO<float>::load(cr + i, cv);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b < nb) {
                        float pv[kE], tv[kE];
                        IO<T>::load(pr + b * CHW + i, pv);
                        IO<float>::load(tr + b * CHW + i, tv);
#pragma unroll
                        for (int e = 0; e < kE; ++e) accum(r[b], pv[e], tv[e], CLIM ? cv[e] : 0.f);
                    }
                }
            }
            // scalar points: the head [0, head) and the tail [vend, W) of a vector row, the whole row otherwise
            const int nhead = vec ? head : 0;
            const int nscal = nhead + (W - vend);
            for (int q = lane; q < nscal; q += 64) {
                const int i = q < nhead ? q : vend + (q - nhead);
                const float cs = CLIM ? cr[i] : 0.f;
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (b < nb) accum(r[b], IO<T>::ld1(pr + b * CHW + i), tr[b * CHW + i], cs);
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

// sums[i] = sum over slabs of part[slab][i] in slab order, i over [B][C][5]
__global__ __launch_bounds__(kT) void geo_sums_finalize(const double* __restrict__ part, double* __restrict__ sums,
                                                        int nslab, long long n) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    for (int q = 0; q < nslab; ++q) v += part[(long long)q * n + i];
    sums[i] = v;
}

template <typename T, int NB>
void launch_sums(const T* pred, const float* tar, const float* clim, const float* wrow, double* part, int B, int C, int H,
                 int W, hipStream_t st) {
    const dim3 grid((unsigned)mk::ceil_div(H, kRows), (unsigned)C);
    if (clim)
        hipLaunchKernelGGL((geo_sums_kernel<T, NB, true>), grid, dim3(kT), 0, st, pred, tar, clim, wrow, part, B, C, H, W);
    else
        hipLaunchKernelGGL((geo_sums_kernel<T, NB, false>), grid, dim3(kT), 0, st, pred, tar, clim, wrow, part, B, C, H, W);
}

template <typename T>
void launch_nb(const T* pred, const float* tar, const float* clim, const float* wrow, double* part, int B, int C, int H,
               int W, hipStream_t st) {
    if (B == 1) launch_sums<T, 1>(pred, tar, clim, wrow, part, B, C, H, W, st);
    else launch_sums<T, 2>(pred, tar, clim, wrow, part, B, C, H, W, st);      // NB = 4 needs 186 VGPRs (2 waves / SIMD)
}

}  // namespace

extern "C" long long mk_geo_metric_workspace(int B, int C, int H) {
    if (B < 1 || C < 1 || H < 1) return 0;
    return (long long)mk::ceil_div(H, kRows) * B * C * kK;
}

extern "C" int mk_geo_metric_sums(const void* pred, int dtype, const float* tar, const float* clim, const float* wrow,
                                  double* workspace, double* sums, int B, int C, int H, int W, void* stream) {
    MK_REQUIRE(pred && tar && wrow && workspace && sums, "null pointer");
    MK_REQUIRE(B >= 1 && C >= 1 && C <= 65535 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE((long long)B * C * H * W < (1LL << 40), "field too large");
    MK_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(mk::aligned_to(pred, dtype == 0 ? 4 : 2), "prediction not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(tar, wrow, clim), "fp32 stream not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        launch_nb<float>((const float*)pred, tar, clim, wrow, workspace, B, C, H, W, st);
    else
        launch_nb<__hip_bfloat16>((const __hip_bfloat16*)pred, tar, clim, wrow, workspace, B, C, H, W, st);
    MK_LAUNCH_CHECK();
    const long long n = (long long)B * C * kK;
    hipLaunchKernelGGL(geo_sums_finalize, dim3((unsigned)mk::ceil_div_ll(n, kT)), dim3(kT), 0, st, workspace, sums,
                       mk::ceil_div(H, kRows), n);
    MK_LAUNCH_CHECK();
    return 0;
}
