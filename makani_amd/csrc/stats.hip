// Dataset statistics (data_process/get_stats.py: global means / stds, mins, maxs, the climatology, the time-difference
// means / stds and the wind-magnitude variance) from ONE pass over a batch x [T][C][H][W] of consecutive fp32 samples.
// Per channel c, with d = x - pivot[c] and e = x_t - x_{t-1} formed in fp64 and w = wrow[h]:
//   sums [C][4] = sum w d, sum w d^2, sum w e, sum w e^2        minmax [C][2] = min, max (NaN if the channel holds one)
//   tsum [C][H][W] += x_0, += x_1, ... in ascending t (fp64, one owner per point)
//   wsums [n_wind][2] = sum m, sum m^2, m = sqrtf(u u + v v) in fp32, every operation rounded on its own
//
// Decomposition: workgroup (slab, c) takes kRows latitude rows of channel c; each wave walks whole rows, a lane 8
// consecutive points per step, and the samples are the INNER loop: the time sum of the lane's points and their previous
// values stay in registers, so tsum is read and written once per call and x once.  All sums are fp64: a lane adds the
// unweighted terms of a row, folds them into its slab sums with the row's weight at the end of the row (as metrics.hip),
// the lanes fold by shuffle, the four waves through LDS in wave order, and each workgroup writes a workspace slot of its
// own; stats_finalize adds the slabs in a fixed order (the scheme of slab_finalize_kernel, stream_io.h, which only adds:
// min and max need a fold of their own, so the three outputs share one finish here).  No atomics: the same bits every run.
//
// The workgroup of channel wind_u[k] also reads channel wind_v[k] at its points (the v channels of the pairs are read
// twice per call).
//
// Any W: a row is walked as a scalar head up to the 16-byte boundary of the first sample, an 8-wide body (16-byte
// accesses) and a scalar tail; when the streams of a row disagree on their alignment the row runs scalar.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <cstdint>

namespace {

constexpr int kT = 256;            // threads per workgroup (4 waves)
constexpr int kE = mk::sio::kVec;  // points per lane per step of the vector body
constexpr int kRows = 8;           // latitude rows per workgroup (16 rows ran 3-5 % slower on an MI355X)
constexpr int kS = 4;              // weighted sums per channel
constexpr int kR = 8;              // values a workgroup reduces: 4 sums, 2 wind sums, min, max

using mk::sio::al16;
using mk::sio::head_points;
using mk::sio::IO;

// min / max that keep a NaN once they met one (v_min_f32 / v_max_f32 drop it)
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// sqrtf(u u + v v): each product, the sum and the root an fp32 rounding of its own (no fma), the root correctly rounded
__device__ __forceinline__ float wind_mag(float u, float v) {
#pragma clang fp contract(off)
    const float uu = u * u;
    const float vv = v * v;
    const float s = uu + vv;
    return sqrtf(s);
}

// N points at p: N = kE through 16-byte accesses (p 16-byte aligned), N = 1 one element
template <int N> struct Pt;
template <> struct Pt<kE> {
    static __device__ __forceinline__ void ldx(const float* p, float (&v)[kE]) { IO<float>::load(p, v); }
    static __device__ __forceinline__ void ldt(const double* p, double (&v)[kE]) {
#pragma unroll
        for (int i = 0; i < kE / 2; ++i) {
            const double2 a = reinterpret_cast<const double2*>(p)[i];
            v[2 * i] = a.x;
            v[2 * i + 1] = a.y;
        }
    }
    static __device__ __forceinline__ void stt(double* p, const double (&v)[kE]) {
#pragma unroll
        for (int i = 0; i < kE / 2; ++i) reinterpret_cast<double2*>(p)[i] = make_double2(v[2 * i], v[2 * i + 1]);
    }
};
template <> struct Pt<1> {
    static __device__ __forceinline__ void ldx(const float* p, float (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void ldt(const double* p, double (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void stt(double* p, const double (&v)[1]) { *p = v[0]; }
};

// what a lane carries: the unweighted sums of the row it walks, the wind sums, min and max
struct Lane {
    double r[kS];
    double wm, wmm;
    float mn, mx;
};

template <int N, bool DIFF, bool WIND>
__device__ __forceinline__ void accum(Lane& a, const float (&x)[N], float (&xp)[N], const float (&v)[N], double (&ts)[N],
                                      double pv) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double dx = (double)x[i];
        ts[i] += dx;
        const double d = dx - pv;
        a.r[0] += d;
        a.r[1] = fma(d, d, a.r[1]);
        if (DIFF) {
            const double e = dx - (double)xp[i];
            a.r[2] += e;
            a.r[3] = fma(e, e, a.r[3]);
        }
        a.mn = nan_min(a.mn, x[i]);
        a.mx = nan_max(a.mx, x[i]);
        if (WIND) {
            const double m = (double)wind_mag(x[i], v[i]);
            a.wm += m;
            a.wmm = fma(m, m, a.wmm);
        }
        xp[i] = x[i];
    }
}

// all T samples of the N points at xr (sample 0); pr: the sample before the first at these points, or null; vr: the
// pair's v channel of sample 0 (WIND); tr: the time sum
template <int N, bool WIND>
__device__ __forceinline__ void walk(Lane& a, const float* xr, const float* pr, const float* vr, double* tr, long long CHW,
                                     int T, double pv) {
    double ts[N];
    float x[N], xp[N], v[N];
    Pt<N>::ldt(tr, ts);
    Pt<N>::ldx(xr, x);
    if (WIND) Pt<N>::ldx(vr, v);
    if (pr) {
        Pt<N>::ldx(pr, xp);
        accum<N, true, WIND>(a, x, xp, v, ts, pv);
    } else {
        accum<N, false, WIND>(a, x, xp, v, ts, pv);
    }
    // not unrolled: two samples in flight cost 4 VGPRs over 128 and a wave per SIMD, and ran 9 % slower
#pragma unroll 1
    for (int t = 1; t < T; ++t) {
        Pt<N>::ldx(xr + t * CHW, x);
        if (WIND) Pt<N>::ldx(vr + t * CHW, v);
        accum<N, true, WIND>(a, x, xp, v, ts, pv);
    }
    Pt<N>::stt(tr, ts);
}

// workspace: psum [nslab][C][4], then pmm [nslab][C][2] (min, max, exact in fp64), then pw [nslab][n_wind][2]
template <bool WIND>
__global__ __launch_bounds__(kT) void field_stats_kernel(const float* __restrict__ x, const float* __restrict__ prev,
                                                         const float* __restrict__ pivot, const float* __restrict__ wrow,
                                                         double* __restrict__ psum, double* __restrict__ pmm,
                                                         double* __restrict__ pw, double* __restrict__ tsum,
                                                         const int* __restrict__ wind_u, const int* __restrict__ wind_v,
                                                         int n_wind, int T, int C, int H, int W) {
    __shared__ double red[kT / 64][kR];
    const int s = blockIdx.x, c = blockIdx.y;
    const int h0 = s * kRows, h1 = min(H, h0 + kRows);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long HW = (long long)H * W, CHW = (long long)C * HW;
    const double pv = pivot ? (double)pivot[c] : 0.0;
    // the first pair whose u channel this is (workgroup-uniform); a v outside [0, C) is no pair: stats_finalize says so
    int kw = -1, cv = 0;
    if (WIND) {
        for (int k = n_wind - 1; k >= 0; --k)
            if (wind_u[k] == c) kw = k;
        if (kw >= 0) {
            cv = wind_v[kw];
            if (cv < 0 || cv >= C) kw = -1;
        }
    }
    Lane a;
#pragma unroll
    for (int k = 0; k < kS; ++k) a.r[k] = 0.0;
    a.wm = a.wmm = 0.0;
    a.mn = __builtin_inff();
    a.mx = -__builtin_inff();
    double acc[kS] = {0.0, 0.0, 0.0, 0.0};
    for (int h = h0 + wave; h < h1; h += kT / 64) {
        const long long ro = (long long)c * HW + (long long)h * W;
        const float* xr = x + ro;
        const float* pr = prev ? prev + ro : nullptr;
        const float* vr = x + (long long)cv * HW + (long long)h * W;
        double* tr = tsum + ro;
        // head: scalar points up to the 16-byte boundary of sample 0; the row is vectorised when every stream is 16-byte
        // aligned there (wave-uniform; the samples' offsets t * CHW repeat modulo 16 bytes with period 4), else scalar
        const int head = head_points(xr, W);
        bool vec = al16(tr + head) && (!pr || al16(pr + head)) && (!(WIND && kw >= 0) || al16(vr + head));
        for (int t = 1; t < min(T, 4); ++t) vec = vec && al16(xr + t * CHW + head);
        const int nv = vec ? (W - head) / kE : 0;
        const int vend = vec ? head + nv * kE : 0;            // scalar points: [0, head) and [vend, W) (all when !vec)
        for (int j = lane; j < nv; j += 64) {
            const int i = head + j * kE;
            if (WIND && kw >= 0) walk<kE, true>(a, xr + i, pr ? pr + i : nullptr, vr + i, tr + i, CHW, T, pv);
            else walk<kE, false>(a, xr + i, pr ? pr + i : nullptr, nullptr, tr + i, CHW, T, pv);
        }
        const int nhead = vec ? head : 0;
        const int nscal = nhead + (W - vend);
        for (int q = lane; q < nscal; q += 64) {
            const int i = q < nhead ? q : vend + (q - nhead);
            if (WIND && kw >= 0) walk<1, true>(a, xr + i, pr ? pr + i : nullptr, vr + i, tr + i, CHW, T, pv);
            else walk<1, false>(a, xr + i, pr ? pr + i : nullptr, nullptr, tr + i, CHW, T, pv);
        }
        const double w = (double)wrow[h];
#pragma unroll
        for (int k = 0; k < kS; ++k) {
            acc[k] = fma(a.r[k], w, acc[k]);
            a.r[k] = 0.0;
        }
    }
    // fixed-order reduction: lanes by shuffle, then the four waves in order
    double v[kR] = {acc[0], acc[1], acc[2], acc[3], a.wm, a.wmm, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.mn = nan_min(a.mn, __shfl_down(a.mn, o, 64));
        a.mx = nan_max(a.mx, __shfl_down(a.mx, o, 64));
    }
    v[6] = (double)a.mn;
    v[7] = (double)a.mx;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kR; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double o[kR];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            o[k] = 0.0;
#pragma unroll
            for (int q = 0; q < kT / 64; ++q) o[k] += red[q][k];
        }
        float mn = (float)red[0][6], mx = (float)red[0][7];
#pragma unroll
        for (int q = 1; q < kT / 64; ++q) {
            mn = nan_min(mn, (float)red[q][6]);
            mx = nan_max(mx, (float)red[q][7]);
        }
        // a NaN in the slab: every sum of the channel is NaN (the difference sums would miss one at t = 0 without prev)
        const bool bad = mn != mn;
        const long long slot = (long long)s * C + c;
#pragma unroll
        for (int k = 0; k < kS; ++k) psum[slot * kS + k] = bad ? (double)mn : o[k];
        pmm[slot * 2] = (double)mn;
        pmm[slot * 2 + 1] = (double)mx;
        if (WIND && kw >= 0) {
            pw[((long long)s * n_wind + kw) * 2] = o[4];
            pw[((long long)s * n_wind + kw) * 2 + 1] = o[5];
        }
    }
}

// one wave per output value: lane q folds slabs q, q + 64, ... in order, then the lanes fold by the same shuffle tree
// every time.  Values [0, 4C) are the sums, [4C, 6C) min / max, the rest the wind sums.
__global__ __launch_bounds__(kT) void stats_finalize(const double* __restrict__ psum, const double* __restrict__ pmm,
                                                     const double* __restrict__ pw, double* __restrict__ sums,
                                                     float* __restrict__ minmax, double* __restrict__ wsums,
                                                     const int* __restrict__ wind_u, const int* __restrict__ wind_v,
                                                     int n_wind, int nslab, int C) {
    const int i = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    const int nS = kS * C, nM = 2 * C, nW = 2 * n_wind;
    if (i >= nS + nM + nW) return;                            // wave-uniform
    const int lane = threadIdx.x & 63;
    if (i < nS) {
        double v = 0.0;
        for (int q = lane; q < nslab; q += 64) v += psum[(long long)q * nS + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sums[i] = v;
    } else if (i < nS + nM) {
        const int j = i - nS;
        const bool mx = j & 1;
        float v = mx ? -__builtin_inff() : __builtin_inff();
        for (int q = lane; q < nslab; q += 64) {
            const float p = (float)pmm[(long long)q * nM + j];
            v = mx ? nan_max(v, p) : nan_min(v, p);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float p = __shfl_down(v, o, 64);
            v = mx ? nan_max(v, p) : nan_min(v, p);
        }
        if (lane == 0) minmax[j] = v;
    } else {
        const int j = i - nS - nM, k = j >> 1;
        // a pair no workgroup served (an index outside [0, C), or a u channel an earlier pair names) has no sums: NaN
        const int cu = wind_u[k], cv = wind_v[k];
        bool served = cu >= 0 && cu < C && cv >= 0 && cv < C;
        for (int p = 0; p < k; ++p) served = served && wind_u[p] != cu;
        double v = 0.0;
        if (served)
            for (int q = lane; q < nslab; q += 64) v += pw[(long long)q * nW + j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) wsums[j] = served ? v : __builtin_nan("");
    }
}

}  // namespace

extern "C" long long mk_field_stats_workspace(int C, int H, int n_wind) {
    if (C < 1 || H < 1 || n_wind < 0) return 0;
    return (long long)mk::ceil_div(H, kRows) * ((long long)C * (kS + 2) + 2LL * n_wind);
}

extern "C" int mk_field_stats(const float* x, const float* prev, const float* pivot, const float* wrow, double* workspace,
                              double* sums, float* minmax, double* tsum, const int* wind_u, const int* wind_v, int n_wind,
                              double* wsums, int T, int C, int H, int W, void* stream) {
    MK_REQUIRE(x && wrow && workspace && sums && minmax && tsum, "null pointer");
    MK_REQUIRE(n_wind >= 0, "negative number of wind pairs");
    MK_REQUIRE(n_wind == 0 || (wind_u && wind_v && wsums), "wind pairs without wind_u, wind_v and wsums");
    MK_REQUIRE(T >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE(C <= 65535 && (long long)C * H * W <= 0x7fffffffLL, "C * H * W beyond the 32-bit grid range");
    MK_REQUIRE(mk::aligned<4>(x, prev, pivot, wrow, minmax, wind_u, wind_v), "32-bit stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(workspace, sums, tsum, wsums), "fp64 stream not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nslab = mk::ceil_div(H, kRows);
    double* psum = workspace;
    double* pmm = psum + (long long)nslab * C * kS;
    double* pw = pmm + (long long)nslab * C * 2;
    const dim3 grid((unsigned)nslab, (unsigned)C);
    if (n_wind > 0)
        hipLaunchKernelGGL(field_stats_kernel<true>, grid, dim3(kT), 0, st, x, prev, pivot, wrow, psum, pmm, pw, tsum, wind_u,
                           wind_v, n_wind, T, C, H, W);
    else
        hipLaunchKernelGGL(field_stats_kernel<false>, grid, dim3(kT), 0, st, x, prev, pivot, wrow, psum, pmm, pw, tsum, wind_u,
                           wind_v, n_wind, T, C, H, W);
    MK_LAUNCH_CHECK();
    const int nval = (kS + 2) * C + 2 * n_wind;
    hipLaunchKernelGGL(stats_finalize, dim3((unsigned)mk::ceil_div(nval, kT / 64)), dim3(kT), 0, st, psum, pmm, pw, sums, minmax,
                       wsums, wind_u, wind_v, n_wind, nslab, C);
    MK_LAUNCH_CHECK();
    return 0;
}
