// Forecast products of an ensemble from ONE pass over its members (mk_ens_products; include/makani_amd.h has the definition):
// ens [B][E][C][H][W] (fp32 or bf16, read as ens.hip reads it) -> out [B][K][Cs][H][W] (fp32 or bf16), K products per point of
// the selected channels: the mean, the standard deviation, order statistics with a linear interpolation (min, max, median, every
// quantile of numpy's `linear` method) and the fraction of members above or below a threshold.
//
// The decomposition, the staging and the sort are those of ens.hip (ens_tile.h): workgroup (slab of 8 rows, selected channel,
// sample), tiles of TP points, one point per thread, the E member streams staged through LDS each from its own 16-byte
// boundary, the members of a point sorted in P registers by a bitonic network with compile-time indices.  What is new:
//
// * the product table is walked at run time, so neither the sorted members nor the K results may sit in a register array that
//   a run-time value indexes (that is scratch memory).  The sorted column goes back into the thread's own LDS column, where a
//   rank is an address, and the K results go into a second LDS region [K][TP];
// * that region leaves through `unstage` with the product stride, so every output plane finds its own 16-byte boundary;
// * the table (kinds, ranks, fractions) is a kernel argument: every lane reads the same entry, the walk is scalar loads.
//
// min / max of the network drop a NaN, so it is looked for before the sort and all K values of the point are set to NaN by
// hand.  No atomics, no workspace, one writer per output element: the same bits every run; capturable.
#include "common.h"
#include "ens_tile.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)   // file scope: what is fused is written as fma, nothing else is

namespace {

constexpr int kMaxProducts = 16;
enum : int { kMean = 0, kStd = 1, kOrder = 2, kAbove = 3, kBelow = 4 };

// the product table, a kernel argument: every lane reads the same entry, so the walk over it is scalar loads
struct ProdTable {
    double fracs[kMaxProducts];
    int kinds[kMaxProducts];
    int orders[kMaxProducts];
    int K;
    int need_std, need_sort;       // a product of kind 1 / of kind 2 is in the table
};

// workgroup (slab, selected channel j, b) as in ens_sums_kernel.  LDS: tile [E][TP] (the members, then each thread's column
// sorted in place), res [K][TP] (the products of the tile, which leave through `unstage`)
template <typename T, typename O, int P, int TP>
__global__ __launch_bounds__(TP) void ens_products_kernel(const T* __restrict__ ens, O* __restrict__ out,
                                                          const int* __restrict__ chans, const float* __restrict__ thr,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          long long bstride, long long estride, long long obstride,
                                                          long long okstride, ProdTable tab, int E, int C, int Cs, int H, int W) {
    extern __shared__ float lds[];                      // tile [E][TP], res [K][TP]
    float* tile = lds;
    float* res = lds + E * TP;
    const int s = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int h0 = s * kRows;
    const int npts = (min(H, h0 + kRows) - h0) * W;
    const long long HW = (long long)H * W;
    const int c = chans ? chans[j] : j;
    const bool outside = (unsigned)c >= (unsigned)C;         // a channel the members do not have: nothing is read, NaN planes
    const T* eb = ens + b * bstride + (outside ? 0 : c) * HW + (long long)h0 * W;
    O* ob = out + b * obstride + j * HW + (long long)h0 * W;
    const bool affine = scale != nullptr;
    const float sj = affine ? scale[j] : 1.0f, tj = affine ? shift[j] : 0.0f;
    const int K = tab.K;
    for (int p0 = 0; p0 < npts; p0 += TP) {
        const int n = min(TP, npts - p0);
        __syncthreads();                                     // the tile before has left
        if (!outside) stage<T, TP>(eb + p0, estride, E, tile, n, tid);
        __syncthreads();
        if (tid < n && outside) {
            for (int i = 0; i < K; ++i) res[i * TP + tid] = NAN;
        } else if (tid < n) {
            float* col = tile + tid;                         // member e of this point: col[e * TP]
            bool bad = false;
            double sm = 0.0;
#pragma unroll 4
            for (int e = 0; e < E; ++e) {                    // in member order
                const float xf = col[e * TP];
                bad = bad || (xf != xf);
                sm += (double)xf;
            }
            const double m = sm / (double)E;                 // a division: E equal members x give m = x exactly
            double sd = 0.0;
            if (tab.need_std) {
                double sv = 0.0;
#pragma unroll 4
                for (int e = 0; e < E; ++e) {
                    const double d = (double)col[e * TP] - m;
                    sv = fma(d, d, sv);
                }
                sd = sqrt(sv / (double)(E - 1));
            }
            if (tab.need_sort) {
                int En = E;                                  // as in ens_sums_kernel (ens.hip): the pad conditions are not hoisted
                asm volatile("" : "+s"(En));
                float x[P];
#pragma unroll
                for (int e = 0; e < P; ++e) x[e] = e < En ? col[(e < En ? e : 0) * TP] : INFINITY;
                sort_ascending<P>(x);
#pragma unroll
                for (int e = 0; e < P; ++e)                  // back into the thread's own column: rank k is col[k * TP]
                    if (e < En) col[e * TP] = x[e];
            }
            for (int i = 0; i < K; ++i) {
                const int kind = tab.kinds[i];
                float v;
                if (kind == kMean) {
                    v = (float)m;
                } else if (kind == kStd) {
                    v = (float)sd;
                } else if (kind == kOrder) {
                    const int k = tab.orders[i];
                    const double t = tab.fracs[i];
                    const float lo = col[k * TP];
                    v = lo;
                    if (t != 0.0) {
                        const float hi = col[(k + 1) * TP];
                        v = (float)fma(t, (double)hi - (double)lo, (double)lo);
                    }
                } else {
                    const float th = thr[(long long)i * Cs + j];
                    int cnt = 0;
                    if (kind == kAbove) {
#pragma unroll 4
                        for (int e = 0; e < E; ++e) cnt += col[e * TP] > th ? 1 : 0;
                    } else {
#pragma unroll 4
                        for (int e = 0; e < E; ++e) cnt += col[e * TP] < th ? 1 : 0;
                    }
                    v = th != th ? NAN : (float)cnt / (float)E;
                }
                if (affine && kind <= kOrder) {
                    v = v * sj;
                    if (kind != kStd) v = v + tj;
                }
                res[i * TP + tid] = bad ? NAN : v;
            }
        }
        __syncthreads();
        unstage<O, TP>(res, ob + p0, okstride, K, n, tid);
    }
}

struct ProdArgs {
    const void* ens;
    void* out;
    const int* chans;
    const float *thr, *scale, *shift;
    long long bstride, estride, obstride, okstride;
    int B, E, C, Cs, H, W;
    hipStream_t st;
};

template <typename T, typename O, int P>
void launch_products_p(const ProdArgs& a, const ProdTable& tab) {
    constexpr int TP = tile_points<P>();
    const size_t lds = (size_t)(a.E + tab.K) * TP * 4;       // at most (32 + 16) * 256 * 4 = 48 KB
    hipLaunchKernelGGL((ens_products_kernel<T, O, P, TP>), dim3((unsigned)mk::ceil_div(a.H, kRows), (unsigned)a.Cs, (unsigned)a.B),
                       dim3(TP), lds, a.st, (const T*)a.ens, (O*)a.out, a.chans, a.thr, a.scale, a.shift, a.bstride, a.estride,
                       a.obstride, a.okstride, tab, a.E, a.C, a.Cs, a.H, a.W);
}

template <typename T, typename O>
void launch_products(const ProdArgs& a, const ProdTable& tab) {
    if (a.E <= 2) launch_products_p<T, O, 2>(a, tab);
    else if (a.E <= 4) launch_products_p<T, O, 4>(a, tab);
    else if (a.E <= 8) launch_products_p<T, O, 8>(a, tab);
    else if (a.E <= 16) launch_products_p<T, O, 16>(a, tab);
    else if (a.E <= 32) launch_products_p<T, O, 32>(a, tab);
    else launch_products_p<T, O, 64>(a, tab);
}

}  // namespace

extern "C" int mk_ens_products(const void* ens, int dtype, long long bstride, long long estride, void* out, int out_dtype,
                               long long obstride, long long okstride, const int* chans, const int* kinds, const int* orders,
                               const double* fracs, const float* thr, const float* scale, const float* shift, int B, int E, int C,
                               int Cs, int K, int H, int W, void* stream) {
    MK_REQUIRE(ens && out && kinds && orders && fracs, "null pointer");
    MK_REQUIRE((dtype == 0 || dtype == 1) && (out_dtype == 0 || out_dtype == 1), "dtype and out_dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(B >= 1 && C >= 1 && Cs >= 1 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE(E >= 2 && E <= kMaxE, "E outside 2 ... 64 (the members of a point are sorted in registers)");
    MK_REQUIRE(K >= 1 && K <= kMaxProducts, "K outside 1 ... 16");
    MK_REQUIRE(chans || Cs == C, "without a channel list Cs must equal C");
    MK_REQUIRE(B <= 65535 && Cs <= 65535, "B or Cs beyond the grid range");
    MK_REQUIRE((long long)kRows * W <= 0x7fffffffLL, "a workgroup's points (8 rows of W) beyond the 32-bit range");
    const long long chw = (long long)C * H * W, ochw = (long long)Cs * H * W;
    MK_REQUIRE(chw < (1LL << 40) && ochw < (1LL << 40), "field too large");
    MK_REQUIRE(estride >= chw && bstride >= chw, "a member's [C][H][W] block must be contiguous: strides below C * H * W");
    MK_REQUIRE(okstride >= ochw && obstride >= ochw, "a product's [Cs][H][W] block must be contiguous: strides below Cs * H * W");
    MK_REQUIRE(estride < (1LL << 44) && bstride < (1LL << 44) && okstride < (1LL << 44) && obstride < (1LL << 44), "stride too large");
    MK_REQUIRE(bstride >= (long long)E * estride || estride >= (long long)B * bstride || B == 1,
               "members of different samples overlap: need bstride >= E * estride or estride >= B * bstride");
    MK_REQUIRE(obstride >= (long long)K * okstride || okstride >= (long long)B * obstride || B == 1,
               "products of different samples overlap: need obstride >= K * okstride or okstride >= B * obstride");
    MK_REQUIRE(mk::aligned_to(ens, dtype == 0 ? 4 : 2) && mk::aligned_to(out, out_dtype == 0 ? 4 : 2),
               "ensemble or products not aligned to their element");
    MK_REQUIRE(mk::aligned<4>(chans, thr, scale, shift), "32-bit table not 4-byte aligned");
    MK_REQUIRE((scale == nullptr) == (shift == nullptr), "scale and shift come together or not at all");
    ProdTable tab = {};
    tab.K = K;
    for (int i = 0; i < K; ++i) {
        const int kind = kinds[i];
        MK_REQUIRE(kind >= kMean && kind <= kBelow, "product kind outside 0 ... 4");
        if (kind == kOrder) {
            const int k = orders[i];
            const double t = fracs[i];
            MK_REQUIRE(t >= 0.0 && t < 1.0, "an order statistic's fraction must lie in [0, 1)");
            MK_REQUIRE(k >= 0 && k < E && (t == 0.0 || k < E - 1), "an order statistic's rank outside 0 ... E - 1 (E - 2 with a fraction)");
            tab.orders[i] = k;
            tab.fracs[i] = t;
            tab.need_sort = 1;
        } else if (kind == kAbove || kind == kBelow) {
            MK_REQUIRE(thr, "a count product needs thresholds");
        } else if (kind == kStd) {
            tab.need_std = 1;
        }
        tab.kinds[i] = kind;
    }
    const ProdArgs a = {ens, out, chans, thr, scale, shift, bstride, estride, obstride, okstride, B, E, C, Cs, H, W, (hipStream_t)stream};
    if (dtype == 0 && out_dtype == 0) launch_products<float, float>(a, tab);
    else if (dtype == 0) launch_products<float, __hip_bfloat16>(a, tab);
    else if (out_dtype == 0) launch_products<__hip_bfloat16, float>(a, tab);
    else launch_products<__hip_bfloat16, __hip_bfloat16>(a, tab);
    MK_LAUNCH_CHECK();
    return 0;
}
