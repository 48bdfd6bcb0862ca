// Per-channel value histograms of a dataset (data_process/get_histograms.py, its second sweep) from ONE pass over a batch
// x [T][C][H][W] of fp32 samples.  Per channel c the caller gives an edge table e = edges[c] of nbins + 1 strictly increasing
// fp64 values, and the counts are the ones the TABLE defines, as np.histogram's are:
//   bin i holds e[i] <= x < e[i + 1], the last bin is closed on the right, points outside [e[0], e[nbins]] and NaNs are not
//   binned; they are counted per channel in outside [C][3] = below, above, NaN.
// A point's bin is guessed by arithmetic, (x - e[0]) nbins / (e[nbins] - e[0]) in fp32, and then corrected against the
// table, so the result does not depend on how good the guess is (a table that is not uniform costs iterations, not counts).
//
// The table is compared in fp32 without losing a bit: for an fp32 x and an fp64 e, x >= e holds exactly when x >= up(e), the
// smallest fp32 that is not below e, and x <= e exactly when x <= down(e).  So LDS holds f[i] = up(e[i]) (half the bytes of
// the fp64 table, fp32 compares); f may repeat a value where two edges lie between two neighbouring fp32 numbers, and such a
// bin holds no fp32 point under either table.
//
// Decomposition: workgroup (slab, c) takes kRows latitude rows of channel c and all T samples; the channel's table and R
// replicas of a uint32 bin array live in LDS.  Every (sample, row) pair is a stream of its own: a wave walks it as a scalar
// head up to ITS 16-byte boundary, an 8-wide body (16-byte accesses) and a scalar tail, so samples whose alignments differ
// (C H W no multiple of four) are vectorised all the same -- a histogram couples no two samples, unlike stats.hip.
//
// Contention.  Weather fields are smooth: the lanes of a wave, and a lane's 8 consecutive points, hit the same few bins, and
// LDS atomics on one address serialise.  Two measures (A/B in DESIGN section 36): lane l adds to replica l % R, the replicas
// an odd number of words apart, so 32 lanes that hit ONE bin hit 32 banks; and a lane merges runs of equal indices among
// its 8 points into one add.  R is the largest power of two <= 32 that keeps table + replicas within kLdsBudget, the LDS at
// which 8 workgroups still fit a CU: replicas that cost occupancy lost more than they won.
//
// Flush: the replicas are folded, and the non-zero bins are added to counts with device-scope 64-bit integer atomics.
// Integer addition commutes and cannot round, so the result is the same bits every run and for every split of the rows:
// that is why atomics are acceptable here, where the floating-point sums of this library avoid them.  No workspace, one
// launch, capturable.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <cstdint>

#ifndef MK_HIST_MERGE
#define MK_HIST_MERGE 1            // merge runs of equal indices among a lane's points (0: one add per point; A/B builds only)
#endif
#ifndef MK_HIST_MAX_REPLICAS
#define MK_HIST_MAX_REPLICAS 32    // upper limit of R (a power of two; A/B builds only)
#endif
#ifndef MK_HIST_ROWS
#define MK_HIST_ROWS 4             // latitude rows per workgroup (A/B builds only)
#endif

namespace {

constexpr int kT = 256;            // threads per workgroup (4 waves)
constexpr int kE = mk::sio::kVec;  // points per lane per step of the vector body
constexpr int kRows = MK_HIST_ROWS;  // latitude rows per workgroup: the table load, the zero fill and the flush are paid per workgroup
constexpr int kMaxBins = 4096;     // table (4097 fp32) + one bin array (4097 words) = 32,776 bytes, + 48 static: four workgroups per CU of 160 KB
constexpr int kLdsBudget = 20 * 1024;   // of table + replicas where R > 1: 8 workgroups (all 32 waves) per CU of 160 KB
constexpr int kMaxReplicas = MK_HIST_MAX_REPLICAS;
constexpr bool kMerge = MK_HIST_MERGE != 0;
static_assert(kMaxReplicas >= 1 && (kMaxReplicas & (kMaxReplicas - 1)) == 0, "a lane finds its replica as lane & (R - 1)");
static_assert(kRows >= 1, "rows per workgroup");

using mk::sio::al16;
using mk::sio::head_points;
using mk::sio::IO;

// words between two replicas: odd, so one bin of replicas 0 ... 31 falls into 32 different banks
__host__ __device__ inline int replica_stride(int nbins) { return nbins | 1; }

inline int replicas_for(int nbins) {
    int r = 1;
    while (2 * r <= kMaxReplicas &&
           (long long)(nbins + 1) * 4 + 2LL * r * replica_stride(nbins) * 4 <= kLdsBudget)
        r *= 2;
    return r;
}

struct Outside {
    unsigned int below, above, nan;
};

// the smallest fp32 >= e and the largest fp32 <= e (e not NaN; beyond the fp32 range they are +-inf or +-FLT_MAX)
__device__ __forceinline__ float f32_up(double e) {
    float f = (float)e;                                  // to nearest: at most one step below e
    if ((double)f < e) {
        const unsigned int b = __float_as_uint(f);
        f = (f == 0.0f) ? __uint_as_float(1u) : __uint_as_float(f > 0.0f ? b + 1u : b - 1u);
    }
    return f;
}
__device__ __forceinline__ float f32_down(double e) { return -f32_up(-e); }

// the bin of x (f[0] <= x <= down(e[nbins])): the arithmetic guess, clamped, then corrected against the table.  Both loops
// end for any table: the first at g = 0 at the latest, the second at g = nbins - 1; for a non-decreasing f they end at the
// one g with f[g] <= x < f[g + 1] (or the last bin).
__device__ __forceinline__ int bin_of(float x, const float* f, int nbins, float f0, float scale) {
    const float t = fminf(fmaxf((x - f0) * scale, 0.0f), (float)(nbins - 1));      // fmaxf drops a NaN guess
    int g = (int)t;
    while (g > 0 && x < f[g]) --g;
    while (g < nbins - 1 && x >= f[g + 1]) ++g;
    return g;
}

// N consecutive points of one lane: classify, bin, add to the lane's replica
template <int N>
__device__ __forceinline__ void add_points(const float (&x)[N], const float* f, unsigned int* bins, int nbins, float f0,
                                           float fn, float scale, Outside& o) {
    int run = -1;                   // the bin of the run that is open, -1: none
    unsigned int len = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float v = x[i];
        int g = -1;
        if (v != v) ++o.nan;
        else if (!(v >= f0)) ++o.below;
        else if (!(v <= fn)) ++o.above;
        else g = bin_of(v, f, nbins, f0, scale);
        if (!kMerge) {
            if (g >= 0) atomicAdd(bins + g, 1u);
        } else if (g == run) {
            ++len;
        } else {
            if (run >= 0) atomicAdd(bins + run, len);
            run = g;
            len = 1;
        }
    }
    if (kMerge && run >= 0) atomicAdd(bins + run, len);
}

__global__ __launch_bounds__(kT) void field_hist_kernel(const float* __restrict__ x, const double* __restrict__ edges,
                                                        unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ outside, int nbins, int R, int T,
                                                        int C, int H, int W) {
    extern __shared__ float lds[];                       // f [nbins + 1] fp32, then R replicas of uint32 bins, `stride` apart
    __shared__ unsigned int red[kT / 64][3];
    float* f = lds;
    unsigned int* bins = reinterpret_cast<unsigned int*>(lds + nbins + 1);
    const int stride = replica_stride(nbins);
    const int s = blockIdx.x, c = blockIdx.y;
    const int h0 = s * kRows, nrows = min(H, h0 + kRows) - h0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long HW = (long long)H * W, CHW = (long long)C * HW;
    const double* ec = edges + (long long)c * (nbins + 1);
    for (int i = threadIdx.x; i <= nbins; i += kT) f[i] = f32_up(ec[i]);
    for (int i = threadIdx.x; i < R * stride; i += kT) bins[i] = 0u;
    __syncthreads();
    const float f0 = f[0], fn = f32_down(ec[nbins]);     // x >= e[0] as x >= f0, x <= e[nbins] as x <= fn
    const float scale = (float)nbins / (fn - f0);
    unsigned int* mine = bins + (lane & (R - 1)) * stride;
    Outside o = {0u, 0u, 0u};
    // stream q = (sample q / nrows, row h0 + q % nrows), one wave per stream
    for (int q = wave; q < nrows * T; q += kT / 64) {
        const int t = q / nrows, h = h0 + q % nrows;
        const float* xr = x + t * CHW + (long long)c * HW + (long long)h * W;
        const int head = head_points(xr, W);
        const int nv = (W - head) / kE;
        const int vend = head + nv * kE;                 // scalar points: [0, head) and [vend, W)
        for (int j = lane; j < nv; j += 64) {
            float v[kE];
            IO<float>::load(xr + head + j * kE, v);
            add_points<kE>(v, f, mine, nbins, f0, fn, scale, o);
        }
        const int nscal = head + (W - vend);
        for (int p = lane; p < nscal; p += 64) {
            const float v[1] = {xr[p < head ? p : vend + (p - head)]};
            add_points<1>(v, f, mine, nbins, f0, fn, scale, o);
        }
    }
    // the three outside counts: lanes by shuffle, the four waves through LDS (a workgroup sees at most 2^32 - 1 points)
    unsigned int v[3] = {o.below, o.above, o.nan};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v[k] += __shfl_down(v[k], d, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) red[wave][k] = v[k];
    }
    __syncthreads();                                     // also: every add to the replicas is done
    for (int b = threadIdx.x; b < nbins; b += kT) {
        unsigned int n = 0u;
        for (int r = 0; r < R; ++r) n += bins[r * stride + b];
        if (n) atomicAdd(counts + (long long)c * nbins + b, (unsigned long long)n);
    }
    if (outside && threadIdx.x < 3) {
        unsigned int n = 0u;
#pragma unroll
        for (int w = 0; w < kT / 64; ++w) n += red[w][threadIdx.x];
        if (n) atomicAdd(outside + (long long)c * 3 + threadIdx.x, (unsigned long long)n);
    }
}

}  // namespace

extern "C" int mk_field_hist(const float* x, const double* edges, long long* counts, long long* outside, int nbins, int T,
                             int C, int H, int W, void* stream) {
    MK_REQUIRE(x && edges && counts, "null pointer");
    MK_REQUIRE(nbins >= 1 && nbins <= kMaxBins, "nbins outside 1 ... 4096 (the edge table and one bin array take 32,776 bytes of LDS there)");
    MK_REQUIRE(T >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE(C <= 65535 && (long long)C * H * W <= 0x7fffffffLL, "C * H * W beyond the 32-bit grid range");
    MK_REQUIRE((long long)(H < kRows ? H : kRows) * W * T <= 0xffffffffLL, "a workgroup's points (rows * W * T) beyond a 32-bit bin");
    MK_REQUIRE(mk::aligned<4>(x), "32-bit stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(edges, counts, outside), "64-bit stream not 8-byte aligned");
    const int R = replicas_for(nbins);
    const size_t lds = (size_t)(nbins + 1) * 4 + (size_t)R * replica_stride(nbins) * 4;
    hipLaunchKernelGGL(field_hist_kernel, dim3((unsigned)mk::ceil_div(H, kRows), (unsigned)C), dim3(kT), lds, (hipStream_t)stream, x,
                       edges, reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(outside), nbins,
                       R, T, C, H, W);
    MK_LAUNCH_CHECK();
    return 0;
}
