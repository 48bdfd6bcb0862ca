// Ensemble scores from ONE pass over an ensemble ens [B][E][C][H][W] (fp32 or bf16; a member's [C][H][W] block contiguous,
// batch and member strides in elements) and a target tar [B][C][H][W] (fp32).  Per point, with x_e the members and y the
// target widened to fp64 (exact), every value is formed in fp64:
//   a = (1/E) sum_e |x_e - y|
//   g = (1/E^2) sum_e sum_f |x_e - x_f|  =  (2/E^2) sum_k (2k - E - 1) x_(k),  k = 1 ... E over the members sorted ascending
//   m = (1/E) sum_e x_e,   q = (m - y)^2,   v = (1/(E - 1)) sum_e (x_e - m)^2   (two-pass about m)
//   r = #{e : x_e < y}     (a tie with the target counts as not less)
// and the pass gives sums [B][C][4] = sum_hw wrow[h] (a, g, q, v), ranks [C][E + 1] += the histogram of r, skipped [C] += the
// points where the target or a member is NaN.  Such a point is not ranked and makes the four sums of its (b, c) NaN.
// CRPS = a - g / 2 (the kernel form of the integral of (F_ens - 1{y <= x})^2), fair CRPS = a - g E / (2 (E - 1)).
//
// The sort.  Members are fp32 (bf16 widens exactly), so they are ORDERED in fp32 without losing a bit and only the weighted
// sum over the order is fp64.  A thread keeps the E members of its point in P registers, P the power of two >= E, padded
// with +inf, and sorts them with a bitonic network whose indices are all compile-time (no scratch memory): the pads end up
// behind the members and the rank weights never touch them.  v_min / v_max return the other operand for a NaN, so a NaN
// would vanish in the network: it is looked for before the sort, and the point's four values are set to NaN by hand.
//
// Decomposition: workgroup (slab, c, b) takes kRows latitude rows of channel c of sample b, which are kRows * W consecutive
// points in every member and in the target, and walks them in tiles of TP points, one point per thread.  A tile is staged
// through LDS, [E + 1][TP] fp32 (members, then the target): stream by stream, each from ITS OWN 16-byte boundary -- a scalar
// head, a body of 16-byte accesses, a scalar tail -- so members whose alignments disagree (C H W or a stride no multiple of
// four) are vectorised all the same, and the (stream, vector) pairs are dealt over all threads.  Then thread t reads column t
// (consecutive lanes, consecutive banks).  Nothing outside the tile's points is read, so a member stride may leave gaps.
//
// Sums: a thread adds w * value in fp64 over its points; lanes fold by shuffle, the waves in order, and the workgroup writes
// its four sums, scaled by 1/E, 2/E^2, 1, 1/(E - 1), to a workspace slot of its own; a finish adds the slabs in a fixed order.
// No floating-point atomics: the same bits every run.  Ranks go to R replicas of a uint32 bin array in LDS (lane -> replica,
// an odd number of words apart) and from there to `ranks` with device-scope 64-bit INTEGER atomics, which commute and do
// not round: the counts are the same every run and for every split of the rows (as hist.hip).  Capturable: two launches, no
// allocation, synchronisation or host copy.
//
// The training loss a - (kappa / 2) g needs the gradient of (sum w a, sum w g) with respect to the members: mk_ens_crps_bwd,
// one launch of the same decomposition and staging.  Per point d|x_e - y|/dx_e = sgn(x_e - y) and
// d sum_ef |x_e - x_f| / dx_e = 2 (L_e - G_e), L_e and G_e the members below and above x_e, counted by comparing ALL PAIRS in
// registers (E <= 16): exact, symmetric among tied members, independent of the member order -- the sorted form of g is not
// differentiated, it hands tied members different values.  The value is formed in fp64, rounded once, put into the thread's
// column of the tile in place of the member, and the tile leaves through `unstage`, the mirror image of `stage`.
#include "common.h"
#include "ens_tile.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)   // file scope: what is fused is written as fma, nothing else is

namespace {

constexpr int kK = 4;              // sums per (sample, channel): a, g, q, v
constexpr int kReplicas = 8;       // of the rank bins, lane & 7
constexpr int kBinStride = kMaxE + 1;   // words between two replicas: odd, one rank of the 8 replicas falls into 8 banks

inline size_t lds_bytes(int E, int TP) {
    return (size_t)(E + 1) * TP * 4 + (size_t)kReplicas * kBinStride * 4 + (size_t)(TP / 64) * kK * 8 + (size_t)(TP / 64) * 4;
}

struct Scales {
    double inv_e, g, inv_em1;      // 1 / E, 2 / E^2, 1 / (E - 1)
};

// partials [nslab][B][C][4]: slab = blockIdx.x, channel = blockIdx.y, sample = blockIdx.z
template <typename T, int P, int TP>
__global__ __launch_bounds__(TP) void ens_sums_kernel(const T* __restrict__ ens, const float* __restrict__ tar,
                                                      const float* __restrict__ wrow, double* __restrict__ part,
                                                      unsigned long long* __restrict__ ranks,
                                                      unsigned long long* __restrict__ skipped, long long bstride,
                                                      long long estride, Scales sc, int B, int E, int C, int H, int W) {
    extern __shared__ float lds[];                           // tile [E + 1][TP], bins [kReplicas][kBinStride], red, redn
    float* tile = lds;
    unsigned int* bins = reinterpret_cast<unsigned int*>(lds + (E + 1) * TP);
    double* red = reinterpret_cast<double*>(bins + kReplicas * kBinStride);      // [TP / 64][4]; 8-byte aligned: 2080 bytes of bins
    unsigned int* redn = reinterpret_cast<unsigned int*>(red + (TP / 64) * kK);  // [TP / 64]
    const int s = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int h0 = s * kRows;
    const int npts = (min(H, h0 + kRows) - h0) * W;          // consecutive points of this slab (kRows * W < 2^31, checked)
    const long long HW = (long long)H * W;
    const T* eb = ens + b * bstride + c * HW + (long long)h0 * W;
    const float* tb = tar + ((long long)b * C + c) * HW + (long long)h0 * W;
    for (int i = tid; i < kReplicas * kBinStride; i += TP) bins[i] = 0u;
    unsigned int* mine = bins + (lane & (kReplicas - 1)) * kBinStride;
    double acc[kK] = {0.0, 0.0, 0.0, 0.0};
    unsigned int nskip = 0u;
    for (int p0 = 0; p0 < npts; p0 += TP) {
        const int n = min(TP, npts - p0);
        __syncthreads();                                     // the tile before is used up (first time: the bins are zero)
        stage<T, TP>(eb + p0, estride, E, tile, n, tid);
        stage<float, TP>(tb + p0, 0, 1, tile + E * TP, n, tid);
        __syncthreads();
        if (tid < n) {
            const float yf = tile[E * TP + tid];
            const double y = (double)yf;
            const float* col = tile + tid;                   // member e of this point: col[e * TP]
            // the sums over the members in member order, from LDS (the registers are the sort's): two passes, v is about m
            bool bad = yf != yf;
            double sa = 0.0, sm = 0.0;
            unsigned int r = 0u;
#pragma unroll 4
            for (int e = 0; e < E; ++e) {
                const float xf = col[e * TP];
                const double xe = (double)xf;
                bad = bad || (xf != xf);
                sa += fabs(xe - y);
                sm += xe;
                r += xf < yf ? 1u : 0u;
            }
            const double m = sm / (double)E;                 // a division: E equal members x give m = x and v = 0 exactly
            double sv = 0.0;
#pragma unroll 4
            for (int e = 0; e < E; ++e) {
                const double d = (double)col[e * TP] - m;
                sv = fma(d, d, sv);
            }
            const double dq = m - y;
            double q = dq * dq;
            // E as the compiler cannot see through it: the P rank weights and P pad conditions below are formed where they
            // are used; as invariants of the tile loop they were hoisted out of it into more than 128 registers
            int En = E;
            asm volatile("" : "+s"(En));
            float x[P];
#pragma unroll
            for (int e = 0; e < P; ++e) x[e] = e < En ? col[(e < En ? e : 0) * TP] : INFINITY;
            sort_ascending<P>(x);
            double sg = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k)                      // the product is exact; a pad (k >= E) has weight 0 and is not read
                sg = fma((double)(k < En ? 2 * k + 1 - En : 0), (double)(k < En ? x[k] : 0.0f), sg);
            if (bad) {
                sa = sg = q = sv = (double)NAN;              // the network drops a NaN: put it back by hand
                ++nskip;
            } else if (ranks) {
                atomicAdd(mine + r, 1u);
            }
            const double w = (double)wrow[h0 + (p0 + tid) / W];
            acc[0] = fma(w, sa, acc[0]);
            acc[1] = fma(w, sg, acc[1]);
            acc[2] = fma(w, q, acc[2]);
            acc[3] = fma(w, sv, acc[3]);
        }
    }
    // fixed-order reduction: lanes by shuffle, then the waves in order (spelled out here as in metrics.hip)
#pragma unroll
    for (int k = 0; k < kK; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave * kK + k] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nskip += __shfl_down(nskip, o, 64);
    if (lane == 0) redn[wave] = nskip;
    __syncthreads();                                         // also: every add to the replicas is done
    if (tid < kK) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < TP / 64; ++q) v += red[q * kK + tid];
        const double scale = tid == 0 ? sc.inv_e : tid == 1 ? sc.g : tid == 2 ? 1.0 : sc.inv_em1;
        part[(((long long)s * B + b) * C + c) * kK + tid] = v * scale;
    }
    if (skipped && tid == 0) {
        unsigned int n = 0u;
#pragma unroll
        for (int q = 0; q < TP / 64; ++q) n += redn[q];
        if (n) atomicAdd(skipped + c, (unsigned long long)n);
    }
    if (ranks) {
        for (int i = tid; i <= E; i += TP) {
            unsigned int n = 0u;
#pragma unroll
            for (int rr = 0; rr < kReplicas; ++rr) n += bins[rr * kBinStride + i];
            if (n) atomicAdd(ranks + (long long)c * (E + 1) + i, (unsigned long long)n);
        }
    }
}

template <typename T, int P>
void launch_p(const T* ens, const float* tar, const float* wrow, double* part, long long* ranks, long long* skipped,
              long long bstride, long long estride, int B, int E, int C, int H, int W, hipStream_t st) {
    constexpr int TP = tile_points<P>();
    const Scales sc = {1.0 / E, 2.0 / ((double)E * E), 1.0 / (E - 1)};
    hipLaunchKernelGGL((ens_sums_kernel<T, P, TP>), dim3((unsigned)mk::ceil_div(H, kRows), (unsigned)C, (unsigned)B), dim3(TP),
                       lds_bytes(E, TP), st, ens, tar, wrow, part, reinterpret_cast<unsigned long long*>(ranks),
                       reinterpret_cast<unsigned long long*>(skipped), bstride, estride, sc, B, E, C, H, W);
}

template <typename T>
void launch_e(const T* ens, const float* tar, const float* wrow, double* part, long long* ranks, long long* skipped,
              long long bstride, long long estride, int B, int E, int C, int H, int W, hipStream_t st) {
#define MK_ENS_CASE(P) launch_p<T, P>(ens, tar, wrow, part, ranks, skipped, bstride, estride, B, E, C, H, W, st)
    if (E <= 2) MK_ENS_CASE(2);
    else if (E <= 4) MK_ENS_CASE(4);
    else if (E <= 8) MK_ENS_CASE(8);
    else if (E <= 16) MK_ENS_CASE(16);
    else if (E <= 32) MK_ENS_CASE(32);
    else MK_ENS_CASE(64);
#undef MK_ENS_CASE
}

// ---- the gradient of (sum_hw w a, sum_hw w g) with respect to the members (mk_ens_crps_bwd; the header has the definition)
constexpr int kMaxLossE = 16;      // all pairs in registers: at most 256 comparisons per point

// v rounded ONCE to T, as the fp32 value the tile holds (the store's conversion of it is exact)
template <typename T> __device__ __forceinline__ float round_once(double v);
template <> __device__ __forceinline__ float round_once<float>(double v) { return (float)v; }
template <> __device__ __forceinline__ float round_once<__hip_bfloat16>(double v) {
    // double -> fp32 -> bf16 rounds twice, and differs from one rounding only where the fp32 value sits exactly half way
    // between two bf16 values although v does not: there the fp32 value is moved one step towards v first
    const float f = (float)v;
    unsigned int u = __float_as_uint(f);
    if ((u & 0xffffu) == 0x8000u && (double)f != v) u = fabs(v) > fabs((double)f) ? u + 1u : u - 1u;
    return __bfloat162float(__float2bfloat16(__uint_as_float(u)));
}

struct GradScales {
    double inv_e, g;               // 1 / E, 2 / E^2
};

// workgroup (slab, c, b) as in ens_sums_kernel; thread t of a tile forms the E gradients of its point and leaves them in its
// column of the tile, which then goes out through `unstage`
template <typename T, int P, int TP>
__global__ __launch_bounds__(TP) void ens_crps_bwd_kernel(const T* __restrict__ ens, const float* __restrict__ tar,
                                                          const float* __restrict__ wrow, const double* __restrict__ gs,
                                                          T* __restrict__ gens, long long bstride, long long estride,
                                                          long long gbstride, long long gestride, GradScales sc, int E, int C,
                                                          int H, int W) {
    extern __shared__ float lds[];                           // tile [E + 1][TP]
    float* tile = lds;
    const int s = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int h0 = s * kRows;
    const int npts = (min(H, h0 + kRows) - h0) * W;
    const long long HW = (long long)H * W;
    const long long off = c * HW + (long long)h0 * W;
    const T* eb = ens + b * bstride + off;
    T* gb = gens + b * gbstride + off;
    const float* tb = tar + ((long long)b * C + c) * HW + (long long)h0 * W;
    const double k0 = gs[((long long)b * C + c) * 2] * sc.inv_e;          // gS0 / E
    const double k1 = gs[((long long)b * C + c) * 2 + 1] * sc.g;          // 2 gS1 / E^2
    for (int p0 = 0; p0 < npts; p0 += TP) {
        const int n = min(TP, npts - p0);
        __syncthreads();                                     // the tile before has left
        stage<T, TP>(eb + p0, estride, E, tile, n, tid);
        stage<float, TP>(tb + p0, 0, 1, tile + E * TP, n, tid);
        __syncthreads();
        if (tid < n) {
            const float yf = tile[E * TP + tid];
            float* col = tile + tid;
            // a pad is NaN: it compares false both ways and counts for nobody
            float x[P];
#pragma unroll
            for (int e = 0; e < P; ++e) x[e] = e < E ? col[(e < E ? e : 0) * TP] : NAN;
            bool bad = yf != yf;
#pragma unroll
            for (int e = 0; e < P; ++e) bad = bad || (e < E && x[e] != x[e]);
            const double w = (double)wrow[h0 + (p0 + tid) / W];
#pragma unroll
            for (int e = 0; e < P; ++e) {
                int d = 0;                                   // L_e - G_e, exact
#pragma unroll
                for (int f = 0; f < P; ++f)
                    if (f != e) d += (x[f] < x[e] ? 1 : 0) - (x[f] > x[e] ? 1 : 0);
                const int sg = (x[e] > yf ? 1 : 0) - (x[e] < yf ? 1 : 0);
                const double v = w * (k0 * (double)sg + k1 * (double)d);
                if (e < E) col[e * TP] = round_once<T>(bad ? (double)NAN : v);
            }
        }
        __syncthreads();
        unstage<T, TP>(tile, gb + p0, gestride, E, n, tid);
    }
}

template <typename T>
void launch_bwd(const T* ens, const float* tar, const float* wrow, const double* gs, T* gens, long long bstride, long long estride,
                long long gbstride, long long gestride, int B, int E, int C, int H, int W, hipStream_t st) {
    constexpr int TP = 256;
    const GradScales sc = {1.0 / E, 2.0 / ((double)E * E)};
    const dim3 grid((unsigned)mk::ceil_div(H, kRows), (unsigned)C, (unsigned)B);
    const size_t lds = (size_t)(E + 1) * TP * 4;
#define MK_ENS_CASE(P)                                                                                                          \
    hipLaunchKernelGGL((ens_crps_bwd_kernel<T, P, TP>), grid, dim3(TP), lds, st, ens, tar, wrow, gs, gens, bstride, estride, \
                       gbstride, gestride, sc, E, C, H, W)
    if (E <= 2) MK_ENS_CASE(2);
    else if (E <= 4) MK_ENS_CASE(4);
    else if (E <= 8) MK_ENS_CASE(8);
    else MK_ENS_CASE(16);
#undef MK_ENS_CASE
}

}  // namespace

extern "C" long long mk_ens_workspace(int B, int C, int H) {
    if (B < 1 || C < 1 || H < 1) return 0;
    return (long long)mk::ceil_div(H, kRows) * B * C * kK;
}

extern "C" int mk_ens_sums(const void* ens, int dtype, long long bstride, long long estride, const float* tar, const float* wrow,
                           double* workspace, double* sums, long long* ranks, long long* skipped, int B, int E, int C, int H,
                           int W, void* stream) {
    MK_REQUIRE(ens && tar && wrow && workspace && sums, "null pointer");
    MK_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE(E >= 2 && E <= kMaxE, "E outside 2 ... 64 (the members of a point are sorted in registers)");
    MK_REQUIRE(B <= 65535 && C <= 65535, "B or C beyond the grid range");
    MK_REQUIRE((long long)kRows * W <= 0x7fffffffLL, "a workgroup's points (8 rows of W) beyond the 32-bit range");
    const long long chw = (long long)C * H * W;
    MK_REQUIRE(chw < (1LL << 40), "field too large");
    MK_REQUIRE(estride >= chw && bstride >= chw, "a member's [C][H][W] block must be contiguous: strides below C * H * W");
    MK_REQUIRE(estride < (1LL << 44) && bstride < (1LL << 44), "stride too large");
    MK_REQUIRE(bstride >= (long long)E * estride || estride >= (long long)B * bstride || B == 1,
               "members of different samples overlap: need bstride >= E * estride or estride >= B * bstride");
    MK_REQUIRE(mk::aligned_to(ens, dtype == 0 ? 4 : 2), "ensemble not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(tar, wrow), "fp32 stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(workspace, sums, ranks, skipped), "64-bit buffer not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        launch_e<float>((const float*)ens, tar, wrow, workspace, ranks, skipped, bstride, estride, B, E, C, H, W, st);
    else
        launch_e<__hip_bfloat16>((const __hip_bfloat16*)ens, tar, wrow, workspace, ranks, skipped, bstride, estride, B, E, C, H,
                                 W, st);
    MK_LAUNCH_CHECK();
    const long long n = (long long)B * C * kK;
    hipLaunchKernelGGL(slab_finalize_kernel<256>, dim3((unsigned)mk::ceil_div_ll(n, 256 / 64)), dim3(256), 0, st, workspace, sums,
                       mk::ceil_div(H, kRows), n);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_ens_crps_bwd(const void* ens, int dtype, long long bstride, long long estride, const float* tar, const float* wrow,
                               const double* gs, void* gens, long long gbstride, long long gestride, int B, int E, int C, int H,
                               int W, void* stream) {
    MK_REQUIRE(ens && tar && wrow && gs && gens, "null pointer");
    MK_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE(E >= 2 && E <= kMaxLossE, "E outside 2 ... 16 (all pairs of a point are compared in registers)");
    MK_REQUIRE(B <= 65535 && C <= 65535, "B or C beyond the grid range");
    MK_REQUIRE((long long)kRows * W <= 0x7fffffffLL, "a workgroup's points (8 rows of W) beyond the 32-bit range");
    const long long chw = (long long)C * H * W;
    MK_REQUIRE(chw < (1LL << 40), "field too large");
    MK_REQUIRE(estride >= chw && bstride >= chw && gestride >= chw && gbstride >= chw,
               "a member's [C][H][W] block must be contiguous: strides below C * H * W");
    MK_REQUIRE(estride < (1LL << 44) && bstride < (1LL << 44) && gestride < (1LL << 44) && gbstride < (1LL << 44), "stride too large");
    MK_REQUIRE(bstride >= (long long)E * estride || estride >= (long long)B * bstride || B == 1,
               "members of different samples overlap: need bstride >= E * estride or estride >= B * bstride");
    MK_REQUIRE(gbstride >= (long long)E * gestride || gestride >= (long long)B * gbstride || B == 1,
               "gradients of different samples overlap: need gbstride >= E * gestride or gestride >= B * gbstride");
    MK_REQUIRE(mk::aligned_to(ens, dtype == 0 ? 4 : 2) && mk::aligned_to(gens, dtype == 0 ? 4 : 2),
               "ensemble or its gradient not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(tar, wrow), "fp32 stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(gs), "64-bit buffer not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        launch_bwd<float>((const float*)ens, tar, wrow, gs, (float*)gens, bstride, estride, gbstride, gestride, B, E, C, H, W, st);
    else
        launch_bwd<__hip_bfloat16>((const __hip_bfloat16*)ens, tar, wrow, gs, (__hip_bfloat16*)gens, bstride, estride, gbstride,
                                   gestride, B, E, C, H, W, st);
    MK_LAUNCH_CHECK();
    return 0;
}
