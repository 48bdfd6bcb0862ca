// Input assembly of the step wrappers (makani/models/preprocessor.py, makani/models/stepper.py): what the reference
// builds with two concatenations, a tile, an in-place mask and the net's own bf16 cast,
//   out = add_static_features(history_normalize(append_unpredicted_features(x)))   [* mask]   [.to(bf16)]
// is one pass here: every source element is read once and every output element written once.
//
// Forward (input_assemble_kernel): one wave per output row (b, oc, h) of W points, waves stride over the rows.  The
// output channel decides the source of the row (wave-uniform): a predicted channel of x (fp32 or bf16), an unpredicted
// channel of u (fp32) or a static feature (fp32, shared by all samples).  Predicted and unpredicted rows are normalised
// with (v - mean) / std, a subtraction and a correctly rounded fp32 division like torch's; rows of a masked output
// channel are then multiplied by the static channel `mask_src` at the same point.  Without statistics the value is
// copied (no arithmetic at all), so the fp32 output equals the torch formulation bit for bit and the bf16 output
// its round-to-nearest-even cast.
//
// Backward (input_assemble_bwd_kernel): the gradient of x only, g_x = (g_out * mask) / std in the order autograd
// takes through the torch formulation, one wave per row of x.
//
// Statistics (history_sums_kernel): per (sample, channel of C + Cu) sum_t w_t sum_hw v and sum_t w_t sum_hw v^2 in
// fp64 from the first addition on (v^2 is exact in fp64).  Workgroup (slab, channel, sample) takes kRows latitude rows
// of every history step and writes its two partials to a workspace slot of its own; the finalize kernel adds the slabs in
// a fixed order.  No atomics: bitwise repeatable.
//
// Any W: a row is walked as a scalar head up to the 16-byte boundary of the stream that is written (read, for the
// sums), an 8-wide vector body (16-byte accesses) and a scalar tail; when the streams of a row disagree on their
// alignment the row runs scalar.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cstdint>

namespace {

constexpr int kT = 256;          // threads per workgroup (4 waves)
constexpr int kE = mk::sio::kVec;  // points per lane per step (the width of IO<T>)
constexpr int kRows = 16;        // latitude rows per workgroup of the sums
constexpr int kK = 2;            // sums per (sample, channel)
constexpr int kGrid = 8192;      // row walkers: at most this many workgroups, waves stride over the rows
constexpr int kMaxMask = 1024;   // masked output channels (a wave scans the list once per row)

using mk::sio::al16;
using mk::sio::head_points;
using mk::sio::IO;

// forward arithmetic of one point: normalise, then mask
template <bool NORM, bool MASK>
__device__ __forceinline__ float fwd_point(float v, float mean, float std, float m) {
    if (NORM) v = (v - mean) / std;
    if (MASK) v = v * m;
    return v;
}

// backward arithmetic of one point, in autograd's order: the mask's product first, then the division
template <bool NORM, bool MASK>
__device__ __forceinline__ float bwd_point(float g, float std, float m) {
    if (MASK) g = g * m;
    if (NORM) g = g / std;
    return g;
}

// dst[i] = f(src[i] [, mrow[i]]) for i in [0, W), one wave.  BWD selects the arithmetic.
template <typename TS, typename TD, bool NORM, bool MASK, bool BWD>
__device__ __forceinline__ void walk_row(const TS* __restrict__ src, TD* __restrict__ dst, const float* __restrict__ mrow,
                                         float mean, float std, int W, int lane) {
    const int head = head_points(dst, W);
    const bool vec = al16(dst + head) && al16(src + head) && (!MASK || al16(mrow + head));
    const int nv = vec ? (W - head) / kE : 0;
    const int vend = vec ? head + nv * kE : 0;            // scalar points: [0, head) and [vend, W) (all when !vec)
    for (int j = lane; j < nv; j += 64) {
        const int i = head + j * kE;
        float v[kE], m[kE];
        IO<TS>::load(src + i, v);
        if (MASK) IO<float>::load(mrow + i, m);
#pragma unroll
        for (int e = 0; e < kE; ++e)
            v[e] = BWD ? bwd_point<NORM, MASK>(v[e], std, MASK ? m[e] : 1.f)
                       : fwd_point<NORM, MASK>(v[e], mean, std, MASK ? m[e] : 1.f);
        IO<TD>::store(dst + i, v);
    }
    const int nhead = vec ? head : 0;
    const int nscal = nhead + (W - vend);
    for (int q = lane; q < nscal; q += 64) {
        const int i = q < nhead ? q : vend + (q - nhead);
        const float v = IO<TS>::ld1(src + i), m = MASK ? mrow[i] : 1.f;
        IO<TD>::st1(dst + i, BWD ? bwd_point<NORM, MASK>(v, std, m) : fwd_point<NORM, MASK>(v, mean, std, m));
    }
}

template <typename TS, typename TD, bool BWD>
__device__ __forceinline__ void walk_row_dyn(const TS* src, TD* dst, const float* mrow, bool norm, float mean, float std, int W,
                                             int lane) {
    if (norm) {
        if (mrow) walk_row<TS, TD, true, true, BWD>(src, dst, mrow, mean, std, W, lane);
        else walk_row<TS, TD, true, false, BWD>(src, dst, nullptr, mean, std, W, lane);
    } else {
        if (mrow) walk_row<TS, TD, false, true, BWD>(src, dst, mrow, mean, std, W, lane);
        else walk_row<TS, TD, false, false, BWD>(src, dst, nullptr, mean, std, W, lane);
    }
}

// wave-uniform: is output channel oc one of the masked ones?
__device__ __forceinline__ bool is_masked(const int* __restrict__ mask_chans, int n_mask, int oc) {
    bool hit = false;
    for (int i = 0; i < n_mask; ++i) hit = hit || (mask_chans[i] == oc);
    return hit;
}

struct Shape {
    int B, T, C, Cu, Cs, H, W;
};

// rows = B * (T (C + Cu) + Cs) * H output rows; wave (blockIdx.x, wave) takes rows blockIdx.x * 4 + wave, + 4 gridDim.x, ...
template <typename TX, typename TO>
__global__ __launch_bounds__(kT) void input_assemble_kernel(const TX* __restrict__ x, const float* __restrict__ u,
                                                            const float* __restrict__ stat, const float* __restrict__ mean,
                                                            const float* __restrict__ std, const int* __restrict__ mask_chans,
                                                            int n_mask, int mask_src, TO* __restrict__ out, Shape s,
                                                            long long rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Cn = s.C + s.Cu, Cd = s.T * Cn, Ct = Cd + s.Cs;
    const long long HW = (long long)s.H * s.W;
    for (long long row = (long long)blockIdx.x * (kT / 64) + wave; row < rows; row += (long long)gridDim.x * (kT / 64)) {
        const long long boc = row / s.H;
        const int h = (int)(row - boc * s.H);
        const int b = (int)(boc / Ct), oc = (int)(boc - (long long)b * Ct);
        TO* dst = out + row * s.W;
        if (oc >= Cd) {                                   // static feature, the same for every sample
            walk_row<float, TO, false, false, false>(stat + (long long)(oc - Cd) * HW + (long long)h * s.W, dst, nullptr, 0.f,
                                                     1.f, s.W, lane);
            continue;
        }
        const int t = oc / Cn, j = oc - t * Cn;
        const bool norm = mean != nullptr;
        const float mu = norm ? mean[(long long)b * Cn + j] : 0.f, sd = norm ? std[(long long)b * Cn + j] : 1.f;
        const float* mrow = is_masked(mask_chans, n_mask, oc) ? stat + (long long)mask_src * HW + (long long)h * s.W : nullptr;
        if (j < s.C)
            walk_row_dyn<TX, TO, false>(x + (((long long)b * s.T + t) * s.C + j) * HW + (long long)h * s.W, dst, mrow, norm, mu,
                                        sd, s.W, lane);
        else
            walk_row_dyn<float, TO, false>(u + (((long long)b * s.T + t) * s.Cu + (j - s.C)) * HW + (long long)h * s.W, dst, mrow,
                                           norm, mu, sd, s.W, lane);
    }
}

// rows = B * T * C * H rows of x
template <typename TG, typename TX>
__global__ __launch_bounds__(kT) void input_assemble_bwd_kernel(const TG* __restrict__ gout, const float* __restrict__ stat,
                                                                const float* __restrict__ std,
                                                                const int* __restrict__ mask_chans, int n_mask, int mask_src,
                                                                TX* __restrict__ gx, Shape s, long long rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Cn = s.C + s.Cu, Ct = s.T * Cn + s.Cs;
    const long long HW = (long long)s.H * s.W;
    for (long long row = (long long)blockIdx.x * (kT / 64) + wave; row < rows; row += (long long)gridDim.x * (kT / 64)) {
        const long long btc = row / s.H;
        const int h = (int)(row - btc * s.H);
        const long long bt = btc / s.C;
        const int c = (int)(btc - bt * s.C);
        const int b = (int)(bt / s.T), t = (int)(bt - (long long)b * s.T);
        const int oc = t * Cn + c;
        const bool norm = std != nullptr;
        const float sd = norm ? std[(long long)b * Cn + c] : 1.f;
        const float* mrow = is_masked(mask_chans, n_mask, oc) ? stat + (long long)mask_src * HW + (long long)h * s.W : nullptr;
        walk_row_dyn<TG, TX, true>(gout + ((long long)b * Ct + oc) * HW + (long long)h * s.W, gx + row * s.W, mrow, norm, 0.f, sd,
                                   s.W, lane);
    }
}

template <typename TS>
__device__ __forceinline__ void sum_row(const TS* __restrict__ r, int W, int lane, double& a1, double& a2) {
    const int head = head_points(r, W);                  // the row's own boundary: a single stream is always vectorised
    const int nv = (W - head) / kE;
    const int vend = head + nv * kE;
    for (int j = lane; j < nv; j += 64) {
        float v[kE];
        IO<TS>::load(r + head + j * kE, v);
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            const double d = (double)v[e];
            a1 += d;
            a2 = fma(d, d, a2);
        }
    }
    const int nscal = head + (W - vend);
    for (int q = lane; q < nscal; q += 64) {
        const double d = (double)IO<TS>::ld1(r + (q < head ? q : vend + (q - head)));
        a1 += d;
        a2 = fma(d, d, a2);
    }
}

// partials [nslab][B][Cn][2]: slab = blockIdx.x, channel j = blockIdx.y, sample b = blockIdx.z
template <typename TX>
__global__ __launch_bounds__(kT) void history_sums_kernel(const TX* __restrict__ x, const float* __restrict__ u,
                                                          const float* __restrict__ wt, double* __restrict__ part, Shape s) {
    __shared__ double red[kT / 64][kK];
    const int slab = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int h0 = slab * kRows, h1 = min(s.H, h0 + kRows);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Cn = s.C + s.Cu;
    const long long HW = (long long)s.H * s.W;
    double acc[kK] = {0.0, 0.0};
    for (int t = 0; t < s.T; ++t) {
        double a1 = 0.0, a2 = 0.0;
        for (int h = h0 + wave; h < h1; h += kT / 64) {
            if (j < s.C)
                sum_row<TX>(x + (((long long)b * s.T + t) * s.C + j) * HW + (long long)h * s.W, s.W, lane, a1, a2);
            else
                sum_row<float>(u + (((long long)b * s.T + t) * s.Cu + (j - s.C)) * HW + (long long)h * s.W, s.W, lane, a1, a2);
        }
        const double w = (double)wt[t];
        acc[0] = fma(a1, w, acc[0]);
        acc[1] = fma(a2, w, acc[1]);
    }
    // fixed-order reduction: lanes by shuffle, then the four waves in order; the fold is spelled out in each kernel,
    // as a shared function it changed the generated code (stream_io.h)
#pragma unroll
    for (int k = 0; k < kK; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kK) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < kT / 64; ++q) v += red[q][threadIdx.x];
        part[(((long long)slab * s.B + b) * Cn + j) * kK + threadIdx.x] = v;
    }
}

dim3 row_grid(long long rows) {
    const long long want = mk::ceil_div_ll(rows, kT / 64);
    return dim3((unsigned)(want < kGrid ? want : kGrid));
}

int check_shape(const Shape& s, const char** why) {
    if (!(s.B >= 1 && s.T >= 1 && s.C >= 1 && s.Cu >= 0 && s.Cs >= 0 && s.H >= 1 && s.W >= 1)) {
        *why = "bad sizes";
        return 1;
    }
    const long long Ct = (long long)s.T * (s.C + s.Cu) + s.Cs;
    if (Ct > (1LL << 24) || (long long)s.B * Ct * s.H * s.W >= (1LL << 40)) {
        *why = "field too large";
        return 1;
    }
    return 0;
}

}  // namespace

extern "C" int mk_input_assemble(const void* x, int x_dtype, const float* u, const float* stat, const float* mean,
                                 const float* std, const int* mask_chans, int n_mask, int mask_src, void* out, int out_dtype,
                                 int B, int T, int C, int Cu, int Cs, int H, int W, void* stream) {
    const Shape s{B, T, C, Cu, Cs, H, W};
    const char* why = "";
    MK_REQUIRE(check_shape(s, &why) == 0, why);
    MK_REQUIRE(x && out, "null pointer");
    MK_REQUIRE((Cu == 0) == (u == nullptr), "u must be given exactly when Cu > 0");
    MK_REQUIRE((Cs == 0) == (stat == nullptr), "stat must be given exactly when Cs > 0");
    MK_REQUIRE((mean == nullptr) == (std == nullptr), "mean and std come together");
    MK_REQUIRE(x_dtype == 0 || x_dtype == 1, "x dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(out_dtype == 0 || out_dtype == 1, "output dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(n_mask >= 0 && n_mask <= kMaxMask, "bad number of masked channels");
    MK_REQUIRE(n_mask == 0 || mask_chans, "null pointer (masked channels)");
    MK_REQUIRE(n_mask == 0 || (mask_src >= 0 && mask_src < Cs), "mask source is not a static channel");
    MK_REQUIRE(mk::aligned_to(x, x_dtype == 0 ? 4 : 2) && mk::aligned_to(out, out_dtype == 0 ? 4 : 2),
               "x or output not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(u, stat, mean, std, mask_chans), "fp32 / int32 stream not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * ((long long)T * (C + Cu) + Cs) * H;
    const dim3 grid = row_grid(rows);
#define MK_ASSEMBLE(TX, TO)                                                                                               \
    hipLaunchKernelGGL((input_assemble_kernel<TX, TO>), grid, dim3(kT), 0, st, (const TX*)x, u, stat, mean, std, mask_chans, \
                       n_mask, mask_src, (TO*)out, s, rows)
    if (x_dtype == 0 && out_dtype == 0) MK_ASSEMBLE(float, float);
    else if (x_dtype == 0) MK_ASSEMBLE(float, __hip_bfloat16);
    else if (out_dtype == 0) MK_ASSEMBLE(__hip_bfloat16, float);
    else MK_ASSEMBLE(__hip_bfloat16, __hip_bfloat16);
#undef MK_ASSEMBLE
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_input_assemble_bwd(const void* gout, int g_dtype, const float* stat, const float* std, const int* mask_chans,
                                     int n_mask, int mask_src, void* gx, int x_dtype, int B, int T, int C, int Cu, int Cs, int H,
                                     int W, void* stream) {
    const Shape s{B, T, C, Cu, Cs, H, W};
    const char* why = "";
    MK_REQUIRE(check_shape(s, &why) == 0, why);
    MK_REQUIRE(gout && gx, "null pointer");
    MK_REQUIRE((Cs == 0) == (stat == nullptr), "stat must be given exactly when Cs > 0");
    MK_REQUIRE(g_dtype == 0 || g_dtype == 1, "gradient dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(x_dtype == 0 || x_dtype == 1, "x dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(n_mask >= 0 && n_mask <= kMaxMask, "bad number of masked channels");
    MK_REQUIRE(n_mask == 0 || mask_chans, "null pointer (masked channels)");
    MK_REQUIRE(n_mask == 0 || (mask_src >= 0 && mask_src < Cs), "mask source is not a static channel");
    MK_REQUIRE(mk::aligned_to(gout, g_dtype == 0 ? 4 : 2) && mk::aligned_to(gx, x_dtype == 0 ? 4 : 2), "gradient not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(stat, std, mask_chans), "fp32 / int32 stream not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * T * C * H;
    const dim3 grid = row_grid(rows);
#define MK_ASSEMBLE_BWD(TG, TX)                                                                                           \
    hipLaunchKernelGGL((input_assemble_bwd_kernel<TG, TX>), grid, dim3(kT), 0, st, (const TG*)gout, stat, std, mask_chans,  \
                       n_mask, mask_src, (TX*)gx, s, rows)
    if (g_dtype == 0 && x_dtype == 0) MK_ASSEMBLE_BWD(float, float);
    else if (g_dtype == 0) MK_ASSEMBLE_BWD(float, __hip_bfloat16);
    else if (x_dtype == 0) MK_ASSEMBLE_BWD(__hip_bfloat16, float);
    else MK_ASSEMBLE_BWD(__hip_bfloat16, __hip_bfloat16);
#undef MK_ASSEMBLE_BWD
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" long long mk_history_workspace(int B, int Cn, int H) {
    if (B < 1 || Cn < 1 || H < 1) return 0;
    return (long long)mk::ceil_div(H, kRows) * B * Cn * kK;
}

extern "C" int mk_history_sums(const void* x, int x_dtype, const float* u, const float* wt, double* workspace, double* sums,
                               int B, int T, int C, int Cu, int H, int W, void* stream) {
    const Shape s{B, T, C, Cu, 0, H, W};
    const char* why = "";
    MK_REQUIRE(check_shape(s, &why) == 0, why);
    MK_REQUIRE(x && wt && workspace && sums, "null pointer");
    MK_REQUIRE((Cu == 0) == (u == nullptr), "u must be given exactly when Cu > 0");
    MK_REQUIRE(x_dtype == 0 || x_dtype == 1, "x dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(C + Cu <= 65535 && B <= 65535, "too many channels or samples for one grid");
    MK_REQUIRE(mk::aligned_to(x, x_dtype == 0 ? 4 : 2), "x not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(u, wt), "fp32 stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(workspace, sums), "fp64 buffer not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nslab = mk::ceil_div(H, kRows);
    const dim3 grid((unsigned)nslab, (unsigned)(C + Cu), (unsigned)B);
    if (x_dtype == 0)
        hipLaunchKernelGGL((history_sums_kernel<float>), grid, dim3(kT), 0, st, (const float*)x, u, wt, workspace, s);
    else
        hipLaunchKernelGGL((history_sums_kernel<__hip_bfloat16>), grid, dim3(kT), 0, st, (const __hip_bfloat16*)x, u, wt,
                           workspace, s);
    MK_LAUNCH_CHECK();
    const long long n = (long long)B * (C + Cu) * kK;
    hipLaunchKernelGGL(slab_finalize_kernel<kT>, dim3((unsigned)mk::ceil_div_ll(n, kT / 64)), dim3(kT), 0, st, workspace, sums,
                       nslab, n);
    MK_LAUNCH_CHECK();
    return 0;
}
