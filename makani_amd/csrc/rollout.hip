// Everything an autoregressive rollout does behind the model call (makani/utils/inferencer.py:167-249 with the step
// wrappers of makani/models/stepper.py), in one pass over the model output.  Per point (b, c, h, w), in this order:
//   v = yn                                   the model output, fp32 or bf16 (widened exactly)
//   v = v * std[b][c] + mean[b][c]           history_denormalize(target=True)
//   v = v * mask[h][w]                       mask_output, for the channels of a list
//   v = x_last + v * scale[c]                add_residual (scale optional)
//   v = x_last                               held channels of a second list (the fork's pred[0, 20] = inpt[0, 20])
//   pred = v                                 written once
//   d = v - tar                              the five sums of metrics.hip and the unweighted sum d d per (b, c)
//   err_map[c][h][w] = (..(err_map + d0 d0) + d1 d1 ..)   over the samples in ascending b, by one thread
//   emit[b][k] = v * escale[k] + eshift[k]   for every k with chan[k] == c (predict's selection and de-normalisation)
// Every product and sum of the field arithmetic is an fp32 rounding of its own: contraction is off for this file as in
// zenith.hip, so pred, the map and the emitted fields equal the torch formulation (one kernel per operation) bit for bit.
// The sums are formed as in metrics.hip: fp32 partials per lane and row (fmaf spelled out), folded into fp64 with the
// row's weight at the end of the row; the sixth sum is the partial of the second without the weight.
//
// Decomposition (that of metrics.hip): workgroup (slab, c) takes kRows latitude rows of channel c for ALL samples, NB <= 2
// at a time; each wave walks whole rows, a lane 8 consecutive points per step.  The climatology, the mask and the map are
// read once per row for the samples of a pass; the map is stored at the end of the pass, and a further pass (B > 2)
// reads it again after the workgroup's barrier -- the same additions in the same order.  Each workgroup writes its
// 6 * B fp64 partials to a workspace slot of its own, the finalize kernel of stream_io.h adds the slabs in a fixed order.
// No atomics: bitwise repeatable.  A point's pred, map and emit value depend on that point only, so a launch on a slice
// of rows gives the slice.
//
// Any W: a row is walked as a scalar head up to the 16-byte boundary of the prediction that is written, an 8-wide
// vector body (16-byte accesses) and a scalar tail; when the streams of a row disagree on their alignment the row runs
// scalar.  An emitted row takes 16-byte stores where its own address allows them, scalar stores otherwise.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cstdint>

#pragma clang fp contract(off)   // file scope: no product is ever fused into a following sum in this translation unit

namespace {

constexpr int kT = 256;          // threads per workgroup (4 waves)
constexpr int kE = mk::sio::kVec;  // points per lane per step (the width of IO<T>)
constexpr int kRows = 16;        // latitude rows per workgroup
constexpr int kK = 6;            // sums per (sample, channel)
constexpr int kMaxList = 1024;   // entries of a channel list (mask, hold, emit)

using mk::sio::al16;
using mk::sio::head_points;
using mk::sio::IO;

struct Args {
    const void* yn;
    const float* mean;
    const float* std;
    const float* mask;
    const int* mask_chans;
    int n_mask;
    const float* x_last;
    long long x_bstride;
    int residual;
    const float* scale;
    const int* hold_chans;
    int n_hold;
    float* pred;
    const float* tar;
    const float* clim;
    const float* wrow;
    double* part;
    float* err_map;
    float* emit;
    const int* emit_chans;
    const float* emit_scale;
    const float* emit_shift;
    int K;
    int B, C, H, W;
};

// what is the same for every point of a (sample, channel): wave-uniform
struct Chan {
    bool norm, masked, resid, scaled, held;
    float sc;
};

// the field arithmetic of one point; each operation rounds on its own (contraction is off)
__device__ __forceinline__ float point(float v, float mu, float sd, float m, float xl, const Chan& ch) {
    if (ch.norm) {
        v = v * sd;
        v = v + mu;
    }
    if (ch.masked) v = v * m;
    if (ch.resid) {
        if (ch.scaled) v = v * ch.sc;
        v = xl + v;
    }
    if (ch.held) v = xl;
    return v;
}

// an emitted value: a rounded product, then a rounded sum; a part that is not given is not formed (-0 stays -0)
__device__ __forceinline__ float emit_point(float v, float es, float ef, bool scaled, bool shifted) {
    if (scaled) v = v * es;
    if (shifted) v = v + ef;
    return v;
}

// the sums of metrics.hip from d = v - t; s[1] also serves the unweighted sixth sum
__device__ __forceinline__ void accum(float (&s)[kK - 1], float d, float p, float t, float c) {
    const float pa = p - c, ta = t - c;
    s[0] += fabsf(d);
    s[1] = fmaf(d, d, s[1]);
    s[2] = fmaf(pa, ta, s[2]);
    s[3] = fmaf(pa, pa, s[3]);
    s[4] = fmaf(ta, ta, s[4]);
}

__device__ __forceinline__ bool in_list(const int* __restrict__ list, int n, int c) {
    bool hit = false;
    for (int i = 0; i < n; ++i) hit = hit || (list[i] == c);
    return hit;
}

// partials [nslab][B][C][6]: slab s = blockIdx.x, channel c = blockIdx.y
template <typename T, int NB, bool SCORE>
__global__ __launch_bounds__(kT) void rollout_tail_kernel(const Args a) {
    __shared__ double red[kT / 64][NB * kK];
    __shared__ int elist[kMaxList];
    __shared__ int nelist;
    const int s = blockIdx.x, c = blockIdx.y;
    const int B = a.B, C = a.C, H = a.H, W = a.W, K = a.K;
    const int h0 = s * kRows, h1 = min(H, h0 + kRows);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long HW = (long long)H * W, CHW = (long long)C * HW;
    const T* __restrict__ yn = (const T*)a.yn;
    const float* __restrict__ xlast = a.x_last;
    const float* __restrict__ tar = a.tar;
    const float* __restrict__ clim = a.clim;
    const float* __restrict__ mask = a.mask;
    float* __restrict__ pred = a.pred;
    float* __restrict__ emit = a.emit;
    float* err_map = SCORE ? a.err_map : nullptr;

    Chan ch;
    ch.norm = a.mean != nullptr;
    ch.masked = in_list(a.mask_chans, a.n_mask, c);
    ch.held = in_list(a.hold_chans, a.n_hold, c);
    ch.resid = a.residual != 0;
    ch.scaled = ch.resid && a.scale != nullptr;
    ch.sc = ch.scaled ? a.scale[c] : 1.f;
    const bool use_x = ch.resid || ch.held;
    const bool use_clim = SCORE && clim != nullptr;
    const bool use_err = err_map != nullptr;

    // the emitted channels that take this channel, in ascending k (K > 0 only)
    if (K > 0) {
        if (threadIdx.x == 0) {
            int n = 0;
            for (int k = 0; k < K; ++k)
                if (a.emit_chans[k] == c) elist[n++] = k;
            nelist = n;
        }
        __syncthreads();
    }
    const int nem = K > 0 ? nelist : 0;

    for (int b0 = 0; b0 < B; b0 += NB) {
        const int nb = min(NB, B - b0);
        float mu[NB], sd[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const bool on = ch.norm && b < nb;
            mu[b] = on ? a.mean[(long long)(b0 + b) * C + c] : 0.f;
            sd[b] = on ? a.std[(long long)(b0 + b) * C + c] : 1.f;
        }
        double acc[NB][kK];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kK; ++k) acc[b][k] = 0.0;
        for (int h = h0 + wave; h < h1; h += kT / 64) {
            const long long ro = (long long)c * HW + (long long)h * W;       // row (c, h) of a [C][H][W] field
            const T* yr = yn + (long long)b0 * CHW + ro;                      // row of sample b0; sample b0 + b: + b * CHW
            float* pr = pred + (long long)b0 * CHW + ro;
            const float* tr = SCORE ? tar + (long long)b0 * CHW + ro : nullptr;
            const float* xr = use_x ? xlast + (long long)b0 * a.x_bstride + ro : nullptr;    // + b * x_bstride
            const float* cr = use_clim ? clim + ro : nullptr;
            const float* mr = ch.masked ? mask + (long long)h * W : nullptr;
            float* er = use_err ? err_map + ro : nullptr;
            float r[NB][kK - 1];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int k = 0; k < kK - 1; ++k) r[b][k] = 0.f;
            // head: scalar points up to the 16-byte boundary of the prediction row that is written; the row is vectorised
            // when every stream of every sample of the pass is 16-byte aligned there (wave-uniform), else walked scalar
            const int head = head_points(pr, W);
            bool vec = (!use_clim || al16(cr + head)) && (!ch.masked || al16(mr + head)) && (!use_err || al16(er + head));
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b < nb)
                    vec = vec && al16(pr + b * CHW + head) && al16(yr + b * CHW + head) && (!SCORE || al16(tr + b * CHW + head)) &&
                          (!use_x || al16(xr + b * a.x_bstride + head));
            const int nv = vec ? (W - head) / kE : 0;
            const int vend = vec ? head + nv * kE : 0;        // scalar points: [0, head) and [vend, W) (all when !vec)
            for (int j = lane; j < nv; j += 64) {
                const int i = head + j * kE;
                float cv[kE], mv[kE], ev[kE];
#pragma unroll
                for (int e = 0; e < kE; ++e) cv[e] = 0.f, mv[e] = 1.f, ev[e] = 0.f;
                if (use_clim) IO<float>::load(cr + i, cv);
                if (ch.masked) IO<float>::load(mr + i, mv);
                if (use_err) IO<float>::load(er + i, ev);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b < nb) {
                        float v[kE], xv[kE], tv[kE];
                        IO<T>::load(yr + b * CHW + i, v);
#pragma unroll
                        for (int e = 0; e < kE; ++e) xv[e] = 0.f;
                        if (use_x) IO<float>::load(xr + b * a.x_bstride + i, xv);
                        if (SCORE) IO<float>::load(tr + b * CHW + i, tv);
#pragma unroll
                        for (int e = 0; e < kE; ++e) v[e] = point(v[e], mu[b], sd[b], mv[e], xv[e], ch);
                        IO<float>::store(pr + b * CHW + i, v);
                        if (SCORE) {
#pragma unroll
                            for (int e = 0; e < kE; ++e) {
                                const float d = v[e] - tv[e];
                                accum(r[b], d, v[e], tv[e], cv[e]);
                                const float dd = d * d;
                                ev[e] = ev[e] + dd;
                            }
                        }
                        for (int m = 0; m < nem; ++m) {
                            const int k = elist[m];
                            const float es = a.emit_scale ? a.emit_scale[k] : 1.f, ef = a.emit_shift ? a.emit_shift[k] : 0.f;
                            float* eo = emit + (((long long)(b0 + b) * K + k) * H + h) * W + i;
                            float o[kE];
#pragma unroll
                            for (int e = 0; e < kE; ++e) o[e] = emit_point(v[e], es, ef, a.emit_scale != nullptr, a.emit_shift != nullptr);
                            if (al16(eo)) {                   // wave-uniform: the lanes are 32 bytes apart
                                IO<float>::store(eo, o);
                            } else {
#pragma unroll
                                for (int e = 0; e < kE; ++e) eo[e] = o[e];
                            }
                        }
                    }
                }
                if (use_err) IO<float>::store(er + i, ev);
            }
            // scalar points: the head [0, head) and the tail [vend, W) of a vector row, the whole row otherwise
            const int nhead = vec ? head : 0;
            const int nscal = nhead + (W - vend);
            for (int q = lane; q < nscal; q += 64) {
                const int i = q < nhead ? q : vend + (q - nhead);
                const float cs = use_clim ? cr[i] : 0.f, ms = ch.masked ? mr[i] : 1.f;
                float es_ = use_err ? er[i] : 0.f;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b < nb) {
                        const float xs = use_x ? xr[b * a.x_bstride + i] : 0.f;
                        const float v = point(IO<T>::ld1(yr + b * CHW + i), mu[b], sd[b], ms, xs, ch);
                        pr[b * CHW + i] = v;
                        if (SCORE) {
                            const float t = tr[b * CHW + i];
                            const float d = v - t;
                            accum(r[b], d, v, t, cs);
                            const float dd = d * d;
                            es_ = es_ + dd;
                        }
                        for (int m = 0; m < nem; ++m) {
                            const int k = elist[m];
                            const float es = a.emit_scale ? a.emit_scale[k] : 1.f, ef = a.emit_shift ? a.emit_shift[k] : 0.f;
                            emit[(((long long)(b0 + b) * K + k) * H + h) * W + i] =
                                emit_point(v, es, ef, a.emit_scale != nullptr, a.emit_shift != nullptr);
                        }
                    }
                }
                if (use_err) er[i] = es_;
            }
            if (SCORE) {
                const double w = (double)a.wrow[h];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
#pragma unroll
                    for (int k = 0; k < kK - 1; ++k) acc[b][k] = fma((double)r[b][k], w, acc[b][k]);
                    acc[b][kK - 1] += (double)r[b][1];
                }
            }
        }
        if (SCORE) {
            // fixed-order reduction: lanes by shuffle, then the four waves in order; the fold is spelled out in each
            // kernel, as a shared function it changed the generated code (stream_io.h)
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
                a.part[(((long long)s * B + b0 + b) * C + c) * kK + k] = v;
            }
        }
        // the next pass reads the map this pass stored (and red[] is free again)
        __syncthreads();
    }
}

template <typename T, int NB>
void launch_score(const Args& a, dim3 grid, hipStream_t st) {
    if (a.tar) hipLaunchKernelGGL((rollout_tail_kernel<T, NB, true>), grid, dim3(kT), 0, st, a);
    else hipLaunchKernelGGL((rollout_tail_kernel<T, NB, false>), grid, dim3(kT), 0, st, a);
}

template <typename T>
void launch_nb(const Args& a, dim3 grid, hipStream_t st) {
    if (a.B == 1) launch_score<T, 1>(a, grid, st);
    else launch_score<T, 2>(a, grid, st);
}

}  // namespace

extern "C" long long mk_rollout_tail_workspace(int B, int C, int H) {
    if (B < 1 || C < 1 || H < 1) return 0;
    return (long long)mk::ceil_div(H, kRows) * B * C * kK;
}

extern "C" int mk_rollout_tail(const void* yn, int dtype, const float* mean, const float* std, const float* mask,
                               const int* mask_chans, int n_mask, const float* x_last, long long x_bstride, int residual,
                               const float* scale, const int* hold_chans, int n_hold, float* pred, const float* tar,
                               const float* clim, const float* wrow, double* workspace, double* sums, float* err_map, float* emit,
                               const int* emit_chans, const float* emit_scale, const float* emit_shift, int K, int B, int C, int H,
                               int W, void* stream) {
    MK_REQUIRE(B >= 1 && C >= 1 && C <= 65535 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE((long long)B * C * H * W < (1LL << 40), "field too large");
    MK_REQUIRE(yn && pred, "null pointer");
    MK_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE((mean == nullptr) == (std == nullptr), "mean and std come together");
    MK_REQUIRE(n_mask >= 0 && n_mask <= kMaxList, "bad number of masked channels");
    MK_REQUIRE(n_mask == 0 || (mask_chans && mask), "null pointer (masked channels need the list and the mask)");
    MK_REQUIRE(n_hold >= 0 && n_hold <= kMaxList, "bad number of held channels");
    MK_REQUIRE(n_hold == 0 || hold_chans, "null pointer (held channels)");
    MK_REQUIRE(residual == 0 || residual == 1, "residual must be 0 or 1");
    MK_REQUIRE((residual == 0 && n_hold == 0) || x_last, "null pointer (x_last is needed by the residual and the held channels)");
    MK_REQUIRE(!x_last || x_bstride >= (long long)C * H * W, "x_last batch stride is shorter than one sample");
    MK_REQUIRE(!x_last || (double)B * (double)x_bstride < (double)(1LL << 40), "field too large");
    MK_REQUIRE(scale == nullptr || residual == 1, "scale without the residual");
    MK_REQUIRE(tar || (!clim && !err_map && !sums), "clim, err_map and sums need a target");
    MK_REQUIRE(!tar || (wrow && workspace && sums), "null pointer (a target needs wrow, workspace and sums)");
    MK_REQUIRE(K >= 0 && K <= kMaxList, "bad number of emitted channels");
    MK_REQUIRE(K == 0 || (emit && emit_chans), "null pointer (emitted channels)");
    MK_REQUIRE(K > 0 || (!emit_scale && !emit_shift), "emit scale or shift without emitted channels");
    MK_REQUIRE(mk::aligned_to(yn, dtype == 0 ? 4 : 2), "model output not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(mean, std, mask, mask_chans, x_last, scale, hold_chans, pred, tar, clim, wrow, err_map, emit, emit_chans,
                              emit_scale, emit_shift),
               "fp32 / int32 stream not 4-byte aligned");
    MK_REQUIRE(mk::aligned<8>(workspace, sums), "fp64 buffer not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    Args g;
    g.yn = yn, g.mean = mean, g.std = std, g.mask = mask, g.mask_chans = mask_chans, g.n_mask = n_mask;
    g.x_last = x_last, g.x_bstride = x_bstride, g.residual = residual, g.scale = scale, g.hold_chans = hold_chans, g.n_hold = n_hold;
    g.pred = pred, g.tar = tar, g.clim = clim, g.wrow = wrow, g.part = workspace, g.err_map = err_map;
    g.emit = emit, g.emit_chans = emit_chans, g.emit_scale = emit_scale, g.emit_shift = emit_shift, g.K = K;
    g.B = B, g.C = C, g.H = H, g.W = W;
    const int nslab = mk::ceil_div(H, kRows);
    const dim3 grid((unsigned)nslab, (unsigned)C);
    if (dtype == 0) launch_nb<float>(g, grid, st);
    else launch_nb<__hip_bfloat16>(g, grid, st);
    MK_LAUNCH_CHECK();
    if (tar) {
        const long long n = (long long)B * C * kK;
        hipLaunchKernelGGL(slab_finalize_kernel<kT>, dim3((unsigned)mk::ceil_div_ll(n, kT / 64)), dim3(kT), 0, st, workspace, sums,
                           nslab, n);
        MK_LAUNCH_CHECK();
    }
    return 0;
}
