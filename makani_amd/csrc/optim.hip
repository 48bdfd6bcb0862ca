// Multi-tensor optimizer kernels: gradient norm / clipping, AdamW / Adam and LAMB over a list of tensors per launch
// (the optimizers the reference trainer builds from `optimizer_type`, makani/utils/trainer.py:448-478, and the
// clip_grad_norm_ of its `max_grad_norm`).
//
// Launch form (as apex's multi_tensor_apply): the tensor list travels BY VALUE in the kernel arguments (pointers,
// lengths, one int per tensor), so a captured launch holds its own pointers and nothing is uploaded.  A list longer
// than one argument block is split over several launches.  Every tensor is a linear run of fp32 in memory order and
// is cut into chunks of kChunk reals (the cut depends only on the length, never on the alignment); each chunk is
// walked as a scalar head up to the next 16-byte boundary, a float4 body and a scalar tail, and when the tensors of
// one entry disagree on their offset modulo 16 bytes the whole chunk runs scalar.  Workgroups take chunks
// grid-stride and find their tensor by binary search over the chunk counts (a prefix sum in LDS).
//
// Norms are deterministic: every chunk writes ONE fp64 partial sum of squares to a slab (fixed order inside the
// chunk), and the finalize kernel adds a tensor's partials in chunk order, then the tensors in list order.  No float
// atomics anywhere.  The clip coefficient is written on the device and read by the update kernels.
//
// Step counts in capturable mode live in a float32 table on the device (one slot per parameter); the kernel that
// increments them is one that runs before every reader in the same step (the finalize of the norm, else a tiny
// kernel of its own), and one lane writes each slot with a plain store.
#include "common.h"
#include "../../include/makani_amd.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr long long kChunk = 16384;            // reals per chunk = 64 KB per stream; 16 float4 per lane
constexpr int kGridCap = 256 * 8;              // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kMax1 = 180;                     // tensors per launch, 1 stream   (8 + 8 + 4 bytes each)
constexpr int kMax4 = 88;                      // tensors per launch, 4 streams  (32 + 8 + 4 bytes each)
constexpr int kMaxFin = 240;                   // tensors per finalize launch

template <int D, int MAXT>
struct TensorList {
    float* ptr[D][MAXT];
    long long n[MAXT];
    int aux[MAXT];          // host step count, or slot in the device step table
    int count;              // tensors in this launch
    int t0;                 // index of tensor 0 in the caller's list (per-tensor norm arrays)
    long long pbase;        // slab index of this launch's first chunk
};
// every launch below stays under the 4 KB of explicit kernel arguments (list + scalars)
static_assert(sizeof(TensorList<4, kMax4>) <= 3900, "kernel argument block");
static_assert(sizeof(TensorList<1, kMax1>) <= 3900, "kernel argument block");

struct FinList {
    long long n[kMaxFin];
    int inc[kMaxFin];       // step-table slots to increment
    int count, ninc, t0;
    long long pbase;
};
static_assert(sizeof(FinList) <= 3900, "kernel argument block");

__host__ __device__ __forceinline__ long long nchunks(long long n) { return (n + kChunk - 1) / kChunk; }

// Chunk prefix over the launch's tensors in LDS; returns the launch's chunk count.
template <int D, int MAXT>
__device__ long long chunk_prefix(const TensorList<D, MAXT>& L, long long* pre) {
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int t = 0; t < L.count; ++t) {
            pre[t] = s;
            s += nchunks(L.n[t]);
        }
        pre[L.count] = s;
    }
    __syncthreads();
    return pre[L.count];
}

__device__ __forceinline__ int find_tensor(const long long* pre, int count, long long c) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Walk elements [beg, end) of tensor t: f(i, float4 lanes...) through head / float4 body / tail.
// Op::scalar(ptrs, i) and Op::vec(ptrs, i4) with i4 the index of the first of 4 elements (16-byte aligned).
template <int D, class Op>
__device__ __forceinline__ void walk(float* const (&ptr)[D], long long beg, long long end, Op& op) {
    const uintptr_t mis = reinterpret_cast<uintptr_t>(ptr[0] + beg) & 15;
    bool same = true;
#pragma unroll
    for (int d = 1; d < D; ++d) same = same && ((reinterpret_cast<uintptr_t>(ptr[d] + beg) & 15) == mis);
    if (!same) {
        for (long long i = beg + threadIdx.x; i < end; i += kThreads) op.scalar(i);
        return;
    }
    long long head = (long long)(((16 - mis) & 15) >> 2);
    if (head > end - beg) head = end - beg;
    if ((long long)threadIdx.x < head) op.scalar(beg + threadIdx.x);
    const long long vb = beg + head;
    const long long nv = (end - vb) >> 2;
    for (long long j = threadIdx.x; j < nv; j += kThreads) op.vec(vb + 4 * j);
    for (long long i = vb + 4 * nv + threadIdx.x; i < end; i += kThreads) op.scalar(i);
}

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < kThreads / 64; ++i) s += red[i];
    }
    return s;          // valid in thread 0
}

__device__ __forceinline__ float4 ld4(const float* p, long long i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ void st4(float* p, long long i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }

// ---------------------------------------------------------------- sum of squares / scale
struct SumsqOp {
    const float* x;
    double acc;
    __device__ void scalar(long long i) { const double a = x[i]; acc = fma(a, a, acc); }
    __device__ void vec(long long i) {
        const float4 v = ld4(x, i);
        acc = fma((double)v.x, (double)v.x, acc);
        acc = fma((double)v.y, (double)v.y, acc);
        acc = fma((double)v.z, (double)v.z, acc);
        acc = fma((double)v.w, (double)v.w, acc);
    }
};

__global__ __launch_bounds__(kThreads) void sumsq_kernel(TensorList<1, kMax1> L, double* __restrict__ partials) {
    __shared__ long long pre[kMax1 + 1];
    __shared__ double red[kThreads / 64];
    const long long total = chunk_prefix(L, pre);
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        const int t = find_tensor(pre, L.count, c);
        const long long beg = (c - pre[t]) * kChunk, end = min(L.n[t], beg + kChunk);
        float* const ptr[1] = {L.ptr[0][t]};
        SumsqOp op{ptr[0], 0.0};
        walk<1>(ptr, beg, end, op);
        const double s = block_sum(op.acc, red);
        if (threadIdx.x == 0) partials[L.pbase + c] = s;
    }
}

struct ScaleOp {
    float* x;
    float c;
    __device__ void scalar(long long i) { x[i] *= c; }
    __device__ void vec(long long i) {
        float4 v = ld4(x, i);
        v.x *= c; v.y *= c; v.z *= c; v.w *= c;
        st4(x, i, v);
    }
};

__global__ __launch_bounds__(kThreads) void scale_kernel(TensorList<1, kMax1> L, const float* __restrict__ coef) {
    __shared__ long long pre[kMax1 + 1];
    const long long total = chunk_prefix(L, pre);
    const float c = *coef;
    for (long long c0 = blockIdx.x; c0 < total; c0 += gridDim.x) {
        const int t = find_tensor(pre, L.count, c0);
        const long long beg = (c0 - pre[t]) * kChunk, end = min(L.n[t], beg + kChunk);
        float* const ptr[1] = {L.ptr[0][t]};
        ScaleOp op{ptr[0], c};
        walk<1>(ptr, beg, end, op);
    }
}

// ---------------------------------------------------------------- finalize: per-tensor sums, total, clip coefficient
// clip_mode: 0 per-tensor sums only, 1 torch clip_grad_norm_ coefficient min(1, max / (G + 1e-6)),
//            2 apex LAMB divisor (G > max ? G / max : 1), 3 the norm alone.
__device__ void finish_total(const double* tsum, int ntotal, int clip_mode, float max_norm, float* norm_out, float* coef_out) {
    if (threadIdx.x != 0 || clip_mode == 0) return;
    double s = 0.0;
    for (int t = 0; t < ntotal; ++t) s += tsum[t];
    const float G = (float)sqrt(s);
    if (norm_out) *norm_out = G;
    if (!coef_out) return;
    if (clip_mode == 1) {
        const float c = max_norm / (G + 1e-6f);
        *coef_out = c < 1.f ? c : 1.f;
    } else if (clip_mode == 2) {
        *coef_out = G > max_norm ? G / max_norm : 1.f;
    }
}

__global__ __launch_bounds__(1024) void finalize_kernel(FinList L, const double* __restrict__ pa, double* __restrict__ ta,
                                                        const double* __restrict__ pb, double* __restrict__ tb,
                                                        int ntotal, int clip_mode, float max_norm, float* norm_out,
                                                        float* coef_out, float* steps) {
    __shared__ long long pre[kMaxFin + 1];
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int t = 0; t < L.count; ++t) {
            pre[t] = s;
            s += nchunks(L.n[t]);
        }
        pre[L.count] = s;
    }
    if (steps && (int)threadIdx.x < L.ninc) steps[L.inc[threadIdx.x]] += 1.f;   // one lane per slot, plain store
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int t = wave; t < L.count; t += nw) {
        const long long b = L.pbase + pre[t], e = L.pbase + pre[t + 1];
        double sa = 0.0, sb = 0.0;
        for (long long i = b + lane; i < e; i += 64) {
            sa += pa[i];
            if (pb) sb += pb[i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sa += __shfl_down(sa, o, 64);
            sb += __shfl_down(sb, o, 64);
        }
        if (lane == 0) {
            ta[L.t0 + t] = sa;
            if (pb) tb[L.t0 + t] = sb;
        }
    }
    if (clip_mode == 0) return;
    __threadfence_block();
    __syncthreads();
    finish_total(ta, ntotal, clip_mode, max_norm, norm_out, coef_out);
}

__global__ void finish_kernel(const double* __restrict__ tsum, int ntotal, int clip_mode, float max_norm, float* norm_out,
                              float* coef_out, FinList inc, float* steps) {
    if (steps && (int)threadIdx.x < inc.ninc) steps[inc.inc[threadIdx.x]] += 1.f;
    finish_total(tsum, ntotal, clip_mode, max_norm, norm_out, coef_out);
}

// ---------------------------------------------------------------- AdamW / Adam
struct AdamScalars {
    float lr, beta1, beta2, eps, wd;
    const float* lr_dev;     // capturable: lr read here
    const float* steps;      // capturable: step table (aux = slot), else aux = step
    const float* coef;       // gradient multiplier (torch clip), or null
    int adamw;
};

struct AdamOp {
    float *p, *g, *m, *v;
    float b1, b2, eps, step_size, bc2_sqrt, decay, l2, gc;
    __device__ __forceinline__ void one(float& pp, float gg, float& mm, float& vv) const {
        gg = fmaf(l2, pp, gg * gc);
        pp *= decay;
        mm = fmaf(b1, mm, (1.f - b1) * gg);
        vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        pp -= step_size * (mm / denom);
    }
    __device__ void scalar(long long i) { one(p[i], g[i], m[i], v[i]); }
    __device__ void vec(long long i) {
        float4 pp = ld4(p, i), mm = ld4(m, i), vv = ld4(v, i);
        const float4 gg = ld4(g, i);
        one(pp.x, gg.x, mm.x, vv.x);
        one(pp.y, gg.y, mm.y, vv.y);
        one(pp.z, gg.z, mm.z, vv.z);
        one(pp.w, gg.w, mm.w, vv.w);
        st4(p, i, pp);
        st4(m, i, mm);
        st4(v, i, vv);
    }
};

__device__ __forceinline__ int step_of(const float* steps, int aux) { return steps ? (int)steps[aux] : aux; }

__global__ __launch_bounds__(kThreads) void adam_kernel(TensorList<4, kMax4> L, AdamScalars s) {
    __shared__ long long pre[kMax4 + 1];
    const long long total = chunk_prefix(L, pre);
    const float lr = s.lr_dev ? *s.lr_dev : s.lr;
    const float gc = s.coef ? *s.coef : 1.f;
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        const int t = find_tensor(pre, L.count, c);
        const long long beg = (c - pre[t]) * kChunk, end = min(L.n[t], beg + kChunk);
        const int step = step_of(s.steps, L.aux[t]);
        // bias corrections in double, rounded once (as mk_adam_step): identical for host and device step counts
        const float bc1 = (float)(1.0 - pow((double)s.beta1, (double)step));
        AdamOp op;
        op.p = L.ptr[0][t]; op.g = L.ptr[1][t]; op.m = L.ptr[2][t]; op.v = L.ptr[3][t];
        op.b1 = s.beta1; op.b2 = s.beta2; op.eps = s.eps; op.gc = gc;
        op.step_size = lr / bc1;
        op.bc2_sqrt = (float)sqrt(1.0 - pow((double)s.beta2, (double)step));
        op.decay = s.adamw ? 1.f - lr * s.wd : 1.f;
        op.l2 = s.adamw ? 0.f : s.wd;
        float* const ptr[4] = {op.p, op.g, op.m, op.v};
        walk<4>(ptr, beg, end, op);
    }
}

// ---------------------------------------------------------------- LAMB (apex FusedLAMB arithmetic, two stages)
struct LambScalars {
    float lr, beta1, beta2, beta3, eps, wd;
    const float* lr_dev;
    const float* steps;
    const float* coef;       // gradient divisor (apex clip), or null
    int adamw, bias_correction, trust;
};

struct LambCoef {
    float b1, b2, b3, eps, wd, bc1, bc2, gdiv;
    int adamw;
    // u from the NEW moments and the OLD parameter: the same expression in both stages
    __device__ __forceinline__ float update(float m, float v, float p) const {
        const float u = (m / bc1) / (sqrtf(v / bc2) + eps);
        return adamw ? fmaf(wd, p, u) : u;
    }
    __device__ __forceinline__ float moments(float p, float g, float& m, float& v) const {
        g = g / gdiv;
        if (!adamw) g = fmaf(wd, p, g);
        m = fmaf(b1, m, b3 * g);
        v = fmaf(b2, v, (1.f - b2) * g * g);
        return update(m, v, p);
    }
};

__device__ __forceinline__ LambCoef lamb_coef(const LambScalars& s, int step) {
    LambCoef k;
    k.b1 = s.beta1; k.b2 = s.beta2; k.b3 = s.beta3; k.eps = s.eps; k.wd = s.wd; k.adamw = s.adamw;
    k.gdiv = s.coef ? *s.coef : 1.f;
    if (s.bias_correction) {
        k.bc1 = (float)(1.0 - pow((double)s.beta1, (double)step));
        k.bc2 = (float)(1.0 - pow((double)s.beta2, (double)step));
    } else {
        k.bc1 = k.bc2 = 1.f;
    }
    return k;
}

struct Lamb1Op {
    float *p, *g, *m, *v;
    LambCoef k;
    double sp, su;
    __device__ __forceinline__ void one(float pp, float gg, float& mm, float& vv) {
        const float u = k.moments(pp, gg, mm, vv);
        sp = fma((double)pp, (double)pp, sp);
        su = fma((double)u, (double)u, su);
    }
    __device__ void scalar(long long i) { one(p[i], g[i], m[i], v[i]); }
    __device__ void vec(long long i) {
        const float4 pp = ld4(p, i), gg = ld4(g, i);
        float4 mm = ld4(m, i), vv = ld4(v, i);
        one(pp.x, gg.x, mm.x, vv.x);
        one(pp.y, gg.y, mm.y, vv.y);
        one(pp.z, gg.z, mm.z, vv.z);
        one(pp.w, gg.w, mm.w, vv.w);
        st4(m, i, mm);
        st4(v, i, vv);
    }
};

__global__ __launch_bounds__(kThreads) void lamb1_kernel(TensorList<4, kMax4> L, LambScalars s, double* __restrict__ part_p,
                                                         double* __restrict__ part_u) {
    __shared__ long long pre[kMax4 + 1];
    __shared__ double red[kThreads / 64];
    const long long total = chunk_prefix(L, pre);
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        const int t = find_tensor(pre, L.count, c);
        const long long beg = (c - pre[t]) * kChunk, end = min(L.n[t], beg + kChunk);
        Lamb1Op op;
        op.p = L.ptr[0][t]; op.g = L.ptr[1][t]; op.m = L.ptr[2][t]; op.v = L.ptr[3][t];
        op.k = lamb_coef(s, step_of(s.steps, L.aux[t]));
        op.sp = op.su = 0.0;
        float* const ptr[4] = {op.p, op.g, op.m, op.v};
        walk<4>(ptr, beg, end, op);
        const double a = block_sum(op.sp, red);
        const double b = block_sum(op.su, red);
        if (threadIdx.x == 0) {
            part_p[L.pbase + c] = a;
            part_u[L.pbase + c] = b;
        }
    }
}

struct Lamb2Op {
    float *p, *m, *v;
    LambCoef k;
    float ratio;
    __device__ __forceinline__ float one(float pp, float mm, float vv) const { return pp - ratio * k.update(mm, vv, pp); }
    __device__ void scalar(long long i) { p[i] = one(p[i], m[i], v[i]); }
    __device__ void vec(long long i) {
        float4 pp = ld4(p, i);
        const float4 mm = ld4(m, i), vv = ld4(v, i);
        pp.x = one(pp.x, mm.x, vv.x);
        pp.y = one(pp.y, mm.y, vv.y);
        pp.z = one(pp.z, mm.z, vv.z);
        pp.w = one(pp.w, mm.w, vv.w);
        st4(p, i, pp);
    }
};

__global__ __launch_bounds__(kThreads) void lamb2_kernel(TensorList<4, kMax4> L, LambScalars s, const double* __restrict__ tp,
                                                         const double* __restrict__ tu) {
    __shared__ long long pre[kMax4 + 1];
    const long long total = chunk_prefix(L, pre);
    const float lr = s.lr_dev ? *s.lr_dev : s.lr;
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        const int t = find_tensor(pre, L.count, c);
        const long long beg = (c - pre[t]) * kChunk, end = min(L.n[t], beg + kChunk);
        Lamb2Op op;
        op.p = L.ptr[0][t]; op.m = L.ptr[2][t]; op.v = L.ptr[3][t];
        op.k = lamb_coef(s, step_of(s.steps, L.aux[t]));
        const float pn = (float)sqrt(tp[L.t0 + t]), un = (float)sqrt(tu[L.t0 + t]);
        op.ratio = (s.trust && pn != 0.f && un != 0.f) ? lr * (pn / un) : lr;
        float* const ptr[3] = {op.p, op.m, op.v};
        walk<3>(ptr, beg, end, op);
    }
}

// ---------------------------------------------------------------- host side
unsigned grid_for(long long chunks) { return (unsigned)std::max(1LL, std::min<long long>(chunks, kGridCap)); }

template <int D, int MAXT>
int fill(TensorList<D, MAXT>& L, int t0, int cnt, const uint64_t* ptrs, const long long* n, const int* aux, long long& pbase) {
    L.count = cnt;
    L.t0 = t0;
    L.pbase = pbase;
    long long ch = 0;
    for (int i = 0; i < cnt; ++i) {
        for (int d = 0; d < D; ++d) L.ptr[d][i] = reinterpret_cast<float*>(ptrs[(long long)(t0 + i) * D + d]);
        L.n[i] = n[t0 + i];
        L.aux[i] = aux ? aux[t0 + i] : 0;
        ch += nchunks(n[t0 + i]);
    }
    pbase += ch;
    return (int)std::min<long long>(ch, kGridCap);
}

bool valid(int T, const uint64_t* ptrs, const long long* n, int D) {
    if (T < 1 || !ptrs || !n) return false;
    for (long long i = 0; i < (long long)T * D; ++i)
        if (!ptrs[i] || (ptrs[i] & 3)) return false;
    for (int t = 0; t < T; ++t)
        if (n[t] < 1) return false;
    return true;
}

int launch_finalize(int T, const long long* n, const double* pa, double* ta, const double* pb, double* tb, int clip_mode,
                    float max_norm, float* norm_out, float* coef_out, float* steps, const int* inc, int ninc,
                    hipStream_t stream) {
    long long pbase = 0;
    const bool fused = T <= kMaxFin && ninc <= kMaxFin;
    int done_inc = 0;
    for (int t0 = 0; t0 < T; t0 += kMaxFin) {
        FinList F;
        F.count = std::min(kMaxFin, T - t0);
        F.t0 = t0;
        F.pbase = pbase;
        for (int i = 0; i < F.count; ++i) {
            F.n[i] = n[t0 + i];
            pbase += nchunks(n[t0 + i]);
        }
        F.ninc = 0;
        if (fused && steps) {
            F.ninc = ninc;
            for (int i = 0; i < ninc; ++i) F.inc[i] = inc[i];
            done_inc = ninc;
        }
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1024), 0, stream, F, pa, ta, pb, tb, T, fused ? clip_mode : 0,
                           max_norm, norm_out, coef_out, fused ? steps : nullptr);
        MK_LAUNCH_CHECK();
    }
    if (!fused) {
        FinList F;
        F.count = 0;
        F.ninc = 0;
        int k = done_inc;
        do {
            F.ninc = std::min(kMaxFin, ninc - k);
            for (int i = 0; i < F.ninc; ++i) F.inc[i] = inc[k + i];
            k += F.ninc;
            const bool last = k >= ninc;
            hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kMaxFin), 0, stream, ta, T, last ? clip_mode : 0, max_norm,
                               norm_out, coef_out, F, steps);
            MK_LAUNCH_CHECK();
        } while (k < ninc);
    }
    return 0;
}

}  // namespace

extern "C" long long mk_mt_chunks(long long n) { return n > 0 ? nchunks(n) : 0; }

extern "C" int mk_mt_sumsq(int T, const uint64_t* x, const long long* n, double* partials, double* tsum, int clip_mode,
                           float max_norm, float* norm_out, float* coef_out, float* steps, const int* inc_slots, int ninc,
                           void* stream) {
    MK_REQUIRE(valid(T, x, n, 1), "bad tensor list (null / not 4-byte aligned / empty)");
    MK_REQUIRE(partials && tsum, "null workspace");
    MK_REQUIRE(clip_mode >= 0 && clip_mode <= 3, "bad clip_mode");
    MK_REQUIRE(ninc == 0 || (steps && inc_slots), "step increments need the step table");
    hipStream_t s = (hipStream_t)stream;
    long long pbase = 0;
    for (int t0 = 0; t0 < T; t0 += kMax1) {
        TensorList<1, kMax1> L;
        const int g = fill(L, t0, std::min(kMax1, T - t0), x, n, nullptr, pbase);
        hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(g)), dim3(kThreads), 0, s, L, partials);
        MK_LAUNCH_CHECK();
    }
    return launch_finalize(T, n, partials, tsum, nullptr, nullptr, clip_mode, max_norm, norm_out, coef_out, steps, inc_slots,
                           ninc, s);
}

extern "C" int mk_mt_norm_finish(int T, const double* tsum, int clip_mode, float max_norm, float* norm_out, float* coef_out,
                                 float* steps, const int* inc_slots, int ninc, void* stream) {
    MK_REQUIRE(T >= 1 && tsum, "bad arguments");
    MK_REQUIRE(clip_mode >= 1 && clip_mode <= 3, "bad clip_mode");
    MK_REQUIRE(ninc == 0 || (steps && inc_slots), "step increments need the step table");
    FinList F;
    F.count = 0;
    int k = 0;
    do {
        F.ninc = std::min(kMaxFin, ninc - k);
        for (int i = 0; i < F.ninc; ++i) F.inc[i] = inc_slots[k + i];
        k += F.ninc;
        const bool last = k >= ninc;
        hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kMaxFin), 0, (hipStream_t)stream, tsum, T, last ? clip_mode : 0,
                           max_norm, norm_out, coef_out, F, steps);
        MK_LAUNCH_CHECK();
    } while (k < ninc);
    return 0;
}

extern "C" int mk_mt_step_inc(float* steps, const int* slots, int nslots, void* stream) {
    MK_REQUIRE(steps && slots && nslots >= 1, "bad arguments");
    for (int k = 0; k < nslots; k += kMaxFin) {
        FinList F;
        F.count = 0;
        F.ninc = std::min(kMaxFin, nslots - k);
        for (int i = 0; i < F.ninc; ++i) F.inc[i] = slots[k + i];
        hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kMaxFin), 0, (hipStream_t)stream, nullptr, 0, 0, 0.f, nullptr,
                           nullptr, F, steps);
        MK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mk_mt_scale(int T, const uint64_t* x, const long long* n, const float* coef, void* stream) {
    MK_REQUIRE(valid(T, x, n, 1) && coef, "bad arguments");
    long long pbase = 0;
    for (int t0 = 0; t0 < T; t0 += kMax1) {
        TensorList<1, kMax1> L;
        const int g = fill(L, t0, std::min(kMax1, T - t0), x, n, nullptr, pbase);
        hipLaunchKernelGGL(scale_kernel, dim3(grid_for(g)), dim3(kThreads), 0, (hipStream_t)stream, L, coef);
        MK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mk_mt_adam(int T, const uint64_t* pgmv, const long long* n, const int* step_or_slot, const float* steps,
                          float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int adamw,
                          const float* coef, void* stream) {
    MK_REQUIRE(valid(T, pgmv, n, 4) && step_or_slot, "bad tensor list (null / not 4-byte aligned / empty)");
    if (!steps)
        for (int t = 0; t < T; ++t) MK_REQUIRE(step_or_slot[t] >= 1, "step counts start at 1");
    AdamScalars s{lr, beta1, beta2, eps, weight_decay, lr_dev, steps, coef, adamw};
    long long pbase = 0;
    for (int t0 = 0; t0 < T; t0 += kMax4) {
        TensorList<4, kMax4> L;
        const int g = fill(L, t0, std::min(kMax4, T - t0), pgmv, n, step_or_slot, pbase);
        hipLaunchKernelGGL(adam_kernel, dim3(grid_for(g)), dim3(kThreads), 0, (hipStream_t)stream, L, s);
        MK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mk_mt_lamb(int stage, int T, const uint64_t* pgmv, const long long* n, const int* step_or_slot,
                          const float* steps, float lr, const float* lr_dev, float beta1, float beta2, float beta3, float eps,
                          float weight_decay, int adamw, int bias_correction, int trust, const float* coef,
                          double* part_p, double* part_u, double* tsum_p, double* tsum_u, void* stream) {
    MK_REQUIRE(stage == 1 || stage == 2, "stage is 1 or 2");
    MK_REQUIRE(valid(T, pgmv, n, 4) && step_or_slot, "bad tensor list (null / not 4-byte aligned / empty)");
    MK_REQUIRE(tsum_p && tsum_u && (stage == 2 || (part_p && part_u)), "null workspace");
    if (!steps)
        for (int t = 0; t < T; ++t) MK_REQUIRE(step_or_slot[t] >= 1, "step counts start at 1");
    hipStream_t st = (hipStream_t)stream;
    LambScalars s{lr, beta1, beta2, beta3, eps, weight_decay, lr_dev, steps, coef, adamw, bias_correction, trust};
    long long pbase = 0;
    for (int t0 = 0; t0 < T; t0 += kMax4) {
        TensorList<4, kMax4> L;
        const int g = fill(L, t0, std::min(kMax4, T - t0), pgmv, n, step_or_slot, pbase);
        if (stage == 1)
            hipLaunchKernelGGL(lamb1_kernel, dim3(grid_for(g)), dim3(kThreads), 0, st, L, s, part_p, part_u);
        else
            hipLaunchKernelGGL(lamb2_kernel, dim3(grid_for(g)), dim3(kThreads), 0, st, L, s, tsum_p, tsum_u);
        MK_LAUNCH_CHECK();
    }
    if (stage == 2) return 0;
    return launch_finalize(T, n, part_p, tsum_p, part_u, tsum_u, 0, 0.f, nullptr, nullptr, nullptr, nullptr, 0, st);
}
