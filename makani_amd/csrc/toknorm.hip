// Layer norm over the TRAILING axis of contiguous rows, with the residual add in front of it fused in: nn.LayerNorm of the ViT
// blocks (makani/models/networks/vit.py:86-118) and nn.LayerNorm((h, w)) of AFNO (afnonet.py:249-250).  `rows` rows of L
// elements, element row stride ld >= L per tensor, fp32 or bf16 per tensor (told at run time: a wave-uniform branch around
// the load or store, nothing else depends on it).  Per row
//   s = x + r (fp32),  mean = sum s / L,  var = sum (s - mean)^2 / L (biased, two passes),  rstd = 1 / sqrt(var + eps),
//   v = w (s - mean) rstd + b (fp32)  ->  y (rounded once), y2 (bf16, the same v rounded once), s_out = s, stats = (mean, rstd).
// Backward, with g = gy + gy2 (fp32), xh = (s - mean) rstd (s recomputed from x and r), s1 = sum w g, s2 = sum w g xh:
//   gx = rstd (w g - s1 / L - xh s2 / L) + gs  ->  gx (x's dtype and ld), gr (r's),  gwb = (sum_rows g xh, sum_rows g).
//
// Ownership.  The row is cut into vectors of 8 consecutive elements; vector v belongs to thread v % T of the team that owns
// the row, which walks its vectors v = t, t + T, ... in order.  Two teams:
//   * L <= 2048: one wavefront (T = 64) per row, four rows per workgroup, the row in registers (NCH = 1, 2 or 4 vectors
//     per lane; 384 and 1024 are the production widths);
//   * longer rows: one workgroup (T = 512) per row, the fp32 row (backward: s and g) in LDS while it fits the 160 KB --
//     L = 16 200, the AFNO row, does, forward and backward -- and read again from global memory (L2: it was just fetched)
//     beyond that.  A thread only ever reads back LDS words it wrote itself, so the row needs no barrier of its own.
// With 16-byte alignment of every pointer and row stride and L a multiple of 8 a vector is one or two 16-byte accesses,
// else eight single elements; the two differ in nothing but the instructions that move the data.
//
// Fixed arithmetic.  A thread adds the 8 elements of a vector in order and its vectors in order; the 64 lanes fold by an
// xor butterfly (1, 2, ..., 32), which leaves the same bits in every lane; the 8 waves of a workgroup exchange their sums
// through LDS and every thread adds them in the order 0 .. 7.  The tree depends on L only: a launch on a subset of the rows,
// at any alignment, gives the bits of that subset.  Contraction is off in this file; what is fused is spelled fmaf.
//
// gwb.  The workgroups are persistent in the backward (row = blockIdx, + gridDim, ...).  A wavefront keeps the column sums
// of its rows in registers, the four wavefronts of a workgroup add theirs in the order 0 .. 3 through LDS and the workgroup
// writes [2][L] fp32 partials to a workspace slot of its own; a workgroup that owns a long row adds each row's terms to its
// slot in place (the first row writes, so the workspace need not be cleared; a column is only ever touched by one thread).
// A finishing launch adds the slots in a fixed order in fp64.  No atomics: bitwise repeatable.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#pragma clang fp contract(off)   // file scope: what is fused is written as fmaf, nothing else is

namespace {

using bf16 = __hip_bfloat16;
using mk::sio::IO;
constexpr int kV = mk::sio::kVec;           // elements per vector
constexpr int kWaveT = 256;                 // wave regime: 4 wavefronts = 4 rows per workgroup
constexpr int kWaveMax = 4 * 64 * kV;       // longest row one wavefront holds in registers (NCH = 4)
constexpr int kBlockT = 512;                // block regime: threads per row
constexpr int kLdsMax = 160 * 1024;         // LDS of a CU, and the most one workgroup may take
constexpr int kLdsFixed = 64;               // bytes in front of the row(s): the wave sums of a block reduction
constexpr int kFwdGrid = 1 << 20;           // forward: one team per workgroup slot up to here, strided beyond
constexpr int kBwdWaveGrid = 1024;          // backward: at most this many persistent workgroups = workspace slots
constexpr int kBwdBlockGrid = 256;

struct Src { const void* p; long long ld; int bf; };      // p == nullptr: absent
struct Dst { void* p; long long ld; int bf; };

struct FwdArgs {
    Src x, r;
    const float *w, *b;
    Dst y, y2, so;
    float* stats;
    long long rows;
    int L;
    float eps;
};
struct BwdArgs {
    Src x, r, gy, gy2, gs;
    const float *stats, *w;
    Dst gx, gr;
    float* ws;      // nullptr: no parameter gradients
    long long rows;
    int L;
};

// elements i0 .. i0 + 7 of a row; n (1 .. 8) of them exist, the others read as zero
template <typename T, bool VEC> __device__ __forceinline__ void ld8(const T* q, int n, float (&v)[kV]) {
    if constexpr (VEC) {
        IO<T>::load(q, v);
    } else {
#pragma unroll
        for (int j = 0; j < kV; ++j) v[j] = j < n ? IO<T>::ld1(q + j) : 0.f;
    }
}
template <typename T, bool VEC> __device__ __forceinline__ void st8(T* q, int n, const float (&v)[kV]) {
    if constexpr (VEC) {
        IO<T>::store(q, v);
    } else {
#pragma unroll
        for (int j = 0; j < kV; ++j)
            if (j < n) IO<T>::st1(q + j, v[j]);
    }
}
template <bool VEC> __device__ __forceinline__ void load8(const Src& t, long long row, int i0, int n, float (&v)[kV]) {
    const long long off = row * t.ld + i0;
    if (t.bf) ld8<bf16, VEC>(static_cast<const bf16*>(t.p) + off, n, v);
    else ld8<float, VEC>(static_cast<const float*>(t.p) + off, n, v);
}
template <bool VEC> __device__ __forceinline__ void store8(const Dst& t, long long row, int i0, int n, const float (&v)[kV]) {
    const long long off = row * t.ld + i0;
    if (t.bf) st8<bf16, VEC>(static_cast<bf16*>(t.p) + off, n, v);
    else st8<float, VEC>(static_cast<float*>(t.p) + off, n, v);
}
// a [L] fp32 parameter, `none` where there is none
template <bool VEC> __device__ __forceinline__ void param8(const float* p, int i0, int n, float none, float (&v)[kV]) {
    if (p) {
        ld8<float, VEC>(p + i0, n, v);
    } else {
#pragma unroll
        for (int j = 0; j < kV; ++j) v[j] = none;
    }
}
// s = x + r
template <bool VEC> __device__ __forceinline__ void load_sum(const Src& x, const Src& r, long long row, int i0, int n, float (&s)[kV]) {
    load8<VEC>(x, row, i0, n, s);
    if (r.p) {
        float t[kV];
        load8<VEC>(r, row, i0, n, t);
#pragma unroll
        for (int j = 0; j < kV; ++j) s[j] += t[j];
    }
}
// g = gy + gy2, either may be absent
template <bool VEC> __device__ __forceinline__ void load_grad(const Src& gy, const Src& gy2, long long row, int i0, int n, float (&g)[kV]) {
    if (gy.p) {
        load_sum<VEC>(gy, gy2, row, i0, n, g);
    } else if (gy2.p) {
        load8<VEC>(gy2, row, i0, n, g);
    } else {
#pragma unroll
        for (int j = 0; j < kV; ++j) g[j] = 0.f;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the sum over the 512 threads, the same bits in every thread; `part` holds kBlockT / 64 floats
__device__ __forceinline__ float block_sum(float v, float* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = part[0];
#pragma unroll
    for (int q = 1; q < kBlockT / 64; ++q) s += part[q];
    __syncthreads();      // `part` is free again
    return s;
}

// ---- the per-vector arithmetic, shared by the two teams ----
__device__ __forceinline__ float vec_sum(const float (&s)[kV], float acc) {
#pragma unroll
    for (int j = 0; j < kV; ++j) acc += s[j];
    return acc;
}
__device__ __forceinline__ float vec_sqdev(const float (&s)[kV], int n, float mean, float acc) {
#pragma unroll
    for (int j = 0; j < kV; ++j) {
        const float d = j < n ? s[j] - mean : 0.f;
        acc = fmaf(d, d, acc);
    }
    return acc;
}
template <bool VEC>
__device__ __forceinline__ void vec_apply(const FwdArgs& a, long long row, int i0, int n, const float (&s)[kV], float mean, float rstd) {
    float w[kV], b[kV], v[kV];
    param8<VEC>(a.w, i0, n, 1.f, w);
    param8<VEC>(a.b, i0, n, 0.f, b);
#pragma unroll
    for (int j = 0; j < kV; ++j) v[j] = fmaf(w[j], (s[j] - mean) * rstd, b[j]);
    if (a.y.p) store8<VEC>(a.y, row, i0, n, v);
    if (a.y2.p) store8<VEC>(a.y2, row, i0, n, v);
}
// backward, first pass over a vector: s1, s2 and the terms of the column sums (aw += g xh, ab += g)
__device__ __forceinline__ void vec_bwd_sums(const float (&s)[kV], const float (&g)[kV], const float (&w)[kV], int n, float mean,
                                             float rstd, float& s1, float& s2, float (&aw)[kV], float (&ab)[kV]) {
#pragma unroll
    for (int j = 0; j < kV; ++j) {
        const float xh = j < n ? (s[j] - mean) * rstd : 0.f;
        const float wg = w[j] * g[j];
        s1 += wg;
        s2 = fmaf(wg, xh, s2);
        aw[j] = fmaf(g[j], xh, aw[j]);
        ab[j] += g[j];
    }
}
template <bool VEC>
__device__ __forceinline__ void vec_bwd_apply(const BwdArgs& a, long long row, int i0, int n, const float (&s)[kV], const float (&g)[kV],
                                              float mean, float rstd, float m1, float m2) {
    float w[kV], v[kV];
    param8<VEC>(a.w, i0, n, 1.f, w);
#pragma unroll
    for (int j = 0; j < kV; ++j) {
        const float xh = (s[j] - mean) * rstd;
        v[j] = rstd * ((w[j] * g[j] - m1) - xh * m2);
    }
    if (a.gs.p) {
        float t[kV];
        load8<VEC>(a.gs, row, i0, n, t);
#pragma unroll
        for (int j = 0; j < kV; ++j) v[j] += t[j];
    }
    store8<VEC>(a.gx, row, i0, n, v);
    if (a.gr.p) store8<VEC>(a.gr, row, i0, n, v);
}

__device__ __forceinline__ int valid(int L, int i0) { return L - i0 < kV ? L - i0 : kV; }      // <= 0: the vector lies beyond the row

// ---- one wavefront per row ----
template <int NCH, bool VEC> __global__ __launch_bounds__(kWaveT) void tok_fwd_wave(const FwdArgs a) {
    const int lane = threadIdx.x & 63;
    const float fl = (float)a.L;
    for (long long row = (long long)blockIdx.x * (kWaveT / 64) + (threadIdx.x >> 6); row < a.rows;
         row += (long long)gridDim.x * (kWaveT / 64)) {
        float s[NCH][kV];
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int i0 = (k * 64 + lane) * kV, n = valid(a.L, i0);
            if (n > 0) {
                load_sum<VEC>(a.x, a.r, row, i0, n, s[k]);
                if (a.so.p) store8<VEC>(a.so, row, i0, n, s[k]);
            } else {
#pragma unroll
                for (int j = 0; j < kV; ++j) s[k][j] = 0.f;
            }
            acc = vec_sum(s[k], acc);
        }
        const float mean = wave_sum(acc) / fl;
        acc = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) acc = vec_sqdev(s[k], valid(a.L, (k * 64 + lane) * kV), mean, acc);
        const float rstd = 1.0f / sqrtf(wave_sum(acc) / fl + a.eps);
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int i0 = (k * 64 + lane) * kV, n = valid(a.L, i0);
            if (n > 0) vec_apply<VEC>(a, row, i0, n, s[k], mean, rstd);
        }
        if (a.stats && lane == 0) {
            a.stats[2 * row] = mean;
            a.stats[2 * row + 1] = rstd;
        }
    }
}

template <int NCH, bool VEC> __global__ __launch_bounds__(kWaveT) void tok_bwd_wave(const BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float fold[2][NCH * 64 * kV];      // the workgroup's column sums
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float fl = (float)a.L;
    float aw[NCH][kV], ab[NCH][kV];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int j = 0; j < kV; ++j) aw[k][j] = ab[k][j] = 0.f;
    for (long long row = (long long)blockIdx.x * (kWaveT / 64) + wv; row < a.rows; row += (long long)gridDim.x * (kWaveT / 64)) {
        const float mean = a.stats[2 * row], rstd = a.stats[2 * row + 1];
        float s[NCH][kV], g[NCH][kV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int i0 = (k * 64 + lane) * kV, n = valid(a.L, i0);
            if (n > 0) {
                float w[kV];
                load_sum<VEC>(a.x, a.r, row, i0, n, s[k]);
                load_grad<VEC>(a.gy, a.gy2, row, i0, n, g[k]);
                param8<VEC>(a.w, i0, n, 1.f, w);
                vec_bwd_sums(s[k], g[k], w, n, mean, rstd, s1, s2, aw[k], ab[k]);
            }
        }
        const float m1 = wave_sum(s1) / fl, m2 = wave_sum(s2) / fl;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int i0 = (k * 64 + lane) * kV, n = valid(a.L, i0);
            if (n > 0) vec_bwd_apply<VEC>(a, row, i0, n, s[k], g[k], mean, rstd, m1, m2);
        }
    }
    if (!a.ws) return;      // uniform over the grid
    for (int q = 0; q < kWaveT / 64; ++q) {      // the wavefronts add in the order 0 .. 3; a lane only touches its own columns
        if (wv == q) {
#pragma unroll
            for (int k = 0; k < NCH; ++k)
#pragma unroll
                for (int j = 0; j < kV; ++j) {
                    const int i = (k * 64 + lane) * kV + j;
                    fold[0][i] = q == 0 ? aw[k][j] : fold[0][i] + aw[k][j];
                    fold[1][i] = q == 0 ? ab[k][j] : fold[1][i] + ab[k][j];
                }
        }
        __syncthreads();
    }
    float* slot = a.ws + (long long)blockIdx.x * 2 * a.L;
    for (int i = threadIdx.x; i < a.L; i += kWaveT) {
        slot[i] = fold[0][i];
        slot[a.L + i] = fold[1][i];
    }
}

// ---- one workgroup per row ----
// the fp32 row in LDS (row + i0, nullptr: not staged) <-> 8 floats
__device__ __forceinline__ void lds_put(float* row, int i0, const float (&v)[kV]) {
    if (row) IO<float>::store(row + i0, v);
}

template <bool VEC> __global__ __launch_bounds__(kBlockT) void tok_fwd_block(const FwdArgs a, const int use_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* part = reinterpret_cast<float*>(smem);
    float* ls = use_lds ? reinterpret_cast<float*>(smem + kLdsFixed) : nullptr;
    const int t = threadIdx.x, nvec = (a.L + kV - 1) / kV;
    const float fl = (float)a.L;
    for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        float s[kV];
        float acc = 0.f;
        for (int v = t; v < nvec; v += kBlockT) {
            const int i0 = v * kV, n = valid(a.L, i0);
            load_sum<VEC>(a.x, a.r, row, i0, n, s);
            if (a.so.p) store8<VEC>(a.so, row, i0, n, s);
            lds_put(ls, i0, s);
            acc = vec_sum(s, acc);
        }
        const float mean = block_sum(acc, part) / fl;
        acc = 0.f;
        for (int v = t; v < nvec; v += kBlockT) {
            const int i0 = v * kV, n = valid(a.L, i0);
            if (ls) IO<float>::load(ls + i0, s);
            else load_sum<VEC>(a.x, a.r, row, i0, n, s);
            acc = vec_sqdev(s, n, mean, acc);
        }
        const float rstd = 1.0f / sqrtf(block_sum(acc, part) / fl + a.eps);
        for (int v = t; v < nvec; v += kBlockT) {
            const int i0 = v * kV, n = valid(a.L, i0);
            if (ls) IO<float>::load(ls + i0, s);
            else load_sum<VEC>(a.x, a.r, row, i0, n, s);
            vec_apply<VEC>(a, row, i0, n, s, mean, rstd);
        }
        if (a.stats && t == 0) {
            a.stats[2 * row] = mean;
            a.stats[2 * row + 1] = rstd;
        }
    }
}

template <bool VEC> __global__ __launch_bounds__(kBlockT) void tok_bwd_block(const BwdArgs a, const int use_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* part = reinterpret_cast<float*>(smem);
    const int t = threadIdx.x, nvec = (a.L + kV - 1) / kV;
    float* ls = use_lds ? reinterpret_cast<float*>(smem + kLdsFixed) : nullptr;
    float* lg = use_lds ? ls + (size_t)nvec * kV : nullptr;
    const float fl = (float)a.L;
    float* slot = a.ws ? a.ws + (long long)blockIdx.x * 2 * a.L : nullptr;
    for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const float mean = a.stats[2 * row], rstd = a.stats[2 * row + 1];
        const bool first = row == blockIdx.x;
        float s[kV], g[kV], w[kV];
        float s1 = 0.f, s2 = 0.f;
        for (int v = t; v < nvec; v += kBlockT) {
            const int i0 = v * kV, n = valid(a.L, i0);
            float aw[kV], ab[kV];
            load_sum<VEC>(a.x, a.r, row, i0, n, s);
            load_grad<VEC>(a.gy, a.gy2, row, i0, n, g);
            param8<VEC>(a.w, i0, n, 1.f, w);
            lds_put(ls, i0, s);
            lds_put(lg, i0, g);
            if (slot && !first) {
                ld8<float, VEC>(slot + i0, n, aw);
                ld8<float, VEC>(slot + a.L + i0, n, ab);
            } else {
#pragma unroll
                for (int j = 0; j < kV; ++j) aw[j] = ab[j] = 0.f;
            }
            vec_bwd_sums(s, g, w, n, mean, rstd, s1, s2, aw, ab);
            if (slot) {
                st8<float, VEC>(slot + i0, n, aw);
                st8<float, VEC>(slot + a.L + i0, n, ab);
            }
        }
        const float m1 = block_sum(s1, part) / fl, m2 = block_sum(s2, part) / fl;
        for (int v = t; v < nvec; v += kBlockT) {
            const int i0 = v * kV, n = valid(a.L, i0);
            if (ls) {
                IO<float>::load(ls + i0, s);
                IO<float>::load(lg + i0, g);
            } else {
                load_sum<VEC>(a.x, a.r, row, i0, n, s);
                load_grad<VEC>(a.gy, a.gy2, row, i0, n, g);
            }
            vec_bwd_apply<VEC>(a, row, i0, n, s, g, mean, rstd, m1, m2);
        }
    }
}

// gwb[i] = sum over the workgroups' slots ws[slot][i], i over [2][L]: one wave per i, lane q adds slots q, q + 64, ... in
// order in fp64, then the lanes fold by the same shuffle tree every time
__global__ __launch_bounds__(256) void tok_finish(const float* __restrict__ ws, float* __restrict__ gwb, int nslot, long long n) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wave-uniform
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int q = lane; q < nslot; q += 64) v += (double)ws[(long long)q * n + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) gwb[i] = (float)v;
}

// an absent tensor restricts nothing
bool elem_ok(const void* p, int bf) { return mk::aligned_to(p, bf ? 2 : 4); }
bool vec_ok(const void* p, long long ld, int bf) { return !p || (mk::aligned<16>(p) && (ld * (bf ? 2 : 4)) % 16 == 0); }

long long min_ll(long long a, long long b) { return a < b ? a : b; }
long long bwd_grid(long long rows, long long L) {
    return L <= kWaveMax ? min_ll(mk::ceil_div_ll(rows, kWaveT / 64), kBwdWaveGrid) : min_ll(rows, kBwdBlockGrid);
}
int chunks(int L) { return L <= 64 * kV ? 1 : L <= 128 * kV ? 2 : 4; }

template <bool VEC> int launch_fwd(const FwdArgs& a, hipStream_t st) {
    if (a.L <= kWaveMax) {
        const dim3 grid((unsigned)min_ll(mk::ceil_div_ll(a.rows, kWaveT / 64), kFwdGrid));
        switch (chunks(a.L)) {
            case 1: hipLaunchKernelGGL((tok_fwd_wave<1, VEC>), grid, dim3(kWaveT), 0, st, a); break;
            case 2: hipLaunchKernelGGL((tok_fwd_wave<2, VEC>), grid, dim3(kWaveT), 0, st, a); break;
            default: hipLaunchKernelGGL((tok_fwd_wave<4, VEC>), grid, dim3(kWaveT), 0, st, a); break;
        }
    } else {
        MK_REQUIRE_AS("mk_token_layernorm_fwd", (mk::raise_lds_limit<tok_fwd_block<VEC>>(kLdsMax) == 0),
                      "cannot raise the dynamic LDS limit on this device");
        const long long want = kLdsFixed + 4LL * mk::ceil_div_ll(a.L, kV) * kV;
        const int use_lds = want <= kLdsMax;
        hipLaunchKernelGGL((tok_fwd_block<VEC>), dim3((unsigned)min_ll(a.rows, kFwdGrid)), dim3(kBlockT),
                           (size_t)(use_lds ? want : kLdsFixed), st, a, use_lds);
    }
    MK_LAUNCH_CHECK_AS("mk_token_layernorm_fwd");
    return 0;
}

template <bool VEC> int launch_bwd(const BwdArgs& a, float* gwb, hipStream_t st) {
    const dim3 grid((unsigned)bwd_grid(a.rows, a.L));
    if (a.L <= kWaveMax) {
        switch (chunks(a.L)) {
            case 1: hipLaunchKernelGGL((tok_bwd_wave<1, VEC>), grid, dim3(kWaveT), 0, st, a); break;
            case 2: hipLaunchKernelGGL((tok_bwd_wave<2, VEC>), grid, dim3(kWaveT), 0, st, a); break;
            default: hipLaunchKernelGGL((tok_bwd_wave<4, VEC>), grid, dim3(kWaveT), 0, st, a); break;
        }
    } else {
        MK_REQUIRE_AS("mk_token_layernorm_bwd", (mk::raise_lds_limit<tok_bwd_block<VEC>>(kLdsMax) == 0),
                      "cannot raise the dynamic LDS limit on this device");
        const long long want = kLdsFixed + 8LL * mk::ceil_div_ll(a.L, kV) * kV;
        const int use_lds = want <= kLdsMax;
        hipLaunchKernelGGL((tok_bwd_block<VEC>), grid, dim3(kBlockT), (size_t)(use_lds ? want : kLdsFixed), st, a, use_lds);
    }
    MK_LAUNCH_CHECK_AS("mk_token_layernorm_bwd");
    if (gwb) {
        hipLaunchKernelGGL(tok_finish, dim3((unsigned)mk::ceil_div_ll(2LL * a.L, 4)), dim3(256), 0, st, a.ws, gwb, (int)grid.x,
                           2LL * a.L);
        MK_LAUNCH_CHECK_AS("mk_token_layernorm_bwd");
    }
    return 0;
}

bool dtype_ok(int d) { return d == 0 || d == 1; }

}  // namespace

extern "C" long long mk_token_layernorm_workspace(long long rows, long long L) {
    if (rows < 1 || L < 1) return 0;
    return bwd_grid(rows, L) * 2 * L;
}

extern "C" int mk_token_layernorm_fwd(const void* x, int x_dtype, long long x_ld, const void* r, int r_dtype, long long r_ld,
                                      const float* weight, const float* bias, void* y, int y_dtype, long long y_ld, void* y2,
                                      long long y2_ld, void* s_out, int s_dtype, long long s_ld, float* stats, long long rows,
                                      long long L, float eps, void* stream) {
    MK_REQUIRE(x && (y || y2), "null pointer: x and at least one of y, y2 are needed");
    MK_REQUIRE(rows >= 1 && L >= 1 && L <= (1 << 30) && rows < (1LL << 40), "bad sizes");
    MK_REQUIRE(dtype_ok(x_dtype) && (!r || dtype_ok(r_dtype)) && (!y || dtype_ok(y_dtype)) && (!s_out || dtype_ok(s_dtype)),
               "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(x_ld >= L && (!r || r_ld >= L) && (!y || y_ld >= L) && (!y2 || y2_ld >= L) && (!s_out || s_ld >= L),
               "a row stride is shorter than the row");
    MK_REQUIRE(elem_ok(x, x_dtype) && elem_ok(r, r_dtype) && elem_ok(y, y_dtype) && elem_ok(y2, 1) && elem_ok(s_out, s_dtype),
               "tensor not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(weight, bias, stats), "fp32 stream not aligned");
    MK_REQUIRE(eps >= 0.f, "eps must not be negative");
    const FwdArgs a{{x, x_ld, x_dtype}, {r, r_ld, r_dtype}, weight, bias, {y, y_ld, y_dtype}, {y2, y2_ld, 1}, {s_out, s_ld, s_dtype},
                    stats, rows, (int)L, eps};
    const bool vec = L % kV == 0 && vec_ok(x, x_ld, x_dtype) && vec_ok(r, r_ld, r_dtype) && vec_ok(y, y_ld, y_dtype) &&
                     vec_ok(y2, y2_ld, 1) && vec_ok(s_out, s_ld, s_dtype) && mk::aligned<16>(weight, bias);
    return vec ? launch_fwd<true>(a, (hipStream_t)stream) : launch_fwd<false>(a, (hipStream_t)stream);
}

extern "C" int mk_token_layernorm_bwd(const void* x, int x_dtype, long long x_ld, const void* r, int r_dtype, long long r_ld,
                                      const void* gy, int gy_dtype, long long gy_ld, const void* gy2, long long gy2_ld,
                                      const void* gs, int gs_dtype, long long gs_ld, const float* stats, const float* weight,
                                      void* gx, void* gr, float* workspace, float* gwb, long long rows, long long L,
                                      void* stream) {
    MK_REQUIRE(x && stats && gx, "null pointer");
    MK_REQUIRE(!gr || r, "gr without r");
    MK_REQUIRE(!gwb || workspace, "parameter gradients need the workspace");
    MK_REQUIRE(rows >= 1 && L >= 1 && L <= (1 << 30) && rows < (1LL << 40), "bad sizes");
    MK_REQUIRE(dtype_ok(x_dtype) && (!r || dtype_ok(r_dtype)) && (!gy || dtype_ok(gy_dtype)) && (!gs || dtype_ok(gs_dtype)),
               "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(x_ld >= L && (!r || r_ld >= L) && (!gy || gy_ld >= L) && (!gy2 || gy2_ld >= L) && (!gs || gs_ld >= L),
               "a row stride is shorter than the row");
    MK_REQUIRE(elem_ok(x, x_dtype) && elem_ok(gx, x_dtype) && elem_ok(r, r_dtype) && elem_ok(gr, r_dtype) && elem_ok(gy, gy_dtype) &&
                   elem_ok(gy2, 1) && elem_ok(gs, gs_dtype), "tensor not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(weight, stats, workspace, gwb), "fp32 stream not aligned");
    const BwdArgs a{{x, x_ld, x_dtype}, {r, r_ld, r_dtype}, {gy, gy_ld, gy_dtype}, {gy2, gy2_ld, 1}, {gs, gs_ld, gs_dtype}, stats, weight,
                    {gx, x_ld, x_dtype}, {gr, r_ld, r_dtype}, gwb ? workspace : nullptr, rows, (int)L};
    const bool vec = L % kV == 0 && vec_ok(x, x_ld, x_dtype) && vec_ok(gx, x_ld, x_dtype) && vec_ok(r, r_ld, r_dtype) &&
                     vec_ok(gr, r_ld, r_dtype) && vec_ok(gy, gy_ld, gy_dtype) && vec_ok(gy2, gy2_ld, 1) && vec_ok(gs, gs_ld, gs_dtype) &&
                     mk::aligned<16>(weight) && (!gwb || mk::aligned<16>(workspace));
    return vec ? launch_bwd<true>(a, gwb, (hipStream_t)stream) : launch_bwd<false>(a, gwb, (hipStream_t)stream);
}
