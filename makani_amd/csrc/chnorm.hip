// Layer norm over the CHANNEL axis of a contiguous NCHW field x[B][C][P], P = H * W, per (b, p): the norm of
// DistributedLayerNorm (makani/mpu/layer_norm.py:117-155, transpose -> nn.LayerNorm -> transpose) without the transposes.
//   mean = sum_c x / C,  var = sum_c (x - mean)^2 / C (biased, two passes),  rstd = 1 / sqrt(var + eps),
//   y_c = act(w_c (x_c - mean) rstd + b_c),  act = exact GELU when fused.
//
// Tiling.  A workgroup of 512 threads owns a tile of TP consecutive pixels of one sample over ALL channels; a channel
// row of the tile is 128 bytes of the input (TP = 32 fp32 / 64 bf16 pixels), eight lanes with one 16-byte vector each,
// so a wave moves eight rows of 128 contiguous bytes per instruction and the 64 "row groups" (threadIdx / 8) of the
// workgroup walk the channels c = rg, rg + 64, ...  The tile is read from HBM once into LDS in the input's own dtype
// (384 channels: 48 KiB) and every later use -- mean, centred variance, apply -- is served from there.  When the tile
// does not fit the 160 KiB (C beyond ~1200 fp32 forward, ~600 backward) the same passes read the tile from global
// memory again (it was just fetched: L2), one element at a time.
//
// Fixed arithmetic per pixel.  A lane accumulates its pixels over the channels of its row group in increasing c, the
// 64 per-row-group partials of a pixel are exchanged through LDS and added in the order rg = 0 .. 63 by one thread.
// The order depends on nothing but C: not on the pixel's place in the tile, the row or the tensor, and not on how the
// tile was brought in (16-byte vectors when P is a multiple of the vector and the pointers are 16-byte aligned, single
// elements otherwise) -- the two paths differ in the copy to LDS and in the stores only.  A spatial shard therefore gives
// the bits of the same slice of the full field.  Contraction is off in this file; the fused operations are spelled fmaf.
//
// Backward.  With xh = (x - mean) rstd, g = gy (or gy gelu'(w xh + b)), s1 = sum_c w g, s2 = sum_c w g xh:
//   gx_c = rstd (w_c g_c - s1 / C - xh_c s2 / C),  gw_c = sum_{b,p} g_c xh_c,  gb_c = sum_{b,p} g_c.
// x and gy tiles sit in LDS; g is recomputed in the second pass (nothing but x and (mean, rstd) is saved by the forward).
// The workgroups are persistent (tile = blockIdx, + gridDim, ...): the channel sums of a tile are folded over the eight
// lanes of a row by a fixed shuffle tree and added, by the one lane that owns the channel, to fp32 accumulators of the
// workgroup; each workgroup writes its [2][C] partials to a workspace slot of its own and a finishing launch adds the
// slots in a fixed order in fp64.  No atomics: bitwise repeatable.
#include "common.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cstdint>

#pragma clang fp contract(off)   // file scope: what is fused is written as fmaf, nothing else is

#include "gelu.h"   // below the pragma: its products and sums stay unfused here, as everything else in this file

namespace {

constexpr int kT = 512;                    // threads per workgroup (8 waves)
constexpr int kLanes = 8;                  // lanes along a channel row of the tile (8 x 16 bytes = 128 bytes of input)
constexpr int kRG = kT / kLanes;           // row groups: channel c belongs to row group c % kRG
constexpr int kLdsMax = 160 * 1024;        // LDS of a CU, and the most one workgroup may take
constexpr int kBwdGrid = 1024;             // backward: at most this many (persistent) workgroups
constexpr int kFwdGrid = 1 << 20;          // forward: one tile per workgroup up to here, strided beyond
constexpr int kMinTP = 32;                 // the smaller of the two tile widths (fp32 input)

using bf16 = __hip_bfloat16;
using mk::gelu::Act;

template <int BYTES> struct alignas(BYTES > 16 ? 16 : BYTES) Raw { unsigned int w[BYTES / 4]; };

// N elements of T at p (aligned to min(16, N sizeof(T)) bytes) <-> N floats.  Kept apart from IO<T> of stream_io.h: with either
// spelling of the store for both, kernels here or there came out with other instructions
template <typename T, int N> __device__ __forceinline__ void load_n(const T* p, float (&v)[N]) {
    const Raw<N * (int)sizeof(T)> r = *reinterpret_cast<const Raw<N * (int)sizeof(T)>*>(p);
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __uint_as_float(r.w[i]);
    } else {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            v[2 * i] = __uint_as_float(r.w[i] << 16);
            v[2 * i + 1] = __uint_as_float(r.w[i] & 0xffff0000u);
        }
    }
}
__device__ __forceinline__ unsigned int bf16_bits(float v) {
    const bf16 h = __float2bfloat16(v);      // round to nearest even, NaN safe
    return (unsigned int)*reinterpret_cast<const unsigned short*>(&h);
}
template <typename T, int N> __device__ __forceinline__ void store_n(T* p, const float (&v)[N]) {
    Raw<N * (int)sizeof(T)> r;
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < N; ++i) r.w[i] = __float_as_uint(v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) r.w[i] = bf16_bits(v[2 * i]) | (bf16_bits(v[2 * i + 1]) << 16);
    }
    *reinterpret_cast<Raw<N * (int)sizeof(T)>*>(p) = r;
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16* p) { return __bfloat162float(*p); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16* p, float v) { *p = __float2bfloat16(v); }
__device__ __forceinline__ void zero1(float* p) { *p = 0.f; }
__device__ __forceinline__ void zero1(bf16* p) { *reinterpret_cast<unsigned short*>(p) = 0; }

// One stream of a tile: rows of TP pixels, served from LDS (row c at lds + c * TP) or, when the tile does not fit, from
// global memory (row c at glob + c * P, pixels past `np` read as zero).  V = pixels per lane.
template <typename T, int V> struct TileView {
    static constexpr int TP = kLanes * V;
    const T* glob;      // pixel 0 of channel 0 of the tile
    T* lds;             // null: global mode
    long long P;
    int np;             // valid pixels of the tile (1 .. TP)

    // bring the tile into LDS (no-op in global mode); pixels past np are zero
    __device__ __forceinline__ void fill(int C, bool aligned) const {
        if (!lds) return;
        const int l = threadIdx.x % kLanes, r0 = threadIdx.x / kLanes;
        if (aligned) {      // np is a multiple of V here: a vector is all valid or all beyond the field
            for (int c = r0; c < C; c += kRG) {
                using R = Raw<V * (int)sizeof(T)>;
                R* dst = reinterpret_cast<R*>(lds + c * TP + l * V);
                if (l * V < np) *dst = *reinterpret_cast<const R*>(glob + (long long)c * P + l * V);
                else *dst = R{};
            }
        } else {
            const int n = C * TP;
            for (int i = threadIdx.x; i < n; i += kT) {
                const int c = i / TP, p = i % TP;
                if (p < np) lds[i] = glob[(long long)c * P + p];
                else zero1(lds + i);
            }
        }
    }
    // the V pixels of this lane in channel row c
    __device__ __forceinline__ void get(int c, float (&v)[V]) const {
        const int l = threadIdx.x % kLanes;
        if (lds) {
            load_n<T, V>(lds + c * TP + l * V, v);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = (l * V + i < np) ? ld1(glob + (long long)c * P + l * V + i) : 0.f;
        }
    }
};

// the V pixels of this lane in channel row c of an output tile
template <typename T, int V>
__device__ __forceinline__ void put(T* glob, long long P, int np, bool aligned, int c, const float (&v)[V]) {
    const int l = threadIdx.x % kLanes;
    T* row = glob + (long long)c * P + l * V;
    if (aligned) {
        if (l * V < np) store_n<T, V>(row, v);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (l * V + i < np) st1(row + i, v[i]);
    }
}

template <int V> __device__ __forceinline__ void put_partials(float* part, const float (&s)[V]) {
    const int l = threadIdx.x % kLanes, r0 = threadIdx.x / kLanes;
    store_n<float, V>(part + r0 * (kLanes * V) + l * V, s);
}
// sum over the row groups in the order 0 .. kRG - 1 for pixel p of the tile
template <int TP> __device__ __forceinline__ float fold_partials(const float* part, int p) {
    float s = 0.f;
#pragma unroll 8
    for (int rg = 0; rg < kRG; ++rg) s += part[rg * TP + p];
    return s;
}

__host__ __device__ constexpr int acc_floats(int C) { return (2 * C + 3) & ~3; }
template <typename TI> constexpr int tile_px() { return kLanes * (16 / (int)sizeof(TI)); }
// LDS bytes in front of the tiles
template <typename TI> constexpr int fwd_lds_fixed() { return (kRG * tile_px<TI>() + 2 * tile_px<TI>()) * 4; }
// backward: pixels per lane = one 16-byte vector of the WIDER of x and gy, so that neither row of a tile exceeds 128 bytes (bf16 x
// with fp32 gy -- a bf16 field whose norm returned fp32 -- stages 32 pixels: 64-byte rows of x, 128-byte rows of gy)
template <typename TX, typename TG> constexpr int bwd_v() { return 16 / (int)(sizeof(TX) > sizeof(TG) ? sizeof(TX) : sizeof(TG)); }
constexpr int bwd_lds_fixed(int tp) { return (2 * kRG * tp + 4 * tp) * 4; }

template <typename TI, typename TO, bool GELU>
__global__ __launch_bounds__(kT) void chan_layernorm_fwd_kernel(const TI* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ b, TO* __restrict__ y,
                                                                float* __restrict__ stats, int C, long long P,
                                                                long long tiles_per_sample, long long ntiles, float eps,
                                                                int use_lds, int aligned) {
    constexpr int V = 16 / (int)sizeof(TI), TP = kLanes * V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* part = reinterpret_cast<float*>(smem);      // [kRG][TP]
    float* stat = part + kRG * TP;                     // [TP][2] = (mean, rstd)
    const int t = threadIdx.x, l = t % kLanes, r0 = t / kLanes;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long bs = tile / tiles_per_sample;
    const long long p0 = (tile - bs * tiles_per_sample) * TP;
    const int np = (int)(P - p0 < TP ? P - p0 : TP);
    const long long base = bs * C * P + p0;
    TileView<TI, V> xt{x + base, use_lds ? reinterpret_cast<TI*>(stat + 2 * TP) : nullptr, P, np};
    xt.fill(C, aligned);
    __syncthreads();

    float acc[V], v[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int c = r0; c < C; c += kRG) {
        xt.get(c, v);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += v[i];
    }
    put_partials<V>(part, acc);
    __syncthreads();
    if (t < TP) stat[2 * t] = fold_partials<TP>(part, t) / (float)C;
    __syncthreads();

    float m[V], r[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        m[i] = stat[2 * (l * V + i)];
        acc[i] = 0.f;
    }
    for (int c = r0; c < C; c += kRG) {
        xt.get(c, v);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float d = v[i] - m[i];
            acc[i] = fmaf(d, d, acc[i]);
        }
    }
    put_partials<V>(part, acc);
    __syncthreads();
    if (t < TP) {
        const float var = fold_partials<TP>(part, t) / (float)C;
        const float rs = 1.0f / sqrtf(var + eps);
        stat[2 * t + 1] = rs;
        if (stats && t < np) {
            float* sp = stats + (bs * P + p0 + t) * 2;
            sp[0] = stat[2 * t];
            sp[1] = rs;
        }
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = stat[2 * (l * V + i) + 1];
    for (int c = r0; c < C; c += kRG) {
        xt.get(c, v);
        const float wc = w ? w[c] : 1.f, bc = b ? b[c] : 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float z = fmaf(wc, (v[i] - m[i]) * r[i], bc);
            v[i] = GELU ? Act<TO>::gelu(z) : z;
        }
        put<TO, V>(y + base, P, np, aligned, c, v);
    }
    __syncthreads();      // a next tile overwrites the LDS tile and `stat`
    }
}

template <typename TX, typename TG, bool GELU>
__global__ __launch_bounds__(kT) void chan_layernorm_bwd_kernel(const TX* __restrict__ x, const TG* __restrict__ gy,
                                                                const float* __restrict__ stats, const float* __restrict__ w,
                                                                const float* __restrict__ b, TX* __restrict__ gx,
                                                                float* __restrict__ ws, int C, long long P,
                                                                long long tiles_per_sample, long long ntiles, int use_lds,
                                                                int aligned) {
    constexpr int V = bwd_v<TX, TG>(), TP = kLanes * V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* part = reinterpret_cast<float*>(smem);      // [2][kRG][TP]
    float* fin = part + 2 * kRG * TP;                  // [TP][4] = (mean, rstd, s1 / C, s2 / C)
    float* lds_acc = fin + 4 * TP;                     // [2][C] (LDS mode), padded to 16 bytes
    TX* lds_x = reinterpret_cast<TX*>(lds_acc + acc_floats(C));
    TG* lds_g = reinterpret_cast<TG*>(lds_x + (size_t)C * TP);
    const int t = threadIdx.x, l = t % kLanes, r0 = t / kLanes;
    // channel sums of this workgroup: row 0 = sum g xh (weight), row 1 = sum g (bias).  Channel c is only ever touched by
    // the lane (c % kRG, 0), so the accumulators need no barrier of their own, in LDS or in the workgroup's workspace slot.
    float* acc = !ws ? nullptr : (use_lds ? lds_acc : ws + (long long)blockIdx.x * 2 * C);
    if (acc && l == 0)
        for (int c = r0; c < C; c += kRG) {
            acc[c] = 0.f;
            acc[C + c] = 0.f;
        }

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long bs = tile / tiles_per_sample;
        const long long p0 = (tile - bs * tiles_per_sample) * TP;
        const int np = (int)(P - p0 < TP ? P - p0 : TP);
        const long long base = bs * C * P + p0;
        TileView<TX, V> xt{x + base, use_lds ? lds_x : nullptr, P, np};
        TileView<TG, V> gt{gy + base, use_lds ? lds_g : nullptr, P, np};
        xt.fill(C, aligned);
        gt.fill(C, aligned);
        if (t < TP) {      // pixels beyond the field: mean = rstd = 0, and with the zero x and gy every term vanishes
            const float* sp = stats + (bs * P + p0 + t) * 2;
            fin[4 * t] = t < np ? sp[0] : 0.f;
            fin[4 * t + 1] = t < np ? sp[1] : 0.f;
        }
        __syncthreads();

        float m[V], r[V], s1[V], s2[V], xv[V], gv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            m[i] = fin[4 * (l * V + i)];
            r[i] = fin[4 * (l * V + i) + 1];
            s1[i] = 0.f;
            s2[i] = 0.f;
        }
        for (int c = r0; c < C; c += kRG) {
            xt.get(c, xv);
            gt.get(c, gv);
            const float wc = w ? w[c] : 1.f, bc = b ? b[c] : 0.f;
            float a = 0.f, bsum = 0.f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float xh = (xv[i] - m[i]) * r[i];
                const float g = GELU ? gv[i] * Act<TX>::gelu_grad(fmaf(wc, xh, bc)) : gv[i];
                const float wg = wc * g;
                s1[i] += wg;
                s2[i] = fmaf(wg, xh, s2[i]);
                a = fmaf(g, xh, a);
                bsum += g;
            }
            if (acc) {      // uniform over the workgroup; the eight lanes of a row are active together
#pragma unroll
                for (int o = 1; o < kLanes; o <<= 1) {
                    a += __shfl_xor(a, o, 64);
                    bsum += __shfl_xor(bsum, o, 64);
                }
                if (l == 0) {
                    acc[c] += a;
                    acc[C + c] += bsum;
                }
            }
        }
        put_partials<V>(part, s1);
        put_partials<V>(part + kRG * TP, s2);
        __syncthreads();
        if (t < 2 * TP) {
            const int q = t / TP, p = t % TP;
            fin[4 * p + 2 + q] = fold_partials<TP>(part + q * kRG * TP, p) / (float)C;
        }
        __syncthreads();

        float m1[V], m2[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            m1[i] = fin[4 * (l * V + i) + 2];
            m2[i] = fin[4 * (l * V + i) + 3];
        }
        for (int c = r0; c < C; c += kRG) {
            xt.get(c, xv);
            gt.get(c, gv);
            const float wc = w ? w[c] : 1.f, bc = b ? b[c] : 0.f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float xh = (xv[i] - m[i]) * r[i];
                const float g = GELU ? gv[i] * Act<TX>::gelu_grad(fmaf(wc, xh, bc)) : gv[i];
                xv[i] = r[i] * ((wc * g - m1[i]) - xh * m2[i]);
            }
            put<TX, V>(gx + base, P, np, aligned, c, xv);
        }
        __syncthreads();      // the next tile overwrites the LDS tiles and `fin`
    }
    if (acc && use_lds && l == 0) {
        float* slot = ws + (long long)blockIdx.x * 2 * C;
        for (int c = r0; c < C; c += kRG) {
            slot[c] = acc[c];
            slot[C + c] = acc[C + c];
        }
    }
}

// gwb[i] = sum over the workgroups' slots ws[slot][i], i over [2][C]: one wave per i, lane q adds slots q, q + 64, ... in
// order in fp64, then the lanes fold by the same shuffle tree every time
__global__ __launch_bounds__(256) void chan_layernorm_finish(const float* __restrict__ ws, float* __restrict__ gwb, int nslot,
                                                             int n) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wave-uniform
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int q = lane; q < nslot; q += 64) v += (double)ws[(long long)q * n + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) gwb[i] = (float)v;
}

long long bwd_grid(long long ntiles) { return ntiles < kBwdGrid ? ntiles : kBwdGrid; }

template <typename TI, typename TO, bool GELU>
int launch_fwd(const void* x, const float* w, const float* b, void* y, float* stats, int B, int C, long long P, float eps,
               hipStream_t st) {
    constexpr int TP = tile_px<TI>();
    MK_REQUIRE((mk::raise_lds_limit<chan_layernorm_fwd_kernel<TI, TO, GELU>>(kLdsMax) == 0), "cannot raise the dynamic LDS limit on this device");
    const long long tps = mk::ceil_div_ll(P, TP), ntiles = tps * B;
    const long long grid = ntiles < kFwdGrid ? ntiles : kFwdGrid;
    const long long want = fwd_lds_fixed<TI>() + (long long)C * TP * (long long)sizeof(TI);
    const int use_lds = want <= kLdsMax;
    const int aligned = P % (16 / (int)sizeof(TI)) == 0 && mk::aligned<16>(x, y);
    hipLaunchKernelGGL((chan_layernorm_fwd_kernel<TI, TO, GELU>), dim3((unsigned)grid), dim3(kT),
                       (size_t)(use_lds ? want : fwd_lds_fixed<TI>()), st, (const TI*)x, w, b, (TO*)y, stats, C, P, tps, ntiles,
                       eps, use_lds, aligned);
    MK_LAUNCH_CHECK();
    return 0;
}

template <typename TX, typename TG, bool GELU>
int launch_bwd(const void* x, const void* gy, const float* stats, const float* w, const float* b, void* gx, float* ws,
               float* gwb, int B, int C, long long P, hipStream_t st) {
    constexpr int V = bwd_v<TX, TG>(), TP = kLanes * V;
    MK_REQUIRE((mk::raise_lds_limit<chan_layernorm_bwd_kernel<TX, TG, GELU>>(kLdsMax) == 0), "cannot raise the dynamic LDS limit on this device");
    const long long tps = mk::ceil_div_ll(P, TP), ntiles = tps * B;
    const long long fixed = bwd_lds_fixed(TP);
    const long long want = fixed + 4LL * acc_floats(C) + (long long)C * TP * (long long)(sizeof(TX) + sizeof(TG));
    const int use_lds = want <= kLdsMax;
    const int aligned = P % V == 0 && mk::aligned<16>(x, gy, gx);
    const long long grid = bwd_grid(ntiles);
    hipLaunchKernelGGL((chan_layernorm_bwd_kernel<TX, TG, GELU>), dim3((unsigned)grid), dim3(kT),
                       (size_t)(use_lds ? want : fixed), st, (const TX*)x, (const TG*)gy, stats, w, b, (TX*)gx,
                       gwb ? ws : nullptr, C, P, tps, ntiles, use_lds, aligned);
    MK_LAUNCH_CHECK();
    if (gwb) {
        hipLaunchKernelGGL(chan_layernorm_finish, dim3((unsigned)mk::ceil_div(2 * C, 4)), dim3(256), 0, st, ws, gwb, (int)grid,
                           2 * C);
        MK_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" long long mk_chan_layernorm_workspace(int B, int C, long long P) {
    if (B < 1 || C < 1 || P < 1) return 0;
    return bwd_grid(mk::ceil_div_ll(P, kMinTP) * B) * 2 * C;
}

extern "C" int mk_chan_layernorm_fwd(const void* x, int x_dtype, const float* weight, const float* bias, void* y, int y_dtype,
                                     float* stats, int B, int C, long long P, float eps, int fuse_gelu, void* stream) {
    MK_REQUIRE(x && y, "null pointer");
    MK_REQUIRE(B >= 1 && C >= 1 && P >= 1, "bad sizes");
    MK_REQUIRE(C <= (1 << 24) && (long long)B * C * P < (1LL << 40), "field too large");
    MK_REQUIRE((x_dtype == 0 || x_dtype == 1) && (y_dtype == 0 || y_dtype == 1), "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(mk::aligned_to(x, x_dtype == 0 ? 4 : 2) && mk::aligned_to(y, y_dtype == 0 ? 4 : 2), "field not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(weight, bias) && mk::aligned<8>(stats), "fp32 stream not aligned");
    MK_REQUIRE(eps >= 0.f, "eps must not be negative");
    hipStream_t st = (hipStream_t)stream;
    const int k = x_dtype * 4 + y_dtype * 2 + (fuse_gelu ? 1 : 0);
    switch (k) {
        case 0: return launch_fwd<float, float, false>(x, weight, bias, y, stats, B, C, P, eps, st);
        case 1: return launch_fwd<float, float, true>(x, weight, bias, y, stats, B, C, P, eps, st);
        case 2: return launch_fwd<float, bf16, false>(x, weight, bias, y, stats, B, C, P, eps, st);
        case 3: return launch_fwd<float, bf16, true>(x, weight, bias, y, stats, B, C, P, eps, st);
        case 4: return launch_fwd<bf16, float, false>(x, weight, bias, y, stats, B, C, P, eps, st);
        case 5: return launch_fwd<bf16, float, true>(x, weight, bias, y, stats, B, C, P, eps, st);
        case 6: return launch_fwd<bf16, bf16, false>(x, weight, bias, y, stats, B, C, P, eps, st);
        default: return launch_fwd<bf16, bf16, true>(x, weight, bias, y, stats, B, C, P, eps, st);
    }
}

extern "C" int mk_chan_layernorm_bwd(const void* x, int x_dtype, const void* gy, int gy_dtype, const float* stats,
                                     const float* weight, const float* bias, void* gx, float* workspace, float* gwb, int B, int C,
                                     long long P, int fuse_gelu, void* stream) {
    MK_REQUIRE(x && gy && stats && gx, "null pointer");
    MK_REQUIRE(!gwb || workspace, "parameter gradients need the workspace");
    MK_REQUIRE(B >= 1 && C >= 1 && P >= 1, "bad sizes");
    MK_REQUIRE(C <= (1 << 24) && (long long)B * C * P < (1LL << 40), "field too large");
    MK_REQUIRE((x_dtype == 0 || x_dtype == 1) && (gy_dtype == 0 || gy_dtype == 1), "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE(mk::aligned_to(x, x_dtype == 0 ? 4 : 2) && mk::aligned_to(gx, x_dtype == 0 ? 4 : 2) &&
                   mk::aligned_to(gy, gy_dtype == 0 ? 4 : 2), "field not aligned to its element");
    MK_REQUIRE(mk::aligned<4>(weight, bias, workspace, gwb) && mk::aligned<8>(stats), "fp32 stream not aligned");
    hipStream_t st = (hipStream_t)stream;
    const int k = x_dtype * 4 + gy_dtype * 2 + (fuse_gelu ? 1 : 0);
    switch (k) {
        case 0: return launch_bwd<float, float, false>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        case 1: return launch_bwd<float, float, true>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        case 2: return launch_bwd<float, bf16, false>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        case 3: return launch_bwd<float, bf16, true>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        case 4: return launch_bwd<bf16, float, false>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        case 5: return launch_bwd<bf16, float, true>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        case 6: return launch_bwd<bf16, bf16, false>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
        default: return launch_bwd<bf16, bf16, true>(x, gy, stats, weight, bias, gx, workspace, gwb, B, C, P, st);
    }
}
