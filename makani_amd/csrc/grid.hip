// Latitude interpolation of [P][Hs][W] planes (fp32 or bf16) onto Hd destination rows, one pass each way (GridConverter:
// equiangular -> Legendre-Gauss).  Forward, per plane p, destination row k and column:
//   a = x'[p][i_k], b = x'[p][i_k + 1], d = fl(b - a)
//   y[p][k] = |w_k| < 0.5 ? fma(w_k, d, a) : fma(fl(w_k - 1), d, b)            (the bits of torch.lerp on the CPU)
// with x' = x, or x' = fl(fl(x - bias[c]) / scale[c]), c = p mod C (an IEEE fp32 division: the loader's numpy expression).
// i_k (int32, in [0, Hs - 2]) and w_k (fp32, any finite value) are device tables; their contents are checked where they
// are built, not here.  a == b gives a, w == 1 gives b.  The file is compiled with contraction off: what is fused is
// written as fmaf.  Backward, per source row j, from the transposed table in CSR form (terms by ascending k, the a-term
// of a destination row before its b-term):
//   gx[p][j] = (fma chain from 0 over the terms t of row j of coef_t * gy[p][k_t]) / scale[c]      (a gather: one writer)
// A source row without terms gets zeros.
//
// Decomposition.  A work item is (plane, band of kBand consecutive rows, chunk of kChunk columns) and belongs to ONE WAVE;
// a workgroup is kWaves independent waves (no LDS, no barrier), the grid is capped and strides over the items, chunk
// fastest.  The wave walks its band downwards.  Forward it keeps the two source rows of the row before in registers: a
// monotone table (the converter's) asks for row i_k + 1 again as the next row's i_k, so every source row is fetched once
// per band (plus one halo row); any other order just loads both rows.  Backward it keeps the last gy row: the a-term row
// of source row j is the b-term row of j + 1.
//
// Alignment.  Rows may start anywhere (element aligned) and the three rows of a step need not agree.  Per step the wave
// looks for a common 16-byte boundary: the scalar head `h` of the stream with the smaller element, accepted when every
// row involved is 16-byte aligned h elements in.  Then lane l takes column l of the head, the 8 columns h + 8 l of the
// body (16-byte accesses) and one column of the tail; otherwise lane l takes columns l + 64 q one by one.  Registers kept
// from the step before are reused only when the layout is the same.  Nothing outside [0, W) of a row is touched, so
// gap columns between rows and planes keep what they hold.  No atomics, no workspace: the same bits every run, capturable.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

#include <cstdint>

#pragma clang fp contract(off)   // file scope: what is fused is written as fmaf, nothing else is

namespace {

constexpr int kV = mk::sio::kVec;          // columns per lane of the vector body
constexpr int kLanes = 64;
constexpr int kChunk = kLanes * kV;        // columns of a row one wave takes (1440: three chunks, the last ragged)
constexpr int kBand = 16;                  // rows a wave walks: a halo row per band costs 1/16 of the source traffic
constexpr int kWaves = 4;                  // waves per workgroup, each with work items of its own
constexpr int kGroupsPerCU = 8;            // grid cap: 32 waves per compute unit, the rest by striding
constexpr int kScalarLayout = -1;
constexpr int kNothingHeld = -2;

using mk::sio::al16;
using mk::sio::IO;

struct Row {
    float v[kV];                           // the body (vector layout) or columns lane + 64 q (scalar layout)
    float h, t;                            // one column of the head and of the tail (vector layout)
};

template <typename T>
__device__ __forceinline__ int head_of(const T* p) {
    return (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
}

// n columns at p -> r in the layout `head` (see the top of the file), normalised on the way in
template <typename S, bool NORM>
__device__ __forceinline__ void load_row(const S* __restrict__ p, int n, int head, int lane, float bias, float scale, Row& r) {
    if (head >= 0) {
        const int nvec = (n - head) / kV, tail0 = head + nvec * kV;
        if (lane < head) r.h = IO<S>::ld1(p + lane);
        if (lane < nvec) IO<S>::load(p + head + lane * kV, r.v);
        if (lane < n - tail0) r.t = IO<S>::ld1(p + tail0 + lane);
    } else {
#pragma unroll
        for (int q = 0; q < kV; ++q)
            if (lane + kLanes * q < n) r.v[q] = IO<S>::ld1(p + lane + kLanes * q);
    }
    if (NORM) {
#pragma unroll
        for (int q = 0; q < kV; ++q) r.v[q] = (r.v[q] - bias) / scale;
        r.h = (r.h - bias) / scale;
        r.t = (r.t - bias) / scale;
    }
}

template <typename D>
__device__ __forceinline__ void store_row(D* __restrict__ p, int n, int head, int lane, const Row& r) {
    if (head >= 0) {
        const int nvec = (n - head) / kV, tail0 = head + nvec * kV;
        if (lane < head) IO<D>::st1(p + lane, r.h);
        if (lane < nvec) IO<D>::store(p + head + lane * kV, r.v);
        if (lane < n - tail0) IO<D>::st1(p + tail0 + lane, r.t);
    } else {
#pragma unroll
        for (int q = 0; q < kV; ++q)
            if (lane + kLanes * q < n) IO<D>::st1(p + lane + kLanes * q, r.v[q]);
    }
}

__device__ __forceinline__ float lerp1(float a, float b, float w, float wm1, bool small) {
    const float d = b - a;
    return small ? fmaf(w, d, a) : fmaf(wm1, d, b);
}

struct Item {
    long long plane;
    int r0, r1, c0, n;                     // rows [r0, r1) of the band, columns [c0, c0 + n)
};

__device__ __forceinline__ Item item_of(long long it, int nchunks, int nbands, int rows, int W) {
    Item m;
    const int chunk = (int)(it % nchunks);
    const long long rest = it / nchunks;
    const int band = (int)(rest % nbands);
    m.plane = rest / nbands;
    m.c0 = chunk * kChunk;
    m.n = min(kChunk, W - m.c0);
    m.r0 = band * kBand;
    m.r1 = min(rows, m.r0 + kBand);
    return m;
}

template <typename S, typename D, bool NORM>
__global__ __launch_bounds__(kWaves* kLanes) void lat_lerp_fwd_kernel(const S* __restrict__ x, D* __restrict__ y,
                                                                      const int* __restrict__ idx, const float* __restrict__ wgt,
                                                                      const float* __restrict__ bias, const float* __restrict__ scale,
                                                                      long long xps, long long xrs, long long yps, long long yrs,
                                                                      int C, int Hd, int W, int nchunks, int nbands, long long nitems) {
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // wave-uniform for the compiler too
    const long long nwaves = (long long)gridDim.x * kWaves;
    for (long long it = (long long)blockIdx.x * kWaves + wave; it < nitems; it += nwaves) {
        const Item m = item_of(it, nchunks, nbands, Hd, W);
        float bs = 0.0f, sc = 1.0f;
        if (NORM) {
            const int c = (int)(m.plane % C);
            bs = bias[c];
            sc = scale[c];
        }
        const S* xp = x + m.plane * xps + m.c0;
        D* yp = y + m.plane * yps + m.c0;
        Row a = {}, b = {}, o = {};
        int held = kNothingHeld, ia = -1;                    // a holds source row ia, b row ia + 1, both in layout `held`
        for (int k = m.r0; k < m.r1; ++k) {
            const int i = idx[k];
            const float w = wgt[k];
            const S* pa = xp + (long long)i * xrs;
            const S* pb = pa + xrs;
            D* py = yp + (long long)k * yrs;
            int head = sizeof(D) < sizeof(S) ? head_of(py) : head_of(pa);
            if (head >= m.n) head = m.n;
            else if (!(al16(pa + head) && al16(pb + head) && al16(py + head))) head = kScalarLayout;
            if (head == held && i == ia) {
                // the pair of the row before
            } else if (head == held && i == ia + 1) {
                a = b;
                load_row<S, NORM>(pb, m.n, head, lane, bs, sc, b);
            } else {
                load_row<S, NORM>(pa, m.n, head, lane, bs, sc, a);
                load_row<S, NORM>(pb, m.n, head, lane, bs, sc, b);
            }
            held = head;
            ia = i;
            const float wm1 = w - 1.0f;
            const bool small = fabsf(w) < 0.5f;
#pragma unroll
            for (int q = 0; q < kV; ++q) o.v[q] = lerp1(a.v[q], b.v[q], w, wm1, small);
            o.h = lerp1(a.h, b.h, w, wm1, small);
            o.t = lerp1(a.t, b.t, w, wm1, small);
            store_row<D>(py, m.n, head, lane, o);
        }
    }
}

// S: the type of gy, D: the type of gx
template <typename S, typename D, bool NORM>
__global__ __launch_bounds__(kWaves* kLanes) void lat_lerp_bwd_kernel(const S* __restrict__ gy, D* __restrict__ gx,
                                                                      const int* __restrict__ rowptr, const int* __restrict__ trow,
                                                                      const float* __restrict__ tcoef, const float* __restrict__ scale,
                                                                      long long gyps, long long gyrs, long long gxps, long long gxrs,
                                                                      int C, int Hs, int W, int nchunks, int nbands, long long nitems) {
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long nwaves = (long long)gridDim.x * kWaves;
    for (long long it = (long long)blockIdx.x * kWaves + wave; it < nitems; it += nwaves) {
        const Item m = item_of(it, nchunks, nbands, Hs, W);
        float sc = 1.0f;
        if (NORM) sc = scale[(int)(m.plane % C)];
        const S* gp = gy + m.plane * gyps + m.c0;
        D* xp = gx + m.plane * gxps + m.c0;
        Row g = {};
        int held = kNothingHeld, kg = -1;                    // g holds row kg of gy in layout `held`
        for (int j = m.r0; j < m.r1; ++j) {
            const int t0 = rowptr[j], t1 = rowptr[j + 1];
            D* pj = xp + (long long)j * gxrs;
            int head = (t1 > t0 && sizeof(S) < sizeof(D)) ? head_of(gp + (long long)trow[t0] * gyrs) : head_of(pj);
            if (head >= m.n) {
                head = m.n;
            } else {
                bool ok = al16(pj + head);
                for (int t = t0; t < t1; ++t) ok = ok && al16(gp + (long long)trow[t] * gyrs + head);
                if (!ok) head = kScalarLayout;
            }
            Row acc = {};
            for (int t = t0; t < t1; ++t) {
                const int k = trow[t];
                const float c = tcoef[t];
                if (!(head == held && k == kg)) {
                    load_row<S, false>(gp + (long long)k * gyrs, m.n, head, lane, 0.0f, 1.0f, g);
                    held = head;
                    kg = k;
                }
#pragma unroll
                for (int q = 0; q < kV; ++q) acc.v[q] = fmaf(c, g.v[q], acc.v[q]);
                acc.h = fmaf(c, g.h, acc.h);
                acc.t = fmaf(c, g.t, acc.t);
            }
            if (NORM) {
#pragma unroll
                for (int q = 0; q < kV; ++q) acc.v[q] = acc.v[q] / sc;
                acc.h = acc.h / sc;
                acc.t = acc.t / sc;
            }
            store_row<D>(pj, m.n, head, lane, acc);
        }
    }
}

struct Plan {
    int nchunks, nbands;
    long long nitems;
    unsigned groups;
};

inline Plan plan_of(long long P, int rows, int W) {
    Plan pl;
    pl.nchunks = mk::ceil_div(W, kChunk);
    pl.nbands = mk::ceil_div(rows, kBand);
    pl.nitems = P * pl.nbands * pl.nchunks;
    const long long want = mk::ceil_div_ll(pl.nitems, kWaves), cap = (long long)mk::cu_count() * kGroupsPerCU;
    pl.groups = (unsigned)(want < cap ? want : cap);
    return pl;
}

template <typename S, typename D, bool NORM>
void launch_fwd(const void* x, void* y, const int* idx, const float* wgt, const float* bias, const float* scale, long long xps,
                long long xrs, long long yps, long long yrs, int C, long long P, int Hd, int W, hipStream_t st) {
    const Plan pl = plan_of(P, Hd, W);
    hipLaunchKernelGGL((lat_lerp_fwd_kernel<S, D, NORM>), dim3(pl.groups), dim3(kWaves * kLanes), 0, st, (const S*)x, (D*)y, idx, wgt,
                       bias, scale, xps, xrs, yps, yrs, C, Hd, W, pl.nchunks, pl.nbands, pl.nitems);
}

template <typename S, typename D, bool NORM>
void launch_bwd(const void* gy, void* gx, const int* rowptr, const int* trow, const float* tcoef, const float* scale, long long gyps,
                long long gyrs, long long gxps, long long gxrs, int C, long long P, int Hs, int W, hipStream_t st) {
    const Plan pl = plan_of(P, Hs, W);
    hipLaunchKernelGGL((lat_lerp_bwd_kernel<S, D, NORM>), dim3(pl.groups), dim3(kWaves * kLanes), 0, st, (const S*)gy, (D*)gx, rowptr,
                       trow, tcoef, scale, gyps, gyrs, gxps, gxrs, C, Hs, W, pl.nchunks, pl.nbands, pl.nitems);
}

// what both entry points ask of their two fields (`who` names the entry point in the message)
int check_fields(const char* who, const void* src, int sdtype, long long sps, long long srs, const void* dst, int ddtype,
                 long long dps, long long drs, long long P, int Hs, int Hd, int W, int dst_rows) {
    MK_REQUIRE_AS(who, src && dst, "null pointer");
    MK_REQUIRE_AS(who, (sdtype == 0 || sdtype == 1) && (ddtype == 0 || ddtype == 1), "dtype must be 0 (fp32) or 1 (bf16)");
    MK_REQUIRE_AS(who, Hs >= 2, "Hs below 2: a destination row blends two source rows");
    MK_REQUIRE_AS(who, Hd >= 1 && W >= 1 && P >= 1, "bad sizes");
    MK_REQUIRE_AS(who, P < (1LL << 40), "too many planes");
    MK_REQUIRE_AS(who, srs >= W && drs >= W, "a row stride below W");
    MK_REQUIRE_AS(who, sps >= 0 && sps < (1LL << 44) && dps < (1LL << 44) && srs < (1LL << 44) && drs < (1LL << 44), "stride out of range");
    MK_REQUIRE_AS(who, P == 1 || dps >= (long long)(dst_rows - 1) * drs + W, "planes of the output overlap");
    MK_REQUIRE_AS(who, mk::aligned_to(src, sdtype == 0 ? 4 : 2) && mk::aligned_to(dst, ddtype == 0 ? 4 : 2),
                  "a field is not aligned to its element");
    return 0;
}

}  // namespace

extern "C" int mk_lat_lerp_chunk(void) { return kChunk; }

extern "C" int mk_lat_lerp_fwd(const void* x, int xdtype, long long xpstride, long long xrstride, void* y, int ydtype,
                               long long ypstride, long long yrstride, const int* idx, const float* wgt, const float* bias,
                               const float* scale, int C, long long P, int Hs, int Hd, int W, void* stream) {
    if (check_fields(__func__, x, xdtype, xpstride, xrstride, y, ydtype, ypstride, yrstride, P, Hs, Hd, W, Hd)) return 1;
    MK_REQUIRE(idx && wgt, "null table pointer");
    MK_REQUIRE(mk::aligned<4>(idx, wgt, bias, scale), "a table is not 4-byte aligned");
    MK_REQUIRE((bias == nullptr) == (scale == nullptr), "bias and scale come together");
    MK_REQUIRE(!bias || C >= 1, "C below 1");
    hipStream_t st = (hipStream_t)stream;
#define MK_GRID_ARGS x, y, idx, wgt, bias, scale, xpstride, xrstride, ypstride, yrstride, C, P, Hd, W, st
#define MK_GRID_CASE(S, D)                                   \
    do {                                                     \
        if (bias) launch_fwd<S, D, true>(MK_GRID_ARGS);      \
        else launch_fwd<S, D, false>(MK_GRID_ARGS);          \
    } while (0)
    if (xdtype == 0 && ydtype == 0) MK_GRID_CASE(float, float);
    else if (xdtype == 0) MK_GRID_CASE(float, __hip_bfloat16);
    else if (ydtype == 0) MK_GRID_CASE(__hip_bfloat16, float);
    else MK_GRID_CASE(__hip_bfloat16, __hip_bfloat16);
#undef MK_GRID_CASE
#undef MK_GRID_ARGS
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_lat_lerp_bwd(const void* gy, int gydtype, long long gypstride, long long gyrstride, void* gx, int gxdtype,
                               long long gxpstride, long long gxrstride, const int* rowptr, const int* term_row,
                               const float* term_coef, const float* scale, int C, long long P, int Hs, int Hd, int W, void* stream) {
    if (check_fields(__func__, gy, gydtype, gypstride, gyrstride, gx, gxdtype, gxpstride, gxrstride, P, Hs, Hd, W, Hs)) return 1;
    MK_REQUIRE(rowptr && term_row && term_coef, "null table pointer");
    MK_REQUIRE(mk::aligned<4>(rowptr, term_row, term_coef, scale), "a table is not 4-byte aligned");
    MK_REQUIRE(!scale || C >= 1, "C below 1");
    hipStream_t st = (hipStream_t)stream;
#define MK_GRID_ARGS gy, gx, rowptr, term_row, term_coef, scale, gypstride, gyrstride, gxpstride, gxrstride, C, P, Hs, W, st
#define MK_GRID_CASE(S, D)                                   \
    do {                                                     \
        if (scale) launch_bwd<S, D, true>(MK_GRID_ARGS);     \
        else launch_bwd<S, D, false>(MK_GRID_ARGS);          \
    } while (0)
    if (gydtype == 0 && gxdtype == 0) MK_GRID_CASE(float, float);
    else if (gydtype == 0) MK_GRID_CASE(float, __hip_bfloat16);
    else if (gxdtype == 0) MK_GRID_CASE(__hip_bfloat16, float);
    else MK_GRID_CASE(__hip_bfloat16, __hip_bfloat16);
#undef MK_GRID_CASE
#undef MK_GRID_ARGS
    MK_LAUNCH_CHECK();
    return 0;
}
