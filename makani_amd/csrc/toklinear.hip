// Token-major linear layers on bf16 MFMA: nn.Linear on [rows, features] activations with [out, in] weights, the qkv / proj /
// fc1 / fc2 / head products of the ViT and the "traditional" MLP and EncoderDecoder.  Both operands are contiguous along the
// contraction, so either one is an MFMA fragment as it lies in memory.
//
//   mk_token_linear_pack       weight (fp32 or bf16 [O, I]) -> bf16 image [O, I], or transposed [I, O]
//   mk_token_linear_fwd        acc[r, o] = sum_i X[r, i] W[o, i] with one of four epilogues; with the transposed image of the
//                              weight and the output gradient as X it is the data gradient as well
//   mk_token_linear_gelu_grad  g * gelu'(pre), the one pointwise pass of a single linear + GELU's backward
//   mk_token_linear_wgrad      dW[o, i] = sum_r dY[r, o] X[r, i] and db[o] = sum_r dY[r, o]: token slabs, then a sum in slab order
//
// Plain C++ on v_mfma_f32_32x32x16_bf16: no inline assembly, no LDS-DMA, nothing summed across workgroups by atomics and no
// workgroup waits on another, so the same inputs give the same bits.  256 threads are 4 waves of 64 x 64 results each (2 x 2
// MFMA tiles); the swept tiles go global -> registers -> LDS with the loads of step t + 1 in flight under the MFMAs of step t,
// as in attn.hip.  The weight (forward) is the A operand, so an accumulator holds 4 consecutive outputs of one token in
// registers 4 g .. 4 g + 3; the epilogue passes the result tile (and the auxiliary's and the addend's) through the LDS of the
// images, so that memory is read and written in whole rows of the tile, 16 bytes a lane.  Row images are XOR-swizzled in 16-byte chunks (chunk ^ (row & 7)); the weight gradient
// contracts over tokens: it keeps token-major images and reads them feature-major with ds_read_b64_tr_b16 (the compiler
// builtin).  A ragged last tile loads zeros and stores nothing in every axis; memory past a row's length is neither read nor
// written.
#include "common.h"
#include "gelu.h"
#include "mfma_tile.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>
#include <cstdint>

namespace {

using mk::mfma::bf16x2;
using mk::mfma::bf16x4;
using mk::mfma::bf16x8;
using mk::mfma::bf_hi;
using mk::mfma::bf_lo;
using mk::mfma::f32x16;
using mk::mfma::read_row_frag;
using mk::mfma::s16x4;
using mk::mfma::tile_row;
using mk::mfma::zero;
typedef __hip_bfloat16 bf16;
using Gelu = mk::gelu::Act<__hip_bfloat16>;

constexpr int kT = 256;                                  // 4 waves
constexpr int kTR = 128, kTC = 128, kTK = 64;            // forward: rows, outputs, contraction step
constexpr int kTO = 128, kTI = 128, kTS = 64;            // weight gradient: outputs, inputs, token step
constexpr int kMaxSlabs = 64;

// ---- a [128][64] tile of a [rows, K] operand: rows of the image are rows of the operand ---------------------------------------
using RowStage = mk::mfma::RowStage<kTR, kTK, kT>;

// ---- a [64 tokens][128 features] tile of an operand that is contracted over its tokens ---------------------------------------
// The image stays token-major as it comes from memory (16-byte stores); ds_read_b64_tr_b16 delivers it feature-major: per group
// of 16 lanes a block of 4 tokens x 16 features, lane 4 q + p giving the address of token q, features 4 p .. 4 p + 3, lane i
// receiving feature i of the 4 tokens (tools/ub/tr_read_ub.hip checks these semantics).  Every lane takes part in every read.
// 16-byte chunk ch of token `row` lies at tok_off: the XOR keeps the transposed reads free of bank conflicts on 256-byte rows.
__device__ __forceinline__ int tok_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

struct TokStage {
    uint4 r[4];
    __device__ __forceinline__ void load(const bf16* base, long long ld, long long rows_valid, int f_valid, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + i * kT, row = v >> 4, c = v & 15;
            r[i] = (row < rows_valid && c * 8 < f_valid) ? *reinterpret_cast<const uint4*>(base + row * ld + c * 8) : make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void put(char* img, int tid) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + i * kT, row = v >> 4, c = v & 15;
            *reinterpret_cast<uint4*>(img + tok_off(row, c)) = r[i];
        }
    }
    // this thread's 8 features (c = tid & 15 in every register) summed over its 4 tokens, in register order
    __device__ __forceinline__ void add_columns(float (&s)[8]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) s[2 * e] += bf_lo(w[e]), s[2 * e + 1] += bf_hi(w[e]);
        }
    }
};
constexpr int kTokBytes = kTS * kTO * 2;
// the MFMA operand of feature f0 + (lane & 31) over the 8 tokens 16 ks + 8 (lane >> 5) .. + 7: two transposed block reads
__device__ __forceinline__ bf16x8 read_tr_frag(char* img, int f0, int ks, int lane) {
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const int ch = (f0 >> 3) + 2 * ((lane >> 4) & 1) + (p >> 1);
    struct { s16x4 lo, hi; } v;
    const int row = 16 * ks + 8 * (lane >> 5) + q;
    v.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (s16x4 __attribute__((address_space(3)))*)(__attribute__((address_space(3))) char*)(img + tok_off(row, ch) + 8 * (p & 1)));
    v.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (s16x4 __attribute__((address_space(3)))*)(__attribute__((address_space(3))) char*)(img + tok_off(row + 4, ch) + 8 * (p & 1)));
    return __builtin_bit_cast(bf16x8, v);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// 16-byte chunk ch (of CH in a row) of row `row` of the result tile in LDS: [128][128] bf16 (CH 16) or [64][128] fp32 (CH 32), both
// 32 KB.  The XOR spreads the 32 rows that a wave writes with one instruction over the banks.
template <int CH>
__device__ __forceinline__ int epi_off(int row, int ch) { return row * (CH * 16) + ((ch ^ (row & (CH - 1))) << 4); }

enum Mode { kPlain = 0, kGelu = 1, kAddend = 2, kAux = 3 };

struct FwdParams {
    const bf16 *x, *w, *aux;
    const float *bias, *addend;
    bf16 *y, *pre;                  // y: the bf16 result of the mode (y, act or the GELU'-scaled product)
    float* out;
    long long ldx, ldw, ldy, ldpre, ldadd, ldout, ldaux, R;
    int O, I, n_ot;
};

template <int MODE>
__global__ __launch_bounds__(kT) void toklinear_fwd_kernel(FwdParams p) {
    __shared__ __attribute__((aligned(16))) char lds[kTR * kTK * 2 + kTC * kTK * 2];        // 32 KB: the two images, then the result tile
    char* const x_img = lds;
    char* const w_img = lds + kTR * kTK * 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const int wr = wave >> 1, wo = wave & 1;            // the wave's 64 rows and 64 outputs of the tile
    const long long bid = blockIdx.x;
    const int ot = (int)(bid % p.n_ot);                 // output tiles of one row tile are neighbours: X stays in L2
    const long long r0 = (bid / p.n_ot) * kTR;
    const int o0 = ot * kTC;
    const bf16* xb = p.x + r0 * p.ldx;
    const bf16* wb = p.w + (long long)o0 * p.ldw;
    const long long rows_x = p.R - r0, rows_w = p.O - o0;

    f32x16 acc[2][2];                                   // [output tile][row tile]
    zero(acc);
    RowStage stx, stw;
    const int nk = (p.I + kTK - 1) / kTK;
    stx.load(xb, p.ldx, rows_x, p.I, tid);
    stw.load(wb, p.ldw, rows_w, p.I, tid);
    for (int t = 0; t < nk; ++t) {
        __syncthreads();                                // the previous step's reads are done
        stx.put(x_img, tid);
        stw.put(w_img, tid);
        __syncthreads();
        if (t + 1 < nk) {
            const int k1 = (t + 1) * kTK;
            stx.load(xb + k1, p.ldx, rows_x, p.I - k1, tid);
            stw.load(wb + k1, p.ldw, rows_w, p.I - k1, tid);
        }
#pragma unroll
        for (int ks = 0; ks < kTK / 16; ++ks) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = read_row_frag<kTK>(w_img, wo * 64 + m * 32 + fr, ks, fh);
#pragma unroll
            for (int n = 0; n < 2; ++n) b[n] = read_row_frag<kTK>(x_img, wr * 64 + n * 32 + fr, ks, fh);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b[n], acc[m][n], 0, 0, 0);
        }
    }

    // acc[m][n][4 g + j] = result[row r0 + 64 wr + 32 n + fr][output o0 + 64 wo + 32 m + 8 g + 4 fh + j].  A lane so holds 8-byte
    // pieces of 32 different rows; the tile goes through LDS, and memory is read and written in whole rows of the tile.
    __syncthreads();                                    // the last step's reads are done: the images are free
    if (MODE == kAddend) {
        // fp32: two half tiles of 64 rows (the rows of n), addend in, sum formed in place by the lane that holds the term, sum out
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (n) __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = tid + i * kT, lr = v >> 5, c = v & 31;
                const long long row = r0 + (lr >> 5) * 64 + n * 32 + (lr & 31);
                const int o = o0 + c * 4;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < p.R && o < p.O) a = *reinterpret_cast<const float4*>(p.addend + row * p.ldadd + o);
                *reinterpret_cast<float4*>(lds + epi_off<32>(lr, c)) = a;
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ol = wo * 64 + m * 32 + 8 * g + 4 * fh;
                    float v[4] = {acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
                    if (p.bias && o0 + ol < p.O) {
                        const float4 b = *reinterpret_cast<const float4*>(p.bias + o0 + ol);
                        v[0] += b.x, v[1] += b.y, v[2] += b.z, v[3] += b.w;
                    }
                    float4* at = reinterpret_cast<float4*>(lds + epi_off<32>(wr * 32 + fr, ol >> 2));
                    const float4 a = *at;
                    *at = make_float4(a.x + (float)(__bf16)v[0], a.y + (float)(__bf16)v[1], a.z + (float)(__bf16)v[2],
                                      a.w + (float)(__bf16)v[3]);
                }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = tid + i * kT, lr = v >> 5, c = v & 31;
                const long long row = r0 + (lr >> 5) * 64 + n * 32 + (lr & 31);
                const int o = o0 + c * 4;
                if (row < p.R && o < p.O)
                    *reinterpret_cast<float4*>(p.out + row * p.ldout + o) = *reinterpret_cast<const float4*>(lds + epi_off<32>(lr, c));
            }
        }
        return;
    }
    if (MODE == kAux) {                                 // the auxiliary's tile, read in whole rows
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int v = tid + i * kT, lr = v >> 4, c = v & 15;
            const long long row = r0 + lr;
            const int o = o0 + c * 8;
            uint4 a = make_uint4(0, 0, 0, 0);
            if (row < p.R && o < p.O) a = *reinterpret_cast<const uint4*>(p.aux + row * p.ldaux + o);
            *reinterpret_cast<uint4*>(lds + epi_off<16>(lr, c)) = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ol = wo * 64 + m * 32 + 8 * g + 4 * fh;
                float v[4] = {acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
                if (MODE != kAux && p.bias && o0 + ol < p.O) {      // O is a multiple of 8: a group of 4 is inside or outside as a whole
                    const float4 b = *reinterpret_cast<const float4*>(p.bias + o0 + ol);
                    v[0] += b.x, v[1] += b.y, v[2] += b.z, v[3] += b.w;
                }
                uint2* at = reinterpret_cast<uint2*>(lds + epi_off<16>(wr * 64 + n * 32 + fr, ol >> 3) + 8 * fh);
                if (MODE == kAux) {                     // this lane's own 8 bytes: read, then overwritten with the result
                    const uint2 a = *at;
                    v[0] *= Gelu::gelu_grad(bf_lo(a.x)), v[1] *= Gelu::gelu_grad(bf_hi(a.x));
                    v[2] *= Gelu::gelu_grad(bf_lo(a.y)), v[3] *= Gelu::gelu_grad(bf_hi(a.y));
                }
                const bf16x4 q = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};      // round to nearest even
                *at = __builtin_bit_cast(uint2, q);
            }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int v = tid + i * kT, lr = v >> 4, c = v & 15;
        const long long row = r0 + lr;
        const int o = o0 + c * 8;
        if (row >= p.R || o >= p.O) continue;
        uint4 q = *reinterpret_cast<const uint4*>(lds + epi_off<16>(lr, c));
        if (MODE == kGelu) {
            if (p.pre) *reinterpret_cast<uint4*>(p.pre + row * p.ldpre + o) = q;
            uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {               // of the rounded pre-activation
                const bf16x2 h = {(__bf16)Gelu::gelu(bf_lo(w[e])), (__bf16)Gelu::gelu(bf_hi(w[e]))};
                w[e] = __builtin_bit_cast(uint32_t, h);
            }
            q = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(p.y + row * p.ldy + o) = q;
    }
}

// ---- weight image ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float as_float(float v) { return v; }
__device__ __forceinline__ float as_float(bf16 v) { return __bfloat162float(v); }

template <typename T>
__global__ __launch_bounds__(kT) void toklinear_pack_kernel(const T* w, long long ldw, bf16* out, long long ldo, int O, int I, int n_it,
                                                            int transpose) {
    __shared__ uint16_t tile[64][66];
    const int tid = threadIdx.x;
    const int i0 = (int)(blockIdx.x % n_it) * 64, o0 = (int)(blockIdx.x / n_it) * 64;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + k * kT, r = idx >> 6, c = idx & 63;
        const float v = (o0 + r < O && i0 + c < I) ? as_float(w[(long long)(o0 + r) * ldw + i0 + c]) : 0.f;
        tile[r][c] = __builtin_bit_cast(uint16_t, (__bf16)v);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = tid + k * kT, r = idx >> 3, ch = idx & 7;
        uint16_t e[8];
        if (!transpose) {
            if (o0 + r >= O || i0 + ch * 8 >= I) continue;
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = tile[r][ch * 8 + j];
            *reinterpret_cast<uint4*>(out + (long long)(o0 + r) * ldo + i0 + ch * 8) = __builtin_bit_cast(uint4, e);
        } else {
            if (i0 + r >= I || o0 + ch * 8 >= O) continue;
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = tile[ch * 8 + j][r];
            *reinterpret_cast<uint4*>(out + (long long)(i0 + r) * ldo + o0 + ch * 8) = __builtin_bit_cast(uint4, e);
        }
    }
}

// ---- g * gelu'(pre) ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void toklinear_gelu_grad_kernel(const bf16* g, long long ldg, const bf16* pre, long long ldpre, bf16* out,
                                                                 long long ldout, long long R, int O) {
    const long long idx = (long long)blockIdx.x * kT + threadIdx.x;
    const int cpr = O / 8;
    const long long row = idx / cpr;
    const int o = (int)(idx % cpr) * 8;
    if (row >= R) return;
    const uint4 a = *reinterpret_cast<const uint4*>(g + row * ldg + o), b = *reinterpret_cast<const uint4*>(pre + row * ldpre + o);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    bf16x8 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        q[2 * e] = (__bf16)(bf_lo(aw[e]) * Gelu::gelu_grad(bf_lo(bw[e])));
        q[2 * e + 1] = (__bf16)(bf_hi(aw[e]) * Gelu::gelu_grad(bf_hi(bw[e])));
    }
    *reinterpret_cast<uint4*>(out + row * ldout + o) = __builtin_bit_cast(uint4, q);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------
struct WgParams {
    const bf16 *dy, *x;
    float *dw, *db;                 // where this launch stores: the results themselves (one slab) or the partial panels
    long long lddy, ldx, lddw, R, steps_per_slab, panel, dbpanel;      // panel / dbpanel: elements between two slabs' stores
    int O, I, n_ot, n_it;
};

__global__ __launch_bounds__(kT) void toklinear_wgrad_kernel(WgParams p) {
    __shared__ __attribute__((aligned(16))) char g_img[kTokBytes];
    __shared__ __attribute__((aligned(16))) char x_img[kTokBytes];
    __shared__ float db_s[16][kTO];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const int wo = wave >> 1, wi = wave & 1;
    const long long bid = blockIdx.x;
    const int it = (int)(bid % p.n_it), ot = (int)((bid / p.n_it) % p.n_ot);
    const long long slab = bid / ((long long)p.n_it * p.n_ot);
    const int o0 = ot * kTO, i0 = it * kTI;
    const long long tok0 = slab * p.steps_per_slab * kTS;
    const long long tok1 = (tok0 + p.steps_per_slab * kTS < p.R) ? tok0 + p.steps_per_slab * kTS : p.R;
    const long long nt = tok1 > tok0 ? (tok1 - tok0 + kTS - 1) / kTS : 0;      // a slab past the last token stores zeros
    const bf16* gb = p.dy + tok0 * p.lddy + o0;
    const bf16* xb = p.x + tok0 * p.ldx + i0;
    const bool want_db = p.db != nullptr && it == 0;

    f32x16 acc[2][2];                                   // [output tile][input tile]
    zero(acc);
    float dbs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    TokStage stg, stx;
    if (nt > 0) {
        stg.load(gb, p.lddy, tok1 - tok0, p.O - o0, tid);
        stx.load(xb, p.ldx, tok1 - tok0, p.I - i0, tid);
    }
    for (long long t = 0; t < nt; ++t) {
        __syncthreads();
        stg.put(g_img, tid);
        stx.put(x_img, tid);
        if (want_db) stg.add_columns(dbs);
        __syncthreads();
        if (t + 1 < nt) {
            const long long s1 = (t + 1) * kTS;
            stg.load(gb + s1 * p.lddy, p.lddy, tok1 - tok0 - s1, p.O - o0, tid);
            stx.load(xb + s1 * p.ldx, p.ldx, tok1 - tok0 - s1, p.I - i0, tid);
        }
#pragma unroll
        for (int ks = 0; ks < kTS / 16; ++ks) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = read_tr_frag(g_img, wo * 64 + m * 32, ks, lane);
#pragma unroll
            for (int n = 0; n < 2; ++n) b[n] = read_tr_frag(x_img, wi * 64 + n * 32, ks, lane);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b[n], acc[m][n], 0, 0, 0);
        }
    }

    float* dst = p.dw + slab * p.panel;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int i = i0 + wi * 64 + n * 32 + fr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + wo * 64 + m * 32 + tile_row(r, fh);
                if (o < p.O && i < p.I) dst[(long long)o * p.lddw + i] = acc[m][n][r];
            }
        }
    if (want_db) {                                      // uniform over the workgroup
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) db_s[tid >> 4][(tid & 15) * 8 + e] = dbs[e];
        __syncthreads();
        if (tid < kTO && o0 + tid < p.O) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += db_s[k][tid];
            p.db[slab * p.dbpanel + o0 + tid] = s;
        }
    }
}

// dW = sum of the slabs' panels and db = sum of their column sums, in slab order
__global__ __launch_bounds__(kT) void toklinear_wgrad_sum_kernel(const float* ws, float* dw, long long lddw, float* db, int O, int I,
                                                                 int slabs) {
    const long long idx = (long long)blockIdx.x * kT + threadIdx.x;
    const long long panel = (long long)O * I, nw = panel / 4;
    if (idx < nw) {
        const long long e = idx * 4;
        float4 s = *reinterpret_cast<const float4*>(ws + e);
        for (int k = 1; k < slabs; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(ws + k * panel + e);
            s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
        }
        *reinterpret_cast<float4*>(dw + (e / I) * lddw + e % I) = s;
    } else if (db != nullptr && idx - nw < O / 4) {
        const long long e = (idx - nw) * 4;
        const float* wb = ws + slabs * panel;
        float4 s = *reinterpret_cast<const float4*>(wb + e);
        for (int k = 1; k < slabs; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(wb + (long long)k * O + e);
            s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
        }
        *reinterpret_cast<float4*>(db + e) = s;
    }
}

// ---- validation ------------------------------------------------------------------------------------------------------------
int check_sizes(const char* who, long long R, int O, int I) {
    MK_REQUIRE_AS(who, R >= 1 && O >= 8 && I >= 8, "bad sizes");
    MK_REQUIRE_AS(who, O % 8 == 0 && I % 8 == 0, "feature counts must be multiples of 8");
    MK_REQUIRE_AS(who, (double)mk::ceil_div_ll(R, 64) * mk::ceil_div(O, 8) < 2147483647.0, "too many rows");
    return 0;
}
// a [rows, len] operand: a 16-byte-aligned base pointer and a row stride in elements, a multiple of 8 of at least len
int check_operand(const char* who, const void* ptr, long long ld, int len) {
    MK_REQUIRE_AS(who, ptr != nullptr, "null pointer");
    MK_REQUIRE_AS(who, mk::aligned<16>(ptr), "operand not 16-byte aligned");
    MK_REQUIRE_AS(who, ld % 8 == 0, "row strides must be multiples of 8 elements");
    MK_REQUIRE_AS(who, ld >= len, "row stride smaller than the row length");
    return 0;
}

// slabs = 0: one workgroup per compute unit where the (O, I) tiles alone do not give that many, every slab at least 4 token
// steps long, and no slab empty
int resolve_slabs(long long R, int O, int I, int slabs) {
    if (slabs > 0) return slabs;
    const long long tiles = (long long)mk::ceil_div(O, kTO) * mk::ceil_div(I, kTI), steps = mk::ceil_div_ll(R, kTS);
    long long s = mk::ceil_div_ll(mk::cu_count(), tiles);
    if (s > steps / 4) s = steps / 4;
    if (s > kMaxSlabs) s = kMaxSlabs;
    if (s < 1) s = 1;
    return (int)mk::ceil_div_ll(steps, mk::ceil_div_ll(steps, s));
}

}  // namespace

extern "C" int mk_token_linear_info(int* tiles) {
    MK_REQUIRE(tiles != nullptr, "null pointer");
    tiles[0] = kTR, tiles[1] = kTC, tiles[2] = kTK;
    tiles[3] = kTO, tiles[4] = kTI, tiles[5] = kTS;
    return 0;
}

extern "C" int mk_token_linear_pack(const void* w, int w_dtype, long long ldw, void* out, long long ldo, int O, int I, int transpose,
                                    void* stream) {
    if (int rc = check_sizes(__func__, 1, O, I)) return rc;
    MK_REQUIRE(w_dtype == 0 || w_dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
    if (int rc = check_operand(__func__, w, ldw, I)) return rc;
    if (int rc = check_operand(__func__, out, ldo, transpose ? O : I)) return rc;
    const int n_it = mk::ceil_div(I, 64);
    const dim3 grid((unsigned)((long long)n_it * mk::ceil_div(O, 64)));
    if (w_dtype == 0)
        hipLaunchKernelGGL(toklinear_pack_kernel<float>, grid, dim3(kT), 0, (hipStream_t)stream, (const float*)w, ldw, (bf16*)out, ldo, O, I,
                           n_it, transpose);
    else
        hipLaunchKernelGGL(toklinear_pack_kernel<bf16>, grid, dim3(kT), 0, (hipStream_t)stream, (const bf16*)w, ldw, (bf16*)out, ldo, O, I,
                           n_it, transpose);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_token_linear_fwd(const void* x, long long ldx, const void* w, long long ldw, const float* bias, void* y, long long ldy,
                                   void* act, long long ldact, void* pre, long long ldpre, const float* addend, long long ldadd,
                                   float* out_f32, long long ldout, const void* aux, long long ldaux, long long R, int O, int I,
                                   void* stream) {
    if (int rc = check_sizes(__func__, R, O, I)) return rc;
    if (int rc = check_operand(__func__, x, ldx, I)) return rc;
    if (int rc = check_operand(__func__, w, ldw, I)) return rc;
    MK_REQUIRE(mk::aligned<16>(bias), "bias not 16-byte aligned");
    int mode;
    if (y && !act && !pre && !addend && !out_f32 && !aux) mode = kPlain;
    else if (act && !y && !addend && !out_f32 && !aux) mode = kGelu;
    else if (addend && out_f32 && !y && !act && !pre && !aux) mode = kAddend;
    else if (y && aux && !bias && !act && !pre && !addend && !out_f32) mode = kAux;
    else MK_REQUIRE(false, "unsupported combination of epilogue pointers");
    FwdParams p{};
    p.x = (const bf16*)x, p.w = (const bf16*)w, p.bias = bias, p.ldx = ldx, p.ldw = ldw, p.R = R, p.O = O, p.I = I;
    p.n_ot = mk::ceil_div(O, kTC);
    if (mode == kPlain || mode == kAux) {
        if (int rc = check_operand(__func__, y, ldy, O)) return rc;
        p.y = (bf16*)y, p.ldy = ldy;
    }
    if (mode == kAux) {
        if (int rc = check_operand(__func__, aux, ldaux, O)) return rc;
        p.aux = (const bf16*)aux, p.ldaux = ldaux;
    }
    if (mode == kGelu) {
        if (int rc = check_operand(__func__, act, ldact, O)) return rc;
        p.y = (bf16*)act, p.ldy = ldact;
        if (pre) {
            if (int rc = check_operand(__func__, pre, ldpre, O)) return rc;
            p.pre = (bf16*)pre, p.ldpre = ldpre;
        }
    }
    if (mode == kAddend) {
        if (int rc = check_operand(__func__, addend, ldadd, O)) return rc;
        if (int rc = check_operand(__func__, out_f32, ldout, O)) return rc;
        p.addend = addend, p.ldadd = ldadd, p.out = out_f32, p.ldout = ldout;
    }
    const dim3 grid((unsigned)(mk::ceil_div_ll(R, kTR) * p.n_ot));
    switch (mode) {
        case kPlain: hipLaunchKernelGGL(toklinear_fwd_kernel<kPlain>, grid, dim3(kT), 0, (hipStream_t)stream, p); break;
        case kGelu: hipLaunchKernelGGL(toklinear_fwd_kernel<kGelu>, grid, dim3(kT), 0, (hipStream_t)stream, p); break;
        case kAddend: hipLaunchKernelGGL(toklinear_fwd_kernel<kAddend>, grid, dim3(kT), 0, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL(toklinear_fwd_kernel<kAux>, grid, dim3(kT), 0, (hipStream_t)stream, p); break;
    }
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_token_linear_gelu_grad(const void* g, long long ldg, const void* pre, long long ldpre, void* out, long long ldout,
                                         long long R, int O, void* stream) {
    if (int rc = check_sizes(__func__, R, O, 8)) return rc;
    if (int rc = check_operand(__func__, g, ldg, O)) return rc;
    if (int rc = check_operand(__func__, pre, ldpre, O)) return rc;
    if (int rc = check_operand(__func__, out, ldout, O)) return rc;
    const long long total = R * (O / 8);
    hipLaunchKernelGGL(toklinear_gelu_grad_kernel, dim3((unsigned)mk::ceil_div_ll(total, kT)), dim3(kT), 0, (hipStream_t)stream,
                       (const bf16*)g, ldg, (const bf16*)pre, ldpre, (bf16*)out, ldout, R, O);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" long long mk_token_linear_wgrad_workspace(long long R, int O, int I, int slabs) {
    if (R < 1 || O < 8 || I < 8 || O % 8 || I % 8 || slabs < 0 || slabs > kMaxSlabs) return -1;
    const int s = resolve_slabs(R, O, I, slabs);
    return s == 1 ? 0 : (long long)s * ((long long)O * I + O) * 4;
}

extern "C" int mk_token_linear_wgrad(const void* dy, long long lddy, const void* x, long long ldx, float* dw, long long lddw, float* db,
                                     void* workspace, long long R, int O, int I, int slabs, void* stream) {
    if (int rc = check_sizes(__func__, R, O, I)) return rc;
    MK_REQUIRE(slabs >= 0 && slabs <= kMaxSlabs, "slabs must be 0 (choose) or 1 ... 64");
    if (int rc = check_operand(__func__, dy, lddy, O)) return rc;
    if (int rc = check_operand(__func__, x, ldx, I)) return rc;
    if (int rc = check_operand(__func__, dw, lddw, I)) return rc;
    MK_REQUIRE(mk::aligned<16>(db), "db not 16-byte aligned");
    const int s = resolve_slabs(R, O, I, slabs);
    MK_REQUIRE(s == 1 || (workspace != nullptr && mk::aligned<16>(workspace)), "workspace null or not 16-byte aligned");
    WgParams p{};
    p.dy = (const bf16*)dy, p.x = (const bf16*)x, p.lddy = lddy, p.ldx = ldx, p.R = R, p.O = O, p.I = I;
    p.n_ot = mk::ceil_div(O, kTO), p.n_it = mk::ceil_div(I, kTI);
    MK_REQUIRE((double)p.n_ot * p.n_it * s < 2147483647.0, "too many tiles");
    p.steps_per_slab = mk::ceil_div_ll(mk::ceil_div_ll(R, kTS), s);
    float* ws = (float*)workspace;
    if (s == 1) {
        p.dw = dw, p.lddw = lddw, p.db = db;
    } else {
        p.panel = (long long)O * I, p.dbpanel = O;
        p.dw = ws, p.lddw = I, p.db = db ? ws + s * p.panel : nullptr;
    }
    hipLaunchKernelGGL(toklinear_wgrad_kernel, dim3((unsigned)((long long)p.n_ot * p.n_it * s)), dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    if (s > 1) {
        const long long total = (long long)O * I / 4 + O / 4;
        hipLaunchKernelGGL(toklinear_wgrad_sum_kernel, dim3((unsigned)mk::ceil_div_ll(total, kT)), dim3(kT), 0, (hipStream_t)stream,
                           (const float*)ws, dw, lddw, db, O, I, s);
        MK_LAUNCH_CHECK();
    }
    return 0;
}
