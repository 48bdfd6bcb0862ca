// Scaled-dot-product attention (non-causal, no mask, no dropout) on bf16 MFMA: the F.scaled_dot_product_attention call of
// the ViT blocks (makani/models/networks/vit.py:44-55).  bf16 in and out, fp32 scores, softmax and accumulators.
//
//   mk_attn_fwd        one workgroup per (batch, head, 128 queries), sweeps the keys in tiles of 64, online softmax
//   mk_attn_bwd_delta  delta = rowsum(dO o O)
//   mk_attn_bwd_dkv    one workgroup per (batch, head, 128 keys), sweeps the queries: dK and dV stay in its accumulators
//   mk_attn_bwd_dq     one workgroup per (batch, head, 128 queries), sweeps the keys: dQ stays in its accumulators
//
// Nothing is summed across workgroups: no atomics, no hand-off, no spin loop; the same inputs give the same bits.
//
// Every product is v_mfma_f32_32x32x16_bf16, 4 waves of 32 "owned" tokens each.  The owned token (the query in fwd / dq,
// the key in dkv) sits on the MFMA lane: the score tile is computed with the owned token as the column, so its 32 x 32
// fp32 result has the other token in the 16 registers of a lane.  Row maximum and row sum of the softmax are then in-lane
// (one exchange with lane ^ 32), and the tile, rounded to bf16, is the B operand of the second product as it stands
// (registers 8 s .. 8 s + 7 are k-step s; element j of lane half h is tile row 16 s + 8 (j >> 2) + 4 h + (j & 3)), which
// accumulates the TRANSPOSED result [d][owned token].  The A operand of that product runs over the swept token for a fixed
// d, so it is read from a transposed LDS image [d][token] that the staging writes next to the row-major one.
//
// The swept tiles go global -> registers -> LDS (plain register staging, the loads of tile t + 1 in flight under the MFMAs
// of tile t).  Row-major images are XOR-swizzled in 16-byte chunks (chunk ^ (row & 7)); transposed images have a pitch of
// rows + 2 elements.  Head sizes are zero-padded in LDS and registers to DP = 64 (D <= 64) or 128: a padded d is never
// read from or written to memory.  A ragged last key tile is masked in the score; rows past the end load as zeros and
// are not stored.
#include "attn_host.h"
#include "mfma_tile.h"
#include "../../include/makani_amd.h"

#include <hip/hip_bf16.h>

namespace {

using mk::mfma::bf16x4;
using mk::mfma::bf16x8;
using mk::mfma::bf_hi;
using mk::mfma::bf_lo;
using mk::mfma::f32x16;
using mk::mfma::read_row_frag;
using mk::mfma::RowStage;
using mk::mfma::tile_row;
using mk::mfma::zero;
using mk::attn::kLog2e;
using mk::attn::kOwn;
typedef __hip_bfloat16 bf16;

constexpr int kT = 256;                 // 4 waves
constexpr int kSweepK = 64;             // key tile of fwd and dq
constexpr float kLn2 = 0.6931471805599453f;

constexpr int padded_d(int D) { return D <= 64 ? 64 : 128; }
constexpr int dkv_sweep(int DP) { return 4096 / DP; }      // query tile of dkv: 64 (DP 64) or 32 (DP 128)

// ---- staging of a [ROWS][D] tile through registers: the row-major image of RowStage, and the transposed one -------------------
template <int ROWS, int DP>
struct Stage : RowStage<ROWS, DP, kT> {
    using RowStage<ROWS, DP, kT>::CPR;
    using RowStage<ROWS, DP, kT>::NV;
    __device__ __forceinline__ void put_cols(char* img, int tid) const {      // [d][row], pitch ROWS + 2
        uint16_t* t = reinterpret_cast<uint16_t*>(img);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = tid + i * kT, row = v / CPR, c = v % CPR;
            const uint32_t w[4] = {this->r[i].x, this->r[i].y, this->r[i].z, this->r[i].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) t[(c * 8 + e) * (ROWS + 2) + row] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
        }
    }
};
template <int ROWS, int DP> constexpr int rows_bytes() { return ROWS * DP * 2; }
template <int ROWS, int DP> constexpr int cols_bytes() { return (DP * (ROWS + 2) * 2 + 15) / 16 * 16; }

// A fragment over the swept token for one d, in the k order of an accumulator tile used as B: rows r0 .. r0 + 3, r0 + 8 .. r0 + 11
template <int ROWS>
__device__ __forceinline__ bf16x8 read_col_frag(const char* img, int d, int r0) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(img + (d * (ROWS + 2) + r0) * 2);
    const uint4 w = make_uint4(p[0], p[1], p[4], p[5]);
    return __builtin_bit_cast(bf16x8, w);
}
__device__ __forceinline__ bf16x8 pack8(const f32x16& x, int s) {           // round to nearest even
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (__bf16)x[8 * s + j];
    return f;
}
// the owned token's row as MFMA fragments, straight from global memory
template <int DP>
__device__ __forceinline__ void load_frags(bf16x8 (&f)[DP / 16], const bf16* row, bool valid, int D, int fh) {
#pragma unroll
    for (int ks = 0; ks < DP / 16; ++ks) {
        const int d = 16 * ks + 8 * fh;
        const uint4 w = (valid && d < D) ? *reinterpret_cast<const uint4*>(row + d) : make_uint4(0, 0, 0, 0);
        f[ks] = __builtin_bit_cast(bf16x8, w);
    }
}
// acc[dt][r] = result[d = 32 dt + tile_row(r)][owned token]: registers 4 g .. 4 g + 3 are 4 consecutive d, one 8-byte store
template <int DP>
__device__ __forceinline__ void store_t(const f32x16 (&acc)[DP / 32], bf16* row, bool valid, int D, int fh, float mul) {
    if (!valid) return;
#pragma unroll
    for (int dt = 0; dt < DP / 32; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * dt + 8 * g + 4 * fh;
            if (d < D) {
                const bf16x4 o = {(__bf16)(acc[dt][4 * g] * mul), (__bf16)(acc[dt][4 * g + 1] * mul),
                                  (__bf16)(acc[dt][4 * g + 2] * mul), (__bf16)(acc[dt][4 * g + 3] * mul)};
                *reinterpret_cast<uint2*>(row + d) = __builtin_bit_cast(uint2, o);
            }
        }
}

struct Params : mk::attn::ParamsOf<bf16> {};
constexpr mk::attn::Family kFamily{128, 8};      // head sizes to 128; strides in units of 8 bf16

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(kT) void attn_fwd_kernel(Params p) {
    constexpr int TK = kSweepK, KS = DP / 16, DT = DP / 32;
    __shared__ __attribute__((aligned(16))) char k_img[rows_bytes<TK, DP>()];
    __shared__ __attribute__((aligned(16))) char vt_img[cols_bytes<TK, DP>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long bid = blockIdx.x;
    const int qt = (int)(bid % p.ntile), h = (int)((bid / p.ntile) % p.H), b = (int)(bid / ((long long)p.ntile * p.H));
    const int q = qt * kOwn + wave * 32 + fr;
    const bool qv = q < p.Nq;
    bf16x8 qf[KS];
    load_frags<DP>(qf, p.q + b * p.sq.b + h * p.sq.h + q * p.sq.n, qv, p.D, fh);
    const bf16* kbase = p.k + b * p.sk.b + h * p.sk.h;
    const bf16* vbase = p.v + b * p.sv.b + h * p.sv.h;

    f32x16 oacc[DT];
    zero(oacc);
    float m = -INFINITY, l = 0.f;       // running maximum (log2 domain) and this lane half's share of the row sum
    Stage<TK, DP> stk, stv;
    const int nt = (p.Nk + TK - 1) / TK;
    stk.load(kbase, p.sk.n, p.Nk, p.D, tid);
    stv.load(vbase, p.sv.n, p.Nk, p.D, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                // the previous tile's reads are done
        stk.put(k_img, tid);
        stv.put_cols(vt_img, tid);
        __syncthreads();
        if (t + 1 < nt) {
            const long long k1 = (long long)(t + 1) * TK;
            stk.load(kbase + k1 * p.sk.n, p.sk.n, p.Nk - (int)k1, p.D, tid);
            stv.load(vbase + k1 * p.sv.n, p.sv.n, p.Nk - (int)k1, p.D, tid);
        }
        const int kleft = p.Nk - t * TK;
        f32x16 s[TK / 32];
        zero(s);
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < TK / 32; ++kb) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)      // S^T[key][query]
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_row_frag<DP>(k_img, kb * 32 + fr, ks, fh), qf[ks], s[kb], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float x = (kb * 32 + tile_row(r, fh) < kleft) ? s[kb][r] * p.c : -INFINITY;
                s[kb][r] = x;
                mx = fmaxf(mx, x);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));      // every tile holds a valid key: finite
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < TK / 32; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[kb][r] - mn);
                s[kb][r] = e;
                sum += e;
            }
        l = l * alpha + sum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
        for (int kb = 0; kb < TK / 32; ++kb)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 pf = pack8(s[kb], ss);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)   // O^T[d][query] += V^T[d][key] P^T[key][query]
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_col_frag<TK>(vt_img, dt * 32 + fr, kb * 32 + 16 * ss + 4 * fh),
                                                                       pf, oacc[dt], 0, 0, 0);
            }
    }
    l += __shfl_xor(l, 32);
    store_t<DP>(oacc, p.o + b * p.so.b + h * p.so.h + q * p.so.n, qv, p.D, fh, 1.f / l);
    if (p.lse_out && qv && fh == 0) p.lse_out[((long long)b * p.H + h) * p.Nq + q] = (m + __builtin_amdgcn_logf(l)) * kLn2;
}

// ---- delta = rowsum(dO o O) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void attn_delta_kernel(Params p, long long total) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % p.Nq), h = (int)((i / p.Nq) % p.H), b = (int)(i / ((long long)p.Nq * p.H));
    const bf16* o = p.o + b * p.so.b + h * p.so.h + q * p.so.n;
    const bf16* g = p.dO + b * p.sdo.b + h * p.sdo.h + q * p.sdo.n;
    float s = 0.f;
    for (int d = 0; d < p.D; d += 8) {
        const uint4 a = *reinterpret_cast<const uint4*>(o + d), c = *reinterpret_cast<const uint4*>(g + d);
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s = fmaf(bf_lo(aw[e]), bf_lo(cw[e]), s);
            s = fmaf(bf_hi(aw[e]), bf_hi(cw[e]), s);
        }
    }
    p.lse_out[i] = s;               // the delta buffer
}

// ---- dQ --------------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(kT) void attn_bwd_dq_kernel(Params p) {
    constexpr int TK = kSweepK, KS = DP / 16, DT = DP / 32;
    __shared__ __attribute__((aligned(16))) char k_img[rows_bytes<TK, DP>()];
    __shared__ __attribute__((aligned(16))) char v_img[rows_bytes<TK, DP>()];
    __shared__ __attribute__((aligned(16))) char kt_img[cols_bytes<TK, DP>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long bid = blockIdx.x;
    const int qt = (int)(bid % p.ntile), h = (int)((bid / p.ntile) % p.H), b = (int)(bid / ((long long)p.ntile * p.H));
    const int q = qt * kOwn + wave * 32 + fr;
    const bool qv = q < p.Nq;
    bf16x8 qf[KS], gf[KS];
    load_frags<DP>(qf, p.q + b * p.sq.b + h * p.sq.h + q * p.sq.n, qv, p.D, fh);
    load_frags<DP>(gf, p.dO + b * p.sdo.b + h * p.sdo.h + q * p.sdo.n, qv, p.D, fh);
    const long long ri = ((long long)b * p.H + h) * p.Nq + q;
    const float lse2 = qv ? p.lse[ri] * kLog2e : 0.f, nd = qv ? -p.delta[ri] : 0.f;
    const bf16* kbase = p.k + b * p.sk.b + h * p.sk.h;
    const bf16* vbase = p.v + b * p.sv.b + h * p.sv.h;

    f32x16 acc[DT];
    zero(acc);
    Stage<TK, DP> stk, stv;
    const int nt = (p.Nk + TK - 1) / TK;
    stk.load(kbase, p.sk.n, p.Nk, p.D, tid);
    stv.load(vbase, p.sv.n, p.Nk, p.D, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        stk.put(k_img, tid);
        stk.put_cols(kt_img, tid);
        stv.put(v_img, tid);
        __syncthreads();
        if (t + 1 < nt) {
            const long long k1 = (long long)(t + 1) * TK;
            stk.load(kbase + k1 * p.sk.n, p.sk.n, p.Nk - (int)k1, p.D, tid);
            stv.load(vbase + k1 * p.sv.n, p.sv.n, p.Nk - (int)k1, p.D, tid);
        }
        const int kleft = p.Nk - t * TK;
#pragma unroll
        for (int kb = 0; kb < TK / 32; ++kb) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = nd;      // dP - delta leaves the chain ready
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_row_frag<DP>(k_img, kb * 32 + fr, ks, fh), qf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_row_frag<DP>(v_img, kb * 32 + fr, ks, fh), gf[ks], dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = (kb * 32 + tile_row(r, fh) < kleft) ? __builtin_amdgcn_exp2f(fmaf(s[r], p.c, -lse2)) : 0.f;
                s[r] = pr * dp[r];                                     // dS^T[key][query] (without the scale)
            }
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 df = pack8(s, ss);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)   // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
                    acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_col_frag<TK>(kt_img, dt * 32 + fr, kb * 32 + 16 * ss + 4 * fh),
                                                                      df, acc[dt], 0, 0, 0);
            }
        }
    }
    store_t<DP>(acc, p.dq + b * p.sdq.b + h * p.sdq.h + q * p.sdq.n, qv, p.D, fh, p.scale);
}

// ---- dK, dV ----------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(kT) void attn_bwd_dkv_kernel(Params p) {
    constexpr int TQ = dkv_sweep(DP), KS = DP / 16, DT = DP / 32;
    __shared__ __attribute__((aligned(16))) char q_img[rows_bytes<TQ, DP>()];
    __shared__ __attribute__((aligned(16))) char g_img[rows_bytes<TQ, DP>()];
    __shared__ __attribute__((aligned(16))) char qt_img[cols_bytes<TQ, DP>()];
    __shared__ __attribute__((aligned(16))) char gt_img[cols_bytes<TQ, DP>()];
    __shared__ float lse_s[TQ], del_s[TQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long bid = blockIdx.x;
    const int kt = (int)(bid % p.ntile), h = (int)((bid / p.ntile) % p.H), b = (int)(bid / ((long long)p.ntile * p.H));
    const int key = kt * kOwn + wave * 32 + fr;
    const bool kv = key < p.Nk;
    bf16x8 kf[KS], vf[KS];
    load_frags<DP>(kf, p.k + b * p.sk.b + h * p.sk.h + key * p.sk.n, kv, p.D, fh);
    load_frags<DP>(vf, p.v + b * p.sv.b + h * p.sv.h + key * p.sv.n, kv, p.D, fh);
    const bf16* qbase = p.q + b * p.sq.b + h * p.sq.h;
    const bf16* gbase = p.dO + b * p.sdo.b + h * p.sdo.h;
    const float* lbase = p.lse + ((long long)b * p.H + h) * p.Nq;
    const float* dbase = p.delta + ((long long)b * p.H + h) * p.Nq;

    f32x16 dk[DT], dv[DT];
    zero(dk);
    zero(dv);
    Stage<TQ, DP> stq, stg;
    float rl = 0.f, rd = 0.f;           // rows past Nq: P is masked below, these only have to be finite
    const int nt = (p.Nq + TQ - 1) / TQ;
    stq.load(qbase, p.sq.n, p.Nq, p.D, tid);
    stg.load(gbase, p.sdo.n, p.Nq, p.D, tid);
    if (tid < TQ && tid < p.Nq) rl = lbase[tid] * kLog2e, rd = dbase[tid];
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        stq.put(q_img, tid);
        stq.put_cols(qt_img, tid);
        stg.put(g_img, tid);
        stg.put_cols(gt_img, tid);
        if (tid < TQ) lse_s[tid] = rl, del_s[tid] = rd;
        __syncthreads();
        if (t + 1 < nt) {
            const long long q1 = (long long)(t + 1) * TQ;
            stq.load(qbase + q1 * p.sq.n, p.sq.n, p.Nq - (int)q1, p.D, tid);
            stg.load(gbase + q1 * p.sdo.n, p.sdo.n, p.Nq - (int)q1, p.D, tid);
            rl = rd = 0.f;
            if (tid < TQ && q1 + tid < p.Nq) rl = lbase[q1 + tid] * kLog2e, rd = dbase[q1 + tid];
        }
        const int qleft = p.Nq - t * TQ;
#pragma unroll
        for (int qb = 0; qb < TQ / 32; ++qb) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = -del_s[qb * 32 + tile_row(r, fh)];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {     // S[query][key], dP[query][key]
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_row_frag<DP>(q_img, qb * 32 + fr, ks, fh), kf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_row_frag<DP>(g_img, qb * 32 + fr, ks, fh), vf[ks], dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = qb * 32 + tile_row(r, fh);
                const float pr = (ql < qleft) ? __builtin_amdgcn_exp2f(fmaf(s[r], p.c, -lse_s[ql])) : 0.f;
                s[r] = pr;
                dp[r] = pr * dp[r];
            }
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 pf = pack8(s, ss), df = pack8(dp, ss);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {  // dV^T[d][key] += dO^T[d][query] P[query][key];  dK^T += Q^T dS
                    dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_col_frag<TQ>(gt_img, dt * 32 + fr, qb * 32 + 16 * ss + 4 * fh),
                                                                     pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_col_frag<TQ>(qt_img, dt * 32 + fr, qb * 32 + 16 * ss + 4 * fh),
                                                                     df, dk[dt], 0, 0, 0);
                }
            }
        }
    }
    store_t<DP>(dv, p.dv + b * p.sdv.b + h * p.sdv.h + key * p.sdv.n, kv, p.D, fh, 1.f);
    store_t<DP>(dk, p.dk + b * p.sdk.b + h * p.sdk.h + key * p.sdk.n, kv, p.D, fh, p.scale);
}

}  // namespace

extern "C" int mk_attn_info(int D, int* tiles) {
    if (int rc = mk::attn::check_head(__func__, kFamily, D)) return rc;
    MK_REQUIRE(tiles != nullptr, "null pointer");
    tiles[0] = kOwn, tiles[1] = kSweepK;                       // fwd: query tile, key tile
    tiles[2] = dkv_sweep(padded_d(D)), tiles[3] = kOwn;        // dkv
    tiles[4] = kOwn, tiles[5] = kSweepK;                       // dq
    return 0;
}

extern "C" int mk_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Nq, int Nk, int D,
                           const long long* strides, float scale, void* stream) {
    Params p{};
    if (int rc = mk::attn::fwd_params(__func__, kFamily, p, (const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, lse, B, H, Nq, Nk,
                                      D, strides, scale))
        return rc;
    const dim3 grid = mk::attn::tile_grid(p);
    if (padded_d(D) == 64) hipLaunchKernelGGL(attn_fwd_kernel<64>, grid, dim3(kT), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(attn_fwd_kernel<128>, grid, dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_attn_bwd_delta(const void* o, const void* dO, float* delta, int B, int H, int Nq, int D, const long long* strides,
                                 void* stream) {
    Params p{};
    if (int rc = mk::attn::delta_params(__func__, kFamily, p, (const bf16*)o, (const bf16*)dO, delta, B, H, Nq, D, strides)) return rc;
    const long long total = (long long)B * H * Nq;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)mk::ceil_div_ll(total, kT)), dim3(kT), 0, (hipStream_t)stream, p, total);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_attn_bwd_dkv(const void* q, const void* k, const void* v, const void* dO, const float* lse, const float* delta,
                               void* dk, void* dv, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale,
                               void* stream) {
    Params p{};
    if (int rc = mk::attn::dkv_params(__func__, kFamily, p, (const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)dO, lse, delta,
                                      (bf16*)dk, (bf16*)dv, B, H, Nq, Nk, D, strides, scale))
        return rc;
    const dim3 grid = mk::attn::tile_grid(p);
    if (padded_d(D) == 64) hipLaunchKernelGGL(attn_bwd_dkv_kernel<64>, grid, dim3(kT), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(attn_bwd_dkv_kernel<128>, grid, dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_attn_bwd_dq(const void* q, const void* k, const void* v, const void* dO, const float* lse, const float* delta,
                              void* dq, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale, void* stream) {
    Params p{};
    if (int rc = mk::attn::dq_params(__func__, kFamily, p, (const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)dO, lse, delta,
                                     (bf16*)dq, B, H, Nq, Nk, D, strides, scale))
        return rc;
    const dim3 grid = mk::attn::tile_grid(p);
    if (padded_d(D) == 64) hipLaunchKernelGGL(attn_bwd_dq_kernel<64>, grid, dim3(kT), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(attn_bwd_dq_kernel<128>, grid, dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}
