// Scaled-dot-product attention (non-causal, no mask, no dropout) with fp32 operands, fp32 output and fp32 lse on the bf16x3
// arithmetic of x3_engine.h: the F.scaled_dot_product_attention call of the ViT blocks (makani/models/networks/vit.py:44-55)
// when the model runs in plain fp32 (amp_mode none).
//
//   mk_attn_x3_fwd        one workgroup per (batch, head, 128 queries), sweeps the keys in tiles of 64, online softmax
//   mk_attn_x3_bwd_delta  delta = rowsum(dO o O)
//   mk_attn_x3_bwd_dkv    one workgroup per (batch, head, 128 keys), sweeps the queries in tiles of 32
//   mk_attn_x3_bwd_dq     one workgroup per (batch, head, 128 queries), sweeps the keys in tiles of 32
//
// The structure is that of attn.hip: the owned token sits on the MFMA lane, the swept tile goes global -> registers -> LDS with a
// transposed image for the second product, the softmax is in-lane, nothing is summed across workgroups.  What differs is the
// arithmetic.  Every fp32 operand of a matrix product is split exactly into three bf16 pieces (split3: x = h + m + l) and a
// product is the six piece products of weight >= 2^-16, smallest first, on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
//   - the owned rows (q, dO in fwd / dq; k, v in dkv) are split once, when they are loaded, and stay in registers as pieces;
//   - the swept tiles are split by the staging pass: an LDS image is three piece images, each laid out as attn.hip lays out its
//     one (row-major: 16-byte chunks XOR-swizzled with the row; transposed: pitch rows + 2);
//   - P and dS, fp32 in the accumulator registers, are split in registers before the product that consumes them.
// Scores, softmax, row sums, lse, delta and all accumulators are fp32.
//
// Head sizes are zero-padded on chip to 64; the 16-wide k-steps and the 32-wide output tiles that lie wholly in the padding get
// no MFMA work (a wave-uniform test).  D > 64 is refused: the pieces of two owned operands at DP = 128 are 192 registers next
// to 128 of accumulators in the dK / dV kernel.
#include "attn_host.h"
#include "x3_engine.h"

namespace {

using mk::attn::kLog2e;
using mk::attn::kOwn;
using mk::mfma::tile_row;
using mk::mfma::zero;

constexpr int kT = 256;                 // 4 waves
constexpr int kDP = 64;                 // padded head size
constexpr int kFwdTK = 64;              // key tile of fwd
constexpr int kBwdT = 32;               // key tile of dq, query tile of dkv
constexpr int KS = kDP / 16, DT = kDP / 32;
constexpr float kLn2 = 0.6931471805599453f;

struct Frag3 { bf16x8 p[3]; };          // the h, m, l pieces of 8 operand elements

__device__ __forceinline__ Frag3 split8(const float (&v)[8]) {
    Split3 s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = split3(v[i]);
    const uint4 h = make_uint4(pack_hi(s[0].h, s[1].h), pack_hi(s[2].h, s[3].h), pack_hi(s[4].h, s[5].h), pack_hi(s[6].h, s[7].h));
    const uint4 m = make_uint4(pack_hi(s[0].m, s[1].m), pack_hi(s[2].m, s[3].m), pack_hi(s[4].m, s[5].m), pack_hi(s[6].m, s[7].m));
    const uint4 l = make_uint4(pack_hi(s[0].l, s[1].l), pack_hi(s[2].l, s[3].l), pack_hi(s[4].l, s[5].l), pack_hi(s[6].l, s[7].l));
    Frag3 f;
    f.p[0] = __builtin_bit_cast(bf16x8, h), f.p[1] = __builtin_bit_cast(bf16x8, m), f.p[2] = __builtin_bit_cast(bf16x8, l);
    return f;
}
// k-step ss of an accumulator tile used as the B operand of the next product (registers 8 ss .. 8 ss + 7)
__device__ __forceinline__ Frag3 split_acc(const f32x16& x, int ss) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = x[8 * ss + j];
    return split8(v);
}
// the six piece products of one 16-k sub-step in the engine's order (x3_mfma_step), for the products contracted over the swept
// token: a = swept operand, b = owned operand
__device__ __forceinline__ f32x16 mfma6(const Frag3& a, const Frag3& b, f32x16 acc) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int t = 0; t < 6; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[PA[t]], b.p[PB[t]], acc, 0, 0, 0);
    return acc;
}

template <int ROWS> constexpr int rows_piece() { return ROWS * kDP * 2; }
template <int ROWS> constexpr int cols_piece() { return (kDP * (ROWS + 2) * 2 + 15) / 16 * 16; }
template <int ROWS> constexpr int rows_bytes() { return 3 * rows_piece<ROWS>(); }
template <int ROWS> constexpr int cols_bytes() { return 3 * cols_piece<ROWS>(); }

// ---- staging of a [ROWS][D] fp32 tile through registers into piece images: row-major and / or transposed -----------------------
template <int ROWS>
struct Stage {
    static constexpr int CPR = kDP / 8, NV = ROWS * CPR / kT;
    static_assert(ROWS * CPR % kT == 0, "tile does not divide among the threads");
    float4 r[NV][2];
    // base: the tile's first row; rows at or past rows_valid and d at or past D become zeros, and are not read
    __device__ __forceinline__ void load(const float* base, long long ld, int rows_valid, int D, int tid) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = tid + i * kT, row = v / CPR, c = v % CPR;
            const bool ok = row < rows_valid && c * 8 < D;
            const float* src = base + row * ld + c * 8;
            r[i][0] = ok ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
            r[i][1] = ok ? *reinterpret_cast<const float4*>(src + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // rows: [piece][row][d], 16-byte chunks swizzled;  cols: [piece][d][row], pitch ROWS + 2.  Either may be null.
    __device__ __forceinline__ void put(char* rows, char* cols, int tid) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = tid + i * kT, row = v / CPR, c = v % CPR;
            const float x[8] = {r[i][0].x, r[i][0].y, r[i][0].z, r[i][0].w, r[i][1].x, r[i][1].y, r[i][1].z, r[i][1].w};
            const Frag3 f = split8(x);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) {
                const uint4 w4 = __builtin_bit_cast(uint4, f.p[pc]);
                if (rows) *reinterpret_cast<uint4*>(rows + pc * rows_piece<ROWS>() + row * (kDP * 2) + ((c ^ (row & 7)) << 4)) = w4;
                if (cols) {
                    uint16_t* t = reinterpret_cast<uint16_t*>(cols + pc * cols_piece<ROWS>());
                    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) t[(c * 8 + e) * (ROWS + 2) + row] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
                }
            }
        }
    }
};

// A fragments: 8 consecutive d of one swept row, and the swept tokens r0 .. r0 + 3, r0 + 8 .. r0 + 11 of one d
template <int ROWS>
__device__ __forceinline__ Frag3 read_rows(const char* img, int row, int ks, int fh) {
    const char* p = img + row * (kDP * 2) + (((2 * ks + fh) ^ (row & 7)) << 4);
    Frag3 f;
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) f.p[pc] = *reinterpret_cast<const bf16x8*>(p + pc * rows_piece<ROWS>());
    return f;
}
template <int ROWS>
__device__ __forceinline__ Frag3 read_cols(const char* img, int d, int r0) {
    Frag3 f;
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(img + pc * cols_piece<ROWS>() + (d * (ROWS + 2) + r0) * 2);
        f.p[pc] = __builtin_bit_cast(bf16x8, make_uint4(p[0], p[1], p[4], p[5]));
    }
    return f;
}
// One 32 x 32 tile of a product contracted over the head axis (S = q k^T, dP = dO v^T): the swept rows `row` of a row-major
// piece image against the owned token's pieces.  The whole contraction is at hand, so "smallest first" runs over ALL of it:
// piece-major, the 2^-16-weight products of every k-step first and the h h products last.  A single dominant term (one key far
// above the others, tests/test_x3_attn_gpu.py::test_attention_spike) then meets 4 roundings at its magnitude, not 24; in the
// k-step-major order the lse of such a row was off by 2.7 units of 2^-23 (smag + |lse| + 1).
template <int ROWS>
__device__ __forceinline__ f32x16 head_product(const char* img, int row, const Frag3 (&b)[KS], int D, int fh, f32x16 acc) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
    Frag3 a[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        if (16 * ks < D) a[ks] = read_rows<ROWS>(img, row, ks, fh);
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            if (16 * ks < D) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks].p[PA[t]], b[ks].p[PB[t]], acc, 0, 0, 0);
    return acc;
}
// the owned token's row as the pieces of its MFMA fragments, straight from global memory
__device__ __forceinline__ void load_frags(Frag3 (&f)[KS], const float* row, bool valid, int D, int fh) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d = 16 * ks + 8 * fh;
        const bool ok = valid && d < D;
        const float4 a = ok ? *reinterpret_cast<const float4*>(row + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 b = ok ? *reinterpret_cast<const float4*>(row + d + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        f[ks] = split8(x);
    }
}
// acc[dt][r] = result[d = 32 dt + tile_row(r)][owned token]: registers 4 g .. 4 g + 3 are 4 consecutive d, one 16-byte store
__device__ __forceinline__ void store_t(const f32x16 (&acc)[DT], float* row, bool valid, int D, int fh, float mul) {
    if (!valid) return;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * dt + 8 * g + 4 * fh;
            if (d < D)
                *reinterpret_cast<float4*>(row + d) =
                    make_float4(acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul, acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul);
        }
}

struct Params : mk::attn::ParamsOf<float> {};
constexpr mk::attn::Family kFamily{kDP, 4};       // head sizes to 64; strides in units of 4 floats

// ---- forward ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void x3_attn_fwd_kernel(Params p) {
    constexpr int TK = kFwdTK;
    __shared__ __attribute__((aligned(16))) char k_img[rows_bytes<TK>()];
    __shared__ __attribute__((aligned(16))) char vt_img[cols_bytes<TK>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long bid = blockIdx.x;
    const int qt = (int)(bid % p.ntile), h = (int)((bid / p.ntile) % p.H), b = (int)(bid / ((long long)p.ntile * p.H));
    const int q = qt * kOwn + wave * 32 + fr;
    const bool qv = q < p.Nq;
    Frag3 qf[KS];
    load_frags(qf, p.q + b * p.sq.b + h * p.sq.h + q * p.sq.n, qv, p.D, fh);
    const float* kbase = p.k + b * p.sk.b + h * p.sk.h;
    const float* vbase = p.v + b * p.sv.b + h * p.sv.h;

    f32x16 oacc[DT];
    zero(oacc);
    float m = -INFINITY, l = 0.f;       // running maximum (log2 domain) and this lane half's share of the row sum
    Stage<TK> stk, stv;
    const int nt = (p.Nk + TK - 1) / TK;
    stk.load(kbase, p.sk.n, p.Nk, p.D, tid);
    stv.load(vbase, p.sv.n, p.Nk, p.D, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                // the previous tile's reads are done
        stk.put(k_img, nullptr, tid);
        stv.put(nullptr, vt_img, tid);
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
            s[kb] = head_product<TK>(k_img, kb * 32 + fr, qf, p.D, fh, s[kb]);      // S^T[key][query]
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
                const Frag3 pf = split_acc(s[kb], ss);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)   // O^T[d][query] += V^T[d][key] P^T[key][query]
                    if (32 * dt < p.D) oacc[dt] = mfma6(read_cols<TK>(vt_img, dt * 32 + fr, kb * 32 + 16 * ss + 4 * fh), pf, oacc[dt]);
            }
    }
    l += __shfl_xor(l, 32);
    store_t(oacc, p.o + b * p.so.b + h * p.so.h + q * p.so.n, qv, p.D, fh, 1.f / l);
    if (p.lse_out && qv && fh == 0) p.lse_out[((long long)b * p.H + h) * p.Nq + q] = (m + __builtin_amdgcn_logf(l)) * kLn2;
}

// ---- delta = rowsum(dO o O) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void x3_attn_delta_kernel(Params p, long long total) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % p.Nq), h = (int)((i / p.Nq) % p.H), b = (int)(i / ((long long)p.Nq * p.H));
    const float* o = p.o + b * p.so.b + h * p.so.h + q * p.so.n;
    const float* g = p.dO + b * p.sdo.b + h * p.sdo.h + q * p.sdo.n;
    float s = 0.f;
    for (int d = 0; d < p.D; d += 4) {
        const float4 a = *reinterpret_cast<const float4*>(o + d), c = *reinterpret_cast<const float4*>(g + d);
        s = fmaf(a.x, c.x, s);
        s = fmaf(a.y, c.y, s);
        s = fmaf(a.z, c.z, s);
        s = fmaf(a.w, c.w, s);
    }
    p.lse_out[i] = s;
}

// ---- dQ --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void x3_attn_bwd_dq_kernel(Params p) {
    constexpr int TK = kBwdT;
    __shared__ __attribute__((aligned(16))) char k_img[rows_bytes<TK>()];
    __shared__ __attribute__((aligned(16))) char v_img[rows_bytes<TK>()];
    __shared__ __attribute__((aligned(16))) char kt_img[cols_bytes<TK>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long bid = blockIdx.x;
    const int qt = (int)(bid % p.ntile), h = (int)((bid / p.ntile) % p.H), b = (int)(bid / ((long long)p.ntile * p.H));
    const int q = qt * kOwn + wave * 32 + fr;
    const bool qv = q < p.Nq;
    Frag3 qf[KS], gf[KS];
    load_frags(qf, p.q + b * p.sq.b + h * p.sq.h + q * p.sq.n, qv, p.D, fh);
    load_frags(gf, p.dO + b * p.sdo.b + h * p.sdo.h + q * p.sdo.n, qv, p.D, fh);
    const long long ri = ((long long)b * p.H + h) * p.Nq + q;
    const float lse2 = qv ? p.lse[ri] * kLog2e : 0.f, nd = qv ? -p.delta[ri] : 0.f;
    const float* kbase = p.k + b * p.sk.b + h * p.sk.h;
    const float* vbase = p.v + b * p.sv.b + h * p.sv.h;

    f32x16 acc[DT];
    zero(acc);
    Stage<TK> stk, stv;
    const int nt = (p.Nk + TK - 1) / TK;
    stk.load(kbase, p.sk.n, p.Nk, p.D, tid);
    stv.load(vbase, p.sv.n, p.Nk, p.D, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        stk.put(k_img, kt_img, tid);
        stv.put(v_img, nullptr, tid);
        __syncthreads();
        if (t + 1 < nt) {
            const long long k1 = (long long)(t + 1) * TK;
            stk.load(kbase + k1 * p.sk.n, p.sk.n, p.Nk - (int)k1, p.D, tid);
            stv.load(vbase + k1 * p.sv.n, p.sv.n, p.Nk - (int)k1, p.D, tid);
        }
        const int kleft = p.Nk - t * TK;
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = nd;      // dP - delta leaves the chain ready
        s = head_product<TK>(k_img, fr, qf, p.D, fh, s);
        dp = head_product<TK>(v_img, fr, gf, p.D, fh, dp);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pr = (tile_row(r, fh) < kleft) ? __builtin_amdgcn_exp2f(fmaf(s[r], p.c, -lse2)) : 0.f;
            s[r] = pr * dp[r];                                     // dS^T[key][query] (without the scale)
        }
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const Frag3 df = split_acc(s, ss);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)   // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
                if (32 * dt < p.D) acc[dt] = mfma6(read_cols<TK>(kt_img, dt * 32 + fr, 16 * ss + 4 * fh), df, acc[dt]);
        }
    }
    store_t(acc, p.dq + b * p.sdq.b + h * p.sdq.h + q * p.sdq.n, qv, p.D, fh, p.scale);
}

// ---- dK, dV ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void x3_attn_bwd_dkv_kernel(Params p) {
    constexpr int TQ = kBwdT;
    __shared__ __attribute__((aligned(16))) char q_img[rows_bytes<TQ>()];
    __shared__ __attribute__((aligned(16))) char g_img[rows_bytes<TQ>()];
    __shared__ __attribute__((aligned(16))) char qt_img[cols_bytes<TQ>()];
    __shared__ __attribute__((aligned(16))) char gt_img[cols_bytes<TQ>()];
    __shared__ float lse_s[TQ], del_s[TQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long bid = blockIdx.x;
    const int kt = (int)(bid % p.ntile), h = (int)((bid / p.ntile) % p.H), b = (int)(bid / ((long long)p.ntile * p.H));
    const int key = kt * kOwn + wave * 32 + fr;
    const bool kv = key < p.Nk;
    Frag3 kf[KS], vf[KS];
    load_frags(kf, p.k + b * p.sk.b + h * p.sk.h + key * p.sk.n, kv, p.D, fh);
    load_frags(vf, p.v + b * p.sv.b + h * p.sv.h + key * p.sv.n, kv, p.D, fh);
    const float* qbase = p.q + b * p.sq.b + h * p.sq.h;
    const float* gbase = p.dO + b * p.sdo.b + h * p.sdo.h;
    const float* lbase = p.lse + ((long long)b * p.H + h) * p.Nq;
    const float* dbase = p.delta + ((long long)b * p.H + h) * p.Nq;

    f32x16 dk[DT], dv[DT];
    zero(dk);
    zero(dv);
    Stage<TQ> stq, stg;
    float rl = 0.f, rd = 0.f;           // rows past Nq: P is masked below, these only have to be finite
    const int nt = (p.Nq + TQ - 1) / TQ;
    stq.load(qbase, p.sq.n, p.Nq, p.D, tid);
    stg.load(gbase, p.sdo.n, p.Nq, p.D, tid);
    if (tid < TQ && tid < p.Nq) rl = lbase[tid] * kLog2e, rd = dbase[tid];
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        stq.put(q_img, qt_img, tid);
        stg.put(g_img, gt_img, tid);
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
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = -del_s[tile_row(r, fh)];
        s = head_product<TQ>(q_img, fr, kf, p.D, fh, s);        // S[query][key], dP[query][key]
        dp = head_product<TQ>(g_img, fr, vf, p.D, fh, dp);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ql = tile_row(r, fh);
            const float pr = (ql < qleft) ? __builtin_amdgcn_exp2f(fmaf(s[r], p.c, -lse_s[ql])) : 0.f;
            s[r] = pr;
            dp[r] = pr * dp[r];
        }
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const Frag3 pf = split_acc(s, ss), df = split_acc(dp, ss);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)    // dV^T[d][key] += dO^T[d][query] P[query][key];  dK^T += Q^T dS
                if (32 * dt < p.D) {
                    dv[dt] = mfma6(read_cols<TQ>(gt_img, dt * 32 + fr, 16 * ss + 4 * fh), pf, dv[dt]);
                    dk[dt] = mfma6(read_cols<TQ>(qt_img, dt * 32 + fr, 16 * ss + 4 * fh), df, dk[dt]);
                }
        }
    }
    store_t(dv, p.dv + b * p.sdv.b + h * p.sdv.h + key * p.sdv.n, kv, p.D, fh, 1.f);
    store_t(dk, p.dk + b * p.sdk.b + h * p.sdk.h + key * p.sdk.n, kv, p.D, fh, p.scale);
}

}  // namespace

extern "C" int mk_attn_x3_info(int D, int* tiles) {
    if (int rc = mk::attn::check_head(__func__, kFamily, D)) return rc;
    MK_REQUIRE(tiles != nullptr, "null pointer");
    tiles[0] = kOwn, tiles[1] = kFwdTK;        // fwd: query tile, key tile
    tiles[2] = kBwdT, tiles[3] = kOwn;         // dkv
    tiles[4] = kOwn, tiles[5] = kBwdT;         // dq
    return 0;
}

extern "C" int mk_attn_x3_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int Nq, int Nk, int D,
                              const long long* strides, float scale, void* stream) {
    Params p{};
    if (int rc = mk::attn::fwd_params(__func__, kFamily, p, q, k, v, o, lse, B, H, Nq, Nk, D, strides, scale)) return rc;
    hipLaunchKernelGGL(x3_attn_fwd_kernel, mk::attn::tile_grid(p), dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_attn_x3_bwd_delta(const float* o, const float* dO, float* delta, int B, int H, int Nq, int D, const long long* strides,
                                    void* stream) {
    Params p{};
    if (int rc = mk::attn::delta_params(__func__, kFamily, p, o, dO, delta, B, H, Nq, D, strides)) return rc;
    const long long total = (long long)B * H * Nq;
    hipLaunchKernelGGL(x3_attn_delta_kernel, dim3((unsigned)mk::ceil_div_ll(total, kT)), dim3(kT), 0, (hipStream_t)stream, p, total);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_attn_x3_bwd_dkv(const float* q, const float* k, const float* v, const float* dO, const float* lse, const float* delta,
                                  float* dk, float* dv, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale,
                                  void* stream) {
    Params p{};
    if (int rc = mk::attn::dkv_params(__func__, kFamily, p, q, k, v, dO, lse, delta, dk, dv, B, H, Nq, Nk, D, strides, scale)) return rc;
    hipLaunchKernelGGL(x3_attn_bwd_dkv_kernel, mk::attn::tile_grid(p), dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_attn_x3_bwd_dq(const float* q, const float* k, const float* v, const float* dO, const float* lse, const float* delta,
                                 float* dq, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale, void* stream) {
    Params p{};
    if (int rc = mk::attn::dq_params(__func__, kFamily, p, q, k, v, dO, lse, delta, dq, B, H, Nq, Nk, D, strides, scale)) return rc;
    hipLaunchKernelGGL(x3_attn_bwd_dq_kernel, mk::attn::tile_grid(p), dim3(kT), 0, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}
