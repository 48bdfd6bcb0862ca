// Token-major linear layers on fp32 rows (nn.Linear of ViT / AFNOv1 / the "traditional" MLP and EncoderDecoder outside autocast:
// layers.py:136-216, vit.py qkv / proj / fc1 / fc2 / head) on the bf16x3 engine: fp32-accurate products without a vendor GEMM.
//   mk_token_linear_x3_fwd    acc[r][o] = sum_k x[r][k] w[o][k]  (w_kmajor 0: F.linear; both operands row-major over the contraction)
//                             acc[r][o] = sum_k x[r][k] w[k][o]  (w_kmajor 1: the data gradient, read from the weight as it is stored)
//                             with one epilogue that applies what it is given: bias, stored pre-activation, exact GELU, addend, GELU'(aux)
//   mk_token_linear_x3_wgrad  dW[o][i] = sum_r dy[r][o] x[r][i]: both operands k-major over the tokens, the tokens cut into slabs of whole
//                             k-steps, one fp32 panel per slab, added in slab order by a second launch; db[o] = sum_r dy[r][o] in float64
// Nothing is summed across workgroups by atomics: the same inputs give the same bits.
#include "x3_engine.h"
#include "gelu.h"

namespace {

using GeluF = mk::gelu::Act<float>;
constexpr int kMaxSlabs = 64;
constexpr int kDbRows = 128;          // token rows of one float64 partial of the bias gradient

// In this order: v = tile + bias[col]; pre = v (if given); v = gelu(v) (if act); v += addend; v *= gelu'(aux); y = v.  Every pointer
// is at the tile's first element (bias: its first column) or null.  A lane owns a column pair: the bias pair is loaded once.
struct TokEpi {
    float* y;
    long long ldy;
    float* pre;
    long long ldpre;
    const float* addend;
    long long ldadd;
    const float* aux;
    long long ldaux;
    const float* bias;
    int act;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
            const float2 bv = bias ? *reinterpret_cast<const float2*>(bias + col) : make_float2(0.f, 0.f);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        float v0 = acc[a][0][r] + bv.x, v1 = acc[a][1][r] + bv.y;
                        if (pre) *reinterpret_cast<float2*>(pre + (long long)row * ldpre + col) = make_float2(v0, v1);
                        if (act) {
                            v0 = GeluF::gelu(v0);
                            v1 = GeluF::gelu(v1);
                        }
                        if (addend) {
                            const float2 ad = *reinterpret_cast<const float2*>(addend + (long long)row * ldadd + col);
                            v0 += ad.x;
                            v1 += ad.y;
                        }
                        if (aux) {
                            const float2 ax = *reinterpret_cast<const float2*>(aux + (long long)row * ldaux + col);
                            v0 *= GeluF::gelu_grad(ax.x);
                            v1 *= GeluF::gelu_grad(ax.y);
                        }
                        *reinterpret_cast<float2*>(y + (long long)row * ldy + col) = make_float2(v0, v1);
                    }
                }
        }
    }
};

struct TokFwdParams {
    const float *x, *w, *bias, *addend, *aux;
    float *y, *pre;
    long long ldx, ldw, ldy, ldpre, ldadd, ldaux, R;
    int O, I, act, tiles_r, tiles_c;
};

template <int KMAJOR>
__global__ __launch_bounds__(XT, 3) void toklinear_x3_fwd_kernel(TokFwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    // work item = a 128-token tile, its O / 128 column tiles back to back on one XCD: they share the x tile in that L2
    const TileId t = decode_block(p.tiles_r, 1, p.tiles_c);
    if (!t.valid) return;
    const long long m0 = (long long)t.batch * XM;
    const int n0 = t.tn * XN;
    const int rvalid = p.R - m0 < XM ? (int)(p.R - m0) : XM, cvalid = p.O - n0;
    RowStager as;
    as.base = p.x + m0 * p.ldx;
    as.ld = p.ldx;
    as.rows = rvalid;
    as.kvalid = p.I;
    TokEpi epi;
    epi.y = p.y + m0 * p.ldy + n0, epi.ldy = p.ldy;
    epi.pre = p.pre ? p.pre + m0 * p.ldpre + n0 : nullptr, epi.ldpre = p.ldpre;
    epi.addend = p.addend ? p.addend + m0 * p.ldadd + n0 : nullptr, epi.ldadd = p.ldadd;
    epi.aux = p.aux ? p.aux + m0 * p.ldaux + n0 : nullptr, epi.ldaux = p.ldaux;
    epi.bias = p.bias ? p.bias + n0 : nullptr;
    epi.act = p.act;
    const int kts = (p.I + XK - 1) / XK;
    if constexpr (KMAJOR) {
        TransStager bs;
        bs.base = p.w + n0;
        bs.ldk = p.ldw;
        bs.k_lo = 0;
        bs.k_hi = p.I;
        bs.cvalid = cvalid;
        x3_tile(as, bs, 0, kts, rvalid, cvalid, epi, lds_x3);
    } else {
        RowStager bs;
        bs.base = p.w + (long long)n0 * p.ldw;
        bs.ld = p.ldw;
        bs.rows = cvalid;
        bs.kvalid = p.I;
        x3_tile(as, bs, 0, kts, rvalid, cvalid, epi, lds_x3);
    }
}

struct TokWgParams {
    const float *dy, *x;
    float* dst;                     // dW itself (one slab) or the first partial panel
    long long lddy, ldx, lddst, panel;
    int R, O, I, nslab, kslab, tiles_o, tiles_i;
};

__global__ __launch_bounds__(XT, 3) void toklinear_x3_wgrad_kernel(TokWgParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.nslab, p.tiles_o, p.tiles_i);      // the tiles of one slab on one XCD: they share its tokens
    if (!t.valid) return;
    const int m0 = t.tm * XM, n0 = t.tn * XN;
    const int ktn = (p.R + XK - 1) / XK, kt0 = t.batch * p.kslab;
    const int kt1 = kt0 + p.kslab < ktn ? kt0 + p.kslab : ktn;
    TransStager as, bs;
    as.base = p.dy + m0;
    as.ldk = p.lddy;
    as.k_lo = 0;
    as.k_hi = p.R;
    as.cvalid = p.O - m0;
    bs.base = p.x + n0;
    bs.ldk = p.ldx;
    bs.k_lo = 0;
    bs.k_hi = p.R;
    bs.cvalid = p.I - n0;
    const StoreEpi epi{p.dst + t.batch * p.panel + (long long)m0 * p.lddst + n0, p.lddst};
    x3_tile(as, bs, kt0, kt1, p.O - m0, p.I - n0, epi, lds_x3);
}

// part[chunk][o] = sum of dy[r][o] over the chunk's kDbRows token rows: float64, four interleaved chains added in a fixed order
__global__ __launch_bounds__(256) void toklinear_x3_db_rows_kernel(const float* __restrict__ dy, long long lddy, double* __restrict__ part,
                                                                    int R, int O, int ocks) {
    const int chunk = blockIdx.x / ocks, o = (blockIdx.x - chunk * ocks) * 256 + threadIdx.x;
    if (o >= O) return;
    const int r0 = chunk * kDbRows, r1 = r0 + kDbRows < R ? r0 + kDbRows : R;
    const float* q = dy + o;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int r = r0;
    for (; r + 4 <= r1; r += 4)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += (double)q[(long long)(r + j) * lddy];
    for (int j = 0; r < r1; ++r, ++j) s[j] += (double)q[(long long)r * lddy];
    part[(long long)chunk * O + o] = (s[0] + s[1]) + (s[2] + s[3]);
}

// dW = the slabs' panels added in slab order (slabs > 1), db = the chunks' float64 partials added in chunk order (db not null)
__global__ __launch_bounds__(256) void toklinear_x3_finish_kernel(const float* __restrict__ panels, float* __restrict__ dw, long long lddw,
                                                                   const double* __restrict__ part, float* __restrict__ db, int O, int I,
                                                                   int slabs, int chunks) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long panel = (long long)O * I, nw = slabs > 1 ? panel / 4 : 0;
    if (idx < nw) {
        const long long e = idx * 4;
        float4 s = *reinterpret_cast<const float4*>(panels + e);
        for (int k = 1; k < slabs; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(panels + k * panel + e);
            s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
        }
        *reinterpret_cast<float4*>(dw + (e / I) * lddw + e % I) = s;
    } else if (db != nullptr && idx - nw < O) {
        const long long o = idx - nw;
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += part[(long long)c * O + o];
        db[o] = (float)s;
    }
}

// a [rows][len] fp32 operand: a 16-byte-aligned base pointer and a row stride in elements, a multiple of 4 of at least len;
// `rows_in_tile`: the rows that one stager's 32-bit byte offsets span (128 tile rows, or the 32 rows of a k-step of a k-major operand)
int tok_operand(const char* who, const void* ptr, long long ld, int len, int rows_in_tile) {
    MK_REQUIRE_AS(who, ptr != nullptr, "null pointer");
    MK_REQUIRE_AS(who, mk::aligned<16>(ptr), "operand not 16-byte aligned");
    MK_REQUIRE_AS(who, ld % 4 == 0, "row strides must be multiples of 4 elements");
    MK_REQUIRE_AS(who, ld >= len, "row stride smaller than the row length");
    MK_REQUIRE_AS(who, (rows_in_tile + 1) * ld * 4 < (1LL << 31), "row stride too large for the 32-bit offsets of one tile");
    return 0;
}

// slab length in k-steps and the slabs that are not empty.  slabs = 0: about three workgroups per compute unit, no slab shorter
// than 4 k-steps
void tok_slabs(int R, int O, int I, int slabs, int& kslab, int& nslab) {
    const int ktn = mk::ceil_div(R, XK);
    long long want = slabs;
    if (slabs <= 0) {
        const long long tiles = (long long)mk::ceil_div(O, XM) * mk::ceil_div(I, XN);
        want = mk::ceil_div_ll(3LL * mk::cu_count(), tiles);
        if (want > ktn / 4) want = ktn / 4;
        if (want > kMaxSlabs) want = kMaxSlabs;
    }
    if (want < 1) want = 1;
    if (want > ktn) want = ktn;
    kslab = mk::ceil_div(ktn, (int)want);
    nslab = mk::ceil_div(ktn, kslab);
}

bool tok_wgrad_sizes_ok(long long R, int O, int I, int slabs) {
    return R >= 1 && R < 2147483647LL - XK && O >= 4 && I >= 4 && O % 4 == 0 && I % 4 == 0 && slabs >= 0 && slabs <= kMaxSlabs;
}

}  // namespace

extern "C" int mk_token_linear_x3_info(int* t) {
    MK_REQUIRE(t != nullptr, "null pointer");
    t[0] = XM, t[1] = XN, t[2] = XK;
    return 0;
}

extern "C" int mk_token_linear_x3_fwd(const float* x, long long x_ld, const float* w, long long w_ld, int w_kmajor, const float* bias,
                                      float* y, long long y_ld, float* pre, long long pre_ld, const float* addend, long long addend_ld,
                                      const float* aux, long long aux_ld, int act, long long R, int O, int I, void* stream) {
    MK_REQUIRE(R >= 1 && O >= 4 && I >= 4, "bad sizes");
    MK_REQUIRE(O % 4 == 0 && I % 4 == 0, "feature counts must be multiples of 4");
    MK_REQUIRE(w_kmajor == 0 || w_kmajor == 1, "w_kmajor must be 0 ([O][I]) or 1 ([I][O])");
    MK_REQUIRE(act == 0 || act == 1, "act must be 0 (none) or 1 (exact GELU)");
    MK_REQUIRE(pre == nullptr || act == 1, "pre is stored only with act = 1");
    MK_REQUIRE(addend == nullptr || (act == 0 && aux == nullptr), "addend cannot be combined with act or aux");
    MK_REQUIRE(aux == nullptr || (act == 0 && bias == nullptr), "aux cannot be combined with act or a bias");
    if (int rc = tok_operand(__func__, x, x_ld, I, XM)) return rc;
    if (int rc = w_kmajor ? tok_operand(__func__, w, w_ld, O, XK) : tok_operand(__func__, w, w_ld, I, XN)) return rc;
    if (int rc = tok_operand(__func__, y, y_ld, O, 0)) return rc;
    if (pre)
        if (int rc = tok_operand(__func__, pre, pre_ld, O, 0)) return rc;
    if (addend)
        if (int rc = tok_operand(__func__, addend, addend_ld, O, 0)) return rc;
    if (aux)
        if (int rc = tok_operand(__func__, aux, aux_ld, O, 0)) return rc;
    MK_REQUIRE(mk::aligned<16>(bias), "bias not 16-byte aligned");
    MK_REQUIRE(mk::ceil_div_ll(R, XM) < 2147483647LL / 2, "too many rows");
    TokFwdParams p{};
    p.x = x, p.w = w, p.bias = bias, p.addend = addend, p.aux = aux, p.y = y, p.pre = pre;
    p.ldx = x_ld, p.ldw = w_ld, p.ldy = y_ld, p.ldpre = pre_ld, p.ldadd = addend_ld, p.ldaux = aux_ld, p.R = R;
    p.O = O, p.I = I, p.act = act;
    p.tiles_r = (int)mk::ceil_div_ll(R, XM), p.tiles_c = mk::ceil_div(O, XN);
    return x3_launch(__func__, w_kmajor ? toklinear_x3_fwd_kernel<1> : toklinear_x3_fwd_kernel<0>, grid_blocks(p.tiles_r, 1, p.tiles_c),
                     stream, p);
}

extern "C" long long mk_token_linear_x3_wgrad_workspace(long long R, int O, int I, int slabs) {
    if (!tok_wgrad_sizes_ok(R, O, I, slabs)) return -1;
    int kslab, nslab;
    tok_slabs((int)R, O, I, slabs, kslab, nslab);
    return (nslab > 1 ? (long long)nslab * O * I * 4 : 0) + mk::ceil_div_ll(R, kDbRows) * O * 8;
}

extern "C" int mk_token_linear_x3_wgrad(const float* dy, long long dy_ld, const float* x, long long x_ld, float* dw, long long dw_ld,
                                        float* db, void* ws, long long R, int O, int I, int slabs, void* stream) {
    MK_REQUIRE(R >= 1 && R < 2147483647LL - XK && O >= 4 && I >= 4, "bad sizes");
    MK_REQUIRE(O % 4 == 0 && I % 4 == 0, "feature counts must be multiples of 4");
    MK_REQUIRE(slabs >= 0 && slabs <= kMaxSlabs, "slabs must be 0 (choose) or 1 ... 64");
    if (int rc = tok_operand(__func__, dy, dy_ld, O, XK)) return rc;
    if (int rc = tok_operand(__func__, x, x_ld, I, XK)) return rc;
    if (int rc = tok_operand(__func__, dw, dw_ld, I, 0)) return rc;
    MK_REQUIRE(mk::aligned<16>(db), "db not 16-byte aligned");
    TokWgParams p{};
    tok_slabs((int)R, O, I, slabs, p.kslab, p.nslab);
    MK_REQUIRE((p.nslab == 1 && db == nullptr) || (ws != nullptr && mk::aligned<16>(ws)), "workspace null or not 16-byte aligned");
    float* panels = static_cast<float*>(ws);
    const long long panel = (long long)O * I;
    double* part = reinterpret_cast<double*>(panels + (p.nslab > 1 ? p.nslab * panel : 0));
    p.dy = dy, p.x = x, p.lddy = dy_ld, p.ldx = x_ld, p.R = (int)R, p.O = O, p.I = I;
    p.tiles_o = mk::ceil_div(O, XM), p.tiles_i = mk::ceil_div(I, XN);
    if (p.nslab == 1) p.dst = dw, p.lddst = dw_ld, p.panel = 0;
    else p.dst = panels, p.lddst = I, p.panel = panel;
    if (int rc = x3_launch(__func__, toklinear_x3_wgrad_kernel, grid_blocks(p.nslab, p.tiles_o, p.tiles_i), stream, p)) return rc;
    const int chunks = (int)mk::ceil_div_ll(R, kDbRows), ocks = mk::ceil_div(O, 256);
    if (db) {
        MK_REQUIRE((long long)chunks * ocks < 2147483647LL, "grid too large");
        hipLaunchKernelGGL(toklinear_x3_db_rows_kernel, dim3((unsigned)(chunks * ocks)), dim3(256), 0, (hipStream_t)stream, dy, dy_ld, part,
                           (int)R, O, ocks);
        MK_LAUNCH_CHECK();
    }
    if (p.nslab > 1 || db) {
        const long long total = (p.nslab > 1 ? panel / 4 : 0) + (db ? O : 0);
        hipLaunchKernelGGL(toklinear_x3_finish_kernel, dim3((unsigned)mk::ceil_div_ll(total, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)panels, dw, dw_ld, (const double*)part, db, O, I, p.nslab, chunks);
        MK_LAUNCH_CHECK();
    }
    return 0;
}
