// 1x1 convolutions on fp32 fields (nn.Conv2d(.., 1) of MLP / EncoderDecoder / skips outside autocast: layers.py:86-216,
// sfnonet.py:207,379,463) on the bf16x3 engine: fp32-accurate products without a vendor GEMM.
//   mode 0:  C[b] = A B[b]          A [M][K] row-major (K a multiple of 4), B[b] [K][N] k-major (the NCHW field, N = H*W even)
//   mode 1:  C[b] += A B[b]         (the skip connection folded into the GEMM: C holds the addend)
//   mode 2:  C += sum_b A[b] B[b]^T  A[b] [M][Kp], B[b] [N][Kp] both row-major over the contraction (the pixels): the weight
//            gradient, the pixels cut into slabs of `kslab` k-steps, one workgroup per (tile, slab), fp32 atomics into C (zeroed by the caller)
//   mode 3:  C[b] = act(A B[b] + bias)
#include "x3_engine.h"

namespace {

// store act(tile + bias[row]) with `rowbias` pointing at the tile's first row (null: no bias) and `act` != 0 the exact (erf)
// GELU: conv + bias + activation of layers.py:158-206 in one launch
struct BiasGeluEpi {
    float* cbase;
    long long ldc;
    const float* rowbias;
    int act;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        const float bv = rowbias ? rowbias[row] : 0.f;
                        float v0 = acc[a][0][r] + bv, v1 = acc[a][1][r] + bv;
                        if (act) {
                            v0 = 0.5f * v0 * (1.f + erff(v0 * 0.70710678118654752440f));
                            v1 = 0.5f * v1 * (1.f + erff(v1 * 0.70710678118654752440f));
                        }
                        *reinterpret_cast<float2*>(cbase + (long long)row * ldc + col) = make_float2(v0, v1);
                    }
                }
        }
    }
};

struct ConvX3Params {
    const float* a;
    const float* b;
    float* c;
    long long lda, ldb, ldc, sa, sb, sc;
    int M, K, N, nwork, tiles_m, tiles_n, nslab, kslab;
    const float* bias;      // mode 3: per-row bias or null
    int act;                // mode 3: 1 = exact GELU
};

template <int MODE>
__global__ __launch_bounds__(XT, 3) void conv_x3_kernel(ConvX3Params p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    // MODE 2: work item = (batch item, pixel slab), all tiles of gW of one item on one XCD.  MODE 0 / 1 / 3: work item = (batch item,
    // 128-pixel tile), its M / 128 row tiles back to back on one XCD -- they share the x tile, the second to sixth find it in
    // that XCD's L2 (with the batch index as the only work index a batch of one ran on ONE of the eight XCDs: 8x slower)
    TileId t = decode_block(p.nwork, p.tiles_m, MODE == 2 ? p.tiles_n : 1);
    if (!t.valid) return;
    if constexpr (MODE != 2) {
        const int w = t.batch;
        t.batch = w / p.tiles_n;
        t.tn = w - t.batch * p.tiles_n;
    }
    const int m0 = t.tm * XM, n0 = t.tn * XN;
    if constexpr (MODE == 2) {
        const int b = t.batch / p.nslab, slab = t.batch - b * p.nslab;
        const int kt0 = slab * p.kslab, ktn = (p.K + XK - 1) / XK;
        const int kt1 = kt0 + p.kslab < ktn ? kt0 + p.kslab : ktn;
        RowStager as, bs;
        as.base = p.a + b * p.sa + (long long)m0 * p.lda;
        as.ld = p.lda;
        as.rows = p.M - m0;
        as.kvalid = p.K;
        bs.base = p.b + b * p.sb + (long long)n0 * p.ldb;
        bs.ld = p.ldb;
        bs.rows = p.N - n0;
        bs.kvalid = p.K;
        const AtomicEpi epi{p.c + (long long)m0 * p.ldc + n0, p.ldc};
        x3_tile(as, bs, kt0, kt1, p.M - m0, p.N - n0, epi, lds_x3);
    } else {
        RowStager as;
        as.base = p.a + (long long)m0 * p.lda;
        as.ld = p.lda;
        as.rows = p.M - m0;
        as.kvalid = (p.K + 3) / 4 * 4;         // whole 16-byte groups: the caller pads the rows of A with zeros
        TransStager bs;
        bs.base = p.b + t.batch * p.sb + n0;
        bs.ldk = p.ldb;
        bs.k_lo = 0;
        bs.k_hi = p.K;
        bs.cvalid = p.N - n0;
        float* cb = p.c + t.batch * p.sc + (long long)m0 * p.ldc + n0;
        const int kts = (p.K + XK - 1) / XK;
        if constexpr (MODE == 0) x3_tile(as, bs, 0, kts, p.M - m0, p.N - n0, StoreEpi{cb, p.ldc}, lds_x3);
        else if constexpr (MODE == 1) x3_tile(as, bs, 0, kts, p.M - m0, p.N - n0, AccumulateEpi{cb, p.ldc}, lds_x3);
        else x3_tile(as, bs, 0, kts, p.M - m0, p.N - n0, BiasGeluEpi{cb, p.ldc, p.bias ? p.bias + m0 : nullptr, p.act}, lds_x3);
    }
}
}  // namespace

static int conv_x3_launch(const float* a, long long lda, const float* b, long long ldb, float* c, long long ldc, int M, int K,
                          long long N, int batch, long long sa, long long sb, long long sc, int mode, const float* bias, int act,
                          void* stream) {
    MK_REQUIRE(a && b && c, "null pointer");
    MK_REQUIRE(M > 0 && K > 0 && N > 0 && batch > 0, "bad sizes");
    MK_REQUIRE(mode >= 0 && mode <= 3, "mode must be 0 (store), 1 (accumulate), 2 (weight gradient) or 3 (store with bias / GELU)");
    MK_REQUIRE(mk::aligned<16>(a, b, c), "operands must be 16-byte aligned");
    ConvX3Params p;
    p.a = a; p.b = b; p.c = c;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.sa = sa; p.sb = sb; p.sc = sc;
    p.M = M; p.K = K;
    p.bias = bias; p.act = act;
    MK_REQUIRE(N < 2147483647LL, "N too large");
    p.N = (int)N;
    p.tiles_m = mk::ceil_div(M, XM);
    p.tiles_n = mk::ceil_div((int)N, XN);
    p.nslab = 1;
    p.kslab = 0;
    if (mode == 2) {
        // A [M][K], B [N][K]: rows start on 16-byte boundaries, whole 4-element groups
        MK_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && K % 4 == 0 && sa % 4 == 0 && sb % 4 == 0, "weight gradient: row strides and the contraction length must be multiples of 4");
        const int ktn = mk::ceil_div(K, XK);
        // enough workgroups to fill the chip: ~6 per CU
        long long want = 1536 / ((long long)p.tiles_m * p.tiles_n * batch);
        if (want < 1) want = 1;
        if (want > ktn) want = ktn;
        p.kslab = mk::ceil_div(ktn, (int)want);
        p.nslab = mk::ceil_div(ktn, p.kslab);
        p.nwork = batch * p.nslab;
    } else {
        MK_REQUIRE(lda % 4 == 0 && lda >= (K + 3) / 4 * 4, "A: the row stride must be a multiple of 4 and cover K rounded up to 4 (zero padded)");
        MK_REQUIRE(N % 2 == 0 && ldb % 2 == 0 && ldc % 2 == 0 && sb % 2 == 0 && sc % 2 == 0, "B / C: even row lengths and strides");
        MK_REQUIRE(33LL * ldb * 4 < (1LL << 31), "B row stride too large for the 32-bit offsets of one k-step");
        MK_REQUIRE((long long)batch * p.tiles_n < 2147483647LL, "too many pixel tiles");
        p.nwork = batch * p.tiles_n;
    }
    void (*const kernels[4])(ConvX3Params) = {conv_x3_kernel<0>, conv_x3_kernel<1>, conv_x3_kernel<2>, conv_x3_kernel<3>};
    return x3_launch(__func__, kernels[mode], grid_blocks(p.nwork, p.tiles_m, mode == 2 ? p.tiles_n : 1), stream, p);
}

extern "C" int mk_conv1x1_x3(const float* a, long long lda, const float* b, long long ldb, float* c, long long ldc, int M, int K,
                             long long N, int batch, long long sa, long long sb, long long sc, int mode, void* stream) {
    MK_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (store), 1 (accumulate) or 2 (weight gradient)");
    return conv_x3_launch(a, lda, b, ldb, c, ldc, M, K, N, batch, sa, sb, sc, mode, nullptr, 0, stream);
}

// C[b] = act(A B[b] + bias): the fp32 convolution with its bias add and (act = 1) exact GELU in the epilogue -- what
// `nn.Conv2d(cin, cout, 1, bias=True)` + `nn.GELU()` (layers.py:95-99, 158-206) compute, in one pass over the output.
extern "C" int mk_conv1x1_x3_bias_act(const float* a, long long lda, const float* b, long long ldb, float* c, long long ldc, int M,
                                      int K, long long N, int batch, long long sb, long long sc, const float* bias, int act,
                                      void* stream) {
    MK_REQUIRE(act == 0 || act == 1, "act must be 0 (none) or 1 (exact GELU)");
    return conv_x3_launch(a, lda, b, ldb, c, ldc, M, K, N, batch, 0, sb, sc, 3, bias, act, stream);
}
