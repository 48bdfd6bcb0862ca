// Latitude DFT of the planar transform (RealFFT2 / InverseRealFFT2, layers.py:219-287) on the bf16x3 engine, truncated to
// the kept frequencies:
//   fwd  c[l][j]  = sum_k W[l][k] xf[k][j]            inv  xf[k][j] = sum_l conj(W[l][k]) c[l][j]
// W = C - i S from mk_latdft_table (the same matrix for every longitudinal mode), j over the mmax_loc * BC complex64
// columns of the latitude-major Fourier rows -- a plain GEMM on rows of 2 * ncols floats.  The two are adjoint to each other.
// One work item per 128-float column tile, its row tiles back to back on one XCD (they share the streamed tile through
// that XCD's L2, as the convolution kernels do).
#include "x3_engine.h"

namespace {

// The table as the A operand: a 128-row tile carries 64 frequencies, per wave-row band the cosine rows of 32
// frequencies (tile rows 64 wr + [0, 32): the accumulators a = 0) and the sine rows of the same 32 (64 wr + [32, 64): a = 1),
// so both products a complex output needs end up in one lane (DftEpi).  Cosine row f of the tile at base[f * ld + k], its
// sine row `part` floats behind; rows < rows (frequencies), k < kvalid (a multiple of 4, rows zero padded to it).
struct DftStager {
    const float* base;
    long long ld, part;
    int rows, kvalid;
    typedef float4 Regs[4];
    static __device__ __forceinline__ int freq(int row) { return ((row >> 6) << 5) + (row & 31); }   // tile row -> frequency
    struct FreqBelow {
        static __device__ __forceinline__ bool live(int row, int rows) { return freq(row) < rows; }
    };
    static __device__ __forceinline__ int row_off(int r) { return plain_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(base);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = tid + q * XT, row = (t >> 6) * 16 + quad_row(t & 63), k = kt * XK + (t & 3) * 8;
            const int f = freq(row), sine = (row >> 5) & 1;
            const unsigned off = (unsigned)((sine * part + (long long)f * ld + k) * 4);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                r[2 * q + h] = x3_load16(rs, (f < rows && k + 4 * h < kvalid) ? off + 16 * h : X3_OOB);
        }
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const { row8_sstore<FreqBelow>(r, img, tid, rows); }
};

// Complex table times interleaved complex columns: `rvalid` counts the tile's FREQUENCIES (<= 64), the cosine and the sine band
// of a wave live together.  acc[0][b] = C x_b, acc[1][b] = S x_b with C - i S the table entry, b = 0 / 1 the real / imaginary
// part of the column; output row f of band wr is
//   CONJ = false  (C - i S)(x0 + i x1) = (C x0 + S x1) + i (C x1 - S x0)      CONJ = true  (C x0 - S x1) + i (C x1 + S x0)
// one 8-byte store per complex output, 256 contiguous bytes per wave and row
template <bool CONJ>
struct DftEpi {
    float* cbase;
    long long ldc;
    static constexpr bool PAIRED_BANDS = true;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                if (row < rvalid) {
                    x3_f2 v2;
                    if constexpr (!CONJ) {
                        v2[0] = acc[0][0][r] + acc[1][1][r];
                        v2[1] = acc[0][1][r] - acc[1][0][r];
                    } else {
                        v2[0] = acc[0][0][r] - acc[1][1][r];
                        v2[1] = acc[0][1][r] + acc[1][0][r];
                    }
                    __builtin_nontemporal_store(v2, reinterpret_cast<x3_f2*>(cbase + (long long)row * ldc + col));
                }
            }
        }
    }
};

struct LatDftParams {
    const float* src;
    const float* tab;     // cosine rows [R][ld]; the sine rows `part` floats behind
    float* dst;
    long long ld, part;
    int K, R, N2;         // contraction length, output rows, floats per row
    int tiles_m, tiles_n;
};

template <bool INV>
__global__ __launch_bounds__(XT, 3) void latdft_x3_kernel(LatDftParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    // the "batch" slot of the decoder carries the COLUMN tile: column tiles spread over the XCDs, the row tiles of one column tile
    // run back to back on one of them
    const TileId t = decode_block(p.tiles_n, p.tiles_m, 1);
    if (!t.valid) return;
    const int r0 = t.tm * (XM / 2), n0 = t.batch * XN;
    DftStager as;
    as.base = p.tab + (long long)r0 * p.ld;
    as.ld = p.ld;
    as.part = p.part;
    as.rows = p.R - r0;
    as.kvalid = (p.K + 3) / 4 * 4;
    TransStager bs;
    bs.base = p.src + n0;
    bs.ldk = p.N2;
    bs.k_lo = 0;
    bs.k_hi = p.K;
    bs.cvalid = p.N2 - n0;
    const DftEpi<INV> epi{p.dst + (long long)r0 * p.N2 + n0, p.N2};
    x3_tile(as, bs, 0, (p.K + XK - 1) / XK, p.R - r0, p.N2 - n0, epi, lds_x3);
}
}  // namespace

static int latdft_launch(bool inv, const float* src, const float* table, float* dst, int nlat, int lmax, long long ncols,
                         void* stream) {
    MK_REQUIRE(src && table && dst, "null pointer");
    MK_REQUIRE(nlat >= 2 && lmax >= 2 && lmax <= nlat && ncols >= 1, "need nlat >= 2, 2 <= lmax <= nlat and at least one column");
    MK_REQUIRE(mk::aligned<16>(table) && mk::aligned<8>(src, dst),
               "the table must be 16-byte aligned, the complex operands 8-byte aligned");
    const long long KP = ((long long)nlat + 3) / 4 * 4, LP = ((long long)lmax + 3) / 4 * 4;
    MK_REQUIRE(mk_latdft_table_len(nlat, lmax) * 4 < (1LL << 31), "table over 2^31 bytes");
    // TransStager: 32-bit byte offsets inside one 32-row k-step of the data operand
    MK_REQUIRE(33LL * 2 * ncols * 4 < (1LL << 31), "operand too large: 33 * 2 * ncols * 4 bytes (one k-step of the data operand) over 2^31");
    LatDftParams p;
    p.src = src;
    p.dst = dst;
    p.N2 = (int)(2 * ncols);
    if (!inv) {
        p.tab = table;
        p.ld = KP;
        p.part = (long long)lmax * KP;
        p.K = nlat;
        p.R = lmax;
    } else {
        p.tab = table + 2 * (long long)lmax * KP;
        p.ld = LP;
        p.part = (long long)nlat * LP;
        p.K = lmax;
        p.R = nlat;
    }
    p.tiles_m = mk::ceil_div(p.R, XM / 2);
    p.tiles_n = mk::ceil_div(p.N2, XN);
    return x3_launch(__func__, inv ? latdft_x3_kernel<true> : latdft_x3_kernel<false>, grid_blocks(p.tiles_n, p.tiles_m, 1), stream, p);
}

extern "C" int mk_latdft_fwd(const float* xf, const float* table, float* c, int nlat, int lmax, long long ncols, void* stream) {
    return latdft_launch(false, xf, table, c, nlat, lmax, ncols, stream);
}

extern "C" int mk_latdft_inv(const float* c, const float* table, float* xf, int nlat, int lmax, long long ncols, void* stream) {
    return latdft_launch(true, c, table, xf, nlat, lmax, ncols, stream);
}
