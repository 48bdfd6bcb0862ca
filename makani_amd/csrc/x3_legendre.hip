// Legendre analysis / synthesis (K2 / K3) on the bf16x3 engine, and the one-time layout of their tables.
#include "x3_engine.h"

namespace {

// The constant operand (Legendre table) as fp32 tiles ([128 rows][32 k] floats = 16 KB per k-step), split into the bf16x3
// pieces while staging.  (A pre-split bf16x3 image -- 24 KB per k-step copied straight into LDS -- was built and measured
// 2 % slower in isolation and 0 - 0.2 ms per step slower, with one half more table bytes; removed in round 3.)
struct F32TileStager {
    const char* base;
    typedef float4 Regs[4];
    static constexpr int TILE_BYTES = XM * XK * 4;
    struct AllRows {   // the tiles are whole: zero padded by mk_legendre_x3_split
        static __device__ __forceinline__ bool live(int, int) { return true; }
    };
    static __device__ __forceinline__ int row_off(int r) { return plain_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const float* p = reinterpret_cast<const float*>(base + (long long)kt * TILE_BYTES);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = tid + q * XT, row = (t >> 6) * 16 + quad_row(t & 63);
            const float* pr = p + row * XK + (t & 3) * 8;
            r[2 * q] = *reinterpret_cast<const float4*>(pr);
            r[2 * q + 1] = *reinterpret_cast<const float4*>(pr + 4);
        }
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const { row8_sstore<AllRows>(r, img, tid, XM); }
};

struct LegX3Params {
    const float* src;
    const char* tab;   // table tiles (mk_legendre_x3_split)
    float* dst;
    int K, L, Mloc, m_off, N2;
    int RT;   // analysis layout: 128-row tiles per m (rows l = m + 128 rt + r);  synthesis layout: k tiles
    int KC;   // analysis layout: 32-k chunks;                                   synthesis layout: 32-l chunks
    int tiles_n;
    int kmajor;   // layout of the Fourier rows: 0 = xf[m][k][:], 1 = xf[k][m][:] (latitude major, distributed SHT)
    int exp;  // ablation switches (MK_X3_EXP), see x3_tile
};

// c[l][m][:] = sum_k W[m][l][k] xf[m][k][:]   (rows l >= m only)
__global__ __launch_bounds__(XT, 3) void legendre_fwd_x3_kernel(LegX3Params p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.Mloc, p.RT, p.tiles_n);
    if (!t.valid) return;
    const int m = t.batch, mg = p.m_off + m;
    const int l0 = mg + t.tm * XM;
    if (l0 >= p.L) return;
    const int n0 = t.tn * XN;
    F32TileStager as;
    as.base = p.tab + ((long long)mg * p.RT + t.tm) * p.KC * F32TileStager::TILE_BYTES;
    TransStager bs;
    bs.base = p.src + (p.kmajor ? (long long)m * p.N2 : (long long)m * p.K * p.N2) + n0;
    bs.ldk = p.kmajor ? (long long)p.Mloc * p.N2 : (long long)p.N2;
    bs.k_lo = 0;
    bs.k_hi = p.K;
    bs.cvalid = p.N2 - n0;
    const StoreEpi epi{p.dst + ((long long)l0 * p.Mloc + m) * p.N2 + n0, (long long)p.Mloc * p.N2};
    x3_tile(as, bs, 0, p.KC, p.L - l0, p.N2 - n0, epi, lds_x3, p.exp);
}

// xf[m][k][:] = sum_{l >= m} P[m][l][k] c[l][m][:]
__global__ __launch_bounds__(XT, 3) void legendre_inv_x3_kernel(LegX3Params p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.Mloc, p.RT, p.tiles_n);
    if (!t.valid) return;
    const int m = t.batch, mg = p.m_off + m;
    const int k0 = t.tm * XM;
    if (k0 >= p.K) return;
    const int n0 = t.tn * XN;
    F32TileStager as;
    as.base = p.tab + ((long long)mg * p.RT + t.tm) * p.KC * F32TileStager::TILE_BYTES;
    TransStager bs;
    bs.base = p.src + (long long)m * p.N2 + n0;
    bs.ldk = (long long)p.Mloc * p.N2;
    bs.k_lo = mg;
    bs.k_hi = p.L;
    bs.cvalid = p.N2 - n0;
    const int kt0 = mg >> 5;
    const StoreEpi epi{p.kmajor ? p.dst + ((long long)k0 * p.Mloc + m) * p.N2 + n0 : p.dst + ((long long)m * p.K + k0) * p.N2 + n0,
                       p.kmajor ? (long long)p.Mloc * p.N2 : (long long)p.N2};
    x3_tile(as, bs, kt0 < p.KC ? kt0 : p.KC, p.KC, p.K - k0, p.N2 - n0, epi, lds_x3, p.exp);
}

// table [M][L][KP] fp32 -> fp32 tiles [block][128 rows][32 k], zero padded.  One thread per (block, row, kk).
__global__ void legendre_x3_split_kernel(const float* __restrict__ tab, void* __restrict__ out, int K, int KP, int L,
                                         int M, int RT, int KC, int inverse, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int kk = (int)(idx & 31);
    const int r = (int)((idx >> 5) & 127);
    long long blk = idx >> 12;
    const int kc = (int)(blk % KC);
    blk /= KC;
    const int rt = (int)(blk % RT);
    const int m = (int)(blk / RT);
    int l, k;
    if (!inverse) {
        l = m + rt * XM + r;
        k = kc * XK + kk;
    } else {
        k = rt * XM + r;
        l = kc * XK + kk;
    }
    float v = 0.f;
    if (l < L && k < K) v = tab[((long long)m * L + l) * KP + k];
    reinterpret_cast<float*>(out)[idx] = v;
}

void x3_layout(int nlat, int lmax, int inverse, int* RT, int* KC) {
    if (!inverse) {
        *RT = mk::ceil_div(lmax, XM);
        *KC = mk::ceil_div(nlat, XK);
    } else {
        *RT = mk::ceil_div(nlat, XM);
        *KC = mk::ceil_div(lmax, XK);
    }
}

// the checks and the launch of both directions, reported under the entry point's name
int legendre_x3_launch(const char* who, bool fwd, const float* src, const void* tab, float* dst, int bc, int nlat, int lmax,
                       int mmax_loc, int m_off, int mmax_glob, int xf_layout, void* stream) {
    MK_REQUIRE_AS(who, src && tab && dst, "null pointer");
    MK_REQUIRE_AS(who, bc > 0 && nlat > 0 && lmax > 0 && mmax_loc > 0, "bad sizes");
    MK_REQUIRE_AS(who, m_off >= 0 && m_off + mmax_loc <= mmax_glob, "mode shard out of range");
    MK_REQUIRE_AS(who, xf_layout == 0 || xf_layout == 1, "xf_layout must be 0 ([M][K][BC]) or 1 ([K][M][BC])");
    LegX3Params p;
    p.kmajor = xf_layout;
    p.src = src;
    p.tab = (const char*)tab;
    p.dst = dst;
    p.K = nlat;
    p.L = lmax;
    p.Mloc = mmax_loc;
    p.m_off = m_off;
    p.N2 = 2 * bc;
    x3_layout(nlat, lmax, fwd ? 0 : 1, &p.RT, &p.KC);
    p.tiles_n = mk::ceil_div(p.N2, XN);
    p.exp = x3_exp();
    const long long nblk = grid_blocks(mmax_loc, p.RT, p.tiles_n);
    // TransStager: 32-bit byte offsets inside one 32-row k-step of the data operand (row stride Mloc * N2 floats at most)
    MK_REQUIRE_AS(who, nblk < 2147483647LL && 33LL * p.Mloc * p.N2 * 4 < (1LL << 31),
               "operand too large: grid over 2^31 blocks, or 33 * mmax_loc * 2 * bc * 4 bytes (one k-step of the data operand) over 2^31");
    return x3_launch(who, fwd ? legendre_fwd_x3_kernel : legendre_inv_x3_kernel, nblk, stream, p);
}

}  // namespace

extern "C" long long mk_legendre_x3_bytes(int nlat, int lmax, int mmax, int inverse) {
    if (nlat <= 0 || lmax <= 0 || mmax <= 0) return 0;
    int RT, KC;
    x3_layout(nlat, lmax, inverse, &RT, &KC);
    return (long long)mmax * RT * KC * F32TileStager::TILE_BYTES;
}

extern "C" int mk_legendre_x3_split(const float* tab, void* out, int nlat, int lmax, int mmax, int inverse, void* stream) {
    MK_REQUIRE(tab && out, "null pointer");
    MK_REQUIRE(nlat > 0 && lmax > 0 && mmax > 0, "bad sizes");
    int RT, KC;
    x3_layout(nlat, lmax, inverse, &RT, &KC);
    const long long total = (long long)mmax * RT * KC * XM * XK;
    const long long nblk = (total + 255) / 256;
    MK_REQUIRE(nblk < 2147483647LL, "grid too large");
    hipLaunchKernelGGL(legendre_x3_split_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, tab,
                       out, nlat, mk_legendre_kpad(nlat), lmax, mmax, RT, KC, inverse, total);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_legendre_fwd_x3_ex(const float* xf, const void* tab_x3, float* c, int bc, int nlat, int lmax,
                                     int mmax_loc, int m_off, int mmax_glob, int xf_layout, void* stream) {
    return legendre_x3_launch(__func__, true, xf, tab_x3, c, bc, nlat, lmax, mmax_loc, m_off, mmax_glob, xf_layout, stream);
}

extern "C" int mk_legendre_fwd_x3(const float* xf, const void* tab_x3, float* c, int bc, int nlat, int lmax, int mmax_loc,
                                  int m_off, int mmax_glob, void* stream) {
    return mk_legendre_fwd_x3_ex(xf, tab_x3, c, bc, nlat, lmax, mmax_loc, m_off, mmax_glob, 0, stream);
}

extern "C" int mk_legendre_inv_x3_ex(const float* c, const void* tab_x3, float* xf, int bc, int nlat, int lmax,
                                     int mmax_loc, int m_off, int mmax_glob, int xf_layout, void* stream) {
    return legendre_x3_launch(__func__, false, c, tab_x3, xf, bc, nlat, lmax, mmax_loc, m_off, mmax_glob, xf_layout, stream);
}

extern "C" int mk_legendre_inv_x3(const float* c, const void* tab_x3, float* xf, int bc, int nlat, int lmax, int mmax_loc,
                                  int m_off, int mmax_glob, void* stream) {
    return mk_legendre_inv_x3_ex(c, tab_x3, xf, bc, nlat, lmax, mmax_loc, m_off, mmax_glob, 0, stream);
}
