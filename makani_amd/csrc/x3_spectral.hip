// The per-degree products on the private spectrum, on the bf16x3 engine: the dhconv spectral filter (K5), the real channel mix
// and the complex channel MLP.  They share the triangular row count -- rows (m <= l, b) per degree; entries with l < m are
// neither read nor written -- and the complex stagers.
#include "x3_engine.h"

namespace {

// rows (local modes with global m <= global l, times the batch) of local degree l
__device__ __forceinline__ int tri_rows(int Mloc, int B, int l_off, int m_off, int l) {
    int nm = l_off + l - m_off + 1;
    nm = nm < 0 ? 0 : (nm > Mloc ? Mloc : nm);
    return nm * B;
}

// The contraction of a weight gradient whose panel is shared by SEVERAL degrees walks their valid rows: k-step kt of the
// workgroup is rows [16 j, 16 j + 16) of degree l0 + kt / KPL, j = kt % KPL, with KPL the k-steps of the group's last (longest)
// degree; rows past a degree's own count read as zero (no load is issued for them).  Stagers take the walk as a compile-time
// option (WALK): without it they stay on the one degree their base points at.
struct DegreeWalk {
    long long lpitch;     // floats per degree
    int l0, KPL;
    int Mloc, B, l_off, m_off;
    // k-step kt -> its degree's first float (from `base`), the step's first row kk0 within the degree and the degree's row count
    __device__ __forceinline__ const float* step(const float* base, int kt, int w, int& kk0, int& rows) const {
        const int li = kt / KPL, l = l0 + li;
        kk0 = (kt - li * KPL) * (XK / 2) + w * 4;
        rows = tri_rows(Mloc, B, l_off, m_off, l);
        return base + (long long)l * lpitch;
    }
};

// Complex k-major B operand: element (kk, o) = (base[(kk * ldk + o) * 2], base[... + 1]), kk < kk_hi,
// o < ovalid.  Complex column o becomes the image rows n = 2o (real part of the product) and 2o + 1
// (imaginary part); complex row kk the contraction indices k = 2kk, 2kk + 1:
//   CONJ_B = false (forward, B = w):       row 2o: [ re, -im ]   row 2o+1: [ im,  re ]
//   CONJ_B = true  (wgrad,  B = gy, the conjugate sits on the A side): row 2o: [ re, im ]  row 2o+1: [ im, -re ]
template <bool CONJ_B, bool WALK = false>
struct CplxStager {
    const float* base;
    long long ldk;
    int kk_hi = 0, ovalid;      // kk_hi: without WALK
    DegreeWalk walk = {};     // with WALK
    typedef float2 Regs[4];
    static __device__ __forceinline__ int row_off(int r) { return pair_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const int w = __builtin_amdgcn_readfirstlane(tid >> 6), o = tid & 63;
        int kk0, hi;
        const float* b = base;
        if constexpr (WALK) {
            b = walk.step(base, kt, w, kk0, hi);
        } else {
            kk0 = kt * (XK / 2) + w * 4;
            hi = kk_hi;
        }
        const bool ook = o < ovalid;
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            r[i] = x3_load8(rs, (ook && kk0 + i < hi) ? (unsigned)((((long long)(kk0 + i)) * ldk + o) * 8) : X3_OOB);
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const {
        const int w = tid >> 6, t = tid & 63;
        float a[8], b[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float re = r[i].x, im = r[i].y;
            a[2 * i] = re;
            a[2 * i + 1] = CONJ_B ? im : -im;
            b[2 * i] = im;
            b[2 * i + 1] = CONJ_B ? -re : re;
        }
        split_store8(a, img + t * XPITCH + w * 16);
        split_store8(b, img + (t + 64) * XPITCH + 128 + w * 16);
    }
};

// Data-gradient B operand: gx[(i,c)] = sum_(o,d) gy[(o,d)] * B[(o,d)][(i,c)] with B = conj(w)^T.  Complex
// w[i][o] at base[(i * O + o) * 2]; image rows n = 2i (-> real part), 2i + 1 (-> imaginary part), contraction
// k = 2o + d:   row 2i: [ re, im ]   row 2i+1: [ -im, re ].   A thread loads 4 consecutive o of one i.
struct DgradStager {
    const float* base;
    int O, ivalid;
    typedef float4 Regs[2];
    static __device__ __forceinline__ int row_off(int r) { return pair_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const int i = (tid >> 6) * 16 + quad_row(tid & 63), o = kt * (XK / 2) + (tid & 3) * 4;
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(base);
        const unsigned off = (unsigned)(((long long)i * O + o) * 8);
#pragma unroll
        for (int h = 0; h < 2; ++h) r[h] = x3_load16(rs, (i < ivalid && o + 2 * h < O) ? off + 16 * h : X3_OOB);
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const {
        const int i = (tid >> 6) * 16 + quad_row(tid & 63), c = tid & 3;
        const float a[8] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w};
        const float b[8] = {-r[0].y, r[0].x, -r[0].w, r[0].z, -r[1].y, r[1].x, -r[1].w, r[1].z};
        split_store8(a, img + i * XPITCH + c * 16);
        split_store8(b, img + (i + 64) * XPITCH + 128 + c * 16);
    }
};

// Weight-gradient operand with the channels as image rows: complex x[r][c] at base[(r * C + c) * 2]; image row c holds, per
// 4 complex rows r < r_hi, [re, im] x 4: contraction index k = (r, re / im).  Two channels per thread.  As the A operand of a
// complex weight gradient, gw[i][(o,d)] = sum_(r,c) A[i][(r,c)] * B[(r,c)][(o,d)], the conjugate is in CplxStager<true>'s signs.
// PAIR: the rows in the pair layout (the B operand: a fragment reads rows 2j + b).
template <bool PAIR, bool WALK>
struct ChanKStager {
    const float* base;    // field + first channel of the tile
    long long C;          // channels (complex row pitch)
    int r_hi = 0, cvalid;       // r_hi: without WALK
    DegreeWalk walk = {};     // with WALK
    typedef float2 Regs[8];
    static __device__ __forceinline__ int row_off(int r) { return PAIR ? pair_off(r) : plain_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const int w = __builtin_amdgcn_readfirstlane(tid >> 6), t = tid & 63;
        int r0, hi;
        const float* b = base;
        if constexpr (WALK) {
            b = walk.step(base, kt, w, r0, hi);
        } else {
            r0 = kt * (XK / 2) + w * 4;
            hi = r_hi;
        }
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(b);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = t + 64 * e;
            const bool cok = c < cvalid;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                r[4 * e + j] = x3_load8(rs, (cok && r0 + j < hi) ? (unsigned)((((long long)(r0 + j)) * C + c) * 8) : X3_OOB);
        }
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const {
        const int w = tid >> 6, t = tid & 63;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float v[8] = {r[4 * e].x, r[4 * e].y, r[4 * e + 1].x, r[4 * e + 1].y,
                                r[4 * e + 2].x, r[4 * e + 2].y, r[4 * e + 3].x, r[4 * e + 3].y};
            split_store8(v, img + row_off(t + 64 * e) + w * 16);
        }
    }
};

// ---------------------------------------------------------------------------
// Complex [I][O] weight panels: dhconv forward / dgrad / wgrad (same contracts as the fp32 kernels of gemm.hip; cin, cout even)
// and the complex channel MLP (SpectralAttention, filter_type="non-linear"): per layer
//   y[l][m][b][o] = act(sum_i x[l][m][b][i] w[l * ws][i][o] + bias[o])
// with one panel per degree (ws = I * O, "l-dependant": the dhconv layout) or one for all (ws = 0, "diagonal"), a complex
// per-channel bias and ComplexReLU `real` / `cartesian`, both applied in fp32 on the accumulator (CplxBiasReluEpi).
// The data gradient multiplies by relu' read off the saved activation OUTPUT of the layer in front (CplxMaskEpi).  The per-degree
// weight gradient is dhconv's; the shared one contracts G consecutive degrees per workgroup into a partial panel (plain stores)
// and a second pass adds the partials in ascending group order: no atomics, the same bits on every run.  The bias gradient is two
// fixed-order passes in float64.
// ---------------------------------------------------------------------------
struct PanelParams {
    const float* a;      // x (fwd, wgrad) or gy (dgrad)
    const float* b;      // w (fwd, dgrad) or gy (wgrad)
    float* dst;
    const float* bias;   // MLP fwd: interleaved complex [O] or null
    const float* aux;    // MLP masked dgrad: saved activation output [L][M][B][I]
    long long ws;        // complex elements between the weight panels of consecutive degrees (0: one shared panel)
    int Lloc, Mloc, B, I, O, l_off, m_off, tiles_m, tiles_n;
    int act;             // MLP: 0 none, 1 ReLU on the real parts, 2 on both (ComplexReLU `real` / `cartesian`)
    int exp;             // ablation switches (MK_X3_EXP), see x3_tile
    int G, ngroups;      // shared wgrad: degrees per workgroup, number of such groups
};

// The tile's columns (2o, 2o + 1) are (re, im) of output channel o, so a lane owns (re, im) of one complex output per register:
// bias / mask in fp32 on the accumulator, one 8-byte store.

// store act(tile + bias[column]); `bias` points at the tile's first column of the interleaved complex bias (null: none)
struct CplxBiasReluEpi {
    float* cbase;
    long long ldc;
    const float* bias;
    int act;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ CplxBiasReluEpi(const PanelParams& p, long long off, long long ldc_, int n0)
        : cbase(p.dst + off), ldc(ldc_), bias(p.bias ? p.bias + n0 : nullptr), act(p.act) {}
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
            const bool relu_re = act >= 1, relu_im = act == 2;
            float b0 = 0.f, b1 = 0.f;
            if (bias) {
                b0 = bias[col];
                b1 = bias[col + 1];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        x3_f2 v2;
                        v2[0] = acc[a][0][r] + b0;
                        v2[1] = acc[a][1][r] + b1;
                        if (relu_re) v2[0] = v2[0] > 0.f ? v2[0] : 0.f;
                        if (relu_im) v2[1] = v2[1] > 0.f ? v2[1] : 0.f;
                        // (plain store: the next product of the chain reads these rows back)
                        *reinterpret_cast<x3_f2*>(cbase + (long long)row * ldc + col) = v2;
                    }
                }
        }
    }
};

// the masked data gradient: store tile * (aux > 0) with `aux` the saved activation output at the tile's origin (row pitch
// ldc); act 1 masks the real parts only, act 2 both
struct CplxMaskEpi {
    float* cbase;
    long long ldc;
    const float* aux;
    int act;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ CplxMaskEpi(const PanelParams& p, long long off, long long ldc_, int)
        : cbase(p.dst + off), ldc(ldc_), aux(p.aux + off), act(p.act) {}
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        const bool both = act == 2;
        if (col < cvalid) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        const long long off = (long long)row * ldc + col;
                        x3_f2 v2;
                        const float2 m = *reinterpret_cast<const float2*>(aux + off);
                        v2[0] = m.x > 0.f ? acc[a][0][r] : 0.f;
                        v2[1] = (!both || m.y > 0.f) ? acc[a][1][r] : 0.f;
                        *reinterpret_cast<x3_f2*>(cbase + off) = v2;
                    }
                }
        }
    }
};

// the plain store of the panel kernels (dhconv, the MLP's first-layer data gradient)
struct PanelStoreEpi : StoreEpi {
    __device__ __forceinline__ PanelStoreEpi(const PanelParams& p, long long off, long long ldc_, int) : StoreEpi{p.dst + off, ldc_} {}
};

// The forward and the data-gradient kernel of complex [I][O] panels.  ABLATE: the kernel takes the MK_X3_EXP switches.  dhconv's
// do, as ever; the channel MLP's do not, as ever: with the run-time switches in its main loop the masked data gradient measured
// 7 % slower (0.487 -> 0.521 ms) than with the loop the compiler builds for exp = 0.

// y[l][r][:] = epilogue(x[l][r][:] * w[l * ws])   (rows r = (m, b) with m <= l)
template <class EPI, bool ABLATE>
__global__ __launch_bounds__(XT, 3) void dhconv_fwd_x3_kernel(PanelParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.Lloc, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int l = p.Lloc - 1 - t.batch;  // heaviest degrees first
    const int R = tri_rows(p.Mloc, p.B, p.l_off, p.m_off, l);
    const int r0 = t.tm * XM;
    if (r0 >= R) return;
    const int n0 = t.tn * XN;
    const long long rowbase = (long long)l * p.Mloc * p.B + r0;
    RowStager as;
    as.base = p.a + rowbase * 2 * p.I;
    as.ld = 2 * p.I;
    as.rows = R - r0;
    as.kvalid = 2 * p.I;
    CplxStager<false> bs;
    bs.base = p.b + ((long long)l * p.ws + n0 / 2) * 2;
    bs.ldk = p.O;
    bs.kk_hi = p.I;
    bs.ovalid = p.O - n0 / 2;
    const EPI epi(p, rowbase * 2 * p.O + n0, 2LL * p.O, n0);
    x3_tile(as, bs, 0, (2 * p.I + XK - 1) / XK, R - r0, 2 * p.O - n0, epi, lds_x3, ABLATE ? p.exp : 0);
}

// gx[l][r][:] = epilogue(gy[l][r][:] * conj(w[l * ws])^T)
template <class EPI, bool ABLATE>
__global__ __launch_bounds__(XT, 3) void dhconv_dgrad_x3_kernel(PanelParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.Lloc, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int l = p.Lloc - 1 - t.batch;
    const int R = tri_rows(p.Mloc, p.B, p.l_off, p.m_off, l);
    const int r0 = t.tm * XM;
    if (r0 >= R) return;
    const int n0 = t.tn * XN;
    const long long rowbase = (long long)l * p.Mloc * p.B + r0;
    RowStager as;
    as.base = p.a + rowbase * 2 * p.O;
    as.ld = 2 * p.O;
    as.rows = R - r0;
    as.kvalid = 2 * p.O;
    DgradStager bs;
    bs.base = p.b + ((long long)l * p.ws + (long long)(n0 / 2) * p.O) * 2;
    bs.O = p.O;
    bs.ivalid = p.I - n0 / 2;
    const EPI epi(p, rowbase * 2 * p.I + n0, 2LL * p.I, n0);
    x3_tile(as, bs, 0, (2 * p.O + XK - 1) / XK, R - r0, 2 * p.I - n0, epi, lds_x3, ABLATE ? p.exp : 0);
}

// gw[l][i][:] = sum_r conj(x[l][r][i]) gy[l][r][:]
__global__ __launch_bounds__(XT, 3) void dhconv_wgrad_x3_kernel(PanelParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.Lloc, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int l = p.Lloc - 1 - t.batch;
    const int R = tri_rows(p.Mloc, p.B, p.l_off, p.m_off, l);   // contraction length (may be 0: the gradient of that degree is zero)
    const int i0 = t.tm * XM;
    if (i0 >= p.I) return;
    const int n0 = t.tn * XN;
    const long long rowbase = (long long)l * p.Mloc * p.B;
    ChanKStager<false, false> as;
    as.base = p.a + (rowbase * p.I + i0) * 2;
    as.C = p.I;
    as.r_hi = R;
    as.cvalid = p.I - i0;
    CplxStager<true> bs;
    bs.base = p.b + (rowbase * p.O + n0 / 2) * 2;
    bs.ldk = p.O;
    bs.kk_hi = R;
    bs.ovalid = p.O - n0 / 2;
    const StoreEpi epi{p.dst + ((long long)l * p.I + i0) * 2 * p.O + n0, 2LL * p.O};
    x3_tile(as, bs, 0, (2 * R + XK - 1) / XK, p.I - i0, 2 * p.O - n0, epi, lds_x3, p.exp);
}

// part[g][i][o] = sum over the valid rows of the degrees of group g of conj(x[.][i]) gy[.][o]
__global__ __launch_bounds__(XT, 3) void spec_cmlp_wgrad_shared_kernel(PanelParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.ngroups, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int g = p.ngroups - 1 - t.batch;
    const int l0 = g * p.G, l1 = l0 + p.G < p.Lloc ? l0 + p.G : p.Lloc;
    // k-steps per degree: those of the group's last (longest) one; 0 = no valid row in the group, the tile stores zeros
    const int KPL = (tri_rows(p.Mloc, p.B, p.l_off, p.m_off, l1 - 1) + XK / 2 - 1) / (XK / 2);
    const int i0 = t.tm * XM, n0 = t.tn * XN;
    if (i0 >= p.I) return;
    ChanKStager<false, true> as;
    as.base = p.a + 2 * i0;
    as.C = p.I;
    as.cvalid = p.I - i0;
    as.walk = {2LL * p.Mloc * p.B * p.I, l0, KPL > 0 ? KPL : 1, p.Mloc, p.B, p.l_off, p.m_off};
    CplxStager<true, true> bs;
    bs.base = p.b + n0;
    bs.ldk = p.O;
    bs.ovalid = p.O - n0 / 2;
    bs.walk = as.walk;
    bs.walk.lpitch = 2LL * p.Mloc * p.B * p.O;
    const StoreEpi epi{p.dst + ((long long)g * p.I + i0) * 2 * p.O + n0, 2LL * p.O};
    x3_tile(as, bs, 0, (l1 - l0) * KPL, p.I - i0, 2 * p.O - n0, epi, lds_x3);
}

// dst[e] = sum_g part[g][e] in ascending g; n4 float4 elements per panel.  Eight panels' loads are issued before their adds (a
// small layer has one panel per degree and few elements: one load in flight per thread is a chain of memory latencies)
__global__ void spec_cmlp_group_sum_kernel(const float4* __restrict__ part, float4* __restrict__ dst, long long n4, int ngroups) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n4) return;
    float4 s = part[e];
    int g = 1;
    for (; g + 8 <= ngroups; g += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[(long long)(g + j) * n4 + e];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s.x += v[j].x;
            s.y += v[j].y;
            s.z += v[j].z;
            s.w += v[j].w;
        }
    }
    for (; g < ngroups; ++g) {
        const float4 v = part[(long long)g * n4 + e];
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
    }
    dst[e] = s;
}

// part[l][c] = sum over the valid rows r of degree l of g[l][r][c], c over the 2 O floats of a row; float64, four interleaved
// chains per thread added in a fixed order
__global__ __launch_bounds__(256) void spec_cmlp_bgrad_rows_kernel(const float* __restrict__ g, double* __restrict__ part, int Mloc,
                                                                   int B, int O2, int l_off, int m_off, int chunks) {
    const int l = blockIdx.x / chunks, c = (blockIdx.x - l * chunks) * 256 + threadIdx.x;
    if (c >= O2) return;
    const int R = tri_rows(Mloc, B, l_off, m_off, l);
    const float* p = g + (long long)l * Mloc * B * O2 + c;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int r = 0;
    for (; r + 4 <= R; r += 4)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += (double)p[(long long)(r + j) * O2];
    for (int j = 0; r < R; ++r, ++j) s[j] += (double)p[(long long)r * O2];
    part[(long long)l * O2 + c] = (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ void spec_cmlp_bgrad_sum_kernel(const double* __restrict__ part, float* __restrict__ gb, int Lloc, int O2) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= O2) return;
    double s = 0.0;
    for (int l = 0; l < Lloc; ++l) s += part[(long long)l * O2 + c];
    gb[c] = (float)s;
}

// degrees per workgroup of the shared weight gradient: about three workgroups per CU
int cmlp_group_size(int lloc, int cin, int cout) {
    const long long tiles = (long long)mk::ceil_div(cin, XM) * mk::ceil_div(2 * cout, XN);
    const long long G = mk::ceil_div_ll((long long)lloc * tiles, 768LL);
    return (int)(G < 1 ? 1 : G);
}

// ---------------------------------------------------------------------------
// Real, degree-independent channel mix on the private spectrum: y[l][m][b][o] = sum_i W[o][i] x[l][m][b][i], W fp32 [O][I].
// A 1x1 convolution without bias commutes with the (channel-blind, linear) spherical harmonic transform, so a convolution
// next to a transform is evaluated here, on ~18x fewer values than on the grid.  The real and the imaginary part of a
// coefficient are two rows of the A image that meet the same W fragment (contraction length I, not the 2I of a block-diagonal
// complex form), and come out of the MFMA as adjacent registers of one lane (CplxRowsEpi).
// ---------------------------------------------------------------------------
struct MixParams {
    const float* a;   // x (fwd), gy (dgrad, wgrad)
    const float* w;   // W (fwd, dgrad) or x (wgrad)
    float* dst;
    int Lloc, Mloc, B, Ca, Cd;   // channels of `a`; channels of dst (fwd, dgrad) or of the second field (wgrad)
    int l_off, m_off, tiles_m, tiles_n;
    int G, ngroups;   // wgrad: degrees per workgroup, number of such groups
};

// Complex rows as the A operand: complex row r (64 per tile), channel i contiguous as (re, im) pairs at base[(r * C + i) * 2];
// image row 2r = real parts, 2r + 1 = imaginary parts, contraction index k = i.  One (row, 8 channels) task per thread:
// 64 contiguous bytes of global memory, two 16-byte vectors per piece into LDS.
struct SpecRowStager {
    const float* base;
    long long ld;       // floats per complex row (2 C)
    int rows, cvalid;   // complex rows of the tile, channels (even)
    typedef float4 Regs[4];
    static __device__ __forceinline__ int row_off(int r) { return pair_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(base);
        const int row = (tid >> 6) * 16 + quad_row(tid & 63), i = kt * XK + (tid & 3) * 8;
        const unsigned off = (unsigned)(((long long)row * ld + 2 * i) * 4);
#pragma unroll
        for (int h = 0; h < 4; ++h) r[h] = x3_load16(rs, (row < rows && i + 2 * h < cvalid) ? off + 16 * h : X3_OOB);
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const {
        const int row = (tid >> 6) * 16 + quad_row(tid & 63), c = tid & 3;
        const float re[8] = {r[0].x, r[0].z, r[1].x, r[1].z, r[2].x, r[2].z, r[3].x, r[3].z};
        const float im[8] = {r[0].y, r[0].w, r[1].y, r[1].w, r[2].y, r[2].w, r[3].y, r[3].w};
        if (row < rows) {
            split_store8(re, img + row * XPITCH + c * 16);
            split_store8(im, img + (row + 64) * XPITCH + 128 + c * 16);
        }
    }
};

// Row-major real operand with even (not necessarily multiple-of-4) row length: RowStager on 8-byte loads, rows in the pair
// layout (it is the B operand here: a fragment reads rows 2j + b).
struct Row2Stager {
    const float* base;
    long long ld;
    int rows, kvalid;
    typedef float2 Regs[8];
    static __device__ __forceinline__ int row_off(int r) { return pair_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(base);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = tid + q * XT, row = (t >> 6) * 16 + quad_row(t & 63), k = kt * XK + (t & 3) * 8;
            const unsigned off = (unsigned)(((long long)row * ld + k) * 4);
#pragma unroll
            for (int h = 0; h < 4; ++h)
                r[4 * q + h] = x3_load8(rs, (row < rows && k + 2 * h < kvalid) ? off + 8 * h : X3_OOB);
        }
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = tid + q * XT, row = (t >> 6) * 16 + quad_row(t & 63);
            const float v[8] = {r[4 * q].x, r[4 * q].y, r[4 * q + 1].x, r[4 * q + 1].y,
                                r[4 * q + 2].x, r[4 * q + 2].y, r[4 * q + 3].x, r[4 * q + 3].y};
            if (row < rows) split_store8(v, img + pair_off(row) + (t & 3) * 16);
        }
    }
};

// store complex rows: tile rows 2r, 2r + 1 are the real and imaginary part of complex row r (SpecRowStager): registers (r, r + 1)
// of a lane are (re, im) of one output, the two column parities two adjacent channels -> one 16-byte store per register pair,
// 512 contiguous bytes per wave.  cbase / ldc address the complex rows ([row][channel][2] floats), cvalid is even.
struct CplxRowsEpi {
    float* cbase;
    long long ldc;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        x3_f4 v4;
                        v4[0] = acc[a][0][r];
                        v4[1] = acc[a][0][r + 1];
                        v4[2] = acc[a][1][r];
                        v4[3] = acc[a][1][r + 1];
                        __builtin_nontemporal_store(v4, reinterpret_cast<x3_f4*>(cbase + (long long)(row >> 1) * ldc + 2 * col));
                    }
                }
        }
    }
};

// TRANS = false: y = x W^T (forward, W [Cd][Ca]);  TRANS = true: gx = gy W (data gradient, W [Ca][Cd])
template <bool TRANS>
__global__ __launch_bounds__(XT, 3) void spec_mix_x3_kernel(MixParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.Lloc, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int l = p.Lloc - 1 - t.batch;  // heaviest degrees first
    const int R = tri_rows(p.Mloc, p.B, p.l_off, p.m_off, l);
    const int r0 = t.tm * (XM / 2);
    if (r0 >= R) return;
    const int n0 = t.tn * XN;
    const long long rowbase = (long long)l * p.Mloc * p.B + r0;
    SpecRowStager as;
    as.base = p.a + rowbase * 2 * p.Ca;
    as.ld = 2LL * p.Ca;
    as.rows = R - r0;
    as.cvalid = p.Ca;
    const CplxRowsEpi epi{p.dst + rowbase * 2 * p.Cd + 2 * n0, 2LL * p.Cd};
    const int kts = (p.Ca + XK - 1) / XK;
    if constexpr (TRANS) {
        TransStager bs;
        bs.base = p.w + n0;
        bs.ldk = p.Cd;
        bs.k_lo = 0;
        bs.k_hi = p.Ca;
        bs.cvalid = p.Cd - n0;
        x3_tile(as, bs, 0, kts, 2 * (R - r0), p.Cd - n0, epi, lds_x3);
    } else {
        Row2Stager bs;
        bs.base = p.w + (long long)n0 * p.Ca;
        bs.ld = p.Ca;
        bs.rows = p.Cd - n0;
        bs.kvalid = p.Ca;
        x3_tile(as, bs, 0, kts, 2 * (R - r0), p.Cd - n0, epi, lds_x3);
    }
}

// gW[o][i] += sum over the valid rows of the group's degrees of re(gy[.][o] conj(x[.][i])); a = gy (Ca = O), w = x (Cd = I)
__global__ __launch_bounds__(XT, 3) void spec_mix_wgrad_x3_kernel(MixParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.ngroups, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int g = p.ngroups - 1 - t.batch;
    const int l0 = g * p.G, l1 = l0 + p.G < p.Lloc ? l0 + p.G : p.Lloc;
    const int KPL = (tri_rows(p.Mloc, p.B, p.l_off, p.m_off, l1 - 1) + XK / 2 - 1) / (XK / 2);
    if (KPL == 0) return;
    const int o0 = t.tm * XM, i0 = t.tn * XN;
    ChanKStager<false, true> as;
    as.base = p.a + 2 * o0;
    as.C = p.Ca;
    as.cvalid = p.Ca - o0;
    as.walk = {2LL * p.Mloc * p.B * p.Ca, l0, KPL, p.Mloc, p.B, p.l_off, p.m_off};
    ChanKStager<true, true> bs;
    bs.base = p.w + 2 * i0;
    bs.C = p.Cd;
    bs.cvalid = p.Cd - i0;
    bs.walk = as.walk;
    bs.walk.lpitch = 2LL * p.Mloc * p.B * p.Cd;
    const AtomicEpi epi{p.dst + (long long)o0 * p.Cd + i0, p.Cd};
    x3_tile(as, bs, 0, (l1 - l0) * KPL, p.Ca - o0, p.Cd - i0, epi, lds_x3);
}

// ---------------------------------------------------------------------------
// Block-diagonal complex MLP on the dense planar spectrum (AFNO2D): the channels are cut into nb blocks and block k has its
// own [ib][ob] panel,   y[r][k ob + o] = act(sum_i x[r][k ib + i] w[k][i][o]).
// The spectrum is dense (no triangle), so it is taken as flat rows r < rows = L * M * B of nb * ib complex channels, and the
// block index is the grid's batch dimension: block k is a pointer offset of k * ib complex columns into rows of the full pitch,
// with the stagers' valid counts set to the block's own extent (a k-step never runs into the next block's channels).
// decode_block keeps the tiles of one block on one XCD, next to that block's panel in its L2.
// The soft-shrink is an epilogue type of its own, compile-time like the other modes: the instantiations of the dense MLP and
// dhconv kernels above are untouched.
// ---------------------------------------------------------------------------
struct BlockParams {
    const float* a;      // x (fwd, wgrad) or gy (dgrad)
    const float* b;      // w (fwd, dgrad) or gy (wgrad)
    float* dst;
    const float* aux;    // masked dgrad: saved activation output [rows][nb * ib]
    int rows, nb, ib, ob, tiles_m, tiles_n;
    float lambda;        // soft-shrink threshold
    int rg, ngroups;     // wgrad: rows per group (a multiple of 16), number of groups
    const float* bias = nullptr;     // fwd with bias: interleaved complex [nb * ob]
};

constexpr int BD_STORE = 0, BD_RELU = 2, BD_SHRINK = 3, BD_MASK = 4;
constexpr int BD_BIAS = 8;      // added to BD_STORE / BD_RELU / BD_SHRINK: a complex bias per column in front of the function

// store f(tile) with f fixed at compile time: nothing, ReLU or soft-shrink on both components (fp32, on the accumulator), or the
// mask (aux > 0) per component with `aux` the saved activation output at the tile's origin (row pitch ldc).  The BD_BIAS modes add
// bias[column] (`bias` at the tile's first column) in fp32 on the accumulator first, as CplxBiasReluEpi does for the dense MLP.
template <int MODE>
struct BlockEpi {
    float* cbase;
    long long ldc;
    const float* aux;
    float lambda;
    const float* bias = nullptr;
    static constexpr int F = MODE & 7;
    static constexpr bool PAIRED_BANDS = false;
    static __device__ __forceinline__ float shrink(float v, float l) { return v > l ? v - l : (v < -l ? v + l : 0.f); }
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
            float b0 = 0.f, b1 = 0.f;
            if constexpr ((MODE & BD_BIAS) != 0) {
                b0 = bias[col];
                b1 = bias[col + 1];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        const long long off = (long long)row * ldc + col;
                        x3_f2 v2;
                        v2[0] = acc[a][0][r];
                        v2[1] = acc[a][1][r];
                        if constexpr ((MODE & BD_BIAS) != 0) {
                            v2[0] += b0;
                            v2[1] += b1;
                        }
                        if constexpr (F == BD_RELU) {
                            v2[0] = v2[0] > 0.f ? v2[0] : 0.f;
                            v2[1] = v2[1] > 0.f ? v2[1] : 0.f;
                        } else if constexpr (F == BD_SHRINK) {
                            v2[0] = shrink(v2[0], lambda);
                            v2[1] = shrink(v2[1], lambda);
                        } else if constexpr (F == BD_MASK) {
                            const float2 m = *reinterpret_cast<const float2*>(aux + off);
                            v2[0] = m.x > 0.f ? v2[0] : 0.f;
                            v2[1] = m.y > 0.f ? v2[1] : 0.f;
                        }
                        // (plain store: the next product of the chain, or the inverse transform, reads these rows back)
                        *reinterpret_cast<x3_f2*>(cbase + off) = v2;
                    }
                }
        }
    }
};

// y[r][k ob + :] = f(x[r][k ib + :] * w[k])
template <int MODE>
__global__ __launch_bounds__(XT, 3) void spec_bdmlp_fwd_kernel(BlockParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.nb, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int k = t.batch, r0 = t.tm * XM, n0 = t.tn * XN;
    const long long ci = (long long)p.nb * p.ib, co = (long long)p.nb * p.ob;
    RowStager as;
    as.base = p.a + ((long long)r0 * ci + (long long)k * p.ib) * 2;
    as.ld = 2 * ci;
    as.rows = p.rows - r0;
    as.kvalid = 2 * p.ib;
    CplxStager<false> bs;
    bs.base = p.b + ((long long)k * p.ib * p.ob + n0 / 2) * 2;
    bs.ldk = p.ob;
    bs.kk_hi = p.ib;
    bs.ovalid = p.ob - n0 / 2;
    const BlockEpi<MODE> epi{p.dst + ((long long)r0 * co + (long long)k * p.ob) * 2 + n0, 2 * co, nullptr, p.lambda,
                             (MODE & BD_BIAS) != 0 ? p.bias + (long long)k * p.ob * 2 + n0 : nullptr};
    x3_tile(as, bs, 0, (2 * p.ib + XK - 1) / XK, p.rows - r0, 2 * p.ob - n0, epi, lds_x3);
}

// gx[r][k ib + :] = f(gy[r][k ob + :] * conj(w[k])^T)
template <int MODE>
__global__ __launch_bounds__(XT, 3) void spec_bdmlp_dgrad_kernel(BlockParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.nb, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int k = t.batch, r0 = t.tm * XM, n0 = t.tn * XN;
    const long long ci = (long long)p.nb * p.ib, co = (long long)p.nb * p.ob;
    RowStager as;
    as.base = p.a + ((long long)r0 * co + (long long)k * p.ob) * 2;
    as.ld = 2 * co;
    as.rows = p.rows - r0;
    as.kvalid = 2 * p.ob;
    DgradStager bs;
    bs.base = p.b + ((long long)k * p.ib * p.ob + (long long)(n0 / 2) * p.ob) * 2;
    bs.O = p.ob;
    bs.ivalid = p.ib - n0 / 2;
    const long long off = ((long long)r0 * ci + (long long)k * p.ib) * 2 + n0;
    const BlockEpi<MODE> epi{p.dst + off, 2 * ci, MODE == BD_MASK ? p.aux + off : nullptr, 0.f};
    x3_tile(as, bs, 0, (2 * p.ob + XK - 1) / XK, p.rows - r0, 2 * p.ib - n0, epi, lds_x3);
}

// part[g][k][i][:] = sum over the rows r of group g of conj(x[r][k ib + i]) gy[r][k ob + :]   (batch index = g * nb + k)
__global__ __launch_bounds__(XT, 3) void spec_bdmlp_wgrad_kernel(BlockParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds_x3[];
    const TileId t = decode_block(p.nb * p.ngroups, p.tiles_m, p.tiles_n);
    if (!t.valid) return;
    const int g = t.batch / p.nb, k = t.batch - g * p.nb;
    const int i0 = t.tm * XM, n0 = t.tn * XN;
    const long long ci = (long long)p.nb * p.ib, co = (long long)p.nb * p.ob;
    const long long rbeg = (long long)g * p.rg;
    const int rcnt = p.rows - rbeg < p.rg ? (int)(p.rows - rbeg) : p.rg;
    ChanKStager<false, false> as;
    as.base = p.a + (rbeg * ci + (long long)k * p.ib + i0) * 2;
    as.C = ci;
    as.r_hi = rcnt;
    as.cvalid = p.ib - i0;
    CplxStager<true> bs;
    bs.base = p.b + (rbeg * co + (long long)k * p.ob + n0 / 2) * 2;
    bs.ldk = co;
    bs.kk_hi = rcnt;
    bs.ovalid = p.ob - n0 / 2;
    const StoreEpi epi{p.dst + (((long long)g * p.nb + k) * p.ib + i0) * 2 * p.ob + n0, 2LL * p.ob};
    x3_tile(as, bs, 0, (2 * rcnt + XK - 1) / XK, p.ib - i0, 2 * p.ob - n0, epi, lds_x3);
}

// out = gy where the same component of the saved soft-shrink output s is non-zero, else 0: softshrink' read off its output
__global__ void spec_bdmlp_mask_kernel(const float4* __restrict__ gy, const float4* __restrict__ s, float4* __restrict__ out,
                                       long long n4) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n4) return;
    const float4 g = gy[e], m = s[e];
    out[e] = make_float4(m.x != 0.f ? g.x : 0.f, m.y != 0.f ? g.y : 0.f, m.z != 0.f ? g.z : 0.f, m.w != 0.f ? g.w : 0.f);
}

// rows per group of the block weight gradient: about two workgroups per CU, whole k-steps (16 complex rows)
int bdmlp_group_rows(int rows, int nb, int ib, int ob) {
    const long long tiles = (long long)nb * mk::ceil_div(ib, XM) * mk::ceil_div(2 * ob, XN);
    const long long want = tiles >= 512 ? 1 : 512 / tiles;
    return (int)(mk::ceil_div_ll(mk::ceil_div_ll(rows, want), 16) * 16);
}

}  // namespace

static int dh_x3_check(const void* a, const void* b, const void* c, int lloc, int mloc, int batch, int cin, int cout,
                       int l_off, int m_off) {
    MK_REQUIRE(a && b && c, "null pointer");
    MK_REQUIRE(lloc > 0 && mloc > 0 && batch > 0 && cin > 0 && cout > 0, "bad sizes");
    MK_REQUIRE(l_off >= 0 && m_off >= 0, "negative shard offset");
    MK_REQUIRE(cin % 2 == 0 && cout % 2 == 0, "the bf16x3 dhconv kernels need even channel counts (use the fp32 kernels)");
    return 0;
}

// the parameters of a panel kernel whose tiles cover `rows_m` rows by 2 * `cols` floats; ws = cin * cout: one panel per degree
static PanelParams panel_params(const float* a, const float* b, float* dst, int lloc, int mloc, int batch, int cin, int cout,
                                int l_off, int m_off, int rows_m, int cols, bool per_degree = true) {
    return PanelParams{a, b, dst, nullptr, nullptr, per_degree ? (long long)cin * cout : 0LL, lloc, mloc, batch, cin, cout,
                       l_off, m_off, mk::ceil_div(rows_m, XM), mk::ceil_div(2 * cols, XN), 0, x3_exp(), 1, 0};
}

extern "C" int mk_dhconv_fwd_x3(const float* x, const float* w, float* y, int lloc, int mloc, int batch, int cin,
                                int cout, int l_off, int m_off, void* stream) {
    if (int e = dh_x3_check(x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    const PanelParams p = panel_params(x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off, mloc * batch, cout);
    return x3_launch(__func__, dhconv_fwd_x3_kernel<PanelStoreEpi, true>, grid_blocks(lloc, p.tiles_m, p.tiles_n), stream, p);
}

extern "C" int mk_dhconv_dgrad_x3(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch, int cin,
                                  int cout, int l_off, int m_off, void* stream) {
    if (int e = dh_x3_check(gy, w, gx, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    const PanelParams p = panel_params(gy, w, gx, lloc, mloc, batch, cin, cout, l_off, m_off, mloc * batch, cin);
    return x3_launch(__func__, dhconv_dgrad_x3_kernel<PanelStoreEpi, true>, grid_blocks(lloc, p.tiles_m, p.tiles_n), stream, p);
}

extern "C" int mk_dhconv_wgrad_x3(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch, int cin,
                                  int cout, int l_off, int m_off, void* stream) {
    if (int e = dh_x3_check(x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    const PanelParams p = panel_params(x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off, cin, cout);
    return x3_launch(__func__, dhconv_wgrad_x3_kernel, grid_blocks(lloc, p.tiles_m, p.tiles_n), stream, p);
}

static int spec_mix_check(const void* a, const void* b, const void* c, int lloc, int mloc, int batch, int cin, int cout, int l_off,
                          int m_off) {
    MK_REQUIRE(a && b && c, "null pointer");
    MK_REQUIRE(lloc > 0 && mloc > 0 && batch > 0 && cin > 0 && cout > 0, "bad sizes");
    MK_REQUIRE(l_off >= 0 && m_off >= 0, "negative shard offset");
    MK_REQUIRE(cin % 2 == 0 && cout % 2 == 0, "the spectral channel mix needs even channel counts");
    MK_REQUIRE(mk::aligned<16>(a, b, c), "operands must be 16-byte aligned");
    const long long cmax = cin > cout ? cin : cout;
    MK_REQUIRE((long long)mloc * batch * cmax * 8 < (1LL << 31) && 33LL * cmax * 4 < (1LL << 31),
               "one degree of the spectrum must stay below 2^31 bytes");
    return 0;
}

static int spec_mix_launch(bool trans, const float* a, const float* w, float* dst, int lloc, int mloc, int batch, int ca, int cd,
                           int l_off, int m_off, void* stream) {
    const MixParams p{a, w, dst, lloc, mloc, batch, ca, cd, l_off, m_off, mk::ceil_div(mloc * batch, XM / 2), mk::ceil_div(cd, XN), 1, 0};
    return x3_launch(__func__, trans ? spec_mix_x3_kernel<true> : spec_mix_x3_kernel<false>, grid_blocks(lloc, p.tiles_m, p.tiles_n),
                     stream, p);
}

extern "C" int mk_spec_mix_fwd(const float* x, const float* w, float* y, int lloc, int mloc, int batch, int cin, int cout,
                               int l_off, int m_off, void* stream) {
    if (int e = spec_mix_check(x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    return spec_mix_launch(false, x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off, stream);
}

extern "C" int mk_spec_mix_dgrad(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch, int cin, int cout,
                                 int l_off, int m_off, void* stream) {
    if (int e = spec_mix_check(gy, w, gx, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    return spec_mix_launch(true, gy, w, gx, lloc, mloc, batch, cout, cin, l_off, m_off, stream);
}

extern "C" int mk_spec_mix_wgrad(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch, int cin, int cout,
                                 int l_off, int m_off, void* stream) {
    if (int e = spec_mix_check(x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    MixParams p{gy, x, gw, lloc, mloc, batch, cout, cin, l_off, m_off, mk::ceil_div(cout, XM), mk::ceil_div(cin, XN), 1, 0};
    // about three workgroups per CU: a workgroup contracts G consecutive degrees into its tile before the atomic epilogue
    long long G = (long long)lloc * p.tiles_m * p.tiles_n / 768;
    p.G = (int)(G < 1 ? 1 : (G > 8 ? 8 : G));
    p.ngroups = mk::ceil_div(lloc, p.G);
    return x3_launch(__func__, spec_mix_wgrad_x3_kernel, grid_blocks(p.ngroups, p.tiles_m, p.tiles_n), stream, p);
}

static int spec_cmlp_check(const void* a, const void* b, const void* c, int lloc, int mloc, int batch, int cin, int cout, int l_off,
                           int m_off, int per_degree, int act) {
    if (int e = spec_mix_check(a, b, c, lloc, mloc, batch, cin, cout, l_off, m_off)) return e;
    MK_REQUIRE(per_degree == 0 || per_degree == 1, "per_degree must be 0 (one shared weight panel) or 1");
    MK_REQUIRE((long long)cin * cout * 8 < (1LL << 31), "one weight panel must stay below 2^31 bytes");
    MK_REQUIRE(act >= 0 && act <= 2, "unknown activation (0 none | 1 real | 2 cartesian)");
    return 0;
}

extern "C" int mk_spec_cmlp_fwd(const float* x, const float* w, const float* bias, float* y, int lloc, int mloc, int batch, int cin,
                                int cout, int l_off, int m_off, int per_degree, int act, void* stream) {
    if (int e = spec_cmlp_check(x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off, per_degree, act)) return e;
    MK_REQUIRE(mk::aligned<8>(bias), "the bias must be 8-byte aligned");
    PanelParams p = panel_params(x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off, mloc * batch, cout, per_degree);
    p.bias = bias;
    p.act = act;
    return x3_launch(__func__, dhconv_fwd_x3_kernel<CplxBiasReluEpi, false>, grid_blocks(lloc, p.tiles_m, p.tiles_n), stream, p);
}

extern "C" int mk_spec_cmlp_dgrad(const float* gy, const float* w, const float* a, float* gx, int lloc, int mloc, int batch, int cin,
                                  int cout, int l_off, int m_off, int per_degree, int act, void* stream) {
    if (int e = spec_cmlp_check(gy, w, gx, lloc, mloc, batch, cin, cout, l_off, m_off, per_degree, act)) return e;
    MK_REQUIRE(mk::aligned<16>(a), "operands must be 16-byte aligned");
    MK_REQUIRE(a == nullptr || act != 0, "a mask operand needs an activation mode (1 real | 2 cartesian)");
    PanelParams p = panel_params(gy, w, gx, lloc, mloc, batch, cin, cout, l_off, m_off, mloc * batch, cin, per_degree);
    p.aux = a;
    p.act = act;
    return x3_launch(__func__, a ? dhconv_dgrad_x3_kernel<CplxMaskEpi, false> : dhconv_dgrad_x3_kernel<PanelStoreEpi, false>,
                     grid_blocks(lloc, p.tiles_m, p.tiles_n), stream, p);
}

extern "C" long long mk_spec_cmlp_wgrad_workspace(int lloc, int cin, int cout, int per_degree) {
    if (per_degree || lloc <= 0 || cin <= 0 || cout <= 0) return 0;
    const int ngroups = mk::ceil_div(lloc, cmlp_group_size(lloc, cin, cout));
    return ngroups > 1 ? (long long)ngroups * cin * cout * 8 : 0;
}

extern "C" int mk_spec_cmlp_wgrad(const float* x, const float* gy, float* gw, void* workspace, int lloc, int mloc, int batch, int cin,
                                  int cout, int l_off, int m_off, int per_degree, void* stream) {
    if (int e = spec_cmlp_check(x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off, per_degree, 0)) return e;
    if (per_degree) return mk_dhconv_wgrad_x3(x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off, stream);
    PanelParams p = panel_params(x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off, cin, cout, false);
    p.G = cmlp_group_size(lloc, cin, cout);
    p.ngroups = mk::ceil_div(lloc, p.G);
    if (p.ngroups > 1) {
        MK_REQUIRE(workspace && mk::aligned<16>(workspace), "the shared weight gradient needs its 16-byte aligned workspace");
        p.dst = static_cast<float*>(workspace);
    }
    if (int e = x3_launch(__func__, spec_cmlp_wgrad_shared_kernel, grid_blocks(p.ngroups, p.tiles_m, p.tiles_n), stream, p)) return e;
    if (p.ngroups > 1) {
        const long long n4 = (long long)cin * cout / 2;      // cin, cout even: a whole number of float4
        hipLaunchKernelGGL(spec_cmlp_group_sum_kernel, dim3((unsigned)mk::ceil_div_ll(n4, 256LL)), dim3(256), 0, (hipStream_t)stream,
                           static_cast<const float4*>(workspace), reinterpret_cast<float4*>(gw), n4, p.ngroups);
        MK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" long long mk_spec_cmlp_bgrad_workspace(int lloc, int cout) {
    return lloc > 0 && cout > 0 ? (long long)lloc * cout * 2 * 8 : 0;
}

extern "C" int mk_spec_cmlp_bgrad(const float* g, float* gb, void* workspace, int lloc, int mloc, int batch, int cout, int l_off,
                                  int m_off, void* stream) {
    if (int e = spec_mix_check(g, gb, workspace, lloc, mloc, batch, cout, cout, l_off, m_off)) return e;
    const int O2 = 2 * cout, chunks = mk::ceil_div(O2, 256);
    MK_REQUIRE((long long)lloc * chunks < 2147483647LL, "grid too large");
    hipLaunchKernelGGL(spec_cmlp_bgrad_rows_kernel, dim3((unsigned)(lloc * chunks)), dim3(256), 0, (hipStream_t)stream, g,
                       static_cast<double*>(workspace), mloc, batch, O2, l_off, m_off, chunks);
    MK_LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_cmlp_bgrad_sum_kernel, dim3((unsigned)mk::ceil_div(O2, 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const double*>(workspace), gb, lloc, O2);
    MK_LAUNCH_CHECK();
    return 0;
}

static int spec_bdmlp_check(const void* a, const void* b, const void* c, int rows, int nb, int ib, int ob) {
    MK_REQUIRE(a && b && c, "null pointer");
    MK_REQUIRE(rows > 0 && nb > 0 && ib > 0 && ob > 0, "bad sizes");
    MK_REQUIRE(ib % 2 == 0 && ob % 2 == 0, "the block MLP needs even block sizes (block offsets must stay 16-byte aligned)");
    MK_REQUIRE(mk::aligned<16>(a, b, c), "operands must be 16-byte aligned");
    const long long cmax = (long long)nb * (ib > ob ? ib : ob);
    // the stagers' 32-bit byte offsets span one row tile of a field (129 rows) and one block's weight panel
    MK_REQUIRE(129LL * cmax * 8 < (1LL << 31) && (long long)ib * ob * 8 < (1LL << 31),
               "one row tile of the spectrum and one weight panel must stay below 2^31 bytes");
    return 0;
}

static BlockParams bdmlp_params(const float* a, const float* b, float* dst, int rows, int nb, int ib, int ob, int rows_m, int cols) {
    return BlockParams{a, b, dst, nullptr, rows, nb, ib, ob, mk::ceil_div(rows_m, XM), mk::ceil_div(2 * cols, XN), 0.f, 0, 1};
}

extern "C" int mk_spec_bdmlp_fwd(const float* x, const float* w, float* y, int rows, int nb, int ib, int ob, int act, float lambda,
                                 void* stream) {
    if (int e = spec_bdmlp_check(x, w, y, rows, nb, ib, ob)) return e;
    MK_REQUIRE(act == 0 || act == 2 || act == 3, "unknown activation (0 none | 2 cartesian ReLU | 3 soft-shrink)");
    MK_REQUIRE(act != 3 || lambda >= 0.f, "the soft-shrink threshold must not be negative");
    BlockParams p = bdmlp_params(x, w, y, rows, nb, ib, ob, rows, ob);
    p.lambda = lambda;
    const long long nblk = grid_blocks(nb, p.tiles_m, p.tiles_n);
    if (act == 2) return x3_launch(__func__, spec_bdmlp_fwd_kernel<BD_RELU>, nblk, stream, p);
    if (act == 3) return x3_launch(__func__, spec_bdmlp_fwd_kernel<BD_SHRINK>, nblk, stream, p);
    return x3_launch(__func__, spec_bdmlp_fwd_kernel<BD_STORE>, nblk, stream, p);
}

extern "C" int mk_spec_bdmlp_fwd_bias(const float* x, const float* w, const float* bias, float* y, int rows, int nb, int ib, int ob,
                                      int act, float lambda, void* stream) {
    if (!bias) return mk_spec_bdmlp_fwd(x, w, y, rows, nb, ib, ob, act, lambda, stream);
    if (int e = spec_bdmlp_check(x, w, y, rows, nb, ib, ob)) return e;
    MK_REQUIRE(mk::aligned<8>(bias), "the complex bias must be 8-byte aligned");
    MK_REQUIRE(act == 0 || act == 2 || act == 3, "unknown activation (0 none | 2 cartesian ReLU | 3 soft-shrink)");
    MK_REQUIRE(act != 3 || lambda >= 0.f, "the soft-shrink threshold must not be negative");
    BlockParams p = bdmlp_params(x, w, y, rows, nb, ib, ob, rows, ob);
    p.lambda = lambda;
    p.bias = bias;
    const long long nblk = grid_blocks(nb, p.tiles_m, p.tiles_n);
    if (act == 2) return x3_launch(__func__, spec_bdmlp_fwd_kernel<BD_BIAS + BD_RELU>, nblk, stream, p);
    if (act == 3) return x3_launch(__func__, spec_bdmlp_fwd_kernel<BD_BIAS + BD_SHRINK>, nblk, stream, p);
    return x3_launch(__func__, spec_bdmlp_fwd_kernel<BD_BIAS + BD_STORE>, nblk, stream, p);
}

extern "C" int mk_spec_bdmlp_dgrad(const float* gy, const float* w, const float* a, float* gx, int rows, int nb, int ib, int ob,
                                   int act, void* stream) {
    if (int e = spec_bdmlp_check(gy, w, gx, rows, nb, ib, ob)) return e;
    MK_REQUIRE(mk::aligned<16>(a), "operands must be 16-byte aligned");
    MK_REQUIRE(act == 0 || act == 2, "unknown mask mode (0 none | 2 cartesian ReLU)");
    MK_REQUIRE((a != nullptr) == (act == 2), "the mask operand and the mask mode go together");
    BlockParams p = bdmlp_params(gy, w, gx, rows, nb, ib, ob, rows, ib);
    p.aux = a;
    return x3_launch(__func__, a ? spec_bdmlp_dgrad_kernel<BD_MASK> : spec_bdmlp_dgrad_kernel<BD_STORE>,
                     grid_blocks(nb, p.tiles_m, p.tiles_n), stream, p);
}

extern "C" long long mk_spec_bdmlp_wgrad_workspace(int rows, int nb, int ib, int ob) {
    if (rows <= 0 || nb <= 0 || ib <= 0 || ob <= 0) return 0;
    const int ngroups = mk::ceil_div(rows, bdmlp_group_rows(rows, nb, ib, ob));
    return ngroups > 1 ? (long long)ngroups * nb * ib * ob * 8 : 0;
}

extern "C" int mk_spec_bdmlp_wgrad(const float* x, const float* gy, float* gw, void* workspace, int rows, int nb, int ib, int ob,
                                   void* stream) {
    if (int e = spec_bdmlp_check(x, gy, gw, rows, nb, ib, ob)) return e;
    BlockParams p = bdmlp_params(x, gy, gw, rows, nb, ib, ob, ib, ob);
    p.rg = bdmlp_group_rows(rows, nb, ib, ob);
    p.ngroups = mk::ceil_div(rows, p.rg);
    const long long cmax = (long long)nb * (ib > ob ? ib : ob);
    MK_REQUIRE((p.rg + 16LL) * cmax * 8 < (1LL << 31), "one row group of the spectrum must stay below 2^31 bytes");
    MK_REQUIRE((long long)nb * p.ngroups < 2147483647LL, "too many row groups");
    if (p.ngroups > 1) {
        MK_REQUIRE(workspace && mk::aligned<16>(workspace), "the block weight gradient needs its 16-byte aligned workspace");
        p.dst = static_cast<float*>(workspace);
    }
    if (int e = x3_launch(__func__, spec_bdmlp_wgrad_kernel, grid_blocks(nb * p.ngroups, p.tiles_m, p.tiles_n), stream, p)) return e;
    if (p.ngroups > 1) {
        const long long n4 = (long long)nb * ib * ob / 2;      // ib, ob even: a whole number of float4
        hipLaunchKernelGGL(spec_cmlp_group_sum_kernel, dim3((unsigned)mk::ceil_div_ll(n4, 256LL)), dim3(256), 0, (hipStream_t)stream,
                           static_cast<const float4*>(workspace), reinterpret_cast<float4*>(gw), n4, p.ngroups);
        MK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mk_spec_bdmlp_mask(const float* gy, const float* s, float* out, long long n, void* stream) {
    MK_REQUIRE(gy && s && out, "null pointer");
    MK_REQUIRE(n > 0 && n % 4 == 0, "the element count must be a positive multiple of 4 floats");
    MK_REQUIRE(mk::aligned<16>(gy, s, out), "operands must be 16-byte aligned");
    const long long nblk = mk::ceil_div_ll(n / 4, 256LL);
    MK_REQUIRE(nblk < 2147483647LL, "grid too large");
    hipLaunchKernelGGL(spec_bdmlp_mask_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(gy), reinterpret_cast<const float4*>(s), reinterpret_cast<float4*>(out), n / 4);
    MK_LAUNCH_CHECK();
    return 0;
}
