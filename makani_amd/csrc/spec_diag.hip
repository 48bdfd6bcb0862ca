// "diagonal" spectral filter on the private spectrum: a separate complex weight for every (l, m),
//     y[l][m][b][o]  = sum_i x[l][m][b][i] * w[i][o][l][m]
//     gx[l][m][b][i] = sum_o gy[l][m][b][o] * conj(w[i][o][l][m])
//     gw[i][o][l][m] = sum_b conj(x[l][m][b][i]) * gy[l][m][b][o]
// x / y / gx / gy: private spectrum [lloc][mloc][batch * chan] complex64, channel contiguous (the layout of mk_dhconv_*);
// w / gw: the parameter as stored, [cin][cout][lloc][mloc] complex64.  Replaces _contract_diagonal
// `einsum("bixy,ioxy->boxy")` (makani/models/common/contractions.py:121-127) and its two gradients without the layout
// round trip of csrc/diag.hip.
//
// One flop per weight byte: HBM bound on the weights.  A workgroup owns a run of `tp` consecutive m of one degree l.  In the
// private layout the spectrum rows of that run are one contiguous block: it goes through LDS once, so that a lane can own
// a position (VEC = 2: two neighbouring ones, one 16-byte access) while the weight rows stream coalesced along m.  Lanes
// sharing a position group split the output channels (the (i, o) pairs for the weight gradient).  Every accumulator is one
// sequential fp32 fma chain in registers, in the order of mk_diag_*; results return through LDS so that the spectrum is stored in
// whole rows.  Every output element has one writer: no atomics, no workspace, the same bits every run and for every cut into shards.
//
// dense = 0 (the spherical pair): positions with global l < m hold no data.  They are never read (the input spectrum's triangle is
// unwritten memory), y / gx are not written there, gw there is an exact zero stored by the weight-gradient kernel itself.  The
// valid positions of a row are a prefix, so runs beyond it return at once and the weight lines there are never requested.
#include <cstdint>

#include "common.h"
#include "../../include/makani_amd.h"

namespace {

constexpr int ST = 256;            // threads
constexpr int SB = 4;              // batch items per pass over the weights (register blocking of forward / dgrad), and per LDS stage
constexpr int STP = 32;            // positions of a run, at most
constexpr int SU = 4;              // contracted channels whose weights a lane has in flight while it uses the SU before them
constexpr int SLDS = 40 * 1024;    // dynamic LDS of a workgroup, at most: four workgroups share a compute unit's 160 KB

struct SdParams {
    const float2* a;     // x (forward, wgrad) or gy (dgrad)
    const float2* b;     // w (forward, dgrad) or gy (wgrad)
    float2* out;
    int lloc, mloc, batch, cin, cout, l_off, m_off, dense;
    int tp, bs, tiles_m;
};

__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 c) {   // c + a * b
    c.x = fmaf(a.x, b.x, c.x);
    c.x = fmaf(-a.y, b.y, c.x);
    c.y = fmaf(a.x, b.y, c.y);
    c.y = fmaf(a.y, b.x, c.y);
    return c;
}
__device__ __forceinline__ float2 cfma_conj_b(float2 a, float2 b, float2 c) {   // c + a * conj(b)
    c.x = fmaf(a.x, b.x, c.x);
    c.x = fmaf(a.y, b.y, c.x);
    c.y = fmaf(a.y, b.x, c.y);
    c.y = fmaf(-a.x, b.y, c.y);
    return c;
}

// number of leading m of local row l that hold data
__device__ __forceinline__ int valid_m(const SdParams& p, int l) {
    if (p.dense) return p.mloc;
    const long long n = (long long)p.l_off + l - p.m_off + 1;
    return n < 0 ? 0 : (n > p.mloc ? p.mloc : (int)n);
}

template <int VEC> __device__ __forceinline__ void load_w(const float2* q, float2 (&v)[VEC]) {
    if constexpr (VEC == 2) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = make_float2(t.x, t.y);
        v[1] = make_float2(t.z, t.w);
    } else {
        v[0] = *q;
    }
}
template <int VEC> __device__ __forceinline__ void store_w(float2* q, const float2 (&v)[VEC]) {
    if constexpr (VEC == 2) {
        *reinterpret_cast<float4*>(q) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    } else {
        *q = v[0];
    }
}

// one lane's share of a staged batch chunk: output channels d = dg, dg + ndg, ... of its VEC positions.  FULL: the chunk holds
// BS batch items; otherwise bs < BS of them (the ragged last chunk) and the others are skipped.
template <bool CONJ, int VEC, int BS, bool FULL>
__device__ __forceinline__ void apply_chunk(const float2* __restrict__ w, const float2* xs, float2* ys, int sx, int sy, int ns, int nd,
                                            int pos0, int dg, int ndg, long long wsr, long long wsd, int bs) {
    for (int d = dg; d < nd; d += ndg) {
        float2 acc[BS][VEC];
#pragma unroll
        for (int bb = 0; bb < BS; ++bb)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[bb][v] = make_float2(0.f, 0.f);
        const float2* wp = w + d * wsd;
        // The weights of U contracted channels are in flight while the U before them are used: two register groups, ping-pong.
        // The chain itself stays sequential in r: the same bits as a plain loop.
        constexpr int U = SU;
        const int nfull = ns / U;
        float2 wa[U][VEC], wb[U][VEC];
        auto load = [&](float2 (&g)[U][VEC], int grp) {
#pragma unroll
            for (int u = 0; u < U; ++u) load_w<VEC>(wp + (long long)(grp * U + u) * wsr, g[u]);
        };
        auto use1 = [&](const float2 (&wv)[VEC], int r) {
#pragma unroll
            for (int bb = 0; bb < BS; ++bb) {
                if (!FULL && bb >= bs) break;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float2 xv = xs[(pos0 + v) * sx + bb * ns + r];
                    acc[bb][v] = CONJ ? cfma_conj_b(xv, wv[v], acc[bb][v]) : cfma(xv, wv[v], acc[bb][v]);
                }
            }
        };
        auto use = [&](const float2 (&g)[U][VEC], int grp) {
#pragma unroll
            for (int u = 0; u < U; ++u) use1(g[u], grp * U + u);
        };
        if (nfull > 0) load(wa, 0);
        int grp = 0;
        for (; grp + 1 < nfull; grp += 2) {
            load(wb, grp + 1);
            use(wa, grp);
            if (grp + 2 < nfull) load(wa, grp + 2);
            use(wb, grp + 1);
        }
        if (grp < nfull) use(wa, grp);
        for (int r = nfull * U; r < ns; ++r) {
            float2 wv[VEC];
            load_w<VEC>(wp + r * wsr, wv);
            use1(wv, r);
        }
#pragma unroll
        for (int bb = 0; bb < BS; ++bb) {
            if (!FULL && bb >= bs) break;
#pragma unroll
            for (int v = 0; v < VEC; ++v) ys[(pos0 + v) * sy + bb * nd + d] = acc[bb][v];
        }
    }
}

// CONJ = false: forward (a = x, contraction over i);  CONJ = true: data gradient (a = gy, contraction over o).  BS = p.bs, the
// batch items of an LDS stage and of one pass over the weights: a kernel of its own each, so that each has its own registers.
template <bool CONJ, int VEC, int BS>
__global__ __launch_bounds__(ST) void spec_diag_apply_kernel(SdParams p) {
    extern __shared__ float2 sd_lds[];
    const int l = blockIdx.x / p.tiles_m, m0 = (blockIdx.x % p.tiles_m) * p.tp;
    const int mv = valid_m(p, l);
    if (m0 >= mv) return;
    const int np = min(p.tp, mv - m0);                      // positions of this run that hold data (a prefix)
    const int ns = CONJ ? p.cout : p.cin, nd = CONJ ? p.cin : p.cout;
    const int pl = p.tp / VEC, lane = threadIdx.x % pl, dg = threadIdx.x / pl, ndg = ST / pl;
    const int pos0 = lane * VEC;
    const long long lm = (long long)p.lloc * p.mloc;
    const long long wsr = CONJ ? lm : (long long)p.cout * lm;      // weight stride of the contracted channel
    const long long wsd = CONJ ? (long long)p.cout * lm : lm;      // and of the output channel
    const float2* w = p.b + (long long)l * p.mloc + m0 + pos0;
    const long long row0 = (long long)l * p.mloc + m0;
    // odd row strides (in complex words): the lanes of a position group read different LDS banks
    float2* xs = sd_lds;
    float2* ys = sd_lds + (long long)p.tp * ((p.bs * ns) | 1);
    for (int b0 = 0; b0 < p.batch; b0 += p.bs) {
        const int bs = min(p.bs, p.batch - b0);
        const int sx = (bs * ns) | 1, sy = (bs * nd) | 1;
        const int nx = bs * ns, ny = bs * nd;
        __syncthreads();                                    // the previous chunk's rows have left ys
        for (int idx = threadIdx.x; idx < np * nx; idx += ST) {
            const int q = idx / nx, rem = idx - q * nx;
            xs[q * sx + rem] = p.a[((row0 + q) * p.batch + b0) * ns + rem];
        }
        __syncthreads();
        if (pos0 < np) {
            if (bs == BS)
                apply_chunk<CONJ, VEC, BS, true>(w, xs, ys, sx, sy, ns, nd, pos0, dg, ndg, wsr, wsd, bs);
            else
                apply_chunk<CONJ, VEC, BS, false>(w, xs, ys, sx, sy, ns, nd, pos0, dg, ndg, wsr, wsd, bs);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < np * ny; idx += ST) {
            const int q = idx / ny, rem = idx - q * ny;
            p.out[((row0 + q) * p.batch + b0) * nd + rem] = ys[q * sy + rem];
        }
    }
}

// a = x, b = gy, out = gw.  A lane owns VEC positions and the (i, o) pairs dg, dg + ndg, ...; a batch beyond one LDS stage
// continues the same fma chain from the value the lane itself stored for the stage before.
template <int VEC>
__global__ __launch_bounds__(ST) void spec_diag_wgrad_kernel(SdParams p) {
    extern __shared__ float2 sd_lds[];
    const int l = blockIdx.x / p.tiles_m, m0 = (blockIdx.x % p.tiles_m) * p.tp;
    const int mv = valid_m(p, l);
    const int np = max(0, min(p.tp, mv - m0));
    const int pl = p.tp / VEC, lane = threadIdx.x % pl, dg = threadIdx.x / pl, ndg = ST / pl;
    const int pos0 = lane * VEC;
    const bool in_row = m0 + pos0 < p.mloc;                 // VEC = 2 only with even mloc: both positions or none
    const long long lm = (long long)p.lloc * p.mloc;
    const int npairs = p.cin * p.cout;
    float2* gw = p.out + (long long)l * p.mloc + m0 + pos0;
    if (np == 0) {                                          // a run in the triangle: exact zeros, nothing read
        if (in_row) {
            float2 z[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) z[v] = make_float2(0.f, 0.f);
            for (int pr = dg; pr < npairs; pr += ndg) store_w<VEC>(gw + pr * lm, z);
        }
        return;
    }
    const long long row0 = (long long)l * p.mloc + m0;
    float2* xs = sd_lds;
    float2* gs = sd_lds + (long long)p.tp * ((p.bs * p.cin) | 1);
    for (int b0 = 0; b0 < p.batch; b0 += p.bs) {
        const int bs = min(p.bs, p.batch - b0);
        const int nx = bs * p.cin, ng = bs * p.cout;
        const int sx = nx | 1, sg = ng | 1;
        __syncthreads();
        for (int idx = threadIdx.x; idx < np * nx; idx += ST) {
            const int q = idx / nx, rem = idx - q * nx;
            xs[q * sx + rem] = p.a[((row0 + q) * p.batch + b0) * p.cin + rem];
        }
        for (int idx = threadIdx.x; idx < np * ng; idx += ST) {
            const int q = idx / ng, rem = idx - q * ng;
            gs[q * sg + rem] = p.b[((row0 + q) * p.batch + b0) * p.cout + rem];
        }
        __syncthreads();
        if (!in_row) continue;
        for (int pr = dg; pr < npairs; pr += ndg) {
            const int i = pr / p.cout, o = pr - i * p.cout;
            float2 acc[VEC];
            if (b0 == 0) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = make_float2(0.f, 0.f);
            } else {
                load_w<VEC>(gw + pr * lm, acc);
            }
            for (int bb = 0; bb < bs; ++bb)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc[v] = cfma_conj_b(gs[(pos0 + v) * sg + bb * p.cout + o], xs[(pos0 + v) * sx + bb * p.cin + i], acc[v]);
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                if (pos0 + v >= np) acc[v] = make_float2(0.f, 0.f);         // in the row, not in the triangle's data
            store_w<VEC>(gw + pr * lm, acc);
        }
    }
}

size_t lds_bytes(int tp, int bs, int n0, int n1) {
    return (size_t)tp * ((size_t)((bs * n0) | 1) + (size_t)((bs * n1) | 1)) * sizeof(float2);
}

// Checks the arguments and chooses the tile: VEC (16-byte weight accesses where every weight row starts on 16 bytes), the run
// length tp and the batch stage bs, shrunk until the two LDS blocks fit.
int sd_setup(const char* who, SdParams& p, int& vec, size_t& lds, const void* a, const void* b, const void* out, const void* w,
             int lloc, int mloc, int batch, int cin, int cout, int l_off, int m_off, int dense) {
    MK_REQUIRE_AS(who, a && b && out, "null pointer");
    MK_REQUIRE_AS(who, mk::aligned<8>(a, b, out), "operands must be 8-byte aligned");
    MK_REQUIRE_AS(who, lloc > 0 && mloc > 0 && batch > 0 && cin > 0 && cout > 0, "bad sizes");
    MK_REQUIRE_AS(who, l_off >= 0 && m_off >= 0 && (dense == 0 || dense == 1), "bad offsets / dense flag");
    MK_REQUIRE_AS(who, (long long)l_off + lloc < 2147483647LL && (long long)m_off + mloc < 2147483647LL,
                  "global degree / order beyond the int range");
    // the two LDS rows of one position and one batch item bound the channel counts (and keep cin * cout, batch * chan in int)
    MK_REQUIRE_AS(who, (long long)cin + cout <= 2500, "cin + cout beyond what the LDS rows of two positions hold (2500)");
    MK_REQUIRE_AS(who, batch <= 65536, "batch beyond the index range (65536)");
    vec = (mloc % 2 == 0 && mk::aligned<16>(w)) ? 2 : 1;
    int tp = STP, bs = batch < SB ? batch : SB;
    while (tp > vec && tp / 2 >= mloc) tp /= 2;
    while (tp > 8 && tp > vec && lds_bytes(tp, bs, cin, cout) > SLDS) tp /= 2;
    while (bs > 1 && lds_bytes(tp, bs, cin, cout) > SLDS) bs = (bs + 1) / 2;
    while (tp > vec && lds_bytes(tp, bs, cin, cout) > SLDS) tp /= 2;
    lds = lds_bytes(tp, bs, cin, cout);
    MK_REQUIRE_AS(who, lds <= SLDS, "tile does not fit LDS");
    const int tiles_m = mk::ceil_div(mloc, tp);
    MK_REQUIRE_AS(who, (long long)tiles_m * lloc < 2147483647LL, "grid too large");
    p = SdParams{(const float2*)a, (const float2*)b, (float2*)out, lloc, mloc, batch, cin, cout, l_off, m_off, dense, tp, bs, tiles_m};
    return 0;
}

template <bool CONJ> int launch_apply(const char* who, const SdParams& p, int vec, size_t lds, void* stream) {
    const dim3 grid((unsigned)(p.tiles_m * p.lloc));
#define MK_SD_CASE(V, B)                                                                                                      \
    case (V) * 8 + (B):                                                                                                       \
        hipLaunchKernelGGL((spec_diag_apply_kernel<CONJ, V, B>), grid, dim3(ST), lds, (hipStream_t)stream, p);               \
        break;
    switch (vec * 8 + p.bs) {
        MK_SD_CASE(1, 1) MK_SD_CASE(1, 2) MK_SD_CASE(1, 3) MK_SD_CASE(1, 4)
        MK_SD_CASE(2, 1) MK_SD_CASE(2, 2) MK_SD_CASE(2, 3) MK_SD_CASE(2, 4)
        default: MK_REQUIRE_AS(who, false, "no kernel for this tile");
    }
#undef MK_SD_CASE
    MK_LAUNCH_CHECK_AS(who);
    return 0;
}

}  // namespace

extern "C" int mk_spec_diag_fwd(const float* x, const float* w, float* y, int lloc, int mloc, int batch, int cin, int cout, int l_off,
                                int m_off, int dense, void* stream) {
    SdParams p;
    int vec;
    size_t lds;
    if (int e = sd_setup(__func__, p, vec, lds, x, w, y, w, lloc, mloc, batch, cin, cout, l_off, m_off, dense)) return e;
    return launch_apply<false>(__func__, p, vec, lds, stream);
}

extern "C" int mk_spec_diag_dgrad(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch, int cin, int cout,
                                  int l_off, int m_off, int dense, void* stream) {
    SdParams p;
    int vec;
    size_t lds;
    if (int e = sd_setup(__func__, p, vec, lds, gy, w, gx, w, lloc, mloc, batch, cin, cout, l_off, m_off, dense)) return e;
    return launch_apply<true>(__func__, p, vec, lds, stream);
}

extern "C" int mk_spec_diag_wgrad(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch, int cin, int cout,
                                  int l_off, int m_off, int dense, void* stream) {
    SdParams p;
    int vec;
    size_t lds;
    if (int e = sd_setup(__func__, p, vec, lds, x, gy, gw, gw, lloc, mloc, batch, cin, cout, l_off, m_off, dense)) return e;
    const dim3 grid((unsigned)(p.tiles_m * lloc));
    if (vec == 2)
        hipLaunchKernelGGL(spec_diag_wgrad_kernel<2>, grid, dim3(ST), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(spec_diag_wgrad_kernel<1>, grid, dim3(ST), lds, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK();
    return 0;
}
