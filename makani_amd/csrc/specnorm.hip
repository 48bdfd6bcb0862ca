// Per-degree power of a packed spectrum and its gradient: what the H1 loss (makani/utils/losses.py:306-318) needs from the
// spherical-harmonic coefficients of a field,
//   P[l][bc] = sum_m w(m_off + m) |c[l][m][bc]|^2,   w(0) = 1, w(m > 0) = 2,
// on the private layout c [L][M][BC] complex64 (channels contiguous) as the Legendre kernels write it.  The L2 norm is
// sum_l P, the H1 seminorm sum_l l (l + 1) P; both are [BC, L] arithmetic and stay with the caller.  The sums add up over
// m shards and concatenate over l shards, so a sharded run all-reduces them instead of gathering the fields.
//
// The Legendre kernels leave the rows with l_off + l < m_off + m unwritten (uninitialised memory): neither kernel ever
// loads from them.  The forward sums the stored triangle only, the backward writes exact zeros there.
//
// Forward (degree_power_kernel): the m range is cut into chunks of kChunk orders (a compile-time constant, counted from
// the first LOCAL order).  One thread per (l, chunk, bc): it walks its chunk's stored orders in ascending m, converts re
// and im to double (the squares are exact), and writes one double to the workspace [L][nchunk][BC].  Lanes run along bc
// and on into the next (l, chunk) row, so a wave is full whatever BC is, and each lane's loads are 8-byte float2 that are
// contiguous across the lanes of a row.  The finalize kernel adds the chunks of (l, bc) in ascending order.  No atomics:
// the order of every addition depends on (M, l_off + l - m_off) only -- not on the launch geometry, and rows of an l
// slice give the bits of the same rows of the whole.
//
// Backward (degree_power_bwd_kernel): gc = 2 w gP[l][bc] c, the product formed in double and rounded once to fp32; one
// thread per complex element, an 8-byte load and an 8-byte store, the gradient in torch's convention (d/d re + i d/d im).
#include "common.h"
#include "../../include/makani_amd.h"

#include <cstdint>

namespace {

constexpr int kT = 256;        // threads per workgroup (4 waves)
constexpr int kChunk = 32;     // orders per forward partial
constexpr int kUnroll = 8;     // independent loads in flight per lane

// number of stored local orders of local degree l: those with m_off + m <= l_off + l, at most M
__device__ __forceinline__ int stored_orders(int l, int M, int l_off, int m_off) {
    const long long last = (long long)l_off + l - m_off;        // last stored local order (may be negative)
    return last < 0 ? 0 : (last + 1 < M ? (int)(last + 1) : M);
}

// part [L][nchunk][BC]
__global__ __launch_bounds__(kT) void degree_power_kernel(const float2* __restrict__ c, double* __restrict__ part, int L, int M,
                                                          int BC, int l_off, int m_off, int nchunk) {
    const long long g = (long long)blockIdx.x * kT + threadIdx.x;
    const long long row = g / BC;                                // (l, chunk)
    if (row >= (long long)L * nchunk) return;
    const int bc = (int)(g - row * BC);
    const int l = (int)(row / nchunk), k = (int)(row - (long long)l * nchunk);
    const int m0 = k * kChunk;
    const int m1 = min(m0 + kChunk, stored_orders(l, M, l_off, m_off));
    const float2* p = c + ((long long)l * M + m0) * BC + bc;
    double acc = 0.0;
    int m = m0;
    for (; m + kUnroll <= m1; m += kUnroll) {
        float2 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = p[(long long)u * BC];
        p += (long long)kUnroll * BC;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const double re = (double)v[u].x, im = (double)v[u].y;
            const double s = re * re + im * im;
            acc += (m_off + m + u == 0) ? s : 2.0 * s;
        }
    }
    for (; m < m1; ++m) {
        const float2 v = *p;
        p += BC;
        const double re = (double)v.x, im = (double)v.y;
        const double s = re * re + im * im;
        acc += (m_off + m == 0) ? s : 2.0 * s;
    }
    part[g] = acc;                                               // g = (l * nchunk + k) * BC + bc
}

// P [L][BC] = the chunks of part [L][nchunk][BC] added in ascending order
__global__ __launch_bounds__(kT) void degree_power_finalize(const double* __restrict__ part, double* __restrict__ P, long long n,
                                                            int BC, int nchunk) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;        // l * BC + bc
    if (i >= n) return;
    const long long l = i / BC;
    const double* p = part + l * nchunk * BC + (i - l * BC);
    double v = 0.0;
    for (int k = 0; k < nchunk; ++k) v += p[(long long)k * BC];
    P[i] = v;
}

__global__ __launch_bounds__(kT) void degree_power_bwd_kernel(const float2* __restrict__ c, const double* __restrict__ gP,
                                                              float2* __restrict__ gc, long long n, int M, int BC, int l_off,
                                                              int m_off) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;        // (l * M + m) * BC + bc
    if (i >= n) return;
    const long long lm = i / BC;
    const int bc = (int)(i - lm * BC);
    const int l = (int)(lm / M), m = (int)(lm - (long long)l * M);
    float2 out = make_float2(0.f, 0.f);
    if ((long long)l_off + l >= (long long)m_off + m) {
        const float2 v = c[i];
        const double k = (m_off + m == 0 ? 2.0 : 4.0) * gP[(long long)l * BC + bc];
        out = make_float2((float)(k * (double)v.x), (float)(k * (double)v.y));
    }
    gc[i] = out;
}

bool sizes_ok(int L, int M, int BC, int l_off, int m_off) {
    return L >= 1 && M >= 1 && BC >= 1 && l_off >= 0 && m_off >= 0 && (long long)l_off + L < (1LL << 30) &&
           (long long)m_off + M < (1LL << 30) && (long long)L * M * BC < (1LL << 38);
}

}  // namespace

extern "C" long long mk_degree_power_workspace(int L, int M, int BC) {
    if (L < 1 || M < 1 || BC < 1) return 0;
    return (long long)L * mk::ceil_div(M, kChunk) * BC;
}

extern "C" int mk_degree_power(const float* c, double* workspace, double* P, int L, int M, int BC, int l_off, int m_off,
                               void* stream) {
    MK_REQUIRE(c && workspace && P, "null pointer");
    MK_REQUIRE(sizes_ok(L, M, BC, l_off, m_off), "bad sizes");
    MK_REQUIRE(mk::aligned<8>(c, workspace, P), "buffer not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = mk::ceil_div(M, kChunk);
    const long long nparts = (long long)L * nchunk * BC;
    hipLaunchKernelGGL(degree_power_kernel, dim3((unsigned)mk::ceil_div_ll(nparts, kT)), dim3(kT), 0, st, (const float2*)c,
                       workspace, L, M, BC, l_off, m_off, nchunk);
    MK_LAUNCH_CHECK();
    const long long n = (long long)L * BC;
    hipLaunchKernelGGL(degree_power_finalize, dim3((unsigned)mk::ceil_div_ll(n, kT)), dim3(kT), 0, st, workspace, P, n, BC,
                       nchunk);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_degree_power_bwd(const float* c, const double* gP, float* gc, int L, int M, int BC, int l_off, int m_off,
                                   void* stream) {
    MK_REQUIRE(c && gP && gc, "null pointer");
    MK_REQUIRE(sizes_ok(L, M, BC, l_off, m_off), "bad sizes");
    MK_REQUIRE(mk::aligned<8>(c, gP, gc), "buffer not 8-byte aligned");
    const long long n = (long long)L * M * BC;
    hipLaunchKernelGGL(degree_power_bwd_kernel, dim3((unsigned)mk::ceil_div_ll(n, kT)), dim3(kT), 0, (hipStream_t)stream,
                       (const float2*)c, gP, (float2*)gc, n, M, BC, l_off, m_off);
    MK_LAUNCH_CHECK();
    return 0;
}
