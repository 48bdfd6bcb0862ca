// The spectral ensemble CRPS: per-degree sums of the CRPS terms of the spherical-harmonic coefficients of E ensemble members
// against a target, and their gradient with respect to the members.  Spectra are the private layout of the Legendre kernels,
//   cp [L][M][B E C] complex64, row (b E + e) C + c  (forward_packed of a prediction [B E, C, H, W], member fastest),
//   ct [L][M][B C]   complex64, row b C + c.
// For a stored coefficient (l_off + l >= m_off + m), every (b, c) and each component k in {re, im} taken as a real number
//   a_k = (1/E) sum_e |x_e - y|,   g_k = (1/E^2) sum_ef |x_e - x_f|,
//   S[l][bc][0] = sum_m w(m_off + m) (a_re + a_im),   S[l][bc][1] = sum_m w(m_off + m) (g_re + g_im),   w(0) = 1, w(m > 0) = 2.
// The rows with l_off + l < m_off + m (unwritten by the Legendre kernels) are never loaded; the gradient has exact zeros there.
//
// Forward (spec_crps_sums_kernel, the structure of degree_power_kernel in specnorm.hip): the m range is cut into chunks of kChunk
// orders counted from the first LOCAL order; one thread per (l, chunk, b, c) walks its stored orders in ascending m.  Lanes run
// along bc = b C + c and on into the next (l, chunk) row, so a wave is full whatever B C is; the E members and the target of a
// coefficient are 8-byte float2 loads, contiguous across the lanes of a channel run.  Per coefficient, in float64 (fp32 widens
// exactly): sum_e |x_e - y| in ascending e and sum_{e < f} |x_e - x_f| in lexicographic (e, f), per component, then re + im, then
// acc += w (.).  A thread writes its pair to the workspace [L][nchunk][BC][2]; the finalize adds the chunks of (l, bc) in ascending
// order and scales by 1 / E and 2 / E^2.  No atomics: the order of every addition depends on (M, l_off + l - m_off) only, so the
// rows of an l slice carry the bits of the same rows of the whole, and every run gives the same bits.  A NaN component in a
// member or the target makes both terms of that coefficient NaN.
//
// Backward (spec_crps_bwd_kernel): one thread per (l, m, b, c), the E members in registers; signs and the counts L_e, G_e of the
// members strictly below / above x_e by comparing ALL PAIRS in fp32 (exact; tied members get equal values, 0 - 0 = 0 for the
// zero imaginary parts of m = 0); per component
//   gcp = w (gS0 sgn(x_e - y) / E + gS1 2 (L_e - G_e) / E^2)
// formed in float64 and rounded once to fp32, E 8-byte stores, torch's complex convention (d/d re + i d/d im).  A NaN component
// in a member or the target makes both components of every member's gradient of that coefficient NaN (the rule of
// mk_ens_crps_bwd).  No workspace, no atomics.
#include "common.h"
#include "../../include/makani_amd.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)   // file scope: every product and sum is rounded on its own, as the header states them

namespace {

constexpr int kT = 256;        // threads per workgroup (4 waves)
constexpr int kChunk = 16;     // orders per forward partial
constexpr int kMaxE = 16;      // all pairs of a coefficient's members in registers

// number of stored local orders of local degree l: those with m_off + m <= l_off + l, at most M
__device__ __forceinline__ int stored_orders(int l, int M, int l_off, int m_off) {
    const long long last = (long long)l_off + l - m_off;        // last stored local order (may be negative)
    return last < 0 ? 0 : (last + 1 < M ? (int)(last + 1) : M);
}

__device__ __forceinline__ bool is_nan2(float2 v) { return v.x != v.x || v.y != v.y; }

// (sum_e |x_e - y|, sum_{e < f} |x_e - x_f|) of one coefficient, re and im added: float64, the order the file comment states
template <int E>
__device__ __forceinline__ void coeff_terms(const float2 (&x)[E], float2 y, double& a, double& g) {
    bool bad = is_nan2(y);
    double xr[E], xi[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        xr[e] = (double)x[e].x;
        xi[e] = (double)x[e].y;
        bad = bad || is_nan2(x[e]);
    }
    const double yr = (double)y.x, yi = (double)y.y;
    double are = 0.0, aim = 0.0, gre = 0.0, gim = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        are += fabs(xr[e] - yr);
        aim += fabs(xi[e] - yi);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int f = e + 1; f < E; ++f) {
            gre += fabs(xr[e] - xr[f]);
            gim += fabs(xi[e] - xi[f]);
        }
    }
    a = bad ? (double)NAN : are + aim;
    g = bad ? (double)NAN : gre + gim;      // a NaN target alone would leave g finite
}

// part [L][nchunk][BC][2]
template <int E>
__global__ __launch_bounds__(kT) void spec_crps_sums_kernel(const float2* __restrict__ cp, const float2* __restrict__ ct,
                                                            double* __restrict__ part, int L, int M, int C, int BC, int l_off,
                                                            int m_off, int nchunk) {
    const long long gi = (long long)blockIdx.x * kT + threadIdx.x;
    const long long row = gi / BC;                               // (l, chunk)
    if (row >= (long long)L * nchunk) return;
    const int bc = (int)(gi - row * BC);
    const int b = bc / C, c = bc - b * C;
    const int l = (int)(row / nchunk), k = (int)(row - (long long)l * nchunk);
    const int m0 = k * kChunk;
    const int m1 = min(m0 + kChunk, stored_orders(l, M, l_off, m_off));
    const long long BEC = (long long)BC * E;
    const float2* px = cp + ((long long)l * M + m0) * BEC + (long long)b * E * C + c;
    const float2* py = ct + ((long long)l * M + m0) * BC + bc;
    double acc0 = 0.0, acc1 = 0.0;
    constexpr int kU = E <= 4 ? 4 : E <= 8 ? 2 : 1;             // coefficients in flight per lane: (E + 1) 8-byte loads each
#pragma unroll kU
    for (int m = m0; m < m1; ++m) {
        float2 x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = px[(long long)e * C];
        const float2 y = *py;
        px += BEC;
        py += BC;
        double a, g;
        coeff_terms<E>(x, y, a, g);
        const double w = (m_off + m == 0) ? 1.0 : 2.0;
        acc0 += w * a;
        acc1 += w * g;
    }
    part[2 * gi] = acc0;                                         // gi = (l * nchunk + k) * BC + bc
    part[2 * gi + 1] = acc1;
}

// S [L][BC][2] = the chunks of part [L][nchunk][BC][2] added in ascending order, times (1 / E, 2 / E^2)
__global__ __launch_bounds__(kT) void spec_crps_finalize(const double* __restrict__ part, double* __restrict__ S, long long n,
                                                         int BC, int nchunk, double s0, double s1) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;        // l * BC + bc
    if (i >= n) return;
    const long long l = i / BC;
    const double* p = part + 2 * (l * nchunk * BC + (i - l * BC));
    double v0 = 0.0, v1 = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        v0 += p[2 * (long long)k * BC];
        v1 += p[2 * (long long)k * BC + 1];
    }
    S[2 * i] = v0 * s0;
    S[2 * i + 1] = v1 * s1;
}

template <int E>
__global__ __launch_bounds__(kT) void spec_crps_bwd_kernel(const float2* __restrict__ cp, const float2* __restrict__ ct,
                                                           const double* __restrict__ gS, float2* __restrict__ gcp, long long n,
                                                           int M, int C, int BC, int l_off, int m_off, double s0, double s1) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;        // (l * M + m) * BC + bc
    if (i >= n) return;
    const long long lm = i / BC;
    const int bc = (int)(i - lm * BC);
    const int b = bc / C, c = bc - b * C;
    const int l = (int)(lm / M), m = (int)(lm - (long long)l * M);
    const long long base = lm * ((long long)BC * E) + (long long)b * E * C + c;
    float2* out = gcp + base;
    if ((long long)l_off + l < (long long)m_off + m) {           // the unstored triangle: nothing is loaded, exact zeros
#pragma unroll
        for (int e = 0; e < E; ++e) out[(long long)e * C] = make_float2(0.f, 0.f);
        return;
    }
    float2 x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = cp[base + (long long)e * C];
    const float2 y = ct[i];
    const double gs0 = gS[2 * ((long long)l * BC + bc)], gs1 = gS[2 * ((long long)l * BC + bc) + 1];
    bool bad = is_nan2(y);
#pragma unroll
    for (int e = 0; e < E; ++e) bad = bad || is_nan2(x[e]);
    const double w = (m_off + m == 0) ? 1.0 : 2.0;
    const double k0 = gs0 * s0;                                 // gS0 / E
    const double k1 = gs1 * s1;                                 // 2 gS1 / E^2
#pragma unroll
    for (int e = 0; e < E; ++e) {
        int dr = 0, di = 0;                                      // L_e - G_e per component, exact
#pragma unroll
        for (int f = 0; f < E; ++f) {
            if (f != e) {
                dr += (x[f].x < x[e].x ? 1 : 0) - (x[f].x > x[e].x ? 1 : 0);
                di += (x[f].y < x[e].y ? 1 : 0) - (x[f].y > x[e].y ? 1 : 0);
            }
        }
        const int sr = (x[e].x > y.x ? 1 : 0) - (x[e].x < y.x ? 1 : 0);
        const int si = (x[e].y > y.y ? 1 : 0) - (x[e].y < y.y ? 1 : 0);
        const double vr = w * (k0 * (double)sr + k1 * (double)dr);
        const double vi = w * (k0 * (double)si + k1 * (double)di);
        out[(long long)e * C] = bad ? make_float2(NAN, NAN) : make_float2((float)vr, (float)vi);
    }
}

const char* check(const void* a, const void* b, const void* c, const void* d, int L, int M, int B, int E, int C, int l_off,
                  int m_off) {
    if (!(a && b && c && d)) return "null pointer";
    if (!(E >= 2 && E <= kMaxE)) return "E outside 2 ... 16 (all pairs of a coefficient's members are compared in registers)";
    if (!(L >= 1 && M >= 1 && B >= 1 && C >= 1 && l_off >= 0 && m_off >= 0 && (long long)l_off + L < (1LL << 30) &&
          (long long)m_off + M < (1LL << 30) && (long long)B * C < (1LL << 30) && (long long)L * M * B * C * E < (1LL << 38)))
        return "bad sizes";
    if (!mk::aligned<8>(a, b, c, d)) return "buffer not 8-byte aligned";
    return nullptr;
}

#define MK_SPEC_CRPS_DISPATCH(CALL)                                                                                              \
    switch (E) {                                                                                                                 \
        case 2: CALL(2); break;                                                                                                  \
        case 3: CALL(3); break;                                                                                                  \
        case 4: CALL(4); break;                                                                                                  \
        case 5: CALL(5); break;                                                                                                  \
        case 6: CALL(6); break;                                                                                                  \
        case 7: CALL(7); break;                                                                                                  \
        case 8: CALL(8); break;                                                                                                  \
        case 9: CALL(9); break;                                                                                                  \
        case 10: CALL(10); break;                                                                                                \
        case 11: CALL(11); break;                                                                                                \
        case 12: CALL(12); break;                                                                                                \
        case 13: CALL(13); break;                                                                                                \
        case 14: CALL(14); break;                                                                                                \
        case 15: CALL(15); break;                                                                                                \
        default: CALL(16); break;                                                                                                \
    }

}  // namespace

extern "C" long long mk_spec_crps_workspace(int L, int M, int BC) {
    if (L < 1 || M < 1 || BC < 1) return 0;
    return (long long)L * mk::ceil_div(M, kChunk) * BC * 2;
}

extern "C" int mk_spec_crps_sums(const float* cp, const float* ct, double* workspace, double* S, int L, int M, int B, int E, int C,
                                 int l_off, int m_off, void* stream) {
    const char* why = check(cp, ct, workspace, S, L, M, B, E, C, l_off, m_off);
    MK_REQUIRE(!why, why);
    hipStream_t st = (hipStream_t)stream;
    const int BC = B * C, nchunk = mk::ceil_div(M, kChunk);
    const long long nparts = (long long)L * nchunk * BC;
    const dim3 grid((unsigned)mk::ceil_div_ll(nparts, kT));
#define MK_CALL(EE)                                                                                                              \
    hipLaunchKernelGGL(spec_crps_sums_kernel<EE>, grid, dim3(kT), 0, st, (const float2*)cp, (const float2*)ct, workspace, \
                       L, M, C, BC, l_off, m_off, nchunk)
    MK_SPEC_CRPS_DISPATCH(MK_CALL)
#undef MK_CALL
    MK_LAUNCH_CHECK();
    const long long n = (long long)L * BC;
    hipLaunchKernelGGL(spec_crps_finalize, dim3((unsigned)mk::ceil_div_ll(n, kT)), dim3(kT), 0, st, workspace,
                       S, n, BC, nchunk, 1.0 / E, 2.0 / ((double)E * E));
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_spec_crps_bwd(const float* cp, const float* ct, const double* gS, float* gcp, int L, int M, int B, int E, int C,
                                int l_off, int m_off, void* stream) {
    const char* why = check(cp, ct, gS, gcp, L, M, B, E, C, l_off, m_off);
    MK_REQUIRE(!why, why);
    hipStream_t st = (hipStream_t)stream;
    const int BC = B * C;
    const long long n = (long long)L * M * BC;
    const dim3 grid((unsigned)mk::ceil_div_ll(n, kT));
    const double s0 = 1.0 / E, s1 = 2.0 / ((double)E * E);
#define MK_CALL(EE)                                                                                                              \
    hipLaunchKernelGGL(spec_crps_bwd_kernel<EE>, grid, dim3(kT), 0, st, (const float2*)cp, (const float2*)ct, gS, \
                       (float2*)gcp, n, M, C, BC, l_off, m_off, s0, s1)
    MK_SPEC_CRPS_DISPATCH(MK_CALL)
#undef MK_CALL
    MK_LAUNCH_CHECK();
    return 0;
}
