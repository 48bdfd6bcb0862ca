// Correlated spherical noise: draws the packed spectrum state [L][M][BC] (complex64, BC fastest) of an isotropic Gaussian
// random field directly, one pass.  For the entry (l, m, bc) of a shard with global offsets (l_off, m_off) and first global
// row row0 (even), with gl = l_off + l, gm = m_off + m, q = (row0 + bc) >> 1, T = t + (t_dev ? *t_dev : 0) mod 2^32:
//   words  = Philox4x32-10(counter (q, gl, gm, T), key (seed low, seed high));    (a, b) = words (0, 1) for the even row
//                                                                                  of the pair, words (2, 3) for the odd one
//   u1 = ((a >> 8) + 1) 2^-24 in (0, 1],  u2 = (b >> 8) 2^-24 in [0, 1)           (both exact in fp32)
//   rad = sqrtf(-2 logf(u1)),  (z_re, z_im) = rad (cospi(2 u2), sinpi(2 u2))       (sincospif: the angle is never rounded)
//   xi  = gm == 0 ? (s sigma_l) z_re + 0 i : (s fl(sigma_l / sqrt 2)) (z_re + i z_im)       s = row_scale[bc] or 1
//   state = phi == 0 ? xi : fl(fl(phi state) + fl(fl(sqrt(1 - phi^2)) xi))                  (AR(1); phi == 0 reads nothing)
// and exact zero where gl < gm.  The counter names global indices only, so a shard's draw is the slice of the full draw
// bit for bit.  The accurate logf / sqrtf / sincospif (no fast-math, no __ intrinsics); contraction off, nothing is fused.
//
// Decomposition.  One thread per (l, m, pair q), q fastest, grid capped and strided: a thread runs the ten rounds once and
// serves rows 2q and 2q + 1.  Even BC: the pair is one 16-byte store (and one 16-byte load with phi > 0); odd BC: 8 bytes
// per row, the missing odd row of the last pair skipped.  The thread index is 32-bit (two 32-bit divisions per thread; a
// 64-bit pair costs about half of the arithmetic of the draw itself): L M ceil(BC / 2) of 2^31 or more, a state of 32 GB, is
// refused.  Element offsets are 64-bit.  No atomics, no workspace: the same bits every run; capturable (t_dev is read on
// the device, so a replay draws anew).
#include "common.h"
#include "philox.h"
#include "../../include/makani_amd.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kGroupsPerCU = 8;            // grid cap; the rest by striding

struct Normal {
    float re, im;
};

__device__ __forceinline__ Normal box_muller(uint32_t a, uint32_t b) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(b >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    return {rad * c, rad * s};
}

// the coefficient of one row from its two words; amp0 = sigma_l, amp = fl(sigma_l / sqrt 2), s the row's scale
__device__ __forceinline__ float2 coefficient(uint32_t a, uint32_t b, bool order0, float amp0, float amp, float s) {
    const Normal z = box_muller(a, b);
    if (order0) return make_float2((s * amp0) * z.re, 0.0f);
    const float w = s * amp;
    return make_float2(w * z.re, w * z.im);
}

__device__ __forceinline__ float2 ar1(float2 old, float2 xi, float phi, float cphi) {
    return make_float2(phi * old.x + cphi * xi.x, phi * old.y + cphi * xi.y);
}

template <bool EVEN, bool AR>
__global__ __launch_bounds__(kThreads) void noise_spectrum_kernel(float2* __restrict__ state, const float* __restrict__ sigma_l,
                                                                  const float* __restrict__ row_scale, uint32_t M, uint32_t NQ, uint32_t total,
                                                                  long long BC, uint32_t l_off, uint32_t m_off, uint32_t q0,
                                                                  uint32_t k0, uint32_t k1, uint32_t t, const int* __restrict__ t_dev,
                                                                  float phi, float cphi) {
    const uint32_t T = t + (t_dev ? (uint32_t)*t_dev : 0u);
    const uint32_t stride = gridDim.x * kThreads;      // below 2^20, total below 2^31: i + stride does not wrap
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
        const uint32_t lm = i / NQ, q = i - lm * NQ;
        const uint32_t l = lm / M, m = lm - l * M;
        const uint32_t gl = l_off + l, gm = m_off + m;
        const long long bc = 2 * (long long)q;
        const bool odd_row = EVEN || bc + 1 < BC;
        float2* p = state + (long long)lm * BC + bc;
        float2 e = make_float2(0.0f, 0.0f), o = e;
        if (gl >= gm) {
            uint32_t w[4] = {q0 + q, gl, gm, T};
            mk::philox4x32_10(w, k0, k1);
            const float amp0 = sigma_l[l];
            const float amp = (float)((double)amp0 * 0.70710678118654752440);
            const float se = row_scale ? row_scale[bc] : 1.0f;
            const float so = (row_scale && odd_row) ? row_scale[bc + 1] : 1.0f;
            e = coefficient(w[0], w[1], gm == 0, amp0, amp, se);
            o = coefficient(w[2], w[3], gm == 0, amp0, amp, so);
            if (AR) {
                if (EVEN) {
                    const float4 old = *reinterpret_cast<const float4*>(p);
                    e = ar1(make_float2(old.x, old.y), e, phi, cphi);
                    o = ar1(make_float2(old.z, old.w), o, phi, cphi);
                } else {
                    e = ar1(p[0], e, phi, cphi);
                    if (odd_row) o = ar1(p[1], o, phi, cphi);
                }
            }
        }
        if (EVEN) {
            *reinterpret_cast<float4*>(p) = make_float4(e.x, e.y, o.x, o.y);
        } else {
            p[0] = e;
            if (odd_row) p[1] = o;
        }
    }
}

void launch(void* state, const float* sigma_l, const float* row_scale, int M, long long BC, long long NQ, long long total,
            int l_off, int m_off, uint32_t q0, uint32_t k0, uint32_t k1, uint32_t t, const int* t_dev, float phi, hipStream_t st) {
    const long long want = mk::ceil_div_ll(total, kThreads), cap = (long long)mk::cu_count() * kGroupsPerCU;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(kThreads);
    const float cphi = (float)std::sqrt(1.0 - (double)phi * (double)phi);
    const bool even = (BC & 1) == 0, ar = phi != 0.0f;
#define MK_NOISE_ARGS (float2*)state, sigma_l, row_scale, (uint32_t)M, (uint32_t)NQ, (uint32_t)total, BC, (uint32_t)l_off, (uint32_t)m_off, q0, k0, k1, t, t_dev, phi, cphi
    if (even && ar) hipLaunchKernelGGL((noise_spectrum_kernel<true, true>), grid, block, 0, st, MK_NOISE_ARGS);
    else if (even) hipLaunchKernelGGL((noise_spectrum_kernel<true, false>), grid, block, 0, st, MK_NOISE_ARGS);
    else if (ar) hipLaunchKernelGGL((noise_spectrum_kernel<false, true>), grid, block, 0, st, MK_NOISE_ARGS);
    else hipLaunchKernelGGL((noise_spectrum_kernel<false, false>), grid, block, 0, st, MK_NOISE_ARGS);
#undef MK_NOISE_ARGS
}

}  // namespace

extern "C" int mk_noise_words(long long seed, long long q, int l, int m, int t, int* out4) {
    MK_REQUIRE(out4, "null pointer");
    MK_REQUIRE(q >= 0 && q < (1LL << 32), "q outside [0, 2^32)");
    uint32_t w[4] = {(uint32_t)q, (uint32_t)l, (uint32_t)m, (uint32_t)t};
    mk::philox4x32_10(w, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32));
    for (int i = 0; i < 4; ++i) out4[i] = (int)w[i];
    return 0;
}

extern "C" int mk_noise_spectrum(void* state, const float* sigma_l, const float* row_scale, int L, int M, long long BC, int l_off,
                                 int m_off, long long row0, long long seed, int t, const int* t_dev, float phi, void* stream) {
    MK_REQUIRE(state && sigma_l, "null pointer");
    MK_REQUIRE(mk::aligned<16>(state), "state is not 16-byte aligned");
    MK_REQUIRE(mk::aligned<4>(sigma_l, row_scale, t_dev), "a table is not 4-byte aligned");
    MK_REQUIRE(L >= 1 && M >= 1 && BC >= 1, "bad sizes");
    MK_REQUIRE(l_off >= 0 && m_off >= 0, "negative offset");
    MK_REQUIRE((long long)l_off + L <= INT32_MAX && (long long)m_off + M <= INT32_MAX, "global degree or order out of range");
    MK_REQUIRE(row0 >= 0 && (row0 & 1) == 0, "row0 must be even and non-negative");
    MK_REQUIRE(phi >= 0.0f && phi < 1.0f, "phi outside [0, 1)");          // NaN fails both comparisons
    MK_REQUIRE(BC < (1LL << 40), "too many rows");
    const long long NQ = (BC + 1) / 2;
    MK_REQUIRE((row0 >> 1) + NQ <= (1LL << 32), "the row pair index q passes 2^32");
    // L M < 2^62 and NQ < 2^40, so the quotient form cannot overflow
    MK_REQUIRE((long long)L * M <= ((1LL << 31) - 1) / NQ, "L * M * ceil(BC / 2) beyond the kernel's 32-bit index (2^31 threads)");
    const long long total = (long long)L * M * NQ;
    const uint32_t k0 = (uint32_t)(uint64_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32), q0 = (uint32_t)(row0 >> 1);
    hipStream_t st = (hipStream_t)stream;
    launch(state, sigma_l, row_scale, M, BC, NQ, total, l_off, m_off, q0, k0, k1, (uint32_t)t, t_dev, phi, st);
    MK_LAUNCH_CHECK();
    return 0;
}
