// GELU (exact erf form, nn.GELU()) and its derivative, for every kernel that applies the activation.
//
// fp32 fields: erff().  bf16 fields and the bf16 epilogues of the pixel-column engine: the normal CDF through
// erfc(|z|/sqrt2) in the Abramowitz-Stegun 7.1.26 rational-exponential form (|error| < 1.5e-7 absolute on erf, three orders
// below the 2^-9 rounding of the stored value): 2 transcendentals + ~12 FMAs instead of erff()'s ~35 instructions plus a
// separate exp for the derivative -- with erff() the norm+GELU passes were VALU-bound (the backward sums pass ran at
// 3.3 TB/s against 5.4 TB/s for the same pass without the activation).
//
// The products and sums below are plain operators, so whether they are fused follows the fp-contract state of the file
// that includes this header at the place of the include: chnorm.hip switches contraction off and includes it below its
// pragma.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

namespace mk {
namespace gelu {

struct PhiPair {
    float Phi, phi;   // standard normal CDF and PDF at x
};
__device__ __forceinline__ PhiPair normal_cdf_pdf(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float q = fmaf(1.061405429f, t, -1.453152027f);
    q = fmaf(q, t, 1.421413741f);
    q = fmaf(q, t, -0.284496736f);
    q = fmaf(q, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);   // exp(-x^2 / 2)
    const float half_erfc = 0.5f * q * t * e;                               // 0.5 erfc(|x| / sqrt2) = Phi(-|x|)
    PhiPair r;
    r.Phi = x < 0.f ? half_erfc : 1.0f - half_erfc;
    r.phi = 0.3989422804014327f * e;
    return r;
}

// the activation by the dtype the result is stored in
template <typename T> struct Act;
template <> struct Act<float> {
    static __device__ __forceinline__ float gelu(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752440f)); }
    static __device__ __forceinline__ float gelu_grad(float z) {
        return 0.5f * (1.f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * __expf(-0.5f * z * z);
    }
};
template <> struct Act<__hip_bfloat16> {
    static __device__ __forceinline__ float gelu(float z) { return z * normal_cdf_pdf(z).Phi; }
    static __device__ __forceinline__ float gelu_grad(float z) {
        const PhiPair c = normal_cdf_pdf(z);
        return fmaf(z, c.phi, c.Phi);
    }
};

}  // namespace gelu
}  // namespace mk
