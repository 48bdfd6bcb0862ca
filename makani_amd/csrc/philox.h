// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), the one
// definition the noise kernel and the host-only mk_noise_words share: the same four words on the host and on the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_PHILOX_HD __host__ __device__ __forceinline__
#else
#define MK_PHILOX_HD inline
#endif

namespace mk {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // Weyl increments of the key

// ctr[4] -> the four output words in place; the key is bumped after each of the first nine rounds
MK_PHILOX_HD void philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * ctr[0], p1 = (uint64_t)kPhiloxM1 * ctr[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1;
        ctr[0] = n0;
        ctr[1] = (uint32_t)p1;
        ctr[2] = n2;
        ctr[3] = (uint32_t)p0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

}  // namespace mk
