// What the kernels on v_mfma_f32_32x32x16_bf16 share: the vector types of the MFMA operands, the C/D row of an accumulator
// register, and a bf16 row tile staged global -> registers -> LDS into an image whose 16-byte chunks are XOR-swizzled
// (chunk ^ (row & 7)), with the fragment read that goes with it.  Users: attn.hip, toklinear.hip (all of it); gemm.hip,
// conv_gemm.hip, x3_engine.h, pce_common.h (the vector types).  The header defines no tile size and no thread count: the files
// pass theirs as template arguments and name what they take with `using` declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

namespace mk {
namespace mfma {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int tile_row(int r, int fh) { return (r & 3) + 8 * (r >> 2) + 4 * fh; }   // C/D row of register r
// the two bf16 of a 32-bit word as fp32
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }

// ---- staging of a [ROWS][KP] bf16 tile through registers, T threads ------------------------------------------------------
template <int ROWS, int KP, int T>
struct RowStage {
    static constexpr int CPR = KP / 8, NV = ROWS * CPR / T;
    static_assert(ROWS * CPR % T == 0, "tile does not divide among the threads");
    uint4 r[NV];
    // base: the tile's first row at its first k; rows at or past rows_valid and k at or past k_valid become zeros, and are not read
    template <typename Rows>
    __device__ __forceinline__ void load(const __hip_bfloat16* base, long long ld, Rows rows_valid, int k_valid, int tid) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = tid + i * T, row = v / CPR, c = v % CPR;
            r[i] = (row < rows_valid && c * 8 < k_valid) ? *reinterpret_cast<const uint4*>(base + row * ld + c * 8) : make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void put(char* img, int tid) const {      // [row][k], 16-byte chunks swizzled
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = tid + i * T, row = v / CPR, c = v % CPR;
            *reinterpret_cast<uint4*>(img + row * (KP * 2) + ((c ^ (row & 7)) << 4)) = r[i];
        }
    }
};

// operand fragment of k-step ks for MFMA row / column `row` of such an image: 8 consecutive k of one row
template <int KP>
__device__ __forceinline__ bf16x8 read_row_frag(const char* img, int row, int ks, int fh) {
    return *reinterpret_cast<const bf16x8*>(img + row * (KP * 2) + (((2 * ks + fh) ^ (row & 7)) << 4));
}

template <int N>
__device__ __forceinline__ void zero(f32x16 (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[i][r] = 0.f;
}
template <int M, int N>
__device__ __forceinline__ void zero(f32x16 (&a)[M][N]) {
#pragma unroll
    for (int m = 0; m < M; ++m) zero(a[m]);
}

}  // namespace mfma
}  // namespace mk
