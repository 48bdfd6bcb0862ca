// Layout conversion between the public torch layout [BC][L][M] complex64 and the
// private channels-last spectral layout [L][M][BC] complex64 (see makani_amd.h).
// A complex transpose of a [BC] x [L*M] matrix through 32 x 32 LDS tiles; HBM bound.
#include "common.h"
#include "layout_elem.h"
#include "../../include/makani_amd.h"

namespace {

constexpr int TS = 32;

// dst[c][r] = src[r][c] for a [R][C] float2 matrix -> [C][R]; optional zero mask on
// the (l, m) index when it is the column (pack: no mask) or row (unpack) index.
// UNPACK: src = private [LM][BC], dst = std [BC][LM], zero where l_off + l < m_off + m.
template <bool UNPACK>
__global__ __launch_bounds__(256) void transpose_c64_kernel(const float2* __restrict__ src, float2* __restrict__ dst,
                                                            int R, int C, int mloc, int l_off, int m_off) {
    __shared__ float2 tile[TS][TS + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const long long tiles_c = (C + TS - 1) / TS;
    const long long bid = blockIdx.x;
    const int r0 = (int)(bid / tiles_c) * TS, c0 = (int)(bid % tiles_c) * TS;
#pragma unroll
    for (int j = 0; j < TS; j += 8) {
        const int r = r0 + ty + j, c = c0 + tx;
        float2 v = make_float2(0.f, 0.f);
        if (r < R && c < C) {
            v = src[(long long)r * C + c];
            if (UNPACK) {  // rows are (l, m)
                const int l = r / mloc, m = r - l * mloc;
                if (l_off + l < m_off + m) v = make_float2(0.f, 0.f);
            }
        }
        tile[ty + j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TS; j += 8) {
        const int c = c0 + ty + j, r = r0 + tx;
        if (r < R && c < C) dst[(long long)c * R + r] = tile[tx][ty + j];
    }
}

// ---- tokens [batch][n][c] <-> fields [batch][c][n] (the channels-last AFNO on the planar transforms) ----
// dst[b][c][r] = src[b][r][c] (+ addend[b][c][r]) for a [R][C] matrix per batch entry, through a 64 x 64 tile of 32-bit words
// (an fp32 value's bits, or a bf16 value's 16 bits: without an addend the elements pass through bit for bit).  Rows of 65 words:
// the row-wise fill and the column-wise drain both touch every bank equally.  Both global sides walk their own contiguous axis.
// VEC: R and C are whole numbers of 16-byte vectors and the operands 16-byte aligned -- a vector is wholly inside the matrix
// or wholly outside; otherwise single elements.  Ragged tiles load and store nothing outside the matrix.
constexpr int LT = 64;

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void transpose_add_kernel(const T* __restrict__ src, const T* __restrict__ addend, T* __restrict__ dst,
                                                            int R, int C, int tiles_r, int tiles_c) {
    using E = LayoutElem<T>;
    __shared__ unsigned tile[LT][LT + 1];
    constexpr int V = 16 / (int)sizeof(T), VPR = LT / V;      // elements per vector, vectors per tile row
    long long bid = blockIdx.x;
    const int c0 = (int)(bid % tiles_c) * LT;
    bid /= tiles_c;
    const int r0 = (int)(bid % tiles_r) * LT;
    const long long base = (bid / tiles_r) * (long long)R * C;
    const int tid = threadIdx.x;
    if constexpr (VEC) {
        for (int e = tid; e < LT * VPR; e += 256) {
            const int r = e / VPR, q = (e % VPR) * V;
            if (r0 + r < R && c0 + q < C) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + base + (long long)(r0 + r) * C + c0 + q);
#pragma unroll
                for (int k = 0; k < V; ++k) tile[r][q + k] = vec_word<T>(v, k);
            }
        }
    } else {
        const int tx = tid & 63, ty = tid >> 6;
        for (int j = ty; j < LT; j += 4)
            if (r0 + j < R && c0 + tx < C) tile[j][tx] = E::bits(src[base + (long long)(r0 + j) * C + c0 + tx]);
    }
    __syncthreads();
    if constexpr (VEC) {
        for (int e = tid; e < LT * VPR; e += 256) {
            const int c = e / VPR, q = (e % VPR) * V;
            if (c0 + c < C && r0 + q < R) {
                const long long off = base + (long long)(c0 + c) * R + r0 + q;
                unsigned w[V];
#pragma unroll
                for (int k = 0; k < V; ++k) w[k] = tile[q + k][c];
                if (addend) {
                    const uint4 a = *reinterpret_cast<const uint4*>(addend + off);
#pragma unroll
                    for (int k = 0; k < V; ++k) w[k] = E::round(E::value(w[k]) + E::value(vec_word<T>(a, k)));
                }
                uint4 o;
                if constexpr (sizeof(T) == 4) o = make_uint4(w[0], w[1], w[2], w[3]);
                else o = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
                *reinterpret_cast<uint4*>(dst + off) = o;
            }
        }
    } else {
        const int tx = tid & 63, ty = tid >> 6;
        for (int j = ty; j < LT; j += 4)
            if (c0 + j < C && r0 + tx < R) {
                const long long off = base + (long long)(c0 + j) * R + r0 + tx;
                unsigned w = tile[tx][j];
                if (addend) w = E::round(E::value(w) + E::value(E::bits(addend[off])));
                dst[off] = E::from(w);
            }
    }
}

template <typename T>
int transpose_add_launch(const char* who, const void* src, const void* addend, void* dst, int batch, int R, int C, void* stream) {
    const long long tiles_r = mk::ceil_div(R, LT), tiles_c = mk::ceil_div(C, LT);
    MK_REQUIRE_AS(who, tiles_r * tiles_c < 2147483647LL / batch, "grid too large");
    constexpr int V = 16 / (int)sizeof(T);
    const bool vec = R % V == 0 && C % V == 0 && mk::aligned<16>(src, addend, dst);
    const auto kernel = vec ? transpose_add_kernel<T, true> : transpose_add_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_r * tiles_c * batch)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const T*>(src), static_cast<const T*>(addend), static_cast<T*>(dst), R, C, (int)tiles_r,
                       (int)tiles_c);
    MK_LAUNCH_CHECK_AS(who);
    return 0;
}

int layout_check(const char* who, const void* a, const void* b, const void* addend, int dtype, int batch, int n, int c) {
    MK_REQUIRE_AS(who, a && b, "null pointer");
    MK_REQUIRE_AS(who, dtype == 0 || dtype == 1, "unknown dtype (0 fp32 | 1 bf16)");
    MK_REQUIRE_AS(who, batch >= 1 && n >= 1 && c >= 1, "bad sizes");
    const uintptr_t item = dtype ? 2 : 4;
    MK_REQUIRE_AS(who, mk::aligned_to(a, item) && mk::aligned_to(b, item) && mk::aligned_to(addend, item),
                  "operands must be aligned to their elements");
    return 0;
}

}  // namespace

extern "C" int mk_tokens_to_fields(const void* tok, void* fld, int dtype, int batch, int n, int c, void* stream) {
    if (int e = layout_check(__func__, tok, fld, nullptr, dtype, batch, n, c)) return e;
    return dtype ? transpose_add_launch<unsigned short>(__func__, tok, nullptr, fld, batch, n, c, stream)
                 : transpose_add_launch<float>(__func__, tok, nullptr, fld, batch, n, c, stream);
}

extern "C" int mk_fields_to_tokens(const void* fld, const void* addend, void* tok, int dtype, int batch, int n, int c, void* stream) {
    if (int e = layout_check(__func__, fld, tok, addend, dtype, batch, n, c)) return e;
    return dtype ? transpose_add_launch<unsigned short>(__func__, fld, addend, tok, batch, c, n, stream)
                 : transpose_add_launch<float>(__func__, fld, addend, tok, batch, c, n, stream);
}

extern "C" int mk_spec_pack(const float* c_std, float* c_prv, int bc, int lloc, int mloc, void* stream) {
    MK_REQUIRE(c_std && c_prv, "null pointer");
    MK_REQUIRE(bc > 0 && lloc > 0 && mloc > 0, "bad sizes");
    const int R = bc, C = lloc * mloc;
    const long long nblk = (long long)mk::ceil_div(R, TS) * mk::ceil_div(C, TS);
    MK_REQUIRE(nblk < 2147483647LL, "grid too large");
    hipLaunchKernelGGL(transpose_c64_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)c_std, (float2*)c_prv, R, C, mloc, 0, 0);
    MK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mk_spec_unpack(const float* c_prv, float* c_std, int bc, int lloc, int mloc, int l_off, int m_off,
                              void* stream) {
    MK_REQUIRE(c_std && c_prv, "null pointer");
    MK_REQUIRE(bc > 0 && lloc > 0 && mloc > 0, "bad sizes");
    const int R = lloc * mloc, C = bc;
    const long long nblk = (long long)mk::ceil_div(R, TS) * mk::ceil_div(C, TS);
    MK_REQUIRE(nblk < 2147483647LL, "grid too large");
    hipLaunchKernelGGL(transpose_c64_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)c_prv, (float2*)c_std, R, C, mloc, l_off, m_off);
    MK_LAUNCH_CHECK();
    return 0;
}
