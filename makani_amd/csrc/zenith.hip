// Cosine of the solar zenith angle on a lat / lon grid from per-time scalars (the unpredicted input channel that the
// reference's loaders compute on the host with makani/third_party/climt/zenith_angle.py):
//   out[n][i][j] = sin_lat[i] * sin_dec[n] + (cos_lat[i] * cos_dec[n]) * cos((gmst[n] + lon[j]) - ra[n])
// in fp32 with exactly the reference's operations and order: every product and sum is rounded on its own, the hour angle
// is (gmst + lon) - ra, the cosine is the accurate cosf (arguments reach 4 pi).  hipcc contracts a * b + c to an fma by
// default (and HIP's __fmul_rn / __fadd_rn are plain operators that it contracts just the same), so contraction is
// switched off for this whole file by the pragma below; the ISA of head, body and tail is v_mul_f32 / v_pk_mul_f32 followed
// by v_add_f32 / v_pk_add_f32 in front of every store (checked with --save-temps); the only fused operations left in the
// kernel are those inside cosf's own polynomial, whose value all rows share through the table.
// The value of a point depends on (n, i, j) only, never on how the field is cut into launches, workgroups or lanes, so a
// shard launched on its own slices of the tables equals the slice of the full field bit for bit.
//
// The kernel only writes.  Workgroup item (time n, chunk of R rows, tile of kTile = 256 columns): each of the 256 threads
// puts one cosine into an LDS table -- one cosf per (time, column), shared by the R rows -- and after one barrier each of
// the four waves walks rows of the chunk: scalar head up to the 16-byte boundary of the output, a body of one 16-byte
// store per lane, scalar tail; per point one LDS read, one product, one sum.  With 256 columns a wave writes a row's
// segment with ONE store instruction, 1 KB without gaps, and goes on to another row; measured that is
// what the store rate hangs on: 4.0 TB/s, against 2.1 / 1.7 / 2.2 TB/s when a wave walks 2 / 4 / 5.6 KB of a row in
// several steps.  Any W, any element-aligned output.  Items are strided over a grid capped as in preproc.hip.  No
// atomics, no allocation, nothing that waits on the host.
#include "common.h"
#include "stream_io.h"
#include "../../include/makani_amd.h"

#include <cstdint>

#pragma clang fp contract(off)   // file scope: no product is ever fused into a following sum in this translation unit

namespace {

constexpr int kT = 256;          // threads per workgroup (4 waves)
constexpr int kE = 4;            // points per lane per step: one 16-byte store
constexpr int kTile = 256;       // columns per cosine table (1 KB of LDS): one store instruction per wave and row
constexpr int kGrid = 8192;      // at most this many workgroups, striding over the items
constexpr int kRowsMax = 32;     // rows per item: from here halved down to kRowsMin while the grid is short of kWant
constexpr int kRowsMin = 8;
constexpr int kWant = 1024;      // workgroups that fill the 256 CUs four times

using mk::sio::head_points;

// the one arithmetic expression of a point, used by head, body and tail alike: a rounded product, then a rounded sum
// (contraction is off, see above)
__device__ __forceinline__ float point(float a, float b, float c) {
    const float bc = b * c;
    return a + bc;
}

// items = n * nchunk * ntile, item = (time * nchunk + chunk) * ntile + tile
__global__ __launch_bounds__(kT) void cos_zenith_kernel(const float* __restrict__ eph, const float* __restrict__ sin_lat,
                                                        const float* __restrict__ cos_lat, const float* __restrict__ lon_rad,
                                                        float* __restrict__ out, int H, int W, int R, int nchunk, int ntile,
                                                        long long items) {
    __shared__ float tab[kTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {         // workgroup-uniform trip count
        const long long tc = item / ntile;
        const int tile = (int)(item - tc * ntile);
        const long long n = tc / nchunk;
        const int chunk = (int)(tc - n * nchunk);
        const int c0 = tile * kTile, wseg = min(kTile, W - c0);
        const float sin_dec = eph[4 * n], cos_dec = eph[4 * n + 1], gmst = eph[4 * n + 2], ra = eph[4 * n + 3];
        __syncthreads();                                                         // the previous item's rows are written
        for (int c = threadIdx.x; c < wseg; c += kT) tab[c] = cosf((gmst + lon_rad[c0 + c]) - ra);
        __syncthreads();
        const int h1 = min(H, (chunk + 1) * R);
        for (int h = chunk * R + wave; h < h1; h += kT / 64) {
            const float a = sin_lat[h] * sin_dec, b = cos_lat[h] * cos_dec;
            float* dst = out + ((n * H + h) * (long long)W + c0);
            const int head = head_points(dst, wseg);
            const int nv = (wseg - head) / kE;
            const int vend = head + nv * kE;                                     // scalar points: [0, head) and [vend, wseg)
            for (int j = lane; j < nv; j += 64) {
                const int i = head + j * kE;
                *reinterpret_cast<float4*>(dst + i) =
                    make_float4(point(a, b, tab[i]), point(a, b, tab[i + 1]), point(a, b, tab[i + 2]), point(a, b, tab[i + 3]));
            }
            const int nscal = head + (wseg - vend);
            for (int q = lane; q < nscal; q += 64) {
                const int i = q < head ? q : vend + (q - head);
                dst[i] = point(a, b, tab[i]);
            }
        }
    }
}

}  // namespace

extern "C" int mk_cos_zenith(const float* eph, const float* sin_lat, const float* cos_lat, const float* lon_rad, float* out,
                             long long n, int H, int W, void* stream) {
    MK_REQUIRE(n >= 0 && H >= 1 && W >= 1, "bad sizes");
    MK_REQUIRE(n <= (1LL << 31) && (double)n * H * W < (double)(1LL << 40), "field too large");
    if (n == 0) return 0;
    MK_REQUIRE(eph && sin_lat && cos_lat && lon_rad && out, "null pointer");
    MK_REQUIRE(mk::aligned<4>(eph, sin_lat, cos_lat, lon_rad, out), "fp32 stream not 4-byte aligned");
    const int ntile = mk::ceil_div(W, kTile);
    int R = kRowsMax;
    while (R > kRowsMin && n * mk::ceil_div(H, R) * ntile < kWant) R /= 2;
    const int nchunk = mk::ceil_div(H, R);
    const long long items = n * nchunk * ntile;
    const dim3 grid((unsigned)(items < kGrid ? items : kGrid));
    hipLaunchKernelGGL(cos_zenith_kernel, grid, dim3(kT), 0, (hipStream_t)stream, eph, sin_lat, cos_lat, lon_rad, out, H, W, R,
                       nchunk, ntile, items);
    MK_LAUNCH_CHECK();
    return 0;
}
