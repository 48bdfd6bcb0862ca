// Patch rows of an image and back (see makani_amd.h): the gather in front of the patch-embedding GEMM of ViT / AFNOv1 and the
// un-patchify behind their heads.  A pure permutation, with at most one rounding (fp32 -> bf16) or an exact widening.
//
//   image  [B][C][H][W],   token rows [B hp wp][ldt],   row r = (b hp + y) wp + x,   element (b, c, y p0 + i, x p1 + j)
//   order 0: f = (c p0 + i) p1 + j        order 1: f = (i p1 + j) C + c
//
// The image is contiguous along W, a token row along f, and no thread mapping walks both: a workgroup stages a tile through LDS,
// one 32-bit word per element as in transpose_add_kernel (csrc/layout.hip), filled along the source's contiguous axis and drained
// along the destination's.  A tile is CC channels x IT patch rows x TX patches x JT patch columns of one (b, y):
//
//   LDS word  (c_l IT + i_l) pitch + x_l JT + jj         (an image row of the tile per LDS row)
//   order 0:  IT = p0 and JT = p1 wherever a patch fits, so a token's tile is CC p0 p1 consecutive features;
//   order 1:  CC = C wherever the channels fit, so a token's tile is IT p1 C consecutive features (p1 C = 584 at C = 73, whatever
//             C is a multiple of); only a C beyond the tile is cut, into chunks of a multiple of 8 channels, which are 16-byte
//             runs where C itself is a multiple of 8 (4 for fp32) and single elements otherwise.
//
// The drain of order 0 walks jj, then the LDS row: pitch = JT (mod 32) puts consecutive features on consecutive banks.  The drain
// of order 1 walks the LDS rows (c_l first): an odd pitch spreads them over all banks.  The fill is row-wise in both.
// PATCH_TILE_WORDS: 36 KB of the 160 KB, four workgroups of 256 threads per compute unit with room to spare -- the passes are
// bound by HBM, and sixteen waves a unit keep enough 16-byte requests in flight; a larger tile would only lengthen the time
// a workgroup holds data without moving it.
#include "common.h"
#include "layout_elem.h"
#include "../../include/makani_amd.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace {

constexpr int PATCH_TILE_WORDS = 9216;
constexpr int PATCH_THREADS = 256;

struct PatchTile {
    int C, H, W, p0, p1, hp, wp, order;
    int CC, IT, TX, JT, pitch;          // the tile
    int nct, nit, nxt, njt;             // tiles per (b, y) along channels, patch rows, patches across, patch columns
    long long ldt;
};

template <typename TS, typename TD> __device__ __forceinline__ unsigned convert_word(unsigned w) {
    if constexpr (std::is_same_v<TS, TD>) return w;                     // bit for bit
    else return LayoutElem<TD>::round(LayoutElem<TS>::value(w));        // fp32 -> bf16 once to nearest even; bf16 -> fp32 exact
}

// what one workgroup moves
struct PatchBlock {
    int c0, i0, j0, CCe, ITe, TXe, Je;
    long long ibase, tbase;             // image element (c0, y p0 + i0, x0 p1 + j0) of sample b; token row of patch x0, feature 0
};

__device__ __forceinline__ PatchBlock patch_block(const PatchTile& g) {
    long long bid = blockIdx.x;
    const int jt = (int)(bid % g.njt); bid /= g.njt;
    const int xt = (int)(bid % g.nxt); bid /= g.nxt;
    const int ct = (int)(bid % g.nct); bid /= g.nct;
    const int it = (int)(bid % g.nit); bid /= g.nit;
    const int y = (int)(bid % g.hp);
    const long long b = bid / g.hp;
    PatchBlock k;
    k.c0 = ct * g.CC; k.i0 = it * g.IT; k.j0 = jt * g.JT;
    const int x0 = xt * g.TX;
    k.CCe = min(g.CC, g.C - k.c0); k.ITe = min(g.IT, g.p0 - k.i0); k.TXe = min(g.TX, g.wp - x0); k.Je = min(g.JT, g.p1 - k.j0);
    k.ibase = ((b * g.C + k.c0) * g.H + (long long)y * g.p0 + k.i0) * g.W + (long long)x0 * g.p1 + k.j0;
    k.tbase = ((b * g.hp + y) * g.wp + x0) * g.ldt;
    return k;
}

// token-side element k of a token's part of the tile, in feature order: (c_l, i_l, jj) with jj fastest for order 0,
// (i_l, jj, c_l) with c_l fastest for order 1
struct TokPos {
    int c_l, i_l, jj;
};

__device__ __forceinline__ TokPos tok_first(const PatchTile& g, const PatchBlock& k, int e) {
    TokPos p;
    if (g.order == 0) {
        const int row = e / k.Je;
        p.jj = e - row * k.Je;
        p.c_l = row / k.ITe;
        p.i_l = row - p.c_l * k.ITe;
    } else {
        const int t = e / k.CCe;
        p.c_l = e - t * k.CCe;
        p.i_l = t / k.Je;
        p.jj = t - p.i_l * k.Je;
    }
    return p;
}

__device__ __forceinline__ void tok_next(const PatchTile& g, const PatchBlock& k, TokPos& p) {
    if (g.order == 0) {
        if (++p.jj == k.Je) {
            p.jj = 0;
            if (++p.i_l == k.ITe) { p.i_l = 0; ++p.c_l; }
        }
    } else {
        if (++p.c_l == k.CCe) {
            p.c_l = 0;
            if (++p.jj == k.Je) { p.jj = 0; ++p.i_l; }
        }
    }
}

__device__ __forceinline__ int tok_lds(const PatchTile& g, const PatchBlock& k, const TokPos& p, int x_l) {
    return (p.c_l * k.ITe + p.i_l) * g.pitch + x_l * k.Je + p.jj;
}

__device__ __forceinline__ long long tok_feat(const PatchTile& g, const PatchBlock& k, const TokPos& p) {
    const long long c = k.c0 + p.c_l, i = k.i0 + p.i_l, j = k.j0 + p.jj;
    return g.order == 0 ? (c * g.p0 + i) * g.p1 + j : (i * g.p1 + j) * g.C + c;
}

// PATCHIFY: src the image, dst the token rows; else the reverse.  IVEC / TVEC: 16-byte accesses on the image / token side (the
// host has checked that every vector lies inside one contiguous run and is aligned), single elements otherwise.
template <typename TS, typename TD, bool PATCHIFY, bool IVEC, bool TVEC>
__global__ __launch_bounds__(PATCH_THREADS) void patch_kernel(const TS* __restrict__ src, TD* __restrict__ dst, const PatchTile g) {
    using TI = std::conditional_t<PATCHIFY, TS, TD>;      // the image's element
    using TT = std::conditional_t<PATCHIFY, TD, TS>;      // the tokens'
    __shared__ unsigned tile[PATCH_TILE_WORDS];
    const PatchBlock k = patch_block(g);
    const int tid = threadIdx.x;
    const int rows = k.CCe * k.ITe, cols = k.TXe * k.Je;        // the image side: rows of cols contiguous elements
    const int per_tok = rows * k.Je;                            // the token side: per_tok elements of each of TXe tokens
    constexpr int VI = IVEC ? 16 / (int)sizeof(TI) : 1, VT = TVEC ? 16 / (int)sizeof(TT) : 1;

    // image <-> LDS, along W
    auto image_pass = [&](auto to_lds) {
        constexpr bool TO_LDS = decltype(to_lds)::value;
        const int vpr = cols / VI;
        for (int e = tid; e < rows * vpr; e += PATCH_THREADS) {
            const int row = e / vpr, col = (e - row * vpr) * VI;
            const int c_l = row / k.ITe, i_l = row - c_l * k.ITe;
            const long long off = k.ibase + ((long long)c_l * g.H + i_l) * g.W + col;
            unsigned* t = tile + row * g.pitch + col;
            if constexpr (TO_LDS) {
                if constexpr (IVEC) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + off);
#pragma unroll
                    for (int q = 0; q < VI; ++q) t[q] = vec_word<TS>(v, q);
                } else {
                    t[0] = LayoutElem<TS>::bits(src[off]);
                }
            } else {
                if constexpr (IVEC) {
                    unsigned w[VI];
#pragma unroll
                    for (int q = 0; q < VI; ++q) w[q] = convert_word<TS, TD>(t[q]);
                    *reinterpret_cast<uint4*>(dst + off) = vec_pack<TD>(w);
                } else {
                    dst[off] = LayoutElem<TD>::from(convert_word<TS, TD>(t[0]));
                }
            }
        }
    };
    // tokens <-> LDS, along f
    auto token_pass = [&](auto to_lds) {
        constexpr bool TO_LDS = decltype(to_lds)::value;
        const int vpt = per_tok / VT;
        for (int e = tid; e < k.TXe * vpt; e += PATCH_THREADS) {
            const int x_l = e / vpt;
            TokPos p = tok_first(g, k, (e - x_l * vpt) * VT);
            const long long off = k.tbase + x_l * g.ldt + tok_feat(g, k, p);
            if constexpr (TO_LDS) {
                if constexpr (TVEC) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + off);
#pragma unroll
                    for (int q = 0; q < VT; ++q) {
                        tile[tok_lds(g, k, p, x_l)] = vec_word<TS>(v, q);
                        tok_next(g, k, p);
                    }
                } else {
                    tile[tok_lds(g, k, p, x_l)] = LayoutElem<TS>::bits(src[off]);
                }
            } else {
                if constexpr (TVEC) {
                    unsigned w[VT];
#pragma unroll
                    for (int q = 0; q < VT; ++q) {
                        w[q] = convert_word<TS, TD>(tile[tok_lds(g, k, p, x_l)]);
                        tok_next(g, k, p);
                    }
                    *reinterpret_cast<uint4*>(dst + off) = vec_pack<TD>(w);
                } else {
                    dst[off] = LayoutElem<TD>::from(convert_word<TS, TD>(tile[tok_lds(g, k, p, x_l)]));
                }
            }
        }
    };
    if constexpr (PATCHIFY) {
        image_pass(std::true_type{});
        __syncthreads();
        token_pass(std::false_type{});
    } else {
        token_pass(std::true_type{});
        __syncthreads();
        image_pass(std::false_type{});
    }
}

int gcd_int(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// The tile of a geometry.  Columns: whole patches, at least 64 elements across and a whole number of 16-byte vectors of either
// dtype where the patch allows; a patch wider than 128 columns is a tile row of its own, one wider than 1024 is cut.  Rows: what
// the order's token side needs contiguous first (see the head of the file), then as much of the rest as fits.  A geometry whose
// rows are few (small C) takes more patches across, so a workgroup still moves a tile's worth.
void choose_tile(PatchTile& g) {
    const int p1 = g.p1;
    if (p1 > 128) {
        g.TX = 1;
        g.JT = std::min(p1, 1024);
    } else {
        const int m = 8 / gcd_int(p1, 8);
        g.TX = std::min(mk::ceil_div(mk::ceil_div(64, p1), m) * m, g.wp);
        g.JT = p1;
        const long long want = (long long)g.C * g.p0 * (g.TX * p1 + 32);       // all rows at this width
        if (g.TX < g.wp && want * 2 <= PATCH_TILE_WORDS) g.TX = (int)std::min((long long)g.wp, g.TX * (PATCH_TILE_WORDS / want));
    }
    const int cols = g.TX * g.JT;
    g.pitch = g.order == 0 ? cols + (((g.JT - cols) % 32) + 32) % 32 : cols | 1;
    const int fit = PATCH_TILE_WORDS / g.pitch;                                 // LDS rows that fit: >= 1 (cols <= 1024 + ...)
    if (g.order == 0) {
        if (g.p0 <= fit) { g.IT = g.p0; g.CC = std::min(g.C, fit / g.p0); }
        else { g.IT = fit; g.CC = 1; }
    } else {
        if (g.C <= fit) { g.CC = g.C; g.IT = std::min(g.p0, fit / g.C); }
        else { g.CC = fit >= 8 ? fit & ~7 : fit; g.IT = 1; }
    }
    g.nct = mk::ceil_div(g.C, g.CC);
    g.nit = mk::ceil_div(g.p0, g.IT);
    g.nxt = mk::ceil_div(g.wp, g.TX);
    g.njt = mk::ceil_div(g.p1, g.JT);
}

// 16-byte accesses on the image side: every tile row starts and ends on a vector
bool image_vec(const PatchTile& g, int V, const void* img) {
    if (!mk::aligned<16>(img) || g.W % V) return false;
    if (g.njt > 1) return g.JT % V == 0 && g.p1 % V == 0;
    return g.nxt == 1 || (g.TX * g.p1) % V == 0;
}

// ... on the token side: every vector of a token's tile is V consecutive features that start on a vector
bool token_vec(const PatchTile& g, int V, const void* tok) {
    if (!mk::aligned<16>(tok) || g.ldt % V) return false;
    const long long F = (long long)g.C * g.p0 * g.p1;
    if (g.order == 0) {
        if (g.JT == g.p1 && g.IT == g.p0 && ((long long)g.CC * g.p0 * g.p1) % V == 0 && F % V == 0) return true;    // one run per token
        return g.p1 % V == 0 && g.JT % V == 0;                                                                       // a run per (c, i)
    }
    if (g.CC == g.C && (g.JT == g.p1 || g.IT == 1) && ((long long)g.JT * g.C) % V == 0 && ((long long)g.p1 * g.C) % V == 0) return true;
    return g.C % V == 0 && g.CC % V == 0;                                                                            // a run per (i, j)
}

template <typename TS, typename TD, bool PATCHIFY>
int patch_launch(const char* who, const void* src, void* dst, const PatchTile& g, int batch, void* stream) {
    using TI = std::conditional_t<PATCHIFY, TS, TD>;
    using TT = std::conditional_t<PATCHIFY, TD, TS>;
    const void* img = PATCHIFY ? src : dst;
    const void* tok = PATCHIFY ? dst : src;
    const bool iv = image_vec(g, 16 / (int)sizeof(TI), img), tv = token_vec(g, 16 / (int)sizeof(TT), tok);
    const long long nblk = (long long)batch * g.hp * g.nit * g.nct * g.nxt * g.njt;
    MK_REQUIRE_AS(who, nblk < 2147483647LL, "grid too large");
    const auto kernel = iv ? (tv ? patch_kernel<TS, TD, PATCHIFY, true, true> : patch_kernel<TS, TD, PATCHIFY, true, false>)
                           : (tv ? patch_kernel<TS, TD, PATCHIFY, false, true> : patch_kernel<TS, TD, PATCHIFY, false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(PATCH_THREADS), 0, (hipStream_t)stream, static_cast<const TS*>(src),
                       static_cast<TD*>(dst), g);
    MK_LAUNCH_CHECK_AS(who);
    return 0;
}

template <bool PATCHIFY>
int patch_entry(const char* who, const void* src, int src_dtype, void* dst, int dst_dtype, const void* img, int img_dtype,
                const void* tok, int tok_dtype, long long ldt, int batch, int C, int H, int W, int p0, int p1, int order, void* stream) {
    MK_REQUIRE_AS(who, img && tok, "null pointer");
    MK_REQUIRE_AS(who, (img_dtype == 0 || img_dtype == 1) && (tok_dtype == 0 || tok_dtype == 1), "unknown dtype (0 fp32 | 1 bf16)");
    MK_REQUIRE_AS(who, order == 0 || order == 1, "unknown order (0 channel-major | 1 channel-minor features)");
    MK_REQUIRE_AS(who, batch >= 1 && C >= 1 && H >= 1 && W >= 1 && p0 >= 1 && p1 >= 1, "bad sizes");
    MK_REQUIRE_AS(who, H % p0 == 0 && W % p1 == 0, "the patch does not divide the grid");
    const long long F = (long long)C * p0 * p1;
    MK_REQUIRE_AS(who, F < 2147483647LL, "a token row is too long");
    MK_REQUIRE_AS(who, ldt >= F, "ldt is smaller than the features of a token");
    MK_REQUIRE_AS(who, mk::aligned_to(img, img_dtype ? 2 : 4) && mk::aligned_to(tok, tok_dtype ? 2 : 4),
                  "operands must be aligned to their elements");
    PatchTile g{};
    g.C = C; g.H = H; g.W = W; g.p0 = p0; g.p1 = p1; g.hp = H / p0; g.wp = W / p1; g.order = order; g.ldt = ldt;
    choose_tile(g);
    MK_REQUIRE_AS(who, g.CC >= 1 && g.IT >= 1 && g.TX >= 1 && g.JT >= 1 && g.TX * g.JT <= g.pitch
                       && (long long)g.CC * g.IT * g.pitch <= PATCH_TILE_WORDS, "internal: the tile does not fit");
    if (src_dtype == 0) {
        return dst_dtype == 0 ? patch_launch<float, float, PATCHIFY>(who, src, dst, g, batch, stream)
                              : patch_launch<float, unsigned short, PATCHIFY>(who, src, dst, g, batch, stream);
    }
    return dst_dtype == 0 ? patch_launch<unsigned short, float, PATCHIFY>(who, src, dst, g, batch, stream)
                          : patch_launch<unsigned short, unsigned short, PATCHIFY>(who, src, dst, g, batch, stream);
}

}  // namespace

extern "C" int mk_patch_tile_info(int C, int H, int W, int p0, int p1, int order, long long ldt, int* tile) {
    MK_REQUIRE(tile, "null pointer");
    MK_REQUIRE(order == 0 || order == 1, "unknown order (0 channel-major | 1 channel-minor features)");
    MK_REQUIRE(C >= 1 && H >= 1 && W >= 1 && p0 >= 1 && p1 >= 1, "bad sizes");
    MK_REQUIRE(H % p0 == 0 && W % p1 == 0, "the patch does not divide the grid");
    MK_REQUIRE((long long)C * p0 * p1 < 2147483647LL && ldt >= (long long)C * p0 * p1, "ldt is smaller than the features of a token");
    PatchTile g{};
    g.C = C; g.H = H; g.W = W; g.p0 = p0; g.p1 = p1; g.hp = H / p0; g.wp = W / p1; g.order = order; g.ldt = ldt;
    choose_tile(g);
    const int out[14] = {g.CC, g.IT, g.TX, g.JT, g.pitch, g.nct, g.nit, g.nxt, g.njt, PATCH_TILE_WORDS,
                         image_vec(g, 4, nullptr), image_vec(g, 8, nullptr), token_vec(g, 4, nullptr), token_vec(g, 8, nullptr)};
    for (int i = 0; i < 14; ++i) tile[i] = out[i];
    return 0;
}

extern "C" int mk_patchify(const void* img, int img_dtype, void* tok, int tok_dtype, long long ldt, int batch, int C, int H, int W,
                           int p0, int p1, int order, void* stream) {
    return patch_entry<true>(__func__, img, img_dtype, tok, tok_dtype, img, img_dtype, tok, tok_dtype, ldt, batch, C, H, W, p0, p1,
                             order, stream);
}

extern "C" int mk_unpatchify(const void* tok, int tok_dtype, long long ldt, void* img, int img_dtype, int batch, int C, int H, int W,
                             int p0, int p1, int order, void* stream) {
    return patch_entry<false>(__func__, tok, tok_dtype, img, img_dtype, img, img_dtype, tok, tok_dtype, ldt, batch, C, H, W, p0, p1,
                              order, stream);
}
