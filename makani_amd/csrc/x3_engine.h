// fp32-accurate GEMM engine on the bf16 matrix cores ("bf16x3") on gfx950: the tile, the stagers and epilogues that more than
// one kernel family uses, and the launch helper.  The families (each with its own stagers and epilogues next to its kernels):
// x3_legendre.hip (K2 / K3), x3_spectral.hip (dhconv K5, channel mix, channel MLP), x3_latdft.hip, x3_conv.hip.
//
// CDNA4 has no TF32 and its fp32 MFMA runs at 1/16 of the bf16 rate.  Every fp32 operand is therefore
// split EXACTLY into three bf16 pieces  x = h + m + l  (8 + 8 + 8 significand bits, by truncation) and a
// product is evaluated as the six piece products of weight >= 2^-16
//     a*b ~= ah*bh + ah*bm + am*bh + ah*bl + am*bm + al*bh          (dropped terms <= 3 * 2^-24 |a b|)
// with v_mfma_f32_32x32x16_bf16 accumulating in fp32: fp32-level accuracy at 16/6 = 2.7x the fp32-MFMA
// rate.  The 1e-5 parity budget of the spectral path is met with two orders of magnitude to spare
// (tests/test_kernels_gpu.py compares against the float64 oracle).
//
// One 256-thread workgroup (4 waves, 2 x 2) owns a 128 x 128 tile of C and walks the contraction in steps
// of 32.  LDS holds ONE stage: per operand 128 rows x [3 pieces][32 k] bf16 (192 B, pitch 208 B so the
// ds_read_b128 fragment reads and the ds_write_b128 staging writes are bank-conflict free); the next
// k-step is prefetched into registers while the MFMAs run and converted / written after a barrier
// (53.5 KB -> 3 workgroups per CU cover each other's staging phases).  Measured alternatives: a register ring
// 2-4 k-steps deep for the streamed operand (2 workgroups per CU) and a 512-thread 256 x 128 tile with two
// LDS stages (1 per CU) were both slower.  Alone, the load stream of the full-resolution analysis takes 0.22 ms
// (~43 GB/s per CU for its HBM / L2 mix) and the MFMA phase 0.19 ms; the two barriers per k-step serialise them inside
// a workgroup and the three workgroups per CU recover about two thirds of the overlap (0.31 ms).  Shrinking the panel
// bytes by a third (fp32 tiles instead of a pre-split image) moves the total by 2 %, and a half-step pipeline (refill k 0..15 of
// the stage while the MFMAs read k 16..31, barriers that wait on nothing) left Legendre unchanged and cost dhconv
// 5-10 %: neither bytes nor the barrier placement is the limit.
// (Found in round 2: the stagers' gload used to finish with `valid ? loaded : 0` selects -- a use of the loaded value, so the
// compiler waited out the whole load latency right after issuing the loads, BEFORE the MFMAs of the current k-step, in all
// five kernels.  The masks were dropped: invalid lanes load zeros (X3_OOB) and the loads fly under the matrix work: dhconv
// forward 0.308 -> 0.269 ms.  Tried on top: a ring two k-steps deep (Legendre 0.29 -> 0.42 ms) and producer / consumer
// workgroups -- four staging waves, four multiplying waves, two LDS stages, one barrier per k-step, one workgroup per CU: 0.317 ms.)
//
// Operands whose contraction index is the slow memory axis (k-major rows, n contiguous) are transposed
// in the staging pass: a thread loads 8 consecutive k of two adjacent columns (float2 per row, 512 B per
// wave and row), splits them and writes one 16-byte [8 k] vector per piece and column.  Constant operands
// (the Legendre tables) are laid out once, tile by tile, so staging them is a straight walk over 16 KB.
#pragma once
#include "common.h"
#include "mfma_tile.h"
#include "tile_map.h"
#include "../../include/makani_amd.h"

#include <cstdint>
#include <cstdlib>

namespace {

using mk::mfma::bf16x8;
using mk::mfma::f32x16;
typedef float x3_f2 __attribute__((ext_vector_type(2)));
typedef float x3_f4 __attribute__((ext_vector_type(4)));

constexpr int XT = 256;                       // threads
constexpr int XM = 128, XN = 128, XK = 32;    // workgroup tile, k-step
constexpr int XPITCH = 208;                   // LDS row pitch: 192 data + 16 pad (13 x 16 B: odd)
constexpr int XROWB = 192;                    // bytes of one row per k-step: [3][32] bf16
constexpr int XIMG = XM * XPITCH + 128;       // one operand image (+128: offset of the odd half, see pair_off)
constexpr int X3_LDS = 2 * XIMG;              // 53,504 B

// LDS row offsets.  plain: row r at r * pitch.  pair: rows 2t, 2t+1 are written by one thread (lane t), so
// they live 64 rows (+128 B) apart -- 8 consecutive lanes then hit 8 consecutive rows (conflict-free
// stores) and a fragment read of 16 consecutive rows still covers all 64 banks.
__device__ __forceinline__ int plain_off(int r) { return r * XPITCH; }
__device__ __forceinline__ int pair_off(int r) { return ((r >> 1) + ((r & 1) << 6)) * XPITCH + ((r & 1) << 7); }

// exact three-way split; the bf16 pieces are the UPPER halves of the returned words
struct Split3 {
    uint32_t h, m, l;
};
__device__ __forceinline__ Split3 split3(float x) {
    Split3 s;
    s.h = __float_as_uint(x) & 0xFFFF0000u;
    const float r1 = x - __uint_as_float(s.h);
    s.m = __float_as_uint(r1) & 0xFFFF0000u;
    s.l = __float_as_uint(r1 - __uint_as_float(s.m));   // <= 8 significant bits left: truncation is exact
    return s;
}
// (upper half of e1) : (upper half of e0)
__device__ __forceinline__ uint32_t pack_hi(uint32_t e0, uint32_t e1) { return __builtin_amdgcn_perm(e1, e0, 0x07060302u); }

// split 8 consecutive-k values and store them as one 16-byte vector per piece at `dst` (+64 B per piece)
__device__ __forceinline__ void split_store8(const float (&v)[8], char* dst) {
    Split3 s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = split3(v[i]);
    uint4 h, m, l;
    h.x = pack_hi(s[0].h, s[1].h); h.y = pack_hi(s[2].h, s[3].h); h.z = pack_hi(s[4].h, s[5].h); h.w = pack_hi(s[6].h, s[7].h);
    m.x = pack_hi(s[0].m, s[1].m); m.y = pack_hi(s[2].m, s[3].m); m.z = pack_hi(s[4].m, s[5].m); m.w = pack_hi(s[6].m, s[7].m);
    l.x = pack_hi(s[0].l, s[1].l); l.y = pack_hi(s[2].l, s[3].l); l.z = pack_hi(s[4].l, s[5].l); l.w = pack_hi(s[6].l, s[7].l);
    *reinterpret_cast<uint4*>(dst) = h;
    *reinterpret_cast<uint4*>(dst + 64) = m;
    *reinterpret_cast<uint4*>(dst + 128) = l;
}

// Branch-free masked loads: a raw buffer load whose lane offset lies past the descriptor's range returns zeros, so an
// invalid lane simply gets the offset X3_OOB -- no exec-mask branch around the load, no `valid ? loaded : 0` select after it
// (a use of the loaded value: the compiler then waits out the load latency on the spot, before the MFMAs of the k-step) and
// no copy out of a conditionally loaded register (same effect).  The loads of a k-step are issued back to back and are
// waited for where the LDS-staging step reads them.  Offsets are bytes from the stager's base pointer (< 2^31).
constexpr unsigned X3_OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x3_rsrc(const float* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
__device__ __forceinline__ float4 x3_load16(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}
__device__ __forceinline__ float2 x3_load8(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
}

// ---------------------------------------------------------------------------
// Stagers: Regs, gload(kt, regs, tid), sstore(regs, image, tid), row_off(r)
// ---------------------------------------------------------------------------
// Dead rows / columns of an image may hold anything: they only feed outputs that are never stored.  Indices
// past the contraction range must read as zero.

// k-major fp32 operand: element (k, c) = base[k * ldk + c]; tile rows are the 128 columns c (pairs 2t, 2t+1
// per lane t), valid for k_lo <= k < k_hi and c < cvalid (cvalid even).
struct TransStager {
    const float* base;
    long long ldk;
    int k_lo, k_hi, cvalid;
    typedef float2 Regs[8];
    static __device__ __forceinline__ int row_off(int r) { return pair_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const int w = tid >> 6, c = (tid & 63) * 2;
        const int k0 = kt * XK + w * 8;
        // the descriptor is rebased to the first row of the k-step (a 64-bit pointer), so the 32-bit offsets only span the
        // 32 rows of the step: operands of any size (k-major Fourier rows of a large batch pass 2^31 bytes: 721 x 241 x 384
        // channels x 8 B = 534 MB per sample) stay addressable; the launchers require 32 * ldk * 4 < 2^31
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(base + (long long)kt * XK * ldk);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + i;
            const bool ok = k >= k_lo && k < k_hi && c < cvalid;
            r[i] = x3_load8(rs, ok ? (unsigned)(((long long)(w * 8 + i) * ldk + c) * 4) : X3_OOB);
        }
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const {
        const int w = tid >> 6, t = tid & 63;
        float a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[i] = r[i].x;
            b[i] = r[i].y;
        }
        split_store8(a, img + t * XPITCH + w * 16);
        split_store8(b, img + (t + 64) * XPITCH + 128 + w * 16);
    }
};

// Lane -> (row within the wave's 16 rows, 16-byte chunk) for loaders that give a row to four consecutive lanes
// (128 contiguous bytes of global memory per row).  ds_write_b128 is serviced in groups of 8 consecutive lanes on
// 32 banks: the two rows of a group must lie 4 rows (4 * 52 = 16 banks mod 32) apart, not 1 (20 banks: the first
// chunk of the second row lands on the banks of the last chunk of the first -- measured as 33 % LDS conflict cycles
// in dhconv_dgrad, `profiles/r01_pmc_util.json`).
__device__ __forceinline__ int quad_row(int lane) { return ((lane >> 3) & 3) + 8 * (lane >> 5) + 4 * ((lane >> 2) & 1); }

// The "row, 8 k per quarter-wave task" image: two (row, 8 k) tasks per thread, each two float4 of one row, stored into the
// plain layout.  ROWS::live(row, rows) tells whether tile row `row` is within the stager's limit `rows` (dead rows are skipped).
struct RowsBelow {
    static __device__ __forceinline__ bool live(int row, int rows) { return row < rows; }
};
template <class ROWS = RowsBelow>
__device__ __forceinline__ void row8_sstore(const float4 (&r)[4], char* img, int tid, int rows) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int t = tid + q * XT, row = (t >> 6) * 16 + quad_row(t & 63);
        const float v[8] = {r[2 * q].x, r[2 * q].y, r[2 * q].z, r[2 * q].w, r[2 * q + 1].x, r[2 * q + 1].y, r[2 * q + 1].z, r[2 * q + 1].w};
        if (ROWS::live(row, rows)) split_store8(v, img + row * XPITCH + (t & 3) * 16);
    }
}

// Row-major fp32 A operand, k contiguous: element (r, k) = base[r * ld + k], rows < rows, k < kvalid
// (kvalid a multiple of 4, rows 16-byte aligned).
struct RowStager {
    const float* base;
    long long ld;
    int rows, kvalid;
    typedef float4 Regs[4];
    static __device__ __forceinline__ int row_off(int r) { return plain_off(r); }
    __device__ __forceinline__ void gload(int kt, Regs& r, int tid) const {
        const __amdgpu_buffer_rsrc_t rs = x3_rsrc(base);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = tid + q * XT, row = (t >> 6) * 16 + quad_row(t & 63), k = kt * XK + (t & 3) * 8;
            const unsigned off = (unsigned)(((long long)row * ld + k) * 4);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                r[2 * q + h] = x3_load16(rs, (row < rows && k + 4 * h < kvalid) ? off + 16 * h : X3_OOB);
        }
    }
    __device__ __forceinline__ void sstore(const Regs& r, char* img, int tid) const { row8_sstore(r, img, tid, rows); }
};

// One k-step (2 x k16) of a wave's 64 x 64 sub-tile from the LDS images: six piece products, smallest first,
// alternating between the two accumulators of a 32-row band.  A band whose rows are all past the valid
// extent gets no MFMA work (wave-uniform test).
__device__ __forceinline__ void x3_mfma_step(const char* As, const char* Bs, const int (&a_off)[2], const int (&b_off)[2],
                                             const bool (&live)[2], f32x16 (&acc)[2][2]) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        bf16x8 bf[2][3];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int p = 0; p < 3; ++p) bf[b][p] = *reinterpret_cast<const bf16x8*>(Bs + b_off[b] + p * 64 + s * 32);
#pragma unroll
        for (int a = 0; a < 2; ++a)
            if (live[a]) {
                bf16x8 af[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) af[p] = *reinterpret_cast<const bf16x8*>(As + a_off[a] + p * 64 + s * 32);
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[t]], bf[b][PB[t]], acc[a][b], 0, 0, 0);
            }
    }
}

// ---------------------------------------------------------------------------
// The tile: C[128 x 128] (+)= A * B over k-steps [kt0, kt1)
// ---------------------------------------------------------------------------
// Accumulator (a, b) of wave (wr, wc) holds rows wr*64 + a*32 + [0,32) and the columns of parity b of
// wc*64 + [0,64) (column 2j + b in MFMA column j), so a lane owns adjacent column pairs and the epilogue
// writes 8-byte values, 256 B per row and wave.
// C/D map of an accumulator: col = lane & 31 (fi), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (kg).
// Both operands are prefetched one k-step ahead into registers.
// EPI is the epilogue, a struct next to the kernel family that needs it (the shared ones follow below):
//   store(acc, wr, wc, fi, kg, rvalid, cvalid)   writes the wave's part of the tile, its pointers are the struct's fields
//   PAIRED_BANDS                                 false: a 32-row band is live while it has a row below rvalid;  true: the two
//                                                bands of a wave are two halves of the same outputs and live together
// `exp`: ablation switches (MK_X3_EXP): 1 no prefetch loads, 2 no staging stores, 4 no MFMAs, 8 / 16 no A / B prefetch -- wrong results
template <class AS, class BS, class EPI>
__device__ __forceinline__ void x3_tile(const AS& as, const BS& bs, int kt0, int kt1, int rvalid, int cvalid, EPI epi,
                                        char* lds, int exp = 0) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: liveness tests stay scalar
    const int wr = wave >> 1, wc = wave & 1;
    const int fi = lane & 31, kg = lane >> 5;
    char* As = lds;
    char* Bs = lds + XIMG;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // The accumulators live in the AccVGPR half of the register file (the empty asm makes the compiler select the AGPR form
    // of the MFMAs, as the vendor GEMM libraries do).  With arch-VGPR accumulators this kernel corrupted LDS-exchange kernels
    // that shared its CUs -- rocFFT's and this package's FFT rows, 16 lanes x one register at a time -- whenever another stream
    // or another process ran them at the same moment (tools/ab/share_stress.py torch_fft@mk_dhconv: 300 of 300 rocFFT results
    // wrong next to the VGPR form, 0 of 300 next to this one; profiles/r03_share_stress.txt).
    asm volatile("" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]));

    bool live[2];
    int a_off[2], b_off[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        a_off[a] = AS::row_off(wr * 64 + a * 32 + fi) + kg * 16;
        b_off[a] = BS::row_off(wc * 64 + 2 * fi + a) + kg * 16;
        if constexpr (EPI::PAIRED_BANDS) live[a] = (wr * 32 < rvalid) && (wc * 64 < cvalid);
        else live[a] = (wr * 64 + a * 32 < rvalid) && (wc * 64 < cvalid);
    }

    typename AS::Regs ra;
    typename BS::Regs rb;
    // Loop shape: an outer loop over k-steps around an unrolled inner loop of ONE step with its own end test.  It is what is
    // left of the register ring (depth 1: no ring registers, no depth parameter) and is kept on purpose: written as a plain
    // `for (kt = kt0; kt < kt1; ++kt)` the same statements compile to another register allocation (one or two more
    // VGPR -> AGPR copies per k-step) that measured 1.7 % slower in the Legendre kernels at 721 latitudes and 2.2 % in the
    // dhconv data gradient.
    if (kt0 < kt1) {
        as.gload(kt0, ra, tid);
        bs.gload(kt0, rb, tid);
        as.sstore(ra, As, tid);
        bs.sstore(rb, Bs, tid);
        __syncthreads();
        if (kt0 + 1 < kt1) as.gload(kt0 + 1, ra, tid);
#pragma unroll
        for (int j = 0; j < 1; ++j)
            if (kt0 + 1 + j < kt1) bs.gload(kt0 + 1 + j, rb, tid);
    }
    for (int ktb = kt0; ktb < kt1; ktb += 1) {
#pragma unroll
        for (int j = 0; j < 1; ++j) {   // the registers hold k-step kt + 1
            const int kt = ktb + j;
            if (kt >= kt1) break;
            if (!(exp & 4)) x3_mfma_step(As, Bs, a_off, b_off, live, acc);
            if (kt + 1 < kt1) {
                __syncthreads();
                if (!(exp & 2)) {
                    as.sstore(ra, As, tid);
                    bs.sstore(rb, Bs, tid);
                }
                __syncthreads();
                if (!(exp & 1)) {
                    if (kt + 2 < kt1 && !(exp & 8)) as.gload(kt + 2, ra, tid);
                    if (kt + 1 + 1 < kt1 && !(exp & 16)) bs.gload(kt + 1 + 1, rb, tid);
                }
            }
        }
    }
    epi.store(acc, wr, wc, fi, kg, rvalid, cvalid);
}

// Epilogues of more than one family.  cbase points at the tile's first element, ldc is the row pitch in floats.

// C = tile.  Nontemporal: the streamed output does not push the re-used panels (Legendre tile images, dhconv operands)
// out of L2.  Isolated launches, same box: Legendre 0.120 / 0.107 -> 0.109 / 0.094 ms at 240 latitudes,
// 0.288 / 0.289 -> 0.283 / 0.272 at 721; dhconv wgrad 0.211 -> 0.203; dhconv forward / dgrad unchanged.
// (Nontemporal LOADS of the streamed operand were measured too: 8-13 % slower.)
struct StoreEpi {
    float* cbase;
    long long ldc;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        x3_f2 v2;
                        v2[0] = acc[a][0][r];
                        v2[1] = acc[a][1][r];
                        __builtin_nontemporal_store(v2, reinterpret_cast<x3_f2*>(cbase + (long long)row * ldc + col));
                    }
                }
        }
    }
};

// C += tile: read-modify-write by the one workgroup that owns the tile
struct AccumulateEpi {
    float* cbase;
    long long ldc;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        float2* d = reinterpret_cast<float2*>(cbase + (long long)row * ldc + col);
                        const float2 o = *d;
                        *d = make_float2(o.x + acc[a][0][r], o.y + acc[a][1][r]);
                    }
                }
        }
    }
};

// C += tile with fp32 atomics: several workgroups contract disjoint k ranges into one tile (cvalid may be odd)
struct AtomicEpi {
    float* cbase;
    long long ldc;
    static constexpr bool PAIRED_BANDS = false;
    __device__ __forceinline__ void store(const f32x16 (&acc)[2][2], int wr, int wc, int fi, int kg, int rvalid, int cvalid) const {
        const int col = wc * 64 + 2 * fi;
        if (col < cvalid) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (row < rvalid) {
                        atomicAdd(cbase + (long long)row * ldc + col, acc[a][0][r]);
                        if (col + 1 < cvalid) atomicAdd(cbase + (long long)row * ldc + col + 1, acc[a][1][r]);
                    }
                }
        }
    }
};

// block -> (batch, tile_m, tile_n) by tile_map.h, and the grid it expects
using mk::decode_block;
using mk::TileId;
[[maybe_unused]] inline long long grid_blocks(int nbatch, int tiles_m, int tiles_n) {
    return (long long)mk::ceil_div(nbatch, 8) * 8 * tiles_m * tiles_n;
}

[[maybe_unused]] inline int x3_exp() {
    static const int v = [] { const char* e = getenv("MK_X3_EXP"); return e ? atoi(e) : 0; }();
    return v;
}

// Launch an engine kernel on `nblk` workgroups (grid_blocks): the grid-size check, the launch and the launch check, reported
// under the name `who` of the calling entry point.
template <class P>
int x3_launch(const char* who, void (*kernel)(P), long long nblk, void* stream, const P& p) {
    MK_REQUIRE_AS(who, nblk < 2147483647LL, "grid too large");
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(XT), X3_LDS, (hipStream_t)stream, p);
    MK_LAUNCH_CHECK_AS(who);
    return 0;
}

}  // namespace
