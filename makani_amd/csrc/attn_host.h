// The host half that attn.hip (bf16) and x3_attn.hip (fp32 on bf16x3) share: the parameter block of their kernels, the
// validation of sizes, operands and strides, and the filling of the block for the four launches.  What a family adds is its
// element type, its `Family` (largest head size, stride unit) and the choice of kernel.
#pragma once
#include "common.h"

#include <string>

namespace mk::attn {

constexpr int kOwn = 128;               // tokens a workgroup owns (32 per wave)
constexpr float kLog2e = 1.4426950408889634f;

struct Str { long long b, h, n; };      // element strides of batch, head, token; the D axis is contiguous
inline Str str_at(const long long* st, int i) { return Str{st[3 * i], st[3 * i + 1], st[3 * i + 2]}; }

// The layout of a kernel's parameter block.  Each file derives its own `Params` from it: the kernels' symbols carry that name.
template <class T>
struct ParamsOf {
    const T *q, *k, *v, *dO;
    T *o, *dq, *dk, *dv;
    float* lse_out;                 // fwd: may be null;  delta kernel: the delta buffer
    const float *lse, *delta;       // bwd
    int B, H, Nq, Nk, D, ntile;     // ntile: owned tiles per (batch, head)
    Str sq, sk, sv, so, sdo, sdq, sdk, sdv;
    float scale, c;                 // c = scale log2(e)
};

struct Family {
    int max_head;                   // head sizes are the multiples of 16 in 16 ... max_head
    int unit;                       // elements in 16 bytes: every stride is a multiple of it
};

inline int check_head(const char* who, const Family& f, int D) {
    MK_REQUIRE_AS(who, D >= 16 && D <= f.max_head && D % 16 == 0,
                  "head size must be a multiple of 16 in 16 ... " + std::to_string(f.max_head));
    return 0;
}
// "too many rows" also bounds the grid: a (batch, head) has no more owned tiles than tokens.
inline int check_sizes(const char* who, const Family& f, int B, int H, int Nq, int Nk, int D) {
    MK_REQUIRE_AS(who, B >= 1 && H >= 1 && Nq >= 1 && Nk >= 1, "bad sizes");
    if (int rc = check_head(who, f, D)) return rc;
    MK_REQUIRE_AS(who, (double)B * H * (Nq > Nk ? Nq : Nk) < 2147483647.0, "too many rows");
    return 0;
}
// n tensors, each a base pointer and (batch, head, token) element strides: multiples of the unit, rows do not overlap
inline int check_operands(const char* who, const Family& f, int n, const void* const* ptr, const long long* st, int D) {
    MK_REQUIRE_AS(who, st != nullptr, "null strides");
    for (int i = 0; i < n; ++i) {
        MK_REQUIRE_AS(who, ptr[i] != nullptr, "null pointer");
        MK_REQUIRE_AS(who, mk::aligned<16>(ptr[i]), "operand not 16-byte aligned");
        for (int j = 0; j < 3; ++j)
            MK_REQUIRE_AS(who, st[3 * i + j] >= 0 && st[3 * i + j] % f.unit == 0,
                          "strides must be non-negative multiples of " + std::to_string(f.unit) + " elements");
        MK_REQUIRE_AS(who, st[3 * i + 2] >= D, "token stride smaller than the head size");
    }
    return 0;
}

// What the three tiled launches share: the checks of sizes and of the n operands, then sizes, tiling (`owned` is the token
// count that is tiled), the strides of q, k, v and the scale.  `p` is value-initialised by the caller; 0, or the refusal's code.
template <class T>
int tiled_params(const char* who, const Family& f, ParamsOf<T>& p, int n, const void* const* ptr, int B, int H, int Nq, int Nk, int D,
                 int owned, const long long* st, float scale) {
    if (int rc = check_sizes(who, f, B, H, Nq, Nk, D)) return rc;
    if (int rc = check_operands(who, f, n, ptr, st, D)) return rc;
    p.B = B, p.H = H, p.Nq = Nq, p.Nk = Nk, p.D = D, p.ntile = mk::ceil_div(owned, kOwn);
    p.sq = str_at(st, 0), p.sk = str_at(st, 1), p.sv = str_at(st, 2);
    p.scale = scale, p.c = scale * kLog2e;
    return 0;
}
template <class T>
dim3 tile_grid(const ParamsOf<T>& p) { return dim3((unsigned)((long long)p.ntile * p.H * p.B)); }

// The four routines behind the entry points: validate, then fill `p`.
template <class T>
int fwd_params(const char* who, const Family& f, ParamsOf<T>& p, const T* q, const T* k, const T* v, T* o, float* lse, int B, int H,
               int Nq, int Nk, int D, const long long* st, float scale) {
    const void* ptr[4] = {q, k, v, o};
    if (int rc = tiled_params(who, f, p, 4, ptr, B, H, Nq, Nk, D, Nq, st, scale)) return rc;
    MK_REQUIRE_AS(who, mk::aligned<4>(lse), "lse not 4-byte aligned");
    p.q = q, p.k = k, p.v = v, p.o = o, p.lse_out = lse, p.so = str_at(st, 3);
    return 0;
}

template <class T>
int delta_params(const char* who, const Family& f, ParamsOf<T>& p, const T* o, const T* dO, float* delta, int B, int H, int Nq, int D,
                 const long long* st) {
    if (int rc = check_sizes(who, f, B, H, Nq, 1, D)) return rc;
    const void* ptr[2] = {o, dO};
    if (int rc = check_operands(who, f, 2, ptr, st, D)) return rc;
    MK_REQUIRE_AS(who, delta != nullptr && mk::aligned<4>(delta), "delta null or not 4-byte aligned");
    p.o = const_cast<T*>(o), p.dO = dO, p.lse_out = delta;
    p.B = B, p.H = H, p.Nq = Nq, p.D = D;
    p.so = str_at(st, 0), p.sdo = str_at(st, 1);
    return 0;
}

template <class T>
int dkv_params(const char* who, const Family& f, ParamsOf<T>& p, const T* q, const T* k, const T* v, const T* dO, const float* lse,
               const float* delta, T* dk, T* dv, int B, int H, int Nq, int Nk, int D, const long long* st, float scale) {
    const void* ptr[6] = {q, k, v, dO, dk, dv};
    if (int rc = tiled_params(who, f, p, 6, ptr, B, H, Nq, Nk, D, Nk, st, scale)) return rc;
    MK_REQUIRE_AS(who, lse && delta && mk::aligned<4>(lse, delta), "lse / delta null or not 4-byte aligned");
    p.q = q, p.k = k, p.v = v, p.dO = dO, p.dk = dk, p.dv = dv, p.lse = lse, p.delta = delta;
    p.sdo = str_at(st, 3), p.sdk = str_at(st, 4), p.sdv = str_at(st, 5);
    return 0;
}

template <class T>
int dq_params(const char* who, const Family& f, ParamsOf<T>& p, const T* q, const T* k, const T* v, const T* dO, const float* lse,
              const float* delta, T* dq, int B, int H, int Nq, int Nk, int D, const long long* st, float scale) {
    const void* ptr[5] = {q, k, v, dO, dq};
    if (int rc = tiled_params(who, f, p, 5, ptr, B, H, Nq, Nk, D, Nq, st, scale)) return rc;
    MK_REQUIRE_AS(who, lse && delta && mk::aligned<4>(lse, delta), "lse / delta null or not 4-byte aligned");
    p.q = q, p.k = k, p.v = v, p.dO = dO, p.dq = dq, p.lse = lse, p.delta = delta;
    p.sdo = str_at(st, 3), p.sdq = str_at(st, 4);
    return 0;
}

}  // namespace mk::attn
