// Shared helpers for the libmakani_amd.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>

namespace mk {

void set_error(const std::string& msg);

// `who`: the function the message names (the _AS forms serve checks that several entry points share)
#define MK_REQUIRE_AS(who, cond, msg)                                             \
    do {                                                                          \
        if (!(cond)) {                                                            \
            ::mk::set_error(std::string(who) + ": " + (msg));                     \
            return 1;                                                             \
        }                                                                         \
    } while (0)
#define MK_REQUIRE(cond, msg) MK_REQUIRE_AS(__func__, cond, msg)

#define MK_LAUNCH_CHECK_AS(who)                                                   \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            ::mk::set_error(std::string(who) + ": " + hipGetErrorString(e__));    \
            return 2;                                                             \
        }                                                                         \
    } while (0)
#define MK_LAUNCH_CHECK() MK_LAUNCH_CHECK_AS(__func__)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline long long ceil_div_ll(long long a, long long b) { return (a + b - 1) / b; }

// Host-side pointer checks.  A null pointer counts as aligned: the checks of optional operands rely on that.
template <uintptr_t BYTES, class... P> inline bool aligned(const P*... p) {
    static_assert(BYTES && (BYTES & (BYTES - 1)) == 0, "a power of two");
    return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t{0}) & (BYTES - 1)) == 0;
}
// the run-time form, for sizes that depend on a dtype code (`bytes` a power of two); null counts as aligned here too
inline bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// Dynamic LDS above 64 KB has to be allowed per kernel AND per device: once for each (instantiation, device) pair, checked.
// `bytes` is applied by the first call for a pair and not looked at again: a kernel's callers pass one constant, the most
// its launches may ever ask for.
template <auto Kernel> int raise_lds_limit(int bytes) {
    static std::atomic<unsigned long long> done{0};      // one bit per device ordinal (< 64)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
    const unsigned long long bit = 1ULL << dev;
    if (done.load(std::memory_order_acquire) & bit) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

// compute units of the current device, asked once per device; 256 (an MI355X) where there is no device to ask
inline int cu_count() {
    static std::atomic<int> known[64];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return 256;
    }
    if ((n = known[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        return 256;
    }
    known[dev].store(n, std::memory_order_relaxed);
    return n;
}

}  // namespace mk
