// mx_common.h -- shared helpers for the gfx950 gossip library (error plumbing, launch math).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/matcha_gossip.h"

namespace mx {

// thread-local last-error text, surfaced through mx_last_error()
void set_error(const char* fmt, ...);

#define MX_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            ::mx::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return MX_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

#define MX_CHECK(cond, ...)                                                                 \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            ::mx::set_error(__VA_ARGS__);                                                   \
            return MX_ERR_INVALID;                                                          \
        }                                                                                   \
    } while (0)

#define MX_LAUNCH_CHECK()                                                                   \
    do {                                                                                    \
        hipError_t e_ = hipGetLastError();                                                  \
        if (e_ != hipSuccess) {                                                             \
            ::mx::set_error("%s:%d launch -> %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return MX_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// compute units of the current device (256 when it cannot be asked)
int cu_count();

// mx_*_layout: the prefix of the segments' tile counts, tile_off[s + 1] = tile_off[s] + ceil(len[s] / tile);
// `who` names the entry point in the error text (the caller has checked the pointers, nseg and tile > 0)
int tile_prefix(const char* who, int tile, const int64_t* seg_len_host, int nseg, int64_t* tile_off_host);

// Plan record geometry (see include/matcha_gossip.h, mx_plan_build)
constexpr int kPlanHeader = 4;
__host__ __device__ inline int64_t plan_words(int n_local, int M) {
    return (int64_t)kPlanHeader + 2 * (int64_t)n_local + (int64_t)n_local * M;
}

// LDS per CU (device attribute; 160 KB on gfx950) and the dynamic LDS that, on top of a kernel's
// static_bytes, admits exactly wg_per_cu of its workgroups per CU: the per-workgroup total sits in
// the middle of that count's window, so allocation rounding cannot tip it into the next count
// (0 when no padding is needed or wg_per_cu <= 0).  Streaming kernels whose every load is issued
// at once run fastest with few tiles in flight per CU (tools/occ_sweep.py, tools/mean_ab.py).
int lds_per_cu();
size_t lds_cap_pad(int static_bytes, int wg_per_cu);
extern int g_mean_wgpc;   // mean_tile_kernel's workgroups per CU on large rounds (mx_mix_set "mean_wgpc")

// Store policy of the streaming kernels' 16-byte row stores (mx_mix_set "store_policy"): when a
// written line leaves the XCD's write-back L2.  nt keeps the line dirty in L2 until it is evicted;
// the sc1 forms write it through and drop it.  No policy changes a bit: no kernel re-reads what it
// wrote and the kernel boundary publishes every store.  Only whole 16-byte stores take a policy --
// element tails and misaligned rows keep their ordinary stores (narrow write-through stores cost
// several times more per byte).
enum StorePolicy { kStorePlain = 0, kStoreNt = 1, kStoreSc1 = 2, kStoreSc1Nt = 3, kStoreSc0Sc1 = 4 };
constexpr int kStorePolicyMax = kStoreSc0Sc1;
// the policy "store_policy" = 0 (auto) gives rounds of more than kStoreAutoBytes that stream with
// non-temporal hints; smaller rounds (rows found again in the L2s or the Infinity Cache by the
// next round) always keep nt.  sc1 nt: the fastest policy of the row kernel and the mean on
// every streamed shape (8 x 25.6M: 0.2616 -> 0.2565 ms, 8 x 36.5M: 0.3725 -> 0.3673 ms,
// 8 x 14.8M: 0.1549 -> 0.1533 ms, mean 8 x 25.6M: 0.2629 -> 0.2584 ms; sc1 and sc0 sc1 in
// between; tools/store_policy_ab.py, profiles/store_policy_ab.json)
constexpr int kStoreAutoPolicy = kStoreSc1Nt;
extern int g_store_policy;   // 0 = auto, 1..kStorePolicyMax = that policy at every size

// The working-set rules every streaming launch shares (each caller brings its own byte count and its
// own auto policy).  Rounds of kCachedLoBytes..kCachedHiBytes, about the 256 MB Infinity Cache, keep
// ordinary (cacheable) accesses: back-to-back rounds then find their rows on die.  Above, and below
// where the rows fit in the L2s, the streaming hints win (figures at mix.hip's choose()).
constexpr int64_t kCachedLoBytes = (int64_t)32 << 20;
constexpr int64_t kCachedHiBytes = (int64_t)320 << 20;
constexpr int64_t kStoreAutoBytes = kCachedHiBytes;
inline bool streams(int64_t ws) { return ws <= kCachedLoBytes || ws > kCachedHiBytes; }
// the store policy of a streaming launch: forced, else above kStoreAutoBytes the caller's auto policy, else nt
inline int store_policy_of(int forced, int64_t ws, int auto_policy) {
    return forced > 0 ? forced : ws > kStoreAutoBytes ? auto_policy : (int)kStoreNt;
}

// A knob of an mx_*_set / mx_*_get pair: its key, where it lives and what it accepts.  knob_set
// stores an accepted value (normalised: kBool to 0 / 1, kTri to 0 / 1 with 2 kept) or refuses with
// "<who>: <key> <value>" and leaves the knob alone; both report "<who>: unknown key '<key>'".  A
// read-only knob is unknown to knob_set.
struct Knob {
    enum Kind { kRange, kOneOf, kBool, kTri };
    const char* key;
    int* slot;
    Kind kind;
    int v[4];          // kRange: [v[0], v[1]]; kOneOf: the accepted values (the last one repeated)
    bool read_only;
};
inline Knob knob_range(const char* key, int* slot, int lo, int hi) { return {key, slot, Knob::kRange, {lo, hi, 0, 0}, false}; }
inline Knob knob_one_of(const char* key, int* slot, int a, int b, int c, int d) {
    return {key, slot, Knob::kOneOf, {a, b, c, d}, false};
}
inline Knob knob_bool(const char* key, int* slot) { return {key, slot, Knob::kBool, {0, 0, 0, 0}, false}; }
inline Knob knob_tri(const char* key, int* slot) { return {key, slot, Knob::kTri, {0, 0, 0, 0}, false}; }
inline Knob knob_read_only(const char* key, int* slot) { return {key, slot, Knob::kRange, {0, 0, 0, 0}, true}; }
int knob_set(const char* who, const Knob* table, int n, const char* key, int value);
int knob_get(const char* who, const Knob* table, int n, const char* key);

#if defined(__HIPCC__)
// One 16-byte store to global memory under policy SP.  The write-through forms have no builtin on
// a plain pointer, so they are inline asm: the compiler does not count such a store on vmcnt (its
// later waits can only wait longer), and the trailing s_nop keeps its next instruction from
// overwriting the data registers before the store has read them.
template <int SP, typename F4>
__device__ __forceinline__ void store16(F4* p, const F4& v) {
    static_assert(sizeof(F4) == 16, "store16 takes 16-byte vectors");
    typedef __attribute__((address_space(1))) F4* G;
    const G g = (G)(p);
    if constexpr (SP == kStoreSc1)
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(g), "v"(v) : "memory");
    else if constexpr (SP == kStoreSc1Nt)
        asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(g), "v"(v) : "memory");
    else if constexpr (SP == kStoreSc0Sc1)
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(g), "v"(v) : "memory");
    else if constexpr (SP == kStoreNt)
        __builtin_nontemporal_store(v, g);
    else
        *g = v;
}
#endif

// numpy legacy_random_binomial(n=1) parameters, computed on the host with glibc libm exactly
// as numpy's legacy_random_binomial_inversion does (see flags.hip).
struct BinomParam {
    double qn;   // exp(1 * log(q)),   q = 1 - pp
    double px1;  // ((1 * pp) * qn) / (1 * q)
    int flip;    // p > 0.5: result is 1 - X
    int pad;
};

}  // namespace mx
