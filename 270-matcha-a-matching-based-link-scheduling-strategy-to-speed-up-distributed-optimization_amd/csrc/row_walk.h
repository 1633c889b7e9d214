// row_walk.h -- what the row kernels share (mix_kernel_rows in mix.hip, mix_bf16_rows in mix_bf16.hip,
// fused_round_rows in fused_round.h): the round's plan record in LDS, the dealing of a staged tile's
// (row, pass) items to the waves, and the partner walk over the tile.  A kernel keeps what is its own --
// how a tile gets into LDS, which rows it deals, a row's degree, and what happens to a finished chain --
// and hands the last three in as callables.  Everything here is inlined; nothing is decided at run time
// that the kernels did not decide before.
//
// The FMA chain of a row is the reference's: partners in ascending matching order, every step one
// __builtin_fmaf in fp32; the kernel's `finish` adds the self term last.
#pragma once
#include "mx_common.h"

namespace mx {
namespace rows {

constexpr int kMaxM = 32;            // matchings a plan record in LDS holds

// the round's plan record (mx_plan_build): header, degrees, self weights, then kMaxM partner slots a row
template <int NS>
struct PlanLds {
    int32_t w[mx::kPlanHeader + 2 * NS + NS * kMaxM];
};

#if defined(__HIPCC__)
typedef float F4 __attribute__((ext_vector_type(4)));         // 4 fp32: one 16-byte access
typedef uint32_t U4 __attribute__((ext_vector_type(4)));      // 8 bf16: one 16-byte access

// Row pointers arrive as generic pointers; accessing them through the global address space makes
// the compiler emit global_load/store (counted on vmcnt only) instead of flat_* (counted on vmcnt
// AND lgkmcnt, so every LDS or scalar-load wait in the loop would also drain the HBM stream).
template <typename T>
using GPtr = __attribute__((address_space(1))) T*;

// 16-byte accesses are legal at row + 4i when the row pointer itself is 16-byte aligned: a scalar
// test of the (wave-uniform) pointer, where the per-segment seg_vec byte would be a vector-memory
// load -- a full round trip at the head of every workgroup before its first tile load
__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// one bf16 element (the tails of a row, and rows that are not aligned)
__device__ __forceinline__ uint32_t ld2(const uint16_t* p) { return *(GPtr<const uint16_t>)(p); }
__device__ __forceinline__ void st2(uint16_t* p, uint32_t v) { *(GPtr<uint16_t>)(p) = (uint16_t)v; }

// The round to mix: `iter`, or with iter_dev (graph-replayable launches) the device counter
// *iter_dev, `iter` then being the schedule length; outside [0, length) the launch is a no-op.
__device__ __forceinline__ int64_t round_of(int64_t iter, const int64_t* iter_dev) {
    if (!iter_dev) return iter;
    const int64_t v = *iter_dev;
    return (v >= 0 && v < iter) ? v : -1;
}

// round `iter`'s record into LDS, by the whole workgroup, and the barrier after it.  TPB is the workgroup
// size where the caller knows it at compile time (the fused kernel); 0 reads blockDim.x, for mix.hip's and
// mix_bf16.hip's load_plan, which serve kernels launched with 256, 512 and 1024 threads.  The two steps
// differ in more than a constant: `i += blockDim.x` is an unsigned add, and turning it into a signed one
// made the compiler widen the loop's induction variable (some 60 instructions more per kernel).
template <int NS, int TPB = 0>
__device__ __forceinline__ void copy_plan(PlanLds<NS>& sp, const int32_t* plan, int64_t iter, int n_local, int M) {
    const int64_t W = mx::plan_words(n_local, M);
    const int32_t* rec = plan + iter * W;
    for (int i = threadIdx.x; i < W;) {
        sp.w[i] = rec[i];
        if constexpr (TPB > 0) i += TPB;
        else i += blockDim.x;
    }
    __syncthreads();
}

// the copied record's tables: deg[r], sw[r] (the self weight) and row r's partner slots src[r * M + e]
struct Plan {
    const int32_t* deg;
    const float* sw;
    const int32_t* src;
};
template <int NS>
__device__ __forceinline__ Plan view(const PlanLds<NS>& sp, int n_local) {
    const int32_t* deg = sp.w + mx::kPlanHeader;
    return {deg, reinterpret_cast<const float*>(deg + n_local), deg + 2 * n_local};
}
// the mask of local rows an active round reads and writes: degree > 0, or every row in idle mode 1
template <int NS>
__device__ __forceinline__ uint64_t local_need(const PlanLds<NS>& sp, int n_local) {
    const bool idle = (sp.w[2] & 1) != 0;
    const int32_t* deg = sp.w + mx::kPlanHeader;
    uint64_t need = 0;
    for (int r = 0; r < n_local; ++r)
        if (deg[r] > 0 || idle) need |= 1ull << r;
    return need;
}

// the two chunk types a tile is staged in: Acc the fp32 accumulator of one chunk, fma one chain step
__device__ __forceinline__ void fma4(F4& a, float w, const F4& x) {
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = __builtin_fmaf(w, x[t], a[t]);
}
// acc[0..7] = fmaf(w, f32(x[0..7]), acc[0..7]); f32() is the exact widening bits << 16
__device__ __forceinline__ void fma8(float (&a)[8], float w, const U4& x) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        a[2 * t] = __builtin_fmaf(w, __builtin_bit_cast(float, x[t] << 16), a[2 * t]);
        a[2 * t + 1] = __builtin_fmaf(w, __builtin_bit_cast(float, x[t] & 0xFFFF0000u), a[2 * t + 1]);
    }
}
struct Fp32 {
    using Chunk = F4;
    using Acc = F4;
    static __device__ __forceinline__ void zero(Acc& a) { a = F4{0.0f, 0.0f, 0.0f, 0.0f}; }
    static __device__ __forceinline__ void fma(Acc& a, float w, const Chunk& x) { fma4(a, w, x); }
};
struct Bf16 {
    using Chunk = U4;
    using Acc = float[8];
    static __device__ __forceinline__ void zero(Acc& a) {
#pragma unroll
        for (int t = 0; t < 8; ++t) a[t] = 0.0f;
    }
    static __device__ __forceinline__ void fma(Acc& a, float w, const Chunk& x) { fma8(a, w, x); }
};

// Wave 0 deals the items (row r, pass q) = r * NQ + q of a tile to the WV waves: lane i ranks item i by
// weight_of(row) (degree + 1, or 0 for a row that is not dealt), heaviest first, and the ranks go to the
// waves in snake order.  wl[wave] then lists the wave's items, the unused entries -1.
template <int NQ, int NI, int WV, class Weight>
__device__ __forceinline__ void deal(int32_t (&wl)[WV][NI / WV], int lane, const Weight& weight_of) {
    const int w = lane < NI ? weight_of(lane / NQ) : 0;
    int rank = 0;
    for (int j = 0; j < NI; ++j) {
        const int wj = __builtin_amdgcn_readlane(w, j);
        rank += (wj > w) || (wj == w && j < lane);
    }
    const int round = rank / WV, within = rank % WV;
    if (lane < NI) wl[(round & 1) ? WV - 1 - within : within][round] = w > 0 ? lane : -1;
}

// a wave's items: ranks grow along its list, so the unused (-1) entries form a suffix (wave-uniform)
template <int N>
__device__ __forceinline__ int count(const int32_t (&list)[N]) {
    int n = 0;
    while (n < N && list[n] >= 0) ++n;
    return __builtin_amdgcn_readfirstlane(n);
}

// The partner walk of one wave over the tile staged in `lds` (CW chunks a row, NQ passes of 64 chunks):
// its items two at a time, interleaved up to the smaller degree for ILP, then the two tails, then
// finish(item, acc) of both; an odd last item alone.  degree_of(row) is the number of partners walked.
template <class Ops, int NQ, int CW, int N, class Degree, class Finish>
__device__ __forceinline__ void walk(const typename Ops::Chunk* lds, const int32_t (&list)[N], int nmy, int lane,
                                     const int32_t* src, int M, float alpha, const Degree& degree_of,
                                     const Finish& finish) {
    using Chunk = typename Ops::Chunk;
    int p = 0;
    for (; p + 1 < nmy; p += 2) {            // two items interleaved
        const int ia = __builtin_amdgcn_readfirstlane(list[p]);
        const int ib = __builtin_amdgcn_readfirstlane(list[p + 1]);
        const int ra = ia / NQ, rb = ib / NQ;
        const int ca = (ia % NQ) * 64 + lane, cb = (ib % NQ) * 64 + lane;
        const int da = degree_of(ra), db = degree_of(rb);
        const int dmin = da < db ? da : db;
        typename Ops::Acc a, b;
        Ops::zero(a);
        Ops::zero(b);
        int e = 0;
        for (; e < dmin; ++e) {
            const int sa = __builtin_amdgcn_readfirstlane(src[ra * M + e]);
            const int sb = __builtin_amdgcn_readfirstlane(src[rb * M + e]);
            const Chunk xa = lds[sa * CW + ca];
            const Chunk xb = lds[sb * CW + cb];
            Ops::fma(a, alpha, xa);
            Ops::fma(b, alpha, xb);
        }
        for (int ea = e; ea < da; ++ea)
            Ops::fma(a, alpha, lds[__builtin_amdgcn_readfirstlane(src[ra * M + ea]) * CW + ca]);
        for (int eb = e; eb < db; ++eb)
            Ops::fma(b, alpha, lds[__builtin_amdgcn_readfirstlane(src[rb * M + eb]) * CW + cb]);
        finish(ia, a);
        finish(ib, b);
    }
    if (p < nmy) {
        const int ia = __builtin_amdgcn_readfirstlane(list[p]);
        const int ra = ia / NQ, ca = (ia % NQ) * 64 + lane;
        const int da = degree_of(ra);
        typename Ops::Acc a;
        Ops::zero(a);
        for (int e = 0; e < da; ++e)
            Ops::fma(a, alpha, lds[__builtin_amdgcn_readfirstlane(src[ra * M + e]) * CW + ca]);
        finish(ia, a);
    }
}
#endif  // __HIPCC__

}  // namespace rows
}  // namespace mx
