// choco_sign.h -- what the scaled-sign compress pass (choco_sign.hip) and the SGD step fused into it
// (choco_sgd.hip) share: the geometry of a work item, the 16-byte accesses and a lane's pass (its sign bits
// packed, its |d| added).  Both kernels give every lane the same columns and add in the same order, so a row's
// scale is the same bits whichever of them computed it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_walk.h"

namespace mx {
namespace choco {

// host side, defined in choco_sign.hip: the persistent grid of a compress-shaped pass over `total` work
// items (mx_choco_sign_set "grid" / "blocks_per_cu"), and the sign_finish launch (one workgroup per row adds
// the row's partials in index order and writes the slot's header)
unsigned sign_grid(int64_t total);
int sign_finish_launch(const double* work, int64_t chunks, int64_t P, char* msgs, int64_t msg_ld_bytes, int nrows,
                       hipStream_t st);

namespace sign {
using namespace mx::rows;        // GPtr, al16, F4
constexpr int kTPB = 256;
constexpr int kWV = kTPB / 64;
constexpr int kItem = 4096;              // columns per work item = per workspace slot = per apply tile
constexpr int kPass = 64 * 4;            // columns a wave covers per pass
constexpr int kNP = kItem / kWV / kPass; // passes per wave: 4
constexpr int kHeader = 64;              // bytes of a slot before its bits
static_assert(kNP * kPass * kWV == kItem, "sign compress geometry");

__host__ __device__ inline int64_t n_items(int64_t P) { return (P + kItem - 1) / kItem; }
__host__ __device__ inline int64_t n_words(int64_t P) { return 2 * ((P + 63) / 64); }   // uint32 words of bits

#if defined(__HIPCC__)
template <bool NT>
__device__ __forceinline__ F4 ld4(const float* p) {
    if constexpr (NT) return __builtin_nontemporal_load((GPtr<const F4>)(p));
    else return *(GPtr<const F4>)(p);
}
template <bool NT>
__device__ __forceinline__ void st4(const F4& v, float* p) {
    if constexpr (NT) __builtin_nontemporal_store(v, (GPtr<F4>)(p));
    else *(GPtr<F4>)(p) = v;
}
__device__ __forceinline__ float ld1(const float* p) { return *(GPtr<const float>)(p); }

// the value of lane + N of the same 16-lane row (row_shl:N; zero past the row's end)
template <int N>
__device__ __forceinline__ uint32_t row_up(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + N, 0xf, 0xf, true);
}

// One pass of a lane: its 4 differences' magnitudes added in column order (returned), and the word of sign
// bits of the 32 columns that start at the lane's own (valid in lanes 0, 8, ... of the wave)
__device__ __forceinline__ double pass_of(const float (&d)[4], uint32_t& word) {
    double acc = 0.0;
    uint32_t v = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc += (double)__builtin_fabsf(d[t]);            // the widening is exact
        v |= (d[t] < 0.0f ? 1u : 0u) << t;               // false for +0, -0 and NaN
    }
    v |= row_up<1>(v) << 4;
    v |= row_up<2>(v) << 8;
    v |= row_up<4>(v) << 16;
    word = v;
    return acc;
}
#endif

}  // namespace sign
}  // namespace choco
}  // namespace mx
