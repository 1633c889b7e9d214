// choco_quant.h -- what the two-launch quantized round (choco_quant.hip) and the one-launch round
// (choco_quant_round.hip) share: the quantizer's constants, its hash, the bucket norm's butterfly, a lane's pass
// and the decode of one code.  The specification is at the head of choco_quant.hip.  Both files give every lane
// the same columns and add in the same order, so a norm is the same bits whichever of them computed it.
#pragma once
#include "choco_sign.h"

namespace mx {
namespace choco {

// host side, defined in choco_quant_round.hip and set through mx_choco_quant_set: the one-launch round's
// persistent grid in workgroups per CU (capped by the tiles), and with a value > 0 its exact size
extern int g_quant_round_blocks_per_cu, g_quant_round_grid;

namespace quant {
using namespace mx::choco::sign;    // the geometry, ld4 / st4 / ld1, row_up; GPtr, al16, F4

constexpr int kBucket = kPass;                 // 256 columns: what a wave covers in one pass

template <int BITS>
struct Lv {
    static_assert(BITS == 4 || BITS == 8, "4 or 8 bits");
    static constexpr int s = (1 << (BITS - 1)) - 1;
    static constexpr double a = (double)kBucket / ((double)s * s), b = 16.0 / s;     // sqrt(256) = 16
    static constexpr double tau = 1.0 + (a < b ? a : b);
    static constexpr float c = (float)(1.0 / (s * tau));
};

__host__ __device__ inline uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

__host__ __device__ inline int64_t n_buckets(int64_t P) { return (P + kBucket - 1) / kBucket; }
__host__ __device__ inline int64_t codes_off(int64_t P) { return kHeader + 64 * n_items(P); }

#if defined(__HIPCC__)
// the value of lane L' of the wave for every lane L, L' = L ^ 1, L ^ 2 (quad_perm), 7 - L within 8 lanes
// (row_half_mirror), 15 - L within 16 (row_mirror)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// Butterfly: every lane ends with the same bits.  After a step all lanes of a group hold the group's sum, so a
// mirror pairs two groups as an xor would; a + b is b + a.
__device__ __forceinline__ double wave_sum(double s) {
    s = __dadd_rn(s, dpp_f64<0xB1>(s));         // quad_perm:[1,0,3,2]
    s = __dadd_rn(s, dpp_f64<0x4E>(s));         // quad_perm:[2,3,0,1]
    s = __dadd_rn(s, dpp_f64<0x141>(s));        // row_half_mirror
    s = __dadd_rn(s, dpp_f64<0x140>(s));        // row_mirror
    s = __dadd_rn(s, __shfl_xor(s, 16, 64));
    s = __dadd_rn(s, __shfl_xor(s, 32, 64));
    return s;
}

// One pass of a lane: its bucket's norm (wave-uniform) and the codes of its 4 columns, column t in bits
// [BITS t, BITS t + BITS).  kc = key + u32(the lane's first column).
template <int BITS>
__device__ __forceinline__ uint32_t quant_pass(const float (&d)[4], uint32_t kc, float& norm) {
    constexpr float sf = (float)Lv<BITS>::s;
    double acc = __dmul_rn((double)d[0], (double)d[0]);              // the widening and the product are exact
#pragma unroll
    for (int t = 1; t < 4; ++t) acc = __dadd_rn(acc, __dmul_rn((double)d[t], (double)d[t]));
    norm = (float)__builtin_sqrt(wave_sum(acc));
    const float inv = norm == 0.0f ? 0.0f : sf / norm;
    uint32_t w = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float xi = __fmul_rn((float)(mix32(kc + (uint32_t)t) >> 8), 0x1p-24f);
        const float v = __fadd_rn(__fmul_rn(__builtin_fabsf(d[t]), inv), xi);
        // floor(min(v, s)) = min(floor(v), s); the guard also keeps a NaN v (fminf would give s) at level 0
        const uint32_t level = v >= 1.0f ? (uint32_t)(int)__builtin_fminf(v, sf) : 0u;
        const uint32_t neg = d[t] < 0.0f ? 1u : 0u;                  // false for +0, -0 and NaN
        w |= ((neg << (BITS - 1)) | level) << (BITS * t);
    }
    return w;
}

// one decoded element of a message: s += w q, and for the row's own message x_hat += q
template <int BITS, bool OWN>
__device__ __forceinline__ void upd(float& sv, float& hv, float w, float unit, uint32_t code) {
    const float mag = __fmul_rn((float)(code & (uint32_t)Lv<BITS>::s), unit);
    const float q = __uint_as_float(__float_as_uint(mag) ^ ((code >> (BITS - 1) & 1u) << 31));
    sv = __fadd_rn(sv, __fmul_rn(w, q));
    if constexpr (OWN) hv = __fadd_rn(hv, q);
}
#endif

}  // namespace quant
}  // namespace choco
}  // namespace mx
