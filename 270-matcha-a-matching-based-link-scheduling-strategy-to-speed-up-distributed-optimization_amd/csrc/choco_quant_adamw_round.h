// choco_quant_adamw_round.h -- the one-launch quantized ChocoSGD round with torch.optim.AdamW's (decoupled = 0:
// Adam's) step on the way in: a sibling of choco_quant_round.h's quant_round over the same storage forms, and its
// host side.  What choco_quant_adamw_round.hip (fp32 models) and choco_quant_adamw_round_bf16.hip (bfloat16 models
// and gradients over fp32 x, x_hat, s, exp_avg and exp_avg_sq) share; the design is at the head of the former.
// quant_pass, apply_item, load_q / store_q, store_x, the tile geometry and the launch's shape checks are
// choco_quant_round.h's own, the update is adam_update.h's adam4: x, x_hat, s and the norms are the bits of
// mx_choco_quant_round on x' = adam(x, g, m, v), m' and v' the bits of the fused AdamW rounds.
#pragma once
#include "adam_update.h"
#include "choco_quant_round.h"

namespace mx {
namespace choco {
namespace qround {
using mx::fused::AdamHyper;
using mx::fused::AdamState;

// the storage forms with Adam's constants in the kernel's last argument (and, in a form with an image, p)
struct AdamFp32Io : Fp32Io {
    struct Tail {
        AdamHyper h;
    };
    static Tail tail(const AdamHyper& h, uint16_t*) { return {h}; }
};
struct AdamBf16Io : Bf16Io {
    struct Tail {
        AdamHyper h;
        uint16_t* p;
    };
    static Tail tail(const AdamHyper& h, uint16_t* p) { return {h, p}; }
};

// what an item streams through the update: g, m and v of a lane's four columns, dead once m', v' and the zeros
// are stored
template <class IO>
struct AdamStream {
    typename IO::GC g;
    F4 m, v;
};
template <class IO, bool NT>
__device__ __forceinline__ AdamStream<IO> load_stream(const typename IO::GT* g, const float* m, const float* v,
                                                      int64_t off, int64_t c, bool vec, int64_t P) {
    AdamStream<IO> sm;
    sm.g = load_q<NT>(g + off, c, vec, P);
    sm.m = load_q<NT>(m + off, c, vec, P);
    sm.v = load_q<NT>(v + off, c, vec, P);
    return sm;
}

template <class IO, int BITS, bool NT>
__global__ __launch_bounds__(kTPB) void quant_adamw_round(float* __restrict__ x, typename IO::GT* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          float* __restrict__ xh, float* __restrict__ s,
                                                          float* __restrict__ norms,
                                                          const int32_t* __restrict__ rec_in,
                                                          const int64_t* __restrict__ iter_dev, RoundDims a,
                                                          typename IO::Tail tl) {
    const AdamHyper& h = tl.h;
    __shared__ uint32_t codes[2][kItems][64];                        // one byte per column, a word per lane
    __shared__ float units[2][kItems];                               // fmul(norm, c) of each item
    // quant_round's rules under STEP: an inactive round of the schedule still steps
    int64_t rnd = a.round;
    const int32_t* __restrict__ rec = rec_in;
    bool on = true;
    if (iter_dev) {
        rnd = *iter_dev;
        if (rnd < 0 || rnd >= a.n_iters) return;                     // outside the schedule: nothing, no step either
        rec = rec_in + rnd * a.words;
        on = rec[0] != 0;
    }
    if (rec[1] != 0 || (rec[2] & 2)) return;                         // receive slots, peer reads: not this kernel's
    AdamState st;
    if (mx::fused::adam_no_step(st, h)) return;                      // an optimizer step below 1: nothing
    mx::fused::adam_setup(st, h);                                    // the step's bias corrections, lr from lr_dev
    const uint32_t kr = mix32(a.seed_mix ^ (uint32_t)rnd);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t* deg = rec + mx::kPlanHeader;
    const int bmask = (1 << a.bshift) - 1;
    const F4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    int par = 0;
    for (int64_t w = blockIdx.x; w < a.tiles; w += gridDim.x, par ^= 1) {
        // the wave's items as quant_round's; only x and x_hat of all four are in flight at once
        int64_t off[kIPW], col[kIPW];
        bool live[kIPW], vec[kIPW];
        F4 xv[kIPW], hv[kIPW];
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            const int64_t b0 = ((w << a.bshift) + (i & bmask)) * kBucket;
            off[q] = (int64_t)r * a.ld;
            col[q] = b0 + lane * 4;
            live[q] = r < a.n_local && b0 < a.P;
            vec[q] = b0 + kBucket <= a.P && al16(x + off[q]) && al16(xh + off[q]) && al16(s + off[q]) &&
                     al16(m + off[q]) && al16(v + off[q]) && IO::al_g(g + off[q]);
            if constexpr (IO::kImage) vec[q] = vec[q] && mx::fused::al8(tl.p + off[q]);
            xv[q] = hv[q] = zero;
            if (live[q]) {
                xv[q] = load_q<NT>(x + off[q], col[q], vec[q], a.P);
                hv[q] = load_q<NT>(xh + off[q], col[q], vec[q], a.P);
            }
        }
        // g, m and v stream through two register sets: item q + 1's loads are issued before item q's update, and
        // an item's set is free again as soon as m', v' and the zeros over g are stored
        AdamStream<IO> sm[2];
        if (live[0]) sm[0] = load_stream<IO, NT>(g, m, v, off[0], col[0], vec[0], a.P);
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            if (q + 1 < kIPW && live[q + 1])
                sm[(q + 1) & 1] = load_stream<IO, NT>(g, m, v, off[q + 1], col[q + 1], vec[q + 1], a.P);
            if (!live[q]) continue;                                  // wave-uniform
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            AdamStream<IO>& cur = sm[q & 1];
            xv[q] = mx::fused::adam4(xv[q], mx::fused::widen4(cur.g), cur.m, cur.v, st.st, h);
            store_q<NT>(cur.m, m + off[q], col[q], vec[q], a.P);
            store_q<NT>(cur.v, v + off[q], col[q], vec[q], a.P);
            if (h.zero_grads) store_q<NT>(IO::zero(), g + off[q], col[q], vec[q], a.P);
            if (!on) {                                               // no active matching: the step alone
                store_x<IO, NT>(xv[q], x, tl, off[q], col[q], vec[q], a.P);
                continue;
            }
            float d[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                d[t] = __fsub_rn(xv[q][t], hv[q][t]);
                if (!vec[q] && col[q] + t >= a.P) d[t] = 0.0f;       // past P: +0 to the norm, a zero code
            }
            const uint32_t key = mix32(kr ^ (uint32_t)(a.row_base + r));
            float norm;
            uint32_t word = quant_pass<BITS>(d, key + (uint32_t)col[q], norm);
            if constexpr (BITS == 4)                                 // nibble t to byte t
                word = (word & 0xfu) | (word & 0xf0u) << 4 | (word & 0xf00u) << 8 | (word & 0xf000u) << 12;
            codes[par][i][lane] = word;
            if (lane == 0) {
                units[par][i] = __fmul_rn(norm, Lv<BITS>::c);
                if (norms) *(GPtr<float>)(norms + (int64_t)r * a.norm_ld + (col[q] >> 8)) = norm;
            }
        }
        if (!on) continue;                                           // kernel-uniform
        __syncthreads();
        // phase 2 is quant_round's: g, m and v are gone, so s of all four items fits beside x' and x_hat
        F4 sv[kIPW];
#pragma unroll
        for (int q = 0; q < kIPW; ++q)
            if (live[q]) sv[q] = load_q<NT>(s + off[q], col[q], vec[q], a.P);
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            if (!live[q]) continue;
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            const int b = i & bmask;
            F4& sq = sv[q];
            const int dg = deg[r];                                 // active partners of the row
            const float sw = __int_as_float(deg[a.n_local + r]);     // the record's self weight
            const int32_t* src = deg + 2 * a.n_local + r * a.M;      // their rows, ascending matching
            for (int e = 0; e < dg; ++e)                             // (the mask: no index leaves the LDS image)
                apply_item<BITS, false>(codes[par], units[par], ((src[e] << a.bshift) + b) & (kItems - 1), lane,
                                        a.alpha, sq, hv[q]);
            apply_item<BITS, true>(codes[par], units[par], i, lane, sw, sq, hv[q]);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                xv[q][c] = __builtin_fmaf(-a.g, hv[q][c], __builtin_fmaf(a.g, sq[c], xv[q][c]));
            store_x<IO, NT>(xv[q], x, tl, off[q], col[q], vec[q], a.P);
            store_q<NT>(sq, s + off[q], col[q], vec[q], a.P);
            store_q<NT>(hv[q], xh + off[q], col[q], vec[q], a.P);
        }
    }
}

// what the four entry points check alike, then the launch
template <class IO>
int adamw_round_launch(const char* who, float* x, typename IO::GT* g, float* m, float* v, float* xhat, float* s,
                       uint16_t* p, int64_t ld, int n_local, int64_t P, int bits, const int32_t* plan_dev,
                       int64_t iter, const int64_t* iter_dev, int M, float alpha, float gamma, int64_t seed,
                       int row_base, float* norms, int64_t norm_ld, float lr, const float* lr_dev, float omb1,
                       float beta2, float omb2, float eps, float wd, int decoupled, int zero_grads,
                       const float* bias_dev, int64_t n_bias, int64_t step, const int64_t* step_dev, void* stream) {
    MX_CHECK(x && g && m && v && xhat && s && plan_dev && bias_dev && (!IO::kImage || p), "%s: null pointer", who);
    MX_CHECK(n_bias >= 1, "%s: n_bias=%lld < 1", who, (long long)n_bias);
    MX_CHECK(step_dev || step >= 1, "%s: optimizer step %lld < 1", who, (long long)step);
    RoundGeo geo;
    if (const int rc = round_geo(who, ld, n_local, P, bits, plan_dev, iter, iter_dev, M, alpha, gamma, seed, row_base,
                                 norms, norm_ld, &geo))
        return rc;
    const AdamHyper h{lr, wd, omb1, beta2, omb2, eps, lr_dev, nullptr, bias_dev, n_bias, step, step_dev,
                      decoupled != 0, zero_grads != 0};
    const auto kern = bits == 4 ? (geo.nt ? quant_adamw_round<IO, 4, true> : quant_adamw_round<IO, 4, false>)
                                : (geo.nt ? quant_adamw_round<IO, 8, true> : quant_adamw_round<IO, 8, false>);
    hipLaunchKernelGGL(kern, dim3(geo.grid), dim3(kTPB), 0, mx::as_stream(stream), x, g, m, v, xhat, s, norms, geo.rec,
                       iter_dev, geo.dims, IO::tail(h, p));
    MX_LAUNCH_CHECK();
    return MX_OK;
}

}  // namespace qround
}  // namespace choco
}  // namespace mx
