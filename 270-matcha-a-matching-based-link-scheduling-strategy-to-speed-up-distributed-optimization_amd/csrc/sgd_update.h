// sgd_update.h -- torch.optim.SGD's update (dampening 0) on fp32 values, as sgd_mix.hip and
// sgd_mix_bf16.hip apply it on the way into LDS: the same functions in both precisions, only load, widen,
// store and pack differ.  The contract is at the head of those files.
#pragma once
#include "fused_round.h"

namespace mx {
namespace fused {

struct SgdHyper {
    float lr, wd, mom;
    const float* lr_dev;   // non-NULL: the learning rate, read when the kernel runs
    const float* gscale;   // non-NULL: float [n_local], row r's gradient is multiplied by gscale[r] (wave-uniform: a scalar load)
    int nesterov, zero_grads;
};

// what a launch derives from SgdHyper: the negated learning rate.  A grouped launch derives the parked
// work item's -lr_r from it and the item's own Geo in the update, never from the prefetched one's
struct SgdState {
    float nlr;
};
__device__ __forceinline__ bool sgd_no_step(SgdState&, const SgdHyper&) { return false; }
__device__ __forceinline__ void sgd_setup(SgdState& st, const SgdHyper& h) { st.nlr = -(h.lr_dev ? *h.lr_dev : h.lr); }

// the update of one element with decay `wd` and negated learning rate `nlr` (the launch's, or a run's
// own); the momentum line always runs, with no first-step case: from a zero buffer
// fadd(fmul(mom, 0), d) == d under IEEE ==
template <bool MOM>
__device__ __forceinline__ float sgd1(float x, float g, float& m, float nlr, float wd, const SgdHyper& h) {
    float d = wd != 0.0f ? __builtin_fmaf(wd, x, g) : g;
    if constexpr (MOM) {
        const float scaled = h.mom * m;             // separately rounded (-ffp-contract=off)
        m = scaled + d;
        d = h.nesterov ? __builtin_fmaf(h.mom, m, d) : m;
    }
    return __builtin_fmaf(nlr, d, x);
}

// a chunk that lies in one run (the whole work item does; ungrouped, the launch is one run): the run's
// constants are scalars
template <bool MOM>
__device__ __forceinline__ F4 sgd4_run(const F4& x, const F4& g, F4& m, float nlr, float wd, const SgdHyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float mt = MOM ? m[t] : 0.0f;
        out[t] = sgd1<MOM>(x[t], g[t], mt, nlr, wd, h);
        if constexpr (MOM) m[t] = mt;
    }
    return out;
}

// a chunk of a work item that holds a run boundary: every element walks forward from the work item's
// first run `r` to its own (a chunk may span four runs) and derives its constants itself.  The walk
// stops at the segment's last run, so columns at or past the segment's length (zero-filled, never
// stored) read inside the tables.
template <bool MOM>
__device__ __forceinline__ F4 sgd4_walk(const F4& x, const F4& g, F4& m, int64_t c, int r, int rhi, float lr,
                                        const Grouped<SgdHyper>& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        while (r + 1 < rhi && h.rn.end[r] <= c + t) ++r;
        const float lr_r = lr * h.rn.scale[r];                       // one rounding; scale 1.0 gives lr
        float mt = MOM ? m[t] : 0.0f;
        out[t] = sgd1<MOM>(x[t], g[t], mt, -lr_r, h.rn.wd[r], h);
        if constexpr (MOM) m[t] = mt;
    }
    return out;
}

// the chunk of an ungrouped launch: sgd4_run(x, g, m, nlr, h.wd, h) written on the vector elements.  Kept
// beside sgd4_run because the two compile to different instruction orders, and the ungrouped kernels keep
// the order (and the measured speed) they had
template <bool MOM>
__device__ __forceinline__ F4 sgd4(const F4& x, const F4& g, F4& m, float nlr, const SgdHyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float d = h.wd != 0.0f ? __builtin_fmaf(h.wd, x[t], g[t]) : g[t];
        if constexpr (MOM) {
            const float scaled = h.mom * m[t];          // separately rounded (-ffp-contract=off)
            m[t] = scaled + d;
            d = h.nesterov ? __builtin_fmaf(h.mom, m[t], d) : m[t];
        }
        out[t] = __builtin_fmaf(nlr, d, x[t]);
    }
    return out;
}

// one chunk of a launch: ungrouped, the launch's constants; grouped, the work item's run or the walk
template <bool MOM, bool GROUPED>
__device__ __forceinline__ F4 sgd_chunk(const F4& x, const F4& g, F4& m, int64_t c, const Geo& gq, const SgdState& st,
                                        const GroupedIf<SgdHyper, GROUPED>& h) {
    if constexpr (GROUPED) {
        return gq.uni ? sgd4_run<MOM>(x, g, m, -(-st.nlr * gq.scale), gq.wd, h)
                      : sgd4_walk<MOM>(x, g, m, c, gq.r0, gq.rhi, -st.nlr, h);
    } else {
        return sgd4<MOM>(x, g, m, st.nlr, h);
    }
}

}  // namespace fused
}  // namespace mx
