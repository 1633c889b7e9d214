// lion_update.h -- the Lion update (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms":
// the sign of an interpolated momentum, decoupled weight decay) on fp32 values, as lion_mix.hip and
// lion_mix_bf16.hip apply it on the way into LDS: the same functions in both precisions, only load,
// widen, store and pack differ.  The contract is at the head of those files.
#pragma once
#include "fused_round.h"

namespace mx {
namespace fused {

struct LionHyper {
    float lr, wd, omb1, omb2;
    const float* lr_dev;   // non-NULL: the learning rate, read when the kernel runs
    const float* gscale;   // non-NULL: float [n_local], row r's gradient is multiplied by gscale[r] (wave-uniform: a scalar load)
    int zero_grads;
};

// what a run derives from the launch's learning rate (ungrouped: the launch is one run of scale 1.0, and
// fmul(lr, 1.0) is lr)
// fmul(x, 1.0f) is x bit for bit (-0.0 and denormals included; a NaN stays a NaN), so "no decay" is a decay
// factor of exactly 1.0f and the update carries no flag
struct LionRun {
    float lr, decay;       // lr_r; wd_r != 0 ? fmaf(-lr_r, wd_r, 1) : 1
};
__device__ __forceinline__ LionRun lion_run(float lr, float wd, float scale) {
    LionRun r;
    r.lr = lr * scale;                                               // one rounding; scale 1.0 gives lr
    r.decay = wd != 0.0f ? __builtin_fmaf(-r.lr, wd, 1.0f) : 1.0f;
    return r;
}

// what a launch derives from LionHyper: its learning rate and, ungrouped, its one run.  A grouped launch
// derives the parked work item's run from `lr` and the item's own Geo in the update (as SGD's does its
// -lr_r), never from the prefetched one's: kept out of the state, the 8-row grouped kernel stays on
// SGD-momentum's occupancy step
struct LionState {
    float lr;
    LionRun rn;
};
// Lion has no step counter: every launch is a step
__device__ __forceinline__ bool lion_no_step(LionState&, const LionHyper&) { return false; }
__device__ __forceinline__ void lion_setup(LionState& s, const LionHyper& h) {
    s.lr = h.lr_dev ? *h.lr_dev : h.lr;
    s.rn = lion_run(s.lr, h.wd, 1.0f);
}
template <bool GROUPED>
__device__ __forceinline__ void lion_begin_item(LionState&, const Geo&, const LionHyper&) {}

// the update of one element with the constants of its run: every line one rounding.  The step is a
// select among x1 - lr, x1 + lr and x1 itself (compares and v_cndmask), never a product with a sign
// value: a zero direction keeps x1 bit for bit, -0.0 included, and a NaN direction gives that NaN
__device__ __forceinline__ float lion1(float x, float g, float& m, const LionRun& r, const LionHyper& h) {
    const float x1 = x * r.decay;
    const float dm = g - m;
    const float c = __builtin_fmaf(h.omb1, dm, m);
    m = __builtin_fmaf(h.omb2, dm, m);
    // independent selects over values that exist already (a nested ?: compiled to branches);
    // fadd(x1, -lr) is fsub(x1, lr) bit for bit
    const float moved = x1 + (c > 0.0f ? -r.lr : r.lr);
    const float out = c == 0.0f ? x1 : moved;
    return c != c ? c : out;
}

// a chunk that lies in one run (the whole work item does; ungrouped, the launch is one run): the run's
// constants are scalars
__device__ __forceinline__ F4 lion4_run(const F4& x, const F4& g, F4& m, const LionRun& r, const LionHyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float mt = m[t];
        out[t] = lion1(x[t], g[t], mt, r, h);
        m[t] = mt;
    }
    return out;
}

// a chunk of a work item that holds a run boundary: every element walks forward from the work item's
// first run `r` to its own (a chunk may span four runs) and derives its constants itself.  The walk
// stops at the segment's last run, so columns at or past the segment's length (zero-filled, never
// stored) read inside the tables.
__device__ __forceinline__ F4 lion4_walk(const F4& x, const F4& g, F4& m, int64_t c, int r, int rhi, float lr,
                                         const Grouped<LionHyper>& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        while (r + 1 < rhi && h.rn.end[r] <= c + t) ++r;
        const LionRun rn = lion_run(lr, h.rn.wd[r], h.rn.scale[r]);
        float mt = m[t];
        out[t] = lion1(x[t], g[t], mt, rn, h);
        m[t] = mt;
    }
    return out;
}

// the chunk of an ungrouped launch: lion4_run with the launch's constants
__device__ __forceinline__ F4 lion4(const F4& x, const F4& g, F4& m, const LionRun& r, const LionHyper& h) {
    return lion4_run(x, g, m, r, h);
}

// one chunk of a launch: ungrouped, the launch's constants; grouped, the work item's run or the walk
template <bool GROUPED>
__device__ __forceinline__ F4 lion_chunk(const F4& x, const F4& g, F4& m, int64_t c, const Geo& gq, const LionState& s,
                                         const GroupedIf<LionHyper, GROUPED>& h) {
    if constexpr (GROUPED) {
        return gq.uni ? lion4_run(x, g, m, lion_run(s.lr, gq.wd, gq.scale), h) : lion4_walk(x, g, m, c, gq.r0, gq.rhi, s.lr, h);
    } else {
        return lion4(x, g, m, s.rn, h);
    }
}

}  // namespace fused
}  // namespace mx
