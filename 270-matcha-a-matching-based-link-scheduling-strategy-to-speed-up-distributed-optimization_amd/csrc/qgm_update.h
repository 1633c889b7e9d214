// qgm_update.h -- quasi-global momentum (Lin et al., ICML 2021, "Quasi-Global Momentum: Accelerating
// Decentralized Deep Learning on Heterogeneous Data"; QG-DSGDm) on fp32 values, as qgm_mix.hip and
// qgm_mix_bf16.hip apply it: the local step on the way into LDS, the buffer update after the round.  The
// same functions in both precisions, only load, widen, store and pack differ.  The contract is at the
// head of those files.
#pragma once
#include "fused_round.h"

namespace mx {
namespace fused {

struct QgmHyper {
    float lr, wd, beta, omu;
    const float* lr_dev;   // non-NULL: the learning rate, read when the kernel runs
    const float* gscale;   // non-NULL: float [n_local], row r's gradient is multiplied by gscale[r] (wave-uniform: a scalar load)
    int zero_grads;
};

// what a launch derives from QgmHyper: its learning rate and, ungrouped, the reciprocal the buffer update
// multiplies by.  A grouped launch derives a work item's (lr_r, rl) from `lr` and the item's own Geo where
// it needs them (as SGD's does its -lr_r), never from the prefetched one's
struct QgmState {
    float lr, rl;          // lr; fdiv(1, lr)
};
// no step counter: every launch is a step
__device__ __forceinline__ bool qgm_no_step(QgmState&, const QgmHyper&) { return false; }
__device__ __forceinline__ void qgm_setup(QgmState& s, const QgmHyper& h) {
    s.lr = h.lr_dev ? *h.lr_dev : h.lr;
    s.rl = __fdiv_rn(1.0f, s.lr);
}

// the local step of one element with decay `wd` and negated learning rate `nlr` (the launch's, or a run's
// own): every line one rounding.  mh is the quasi-global buffer, read only here: the local momentum m
// lives in a register and is never stored
template <bool NESTEROV>
__device__ __forceinline__ float qgm1(float x, float g, float mh, float nlr, float wd, const QgmHyper& h) {
    const float d = wd != 0.0f ? __builtin_fmaf(wd, x, g) : g;
    const float scaled = h.beta * mh;                   // separately rounded (-ffp-contract=off)
    const float m = scaled + d;
    const float s = NESTEROV ? __builtin_fmaf(h.beta, m, d) : m;
    return __builtin_fmaf(nlr, s, x);
}

// a chunk that lies in one run (the whole work item does; ungrouped, the launch is one run): the run's
// constants are scalars
template <bool NESTEROV>
__device__ __forceinline__ F4 qgm4_run(const F4& x, const F4& g, const F4& mh, float nlr, float wd, const QgmHyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) out[t] = qgm1<NESTEROV>(x[t], g[t], mh[t], nlr, wd, h);
    return out;
}

// the run of column c: a walk forward from the work item's first run `r`; it stops at the segment's last
// run, so columns at or past the segment's length (zero-filled, never stored) read inside the tables
__device__ __forceinline__ int qgm_run_of(int r, int rhi, int64_t c, const Runs& rn) {
    while (r + 1 < rhi && rn.end[r] <= c) ++r;
    return r;
}

// a chunk of a work item that holds a run boundary: every element resolves its own run (a chunk may span
// four) and derives its constants itself
template <bool NESTEROV>
__device__ __forceinline__ F4 qgm4_walk(const F4& x, const F4& g, const F4& mh, int64_t c, int r, int rhi, float lr,
                                        const Grouped<QgmHyper>& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        r = qgm_run_of(r, rhi, c + t, h.rn);
        const float lr_r = lr * h.rn.scale[r];                       // one rounding; scale 1.0 gives lr
        out[t] = qgm1<NESTEROV>(x[t], g[t], mh[t], -lr_r, h.rn.wd[r], h);
    }
    return out;
}

// one chunk of the local step: ungrouped, the launch's constants; grouped, the work item's run or the walk
template <bool NESTEROV, bool GROUPED>
__device__ __forceinline__ F4 qgm_chunk(const F4& x, const F4& g, const F4& mh, int64_t c, const Geo& gq,
                                        const QgmState& st, const GroupedIf<QgmHyper, GROUPED>& h) {
    if constexpr (GROUPED) {
        return gq.uni ? qgm4_run<NESTEROV>(x, g, mh, -(st.lr * gq.scale), gq.wd, h)
                      : qgm4_walk<NESTEROV>(x, g, mh, c, gq.r0, gq.rhi, st.lr, h);
    } else {
        return qgm4_run<NESTEROV>(x, g, mh, -st.lr, h.wd, h);
    }
}

// the buffer update of one element after the round: x the value the row held before this launch, y the
// mixed value about to be stored.  lr_r == 0 (a frozen run, lr = 0) keeps mh bit for bit: q is 0 * Inf there
__device__ __forceinline__ float qgm_buf1(float x, float y, float mh, float lr_r, float rl, const QgmHyper& h) {
    const float moved = x - y;
    const float q = moved * rl;                          // separately rounded (-ffp-contract=off)
    const float fresh = __builtin_fmaf(h.omu, q - mh, mh);
    return lr_r != 0.0f ? fresh : mh;
}

// one chunk of the buffer update: ungrouped, the launch's (lr, rl); grouped, the work item's run (one
// division per chunk, wave-uniform) or each element's own
template <bool GROUPED>
__device__ __forceinline__ F4 qgm_buf_chunk(const F4& x, const F4& y, const F4& mh, int64_t c, const Geo& gq,
                                            const QgmState& st, const GroupedIf<QgmHyper, GROUPED>& h) {
    F4 out;
    if constexpr (GROUPED) {
        if (gq.uni) {
            const float lr_r = st.lr * gq.scale;
            const float rl = __fdiv_rn(1.0f, lr_r);
#pragma unroll
            for (int t = 0; t < 4; ++t) out[t] = qgm_buf1(x[t], y[t], mh[t], lr_r, rl, h);
        } else {
            int r = gq.r0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                r = qgm_run_of(r, gq.rhi, c + t, h.rn);
                const float lr_r = st.lr * h.rn.scale[r];
                out[t] = qgm_buf1(x[t], y[t], mh[t], lr_r, __fdiv_rn(1.0f, lr_r), h);
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) out[t] = qgm_buf1(x[t], y[t], mh[t], st.lr, st.rl, h);
    }
    return out;
}

}  // namespace fused
}  // namespace mx
