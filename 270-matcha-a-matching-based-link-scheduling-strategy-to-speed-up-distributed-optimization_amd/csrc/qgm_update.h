// qgm_update.h -- quasi-global momentum (Lin et al., ICML 2021, "Quasi-Global Momentum: Accelerating
// Decentralized Deep Learning on Heterogeneous Data"; QG-DSGDm) on fp32 values, as qgm_mix.hip and
// qgm_mix_bf16.hip apply it: the local step on the way into LDS, the buffer update after the round.  The
// same functions in both precisions, only load, widen, store and pack differ.  The contract is at the
// head of those files.
// After the arithmetic: the one policy template of both families over a storage form (fused_round.h) and
// their one host function template.
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

// the policy of both families: x (the fp32 row, or the master), g and the buffer mh (table `m`); wide
// accesses only where x and mh of the (segment, row) are 16-byte aligned and the form's arrays to its own
// accesses.  PLAIN: x and mh are staged with plain loads where the launch streams (knob "stage_plain", the
// default), so that the finish side's reload finds more of their lines cached
template <class F, bool NESTEROV, bool PLAIN>
struct QgmRows {
    static constexpr bool kAfterMix = true;
    using Form = F;
    using Hyper = QgmHyper;
    using State = QgmState;
    struct Tabs {
        float* const* x;
        typename Form::GT* const* g;
        float* const* m;
        typename Form::PTab p;
    };
    struct Lane {
        F4 X[kB], Mv[kB];
        typename Form::GC G[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.x[gq.base + k]) && Form::al(tb, gq, k) && al16(tb.m[gq.base + k]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        constexpr bool XNT = NT && !PLAIN;
        ln.X[t] = load_chunk<XNT>(tb.x[gq.base + k], c, gq.lim, vec);
        ln.G[t] = load_chunk<NT>(tb.g[gq.base + k], c, gq.lim, vec);
        ln.Mv[t] = load_chunk<XNT>(tb.m[gq.base + k], c, gq.lim, vec);
    }
    static __device__ __forceinline__ bool no_step(State& st, const Hyper& h) { return qgm_no_step(st, h); }
    static __device__ __forceinline__ void setup(State& st, const Hyper& h) { qgm_setup(st, h); }
    template <bool GROUPED>
    static __device__ __forceinline__ void begin_item(State&, const Geo&, const Hyper&) {}
    template <bool GROUPED>
    static __device__ __forceinline__ F4 update(Lane& ln, int t, int k, int64_t c, const Geo& gq, const State& st,
                                                const GroupedIf<Hyper, GROUPED>& h) {
        return qgm_chunk<NESTEROV, GROUPED>(ln.X[t], grad_of(ln.G[t], h, k), ln.Mv[t], c, gq, st, h);
    }
    // the staging lane stores the zeros over g and nothing else: mh belongs to the lane that finishes
    template <int SP>
    static __device__ __forceinline__ void keep(const Lane&, int, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec, const Hyper& h) {
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, Form::zero());
    }
    template <bool GROUPED, int SP>
    static __device__ __forceinline__ void after_mix(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                     const F4& acc, const State& st,
                                                     const GroupedIf<Hyper, GROUPED>& h) {
        const F4 x = load_chunk<false>(tb.x[gq.base + k], c, gq.lim, vec);     // the row before this launch
        const F4 mh = load_chunk<false>(tb.m[gq.base + k], c, gq.lim, vec);
        store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, qgm_buf_chunk<GROUPED>(x, acc, mh, c, gq, st, h));
        Form::template store<SP>(tb, gq, k, c, vec, acc);
    }
};

// a QGM family's knobs: Tune's, and "stage_plain": 1 = x and mh staged with plain loads (see QgmRows); 0 =
// with nt loads, as g
struct QgmTune : Tune {
    int stage_plain = 1;
    int set(const char* who, const char* key, int value) {
        if (key && !strcmp(key, "stage_plain")) {
            MX_CHECK(value == 0 || value == 1, "%s: stage_plain %d", who, value);
            stage_plain = value;
            return MX_OK;
        }
        return Tune::set(who, key, value);
    }
    int get(const char* who, const char* key) const {
        if (key && !strcmp(key, "stage_plain")) return stage_plain;
        return Tune::get(who, key);
    }
};

// the host side of both families: Mix<NESTEROV, PLAIN> is the family's named policy, Call its call record
template <template <bool, bool> class Mix, class Call>
int qgm_round(const QgmTune& tune, const Call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
              const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    using Form = typename Mix<false, false>::Form;
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(Form::tables(c) && c->seg_len_dev && c->tile_off_dev && c->plan_dev, "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(c->m_ptrs_dev, "%s: null buffer table (quasi-global momentum always carries its buffer)", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: the form's, mh read + written, g zeroed
    const int bpe = Form::kBytes + 8 + (c->zero_grads ? (int)sizeof(typename Form::GT) : 0);
    const QgmHyper h{lr, c->wd, c->beta, c->omu, lr_dev, gscale, c->zero_grads != 0};
#define MX_QGM(N, P) Form::template run<Mix<N, P>>(tune, r, bpe, h, runs, c, c->m_ptrs_dev)
    if (c->nesterov) return tune.stage_plain ? MX_QGM(true, true) : MX_QGM(true, false);
    return tune.stage_plain ? MX_QGM(false, true) : MX_QGM(false, false);
#undef MX_QGM
}

}  // namespace fused
}  // namespace mx
