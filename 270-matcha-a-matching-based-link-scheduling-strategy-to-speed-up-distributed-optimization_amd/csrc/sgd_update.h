// sgd_update.h -- torch.optim.SGD's update (dampening 0) on fp32 values, as sgd_mix.hip and
// sgd_mix_bf16.hip apply it on the way into LDS: the same functions in both precisions, only load, widen,
// store and pack differ.  The contract is at the head of those files.
// After the arithmetic: the one policy template of both families over a storage form (fused_round.h) and
// their one host function template.
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

// the policy of both families: x (the fp32 row, or the master), g and m; wide accesses only where x and m
// of the (segment, row) are 16-byte aligned and the form's arrays to its own accesses
template <class F, bool MOM>
struct SgdRows {
    using Form = F;
    using Hyper = SgdHyper;
    using State = SgdState;
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
        bool v = al16(tb.x[gq.base + k]) && Form::al(tb, gq, k);
        if constexpr (MOM) v = v && al16(tb.m[gq.base + k]);
        return v;
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        ln.X[t] = load_chunk<NT>(tb.x[gq.base + k], c, gq.lim, vec);
        ln.G[t] = load_chunk<NT>(tb.g[gq.base + k], c, gq.lim, vec);
        if constexpr (MOM) ln.Mv[t] = load_chunk<NT>(tb.m[gq.base + k], c, gq.lim, vec);
    }
    static __device__ __forceinline__ bool no_step(State& st, const Hyper& h) { return sgd_no_step(st, h); }
    static __device__ __forceinline__ void setup(State& st, const Hyper& h) { sgd_setup(st, h); }
    template <bool GROUPED>
    static __device__ __forceinline__ void begin_item(State&, const Geo&, const Hyper&) {}
    template <bool GROUPED>
    static __device__ __forceinline__ F4 update(Lane& ln, int t, int k, int64_t c, const Geo& gq, const State& st,
                                                const GroupedIf<Hyper, GROUPED>& h) {
        return sgd_chunk<MOM, GROUPED>(ln.X[t], grad_of(ln.G[t], h, k), ln.Mv[t], c, gq, st, h);
    }
    template <int SP>
    static __device__ __forceinline__ void keep(const Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec, const Hyper& h) {
        if constexpr (MOM) store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, ln.Mv[t]);
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, Form::zero());
    }
    template <int SP>
    static __device__ __forceinline__ void finish(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                  const F4& acc) {
        Form::template store<SP>(tb, gq, k, c, vec, acc);
    }
};

// the host side of both families: Mix<MOM> is the family's named policy, Call its call record
template <template <bool> class Mix, class Call>
int sgd_round(const Tune& tune, const Call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
              const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    using Form = typename Mix<true>::Form;
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(Form::tables(c) && c->seg_len_dev && c->tile_off_dev && c->plan_dev, "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK((c->mom != 0.0f) == (c->m_ptrs_dev != nullptr), "%s: the momentum table is given exactly when mom != 0",
             who);
    MX_CHECK(c->mom != 0.0f || !c->nesterov, "%s: nesterov needs momentum", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    const bool mom = c->mom != 0.0f;
    // bytes the round moves: the form's, m read + written, g zeroed
    const int bpe = Form::kBytes + (mom ? 8 : 0) + (c->zero_grads ? (int)sizeof(typename Form::GT) : 0);
    const SgdHyper h{lr, c->wd, c->mom, lr_dev, gscale, c->nesterov != 0, c->zero_grads != 0};
    return mom ? Form::template run<Mix<true>>(tune, r, bpe, h, runs, c, c->m_ptrs_dev)
               : Form::template run<Mix<false>>(tune, r, bpe, h, runs, c, c->m_ptrs_dev);
}

}  // namespace fused
}  // namespace mx
