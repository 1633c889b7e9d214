// lion_update.h -- the Lion update (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms":
// the sign of an interpolated momentum, decoupled weight decay) on fp32 values, as lion_mix.hip and
// lion_mix_bf16.hip apply it on the way into LDS: the same functions in both precisions, only load,
// widen, store and pack differ.  The contract is at the head of those files.
// After the arithmetic: the one policy template of both families over a storage form (fused_round.h) and
// their one host function template.
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

// the policy of both families: x (the fp32 row, or the master), g and m.  m is fp32 (MB16 = false) or, in
// the bf16 family alone, bf16 (MB16 = true: held in flight as its 8 bytes, widened for the update and
// rounded once on the way back).  Wide accesses only where x of the (segment, row) is 16-byte aligned and m
// and the form's arrays to their own accesses
template <class F, bool MB16>
struct LionRows {
    using Form = F;
    using Hyper = LionHyper;
    using State = LionState;
    using MT = std::conditional_t<MB16, uint16_t, float>;
    using MC = std::conditional_t<MB16, U2, F4>;
    struct Tabs {
        float* const* x;
        typename Form::GT* const* g;
        MT* const* m;
        typename Form::PTab p;
    };
    struct Lane {
        F4 X[kB];
        MC Mv[kB];
        typename Form::GC G[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        const bool v = al16(tb.x[gq.base + k]) && Form::al(tb, gq, k);
        if constexpr (MB16) return v && al8(tb.m[gq.base + k]);
        else return v && al16(tb.m[gq.base + k]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        ln.X[t] = load_chunk<NT>(tb.x[gq.base + k], c, gq.lim, vec);
        ln.G[t] = load_chunk<NT>(tb.g[gq.base + k], c, gq.lim, vec);
        ln.Mv[t] = load_chunk<NT>(tb.m[gq.base + k], c, gq.lim, vec);
    }
    static __device__ __forceinline__ bool no_step(State& st, const Hyper& h) { return lion_no_step(st, h); }
    static __device__ __forceinline__ void setup(State& st, const Hyper& h) { lion_setup(st, h); }
    template <bool GROUPED>
    static __device__ __forceinline__ void begin_item(State& st, const Geo& cur, const Hyper& h) {
        lion_begin_item<GROUPED>(st, cur, h);
    }
    template <bool GROUPED>
    static __device__ __forceinline__ F4 update(Lane& ln, int t, int k, int64_t c, const Geo& gq, const State& st,
                                                const GroupedIf<Hyper, GROUPED>& h) {
        if constexpr (MB16) {
            F4 m32 = widen4(ln.Mv[t]);
            const F4 out = lion_chunk<GROUPED>(ln.X[t], grad_of(ln.G[t], h, k), m32, c, gq, st, h);
            ln.Mv[t] = pack4(m32);                                                  // the one rounding of m'
            return out;
        } else {
            return lion_chunk<GROUPED>(ln.X[t], grad_of(ln.G[t], h, k), ln.Mv[t], c, gq, st, h);
        }
    }
    template <int SP>
    static __device__ __forceinline__ void keep(const Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec, const Hyper& h) {
        store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, ln.Mv[t]);
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, Form::zero());
    }
    template <int SP>
    static __device__ __forceinline__ void finish(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                  const F4& acc) {
        Form::template store<SP>(tb, gq, k, c, vec, acc);
    }
};

// the host side of both families: Mix is the family's named policy with an fp32 momentum, MixB16 the one
// with a bf16 momentum (the bf16 family's call record says which; the fp32 family names Mix twice), Call
// the call record
template <class Mix, class MixB16, class Call>
int lion_round(const Tune& tune, const Call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
               const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    using Form = typename Mix::Form;
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(Form::tables(c) && c->seg_len_dev && c->tile_off_dev && c->plan_dev, "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(c->m_ptrs_dev, "%s: null momentum table (Lion always carries momentum)", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: the form's, m read + written, g zeroed
    const int zero = c->zero_grads ? (int)sizeof(typename Form::GT) : 0;
    const LionHyper h{lr, c->wd, c->omb1, c->omb2, lr_dev, gscale, c->zero_grads != 0};
    if constexpr (!std::is_same_v<Mix, MixB16>) {
        if (c->m_bf16)
            return Form::template run<MixB16>(tune, r, Form::kBytes + 4 + zero, h, runs, c,
                                              reinterpret_cast<uint16_t* const*>(c->m_ptrs_dev));
    }
    return Form::template run<Mix>(tune, r, Form::kBytes + 8 + zero, h, runs, c,
                                   reinterpret_cast<float* const*>(c->m_ptrs_dev));
}

}  // namespace fused
}  // namespace mx
