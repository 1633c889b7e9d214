// gt_update.h -- gradient tracking (DIGing / DSGT / GT-DSGD: Di Lorenzo & Scutari 2016; Nedic, Olshevsky & Shi
// 2017; Pu & Nedic 2021) on fp32 values, as gt_track.hip, gt_track_bf16.hip and gt_step_bf16.hip apply it.
// Every worker keeps a tracker y of the network's mean gradient and steps along it; the trackers are gossiped
// with the round's own matrix, so an iteration is TWO launches on one plan record:
//     track   y' = y + (gs - gp), gp = gs, g = 0 under zero_grads, then the round on the y' values
//     step    torch.optim.SGD's update with y in the gradient's place, then the round on the x' values
// The track launch is the policy below over the gradient's storage.  The step launch is sgd_update.h's SgdRows
// as it stands: for fp32 rows mx_sgd_mix itself with the tracker's table as its g, for bf16 rows over fp32
// masters SgdRows over Fp32GradForm (gt_step_bf16.hip).  The contract is at the head of those files.
#pragma once
#include "sgd_update.h"

namespace mx {
namespace fused {

// the track launch has no learning rate and no weight decay: it never reads x
struct GtHyper {
    const float* gscale;   // non-NULL: float [n_local], row r's gradient is multiplied by gscale[r] (wave-uniform: a scalar load)
    int zero_grads;
};
struct GtState {};

// one chunk of the track update, every line one rounding (-ffp-contract=off): gs is the gradient as it enters
// the tracker (widened, clip factor included), gp the value that entered it one iteration ago.  From zeros
// y' = g falls out: there is no first-step case
__device__ __forceinline__ F4 gt_track4(const F4& y, const F4& gs, const F4& gp) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float d = gs[t] - gp[t];
        out[t] = y[t] + d;
    }
    return out;
}

// the policy of both track families: x is the tracker y (the mixed fp32 row; it has no bf16 image), g the
// gradient in the form's storage, m the previous gradient gp (always fp32); wide accesses only where y and gp
// of the (segment, row) are 16-byte aligned and g to the form's own access
template <class F>
struct GtTrackRows {
    using Form = F;
    using Hyper = GtHyper;
    using State = GtState;
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
        ln.X[t] = load_chunk<NT>(tb.x[gq.base + k], c, gq.lim, vec);
        ln.G[t] = load_chunk<NT>(tb.g[gq.base + k], c, gq.lim, vec);
        ln.Mv[t] = load_chunk<NT>(tb.m[gq.base + k], c, gq.lim, vec);
    }
    static __device__ __forceinline__ bool no_step(State&, const Hyper&) { return false; }
    static __device__ __forceinline__ void setup(State&, const Hyper&) {}
    template <bool GROUPED>
    static __device__ __forceinline__ void begin_item(State&, const Geo&, const Hyper&) {}
    // gp takes the value that entered the tracker, so that the differences telescope exactly as it saw them
    template <bool GROUPED>
    static __device__ __forceinline__ F4 update(Lane& ln, int t, int k, int64_t, const Geo&, const State&,
                                                const GroupedIf<Hyper, GROUPED>& h) {
        const F4 gs = grad_of(ln.G[t], h, k);
        const F4 out = gt_track4(ln.X[t], gs, ln.Mv[t]);
        ln.Mv[t] = gs;
        return out;
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

// the host side of both track families: Track is the family's named policy, Call its call record.  The
// family signature's lr, lr_dev and parameter runs are accepted and unused (the runs are still checked, so a
// broken record is refused by both launches of an iteration alike): every launch is the ungrouped kernel
template <class Track, class Call>
int gt_track_round(const Tune& tune, const Call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                   const int64_t* iter_dev, float, const float*, void* stream, const char* who) {
    using Form = typename Track::Form;
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(Form::tables(c) && c->gp_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev, "%s: null pointer",
             who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: the form's, gp read + written, g zeroed
    const int bpe = Form::kBytes + 8 + (c->zero_grads ? (int)sizeof(typename Form::GT) : 0);
    const GtHyper h{gscale, c->zero_grads != 0};
    return Form::template run<Track>(tune, r, bpe, h, nullptr, c, c->gp_ptrs_dev);
}

// the host side of the mixed-precision step family: sgd_round, after the two things the step launch refuses.
// The tracker is state, not a consumed gradient, and the clip factor entered it in the track launch
template <template <bool> class Mix, class Call>
int gt_step_round(const Tune& tune, const Call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                  const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(!c || !c->zero_grads, "%s: zero_grads on the step record (the zeros over g are the track launch's)", who);
    MX_CHECK(!gscale, "%s: clip factors on the step launch (they enter the tracker in the track launch)", who);
    return sgd_round<Mix>(tune, c, runs, gscale, iter, iter_dev, lr, lr_dev, stream, who);
}

}  // namespace fused
}  // namespace mx
