// adam_update.h -- torch.optim.AdamW's / Adam's single-tensor update on fp32 values, as adamw_mix.hip and
// adamw_mix_bf16.hip apply it on the way into LDS: the same functions in both precisions, only load,
// widen, store and pack differ.  The contract is at the head of those files.
// After the arithmetic: the one policy template of both families over a storage form (fused_round.h) and
// their one host function template.
#pragma once
#include "fused_round.h"

namespace mx {
namespace fused {

struct AdamHyper {
    float lr, wd, omb1, beta2, omb2, eps;
    const float* lr_dev;       // non-NULL: the learning rate, read when the kernel runs
    const float* gscale;       // non-NULL: float [n_local], row r's gradient is multiplied by gscale[r] (wave-uniform: a scalar load)
    const float* bias;         // float [n_bias][2]: (bc1, bc2s) of step t at entry min(t, n_bias) - 1
    int64_t n_bias;
    int64_t step;              // the optimizer step t >= 1; with step_dev, *step_dev when the kernel runs
    const int64_t* step_dev;
    int decoupled, zero_grads;
};

// what a launch (grouped: a run) derives from AdamHyper, the step and the bias table
struct Step {
    float nss, decay, bc2s;    // -(lr / bc1), 1 - lr * wd, sqrt(1 - beta2^t)
    bool dec, l2;              // decoupled decay (AdamW) / L2 term in the gradient (Adam), each only with wd != 0
};

// what a run derives from the launch's learning rate and bias corrections (ungrouped: the launch is one
// run of scale 1.0, and fmul(lr, 1.0) is lr)
__device__ __forceinline__ Step run_step(float lr, float bc1, float bc2s, float wd, float scale, int decoupled) {
    const float lr_r = lr * scale;                                   // one rounding; scale 1.0 gives lr
    Step s;
    s.nss = -__fdiv_rn(lr_r, bc1);
    s.bc2s = bc2s;
    s.dec = wd != 0.0f && decoupled;
    s.l2 = wd != 0.0f && !decoupled;
    s.decay = __builtin_fmaf(-lr_r, wd, 1.0f);
    return s;
}

struct AdamState {
    int64_t tstep;             // the optimizer step of this launch
    Step st;                   // the launch's; GROUPED: the parked work item's run's when the item lies in one run
    float lr, bc1;             // GROUPED: what run_step needs per work item / per element
};
// true: no such optimizer step (a step counter below 1), the launch writes nothing
__device__ __forceinline__ bool adam_no_step(AdamState& s, const AdamHyper& h) {
    s.tstep = h.step_dev ? *h.step_dev : h.step;
    return s.tstep < 1;
}
__device__ __forceinline__ void adam_setup(AdamState& s, const AdamHyper& h) {
    const int64_t bi = (s.tstep < h.n_bias ? s.tstep : h.n_bias) - 1;
    const float lr = h.lr_dev ? *h.lr_dev : h.lr;
    s.lr = lr;
    s.bc1 = h.bias[2 * bi];
    s.st.nss = -__fdiv_rn(lr, h.bias[2 * bi]);
    s.st.bc2s = h.bias[2 * bi + 1];
    s.st.dec = h.wd != 0.0f && h.decoupled;
    s.st.l2 = h.wd != 0.0f && !h.decoupled;
    s.st.decay = __builtin_fmaf(-lr, h.wd, 1.0f);
}
// GROUPED: st is re-derived at the top of each work item's pass, from the parked item's own Geo, never
// from the prefetched one's
template <bool GROUPED>
__device__ __forceinline__ void adam_begin_item(AdamState& s, const Geo& cur, const AdamHyper& h) {
    if constexpr (GROUPED) {
        if (cur.uni) s.st = run_step(s.lr, s.bc1, s.st.bc2s, cur.wd, cur.scale, h.decoupled);
    }
}

// the update of one element with decay `wd` (the launch's, or a run's own): every line one rounding
// (-ffp-contract=off keeps the products below out of the fmas)
__device__ __forceinline__ float adam1(float x, float g, float& m, float& v, const Step& s, float wd,
                                       const AdamHyper& h) {
    const float x1 = s.dec ? x * s.decay : x;
    const float g1 = s.l2 ? __builtin_fmaf(wd, x, g) : g;
    const float dm = g1 - m;
    m = __builtin_fmaf(h.omb1, dm, m);
    const float gg = g1 * g1;
    const float bv = h.beta2 * v;
    v = __builtin_fmaf(h.omb2, gg, bv);
    const float root = __builtin_sqrtf(v);                           // correctly rounded (see the head of adamw_mix.hip)
    const float den = __fdiv_rn(root, s.bc2s) + h.eps;
    return __builtin_fmaf(s.nss, __fdiv_rn(m, den), x1);
}

// a chunk that lies in one run (the whole work item does; ungrouped, the launch is one run): the run's
// constants are scalars
__device__ __forceinline__ F4 adam4_run(const F4& x, const F4& g, F4& m, F4& v, const Step& s, float wd,
                                        const AdamHyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float mt = m[t], vt = v[t];
        out[t] = adam1(x[t], g[t], mt, vt, s, wd, h);
        m[t] = mt;
        v[t] = vt;
    }
    return out;
}

// a chunk of a work item that holds a run boundary: every element walks forward from the work item's
// first run `r` to its own (a chunk may span four runs) and derives its constants itself.  The walk
// stops at the segment's last run, so columns at or past the segment's length (zero-filled, never
// stored) read inside the tables.
__device__ __forceinline__ F4 adam4_walk(const F4& x, const F4& g, F4& m, F4& v, int64_t c, int r, int rhi, float lr,
                                         float bc1, float bc2s, const Grouped<AdamHyper>& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        while (r + 1 < rhi && h.rn.end[r] <= c + t) ++r;
        const float wd = h.rn.wd[r];
        const Step s = run_step(lr, bc1, bc2s, wd, h.rn.scale[r], h.decoupled);
        float mt = m[t], vt = v[t];
        out[t] = adam1(x[t], g[t], mt, vt, s, wd, h);
        m[t] = mt;
        v[t] = vt;
    }
    return out;
}

// the chunk of an ungrouped launch: adam4_run(x, g, m, v, s, h.wd, h) written on the vector elements.
// Kept beside adam4_run because the two compile to different register counts (the 8-row mixed-precision
// class: 73 VGPRs / 6 waves per SIMD here, 72 / 7 through adam4_run), and the ungrouped kernels keep the
// occupancy (and the measured speed) they had
__device__ __forceinline__ F4 adam4(const F4& x, const F4& g, F4& m, F4& v, const Step& s, const AdamHyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float x1 = s.dec ? x[t] * s.decay : x[t];
        const float g1 = s.l2 ? __builtin_fmaf(h.wd, x[t], g[t]) : g[t];
        const float dm = g1 - m[t];
        m[t] = __builtin_fmaf(h.omb1, dm, m[t]);
        const float gg = g1 * g1;
        const float bv = h.beta2 * v[t];
        v[t] = __builtin_fmaf(h.omb2, gg, bv);
        const float root = __builtin_sqrtf(v[t]);                    // correctly rounded (see the head of adamw_mix.hip)
        const float den = __fdiv_rn(root, s.bc2s) + h.eps;
        out[t] = __builtin_fmaf(s.nss, __fdiv_rn(m[t], den), x1);
    }
    return out;
}

// one chunk of a launch: ungrouped, the launch's constants; grouped, the work item's run or the walk
template <bool GROUPED>
__device__ __forceinline__ F4 adam_chunk(const F4& x, const F4& g, F4& m, F4& v, int64_t c, const Geo& gq,
                                         const AdamState& s, const GroupedIf<AdamHyper, GROUPED>& h) {
    if constexpr (GROUPED) {
        return gq.uni ? adam4_run(x, g, m, v, s.st, gq.wd, h)
                      : adam4_walk(x, g, m, v, c, gq.r0, gq.rhi, s.lr, s.bc1, s.st.bc2s, h);
    } else {
        return adam4(x, g, m, v, s.st, h);
    }
}

// the policy of both families: x (the fp32 row, or the master), g, m and v; wide accesses only where x, m
// and v of the (segment, row) are 16-byte aligned and the form's arrays to its own accesses
template <class F>
struct AdamRows {
    using Form = F;
    using Hyper = AdamHyper;
    using State = AdamState;
    struct Tabs {
        float* const* x;
        typename Form::GT* const* g;
        float* const* m;
        float* const* v;
        typename Form::PTab p;
    };
    struct Lane {
        F4 X[kB], Mv[kB], Vv[kB];
        typename Form::GC G[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.x[gq.base + k]) && al16(tb.m[gq.base + k]) && al16(tb.v[gq.base + k]) && Form::al(tb, gq, k);
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        ln.X[t] = load_chunk<NT>(tb.x[gq.base + k], c, gq.lim, vec);
        ln.G[t] = load_chunk<NT>(tb.g[gq.base + k], c, gq.lim, vec);
        ln.Mv[t] = load_chunk<NT>(tb.m[gq.base + k], c, gq.lim, vec);
        ln.Vv[t] = load_chunk<NT>(tb.v[gq.base + k], c, gq.lim, vec);
    }
    static __device__ __forceinline__ bool no_step(State& st, const Hyper& h) { return adam_no_step(st, h); }
    static __device__ __forceinline__ void setup(State& st, const Hyper& h) { adam_setup(st, h); }
    template <bool GROUPED>
    static __device__ __forceinline__ void begin_item(State& st, const Geo& cur, const Hyper& h) {
        adam_begin_item<GROUPED>(st, cur, h);
    }
    template <bool GROUPED>
    static __device__ __forceinline__ F4 update(Lane& ln, int t, int k, int64_t c, const Geo& gq, const State& st,
                                                const GroupedIf<Hyper, GROUPED>& h) {
        return adam_chunk<GROUPED>(ln.X[t], grad_of(ln.G[t], h, k), ln.Mv[t], ln.Vv[t], c, gq, st, h);
    }
    template <int SP>
    static __device__ __forceinline__ void keep(const Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec, const Hyper& h) {
        store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, ln.Mv[t]);
        store_chunk<SP>(tb.v[gq.base + k], c, gq.lim, vec, ln.Vv[t]);
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, Form::zero());
    }
    template <int SP>
    static __device__ __forceinline__ void finish(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                  const F4& acc) {
        Form::template store<SP>(tb, gq, k, c, vec, acc);
    }
};

// the host side of both families: Mix is the family's named policy, Call its call record
template <class Mix, class Call>
int adamw_round(const Tune& tune, const Call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                const int64_t* iter_dev, int64_t step, const int64_t* step_dev, float lr, const float* lr_dev,
                void* stream, const char* who) {
    using Form = typename Mix::Form;
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(Form::tables(c) && c->m_ptrs_dev && c->v_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev &&
                 c->bias_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(c->n_bias >= 1, "%s: n_bias=%lld < 1", who, (long long)c->n_bias);
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(step_dev || step >= 1, "%s: optimizer step %lld < 1", who, (long long)step);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: the form's, m and v read + written, g zeroed
    const int bpe = Form::kBytes + 16 + (c->zero_grads ? (int)sizeof(typename Form::GT) : 0);
    const AdamHyper h{lr, c->wd, c->omb1, c->beta2, c->omb2, c->eps, lr_dev, gscale, c->bias_dev, c->n_bias, step, step_dev,
                      c->decoupled != 0, c->zero_grads != 0};
    return Form::template run<Mix>(tune, r, bpe, h, runs, c, c->m_ptrs_dev, c->v_ptrs_dev);
}

}  // namespace fused
}  // namespace mx
