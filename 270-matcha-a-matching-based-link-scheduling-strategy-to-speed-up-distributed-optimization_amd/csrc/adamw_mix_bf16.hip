// adamw_mix_bf16.hip -- mixed-precision AdamW / Adam fused into the mixing round: bfloat16 models and
// gradients, fp32 master weights, exp_avg and exp_avg_sq (local-only groups).  One launch per training
// iteration.
//
// adamw_mix.hip's launch for models held in bfloat16, with sgd_mix_bf16.hip's load and store sides.  The
// fp32 master rows are what the optimizer updates and the round mixes, so nothing is lost to bf16
// rounding between rounds; the bf16 model row is the rounded image of the master, rewritten by every
// launch.  Per (segment, row) five arrays:
//     w  fp32 master      read and written in place
//     g  bf16 gradient    read; overwritten with zeros when zero_grads
//     m  fp32 exp_avg     read and written
//     v  fp32 exp_avg_sq  read and written
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (torch.optim.AdamW's / Adam's single-tensor update on the fp32 masters; every
// line one IEEE fp32 rounding: -ffp-contract=off, explicit fmas, correctly rounded sqrt and division,
// denormals kept):
//     g32 = f32(g)                                        exact widening, bits << 16
//     decay = fmaf(-lr, wd, 1)                            once per launch
//     w1 = (wd != 0 &&  decoupled) ? fmul(w, decay) : w
//     g1 = (wd != 0 && !decoupled) ? fmaf(wd, w, g32) : g32
//     m' = fmaf(omb1, fsub(g1, m), m)
//     v' = fmaf(omb2, fmul(g1, g1), fmul(beta2, v))
//     den = fadd(fdiv(fsqrt(v'), bc2s), eps)
//     ss  = fdiv(lr, bc1)                                 once per launch
//     w'  = fmaf(-ss, fdiv(m', den), w1)
//     w   = the round of sgd_mix.hip on the w' values: per output row the partners' columns in ascending
//           matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//           leaves alone, and every row of an all-zero round, keeps w' as it is
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// (bc1, bc2s) = (1 - beta1^t, sqrt(1 - beta2^t)) of optimizer step t come from adamw_mix.hip's host-built
// device table at entry min(t, n_bias) - 1; t is an argument or, for graph replay, a device counter.
// Nothing computes pow on the device.  The square root is __builtin_sqrtf and not __fsqrt_rn, the
// division __fdiv_rn: see the head of adamw_mix.hip.
//
// p is written for every row in every launch that runs, rows the round leaves alone included: their w
// changed by the optimizer step.  A device counter outside the schedule, a step counter below 1 and a
// plan record with the peer-reads bit each make the launch a complete no-op.  Nothing is written at or
// past a row's length in any array.
//
// Traffic per element: read w (4), g (2), m (4), v (4), write w (4), m (4), v (4), p (2) = 28 bytes (30
// when the gradients are zeroed) against 100 for the unfused op sequence.
//
// A lane holds 4 elements: 16-byte accesses on w, m and v, 8-byte accesses on g and p.  Alignment rule:
// the vector path is taken where w, m and v of the (segment, row) are 16-byte aligned, g and p are
// 8-byte aligned and the 4 elements are in range; everything else goes element by element (4-byte /
// 2-byte accesses), zero-filled past the end.
//
// In place: a tile's w' of every row is parked in LDS as fp32 (barrier) before any w row of it is stored,
// and different work items never share a column.  m and v are read and written by the same lane only, so
// they are stored when their chunk is staged; so are the zeros over g.  Because every row is read in
// every round, the first loads are issued before the plan record is looked at.  No receive slots:
// n_slots == n_local.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<AdamwMixBf16, ...>).
#include "adam_update.h"

namespace {
using namespace mx::fused;

// w, m and v as fp32, g and p as bf16; wide accesses only where the (segment, row)'s w, m and v are
// 16-byte and g and p 8-byte aligned
struct AdamwMixBf16 {
    using Hyper = AdamHyper;
    using State = AdamState;
    struct Tabs {
        float* const* w;
        uint16_t* const* g;
        float* const* m;
        float* const* v;
        uint16_t* const* p;
    };
    struct Lane {
        F4 X[kB], Mv[kB], Vv[kB];
        U2 G[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.w[gq.base + k]) && al16(tb.m[gq.base + k]) && al16(tb.v[gq.base + k]) && al8(tb.g[gq.base + k]) && al8(tb.p[gq.base + k]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        ln.X[t] = load_chunk<NT>(tb.w[gq.base + k], c, gq.lim, vec);
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
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, U2{0u, 0u});
    }
    template <int SP>
    static __device__ __forceinline__ void finish(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                  const F4& acc) {
        store_chunk<SP>(tb.w[gq.base + k], c, gq.lim, vec, acc);
        store_chunk<SP>(tb.p[gq.base + k], c, gq.lim, vec, pack4(acc));         // the model row: bf16 of the stored w
    }
};

Tune g_tune;

int adamw_mix_bf16(const mx_adamw_mix_bf16_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                   const int64_t* iter_dev, int64_t step, const int64_t* step_dev, float lr, const float* lr_dev,
                   void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->w_ptrs_dev && c->g_ptrs_dev && c->m_ptrs_dev && c->v_ptrs_dev && c->p_ptrs_dev && c->seg_len_dev &&
                 c->tile_off_dev && c->plan_dev && c->bias_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(c->n_bias >= 1, "%s: n_bias=%lld < 1", who, (long long)c->n_bias);
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(step_dev || step >= 1, "%s: optimizer step %lld < 1", who, (long long)step);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: w, m, v read + written, g read (+ zeroed), p written
    const int bpe = 28 + (c->zero_grads ? 2 : 0);
    const AdamHyper h{lr, c->wd, c->omb1, c->beta2, c->omb2, c->eps, lr_dev, gscale, c->bias_dev, c->n_bias, step, step_dev,
                      c->decoupled != 0, c->zero_grads != 0};
    return dispatch<AdamwMixBf16>(g_tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev, c->v_ptrs_dev,
                                  c->p_ptrs_dev);
}
}  // namespace

extern "C" int mx_adamw_mix_bf16_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_adamw_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_adamw_mix_bf16_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_adamw_mix_bf16_set(const char* key, int value) {
    return g_tune.set("mx_adamw_mix_bf16_set", key, value);
}

extern "C" int mx_adamw_mix_bf16_get(const char* key) { return g_tune.get("mx_adamw_mix_bf16_get", key); }

extern "C" int mx_adamw_mix_bf16(const mx_adamw_mix_bf16_call* c, int64_t iter, int64_t step, float lr,
                                 const float* lr_dev, void* stream) {
    return adamw_mix_bf16(c, nullptr, nullptr, iter, nullptr, step, nullptr, lr, lr_dev, stream, "mx_adamw_mix_bf16");
}

extern "C" int mx_adamw_mix_bf16_scaled(const mx_adamw_mix_bf16_call* c, const float* gscale_dev, int64_t iter,
                                        int64_t step, float lr, const float* lr_dev, void* stream) {
    return adamw_mix_bf16(c, nullptr, gscale_dev, iter, nullptr, step, nullptr, lr, lr_dev, stream, "mx_adamw_mix_bf16_scaled");
}

extern "C" int mx_adamw_mix_bf16_at(const mx_adamw_mix_bf16_call* c, const int64_t* iter_dev, int64_t n_iters,
                                    const int64_t* step_dev, float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev && step_dev, "mx_adamw_mix_bf16_at: null iteration or step counter");
    return adamw_mix_bf16(c, nullptr, nullptr, n_iters, iter_dev, 0, step_dev, lr, lr_dev, stream, "mx_adamw_mix_bf16_at");
}

extern "C" int mx_adamw_mix_bf16_scaled_at(const mx_adamw_mix_bf16_call* c, const float* gscale_dev,
                                           const int64_t* iter_dev, int64_t n_iters, const int64_t* step_dev,
                                           float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev && step_dev, "mx_adamw_mix_bf16_scaled_at: null iteration or step counter");
    return adamw_mix_bf16(c, nullptr, gscale_dev, n_iters, iter_dev, 0, step_dev, lr, lr_dev, stream,
                          "mx_adamw_mix_bf16_scaled_at");
}

extern "C" int mx_adamw_mix_bf16_grouped(const mx_adamw_mix_bf16_call* c, const mx_param_runs* runs,
                                         const float* gscale_dev, int64_t iter, int64_t step, float lr,
                                         const float* lr_dev, void* stream) {
    return adamw_mix_bf16(c, runs, gscale_dev, iter, nullptr, step, nullptr, lr, lr_dev, stream,
                          "mx_adamw_mix_bf16_grouped");
}

extern "C" int mx_adamw_mix_bf16_grouped_at(const mx_adamw_mix_bf16_call* c, const mx_param_runs* runs,
                                            const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters,
                                            const int64_t* step_dev, float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev && step_dev, "mx_adamw_mix_bf16_grouped_at: null iteration or step counter");
    return adamw_mix_bf16(c, runs, gscale_dev, n_iters, iter_dev, 0, step_dev, lr, lr_dev, stream,
                          "mx_adamw_mix_bf16_grouped_at");
}
