// adamw_mix.hip -- the AdamW / Adam update of every local worker fused into the mixing round (fp32
// rows, local-only groups): one launch per training iteration instead of n optimizer steps + one mix.
//
// Each row's x, g, m (exp_avg) and v (exp_avg_sq) elements are read once, torch.optim.AdamW's (decoupled)
// or torch.optim.Adam's (L2) single-tensor update is applied on the way into LDS, every operation one
// IEEE fp32 rounding (-ffp-contract=off, explicit fmas, correctly rounded sqrt and division)
//     decay = fmaf(-lr, wd, 1)                          once per launch
//     x1 = (wd != 0 &&  decoupled) ? fmul(x, decay) : x           p.mul_(1 - lr*wd)
//     g1 = (wd != 0 && !decoupled) ? fmaf(wd, x, g) : g           g.add(p, alpha=wd)
//     m' = fmaf(omb1, fsub(g1, m), m)                             exp_avg.lerp_(g, 1 - beta1)
//     v' = fmaf(omb2, fmul(g1, g1), fmul(beta2, v))               exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
//     den = fadd(fdiv(fsqrt(v'), bc2s), eps)
//     ss  = fdiv(lr, bc1)                               once per launch
//     x'  = fmaf(-ss, fdiv(m', den), x1)
// and the round of mix.hip's mix_kernel_rows then runs on the staged x' values exactly as in sgd_mix.hip:
// per output row the partners' columns in ascending matching order, the self term last, every step one
// __builtin_fmaf.  Rows the plan record does not read and write, and every row of a round whose flags
// are all zero, get x' stored as it is: an all-zero round is the optimizer step alone, not a no-op.
//
// (bc1, bc2s) = (1 - beta1^t, sqrt(1 - beta2^t)) of optimizer step t come from a host-built device table
// at entry min(t, n_bias) - 1 (the table ends where both are exactly 1.0f); t is an argument or, for
// graph replay, a device counter.  Nothing computes pow on the device.
//
// The square root is __builtin_sqrtf, which hipcc expands to v_sqrt_f32 on a scaled input plus the two-fma
// correction to the correctly rounded result (denormals kept: float_denorm_mode_32 = 3).  __fsqrt_rn is
// NOT used: in this ROCm's headers it is __ocml_native_sqrt_f32, the bare 1-ulp v_sqrt_f32.  The
// division is __fdiv_rn: v_div_scale / v_rcp / fma refinement / v_div_fmas / v_div_fixup.
//
// Traffic per element: read x, g, m, v, write x, m, v = 28 bytes (32 when the gradients are zeroed)
// against 88 for the torch op sequence followed by the mixing round.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  m and v are read and written by the same lane only, so
// they are stored when their chunk is staged; so are the zeros over g with zero_grads.  Because every
// row is read in every round, the first loads are issued before the plan record is looked at.
//
// No receive slots: n_slots == n_local, the plan's n_remote is 0; a record with the peer-reads bit, a
// round counter outside the schedule and a step counter below 1 each make the launch write nothing.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<AdamwMix, ...>).
#include "adam_update.h"

namespace {
using namespace mx::fused;

// x, g, m and v as fp32; 16-byte accesses only where x, g, m and v of the (segment, row) are all 16-byte
// aligned
struct AdamwMix {
    using Hyper = AdamHyper;
    using State = AdamState;
    struct Tabs {
        float* const* x;
        float* const* g;
        float* const* m;
        float* const* v;
    };
    struct Lane {
        F4 X[kB], G[kB], Mv[kB], Vv[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.x[gq.base + k]) && al16(tb.g[gq.base + k]) && al16(tb.m[gq.base + k]) && al16(tb.v[gq.base + k]);
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
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, F4{0.0f, 0.0f, 0.0f, 0.0f});
    }
    template <int SP>
    static __device__ __forceinline__ void finish(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                  const F4& acc) {
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
    }
};

Tune g_tune;

int adamw_mix(const mx_adamw_mix_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
              const int64_t* iter_dev, int64_t step, const int64_t* step_dev, float lr, const float* lr_dev,
              void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->x_ptrs_dev && c->g_ptrs_dev && c->m_ptrs_dev && c->v_ptrs_dev && c->seg_len_dev && c->tile_off_dev &&
                 c->plan_dev && c->bias_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(c->n_bias >= 1, "%s: n_bias=%lld < 1", who, (long long)c->n_bias);
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(step_dev || step >= 1, "%s: optimizer step %lld < 1", who, (long long)step);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: x, m, v read + written, g read (+ zeroed)
    const int bpe = 4 * (7 + (c->zero_grads ? 1 : 0));
    const AdamHyper h{lr, c->wd, c->omb1, c->beta2, c->omb2, c->eps, lr_dev, gscale, c->bias_dev, c->n_bias, step, step_dev,
                      c->decoupled != 0, c->zero_grads != 0};
    return dispatch<AdamwMix>(g_tune, r, bpe, h, runs, c->x_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev, c->v_ptrs_dev);
}
}  // namespace

extern "C" int mx_adamw_mix_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_adamw_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_adamw_mix_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_adamw_mix_set(const char* key, int value) { return g_tune.set("mx_adamw_mix_set", key, value); }

extern "C" int mx_adamw_mix_get(const char* key) { return g_tune.get("mx_adamw_mix_get", key); }

extern "C" int mx_adamw_mix(const mx_adamw_mix_call* c, int64_t iter, int64_t step, float lr, const float* lr_dev,
                            void* stream) {
    return adamw_mix(c, nullptr, nullptr, iter, nullptr, step, nullptr, lr, lr_dev, stream, "mx_adamw_mix");
}

extern "C" int mx_adamw_mix_scaled(const mx_adamw_mix_call* c, const float* gscale_dev, int64_t iter, int64_t step,
                                   float lr, const float* lr_dev, void* stream) {
    return adamw_mix(c, nullptr, gscale_dev, iter, nullptr, step, nullptr, lr, lr_dev, stream, "mx_adamw_mix_scaled");
}

extern "C" int mx_adamw_mix_at(const mx_adamw_mix_call* c, const int64_t* iter_dev, int64_t n_iters,
                               const int64_t* step_dev, float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev && step_dev, "mx_adamw_mix_at: null iteration or step counter");
    return adamw_mix(c, nullptr, nullptr, n_iters, iter_dev, 0, step_dev, lr, lr_dev, stream, "mx_adamw_mix_at");
}

extern "C" int mx_adamw_mix_scaled_at(const mx_adamw_mix_call* c, const float* gscale_dev, const int64_t* iter_dev,
                                      int64_t n_iters, const int64_t* step_dev, float lr, const float* lr_dev,
                                      void* stream) {
    MX_CHECK(iter_dev && step_dev, "mx_adamw_mix_scaled_at: null iteration or step counter");
    return adamw_mix(c, nullptr, gscale_dev, n_iters, iter_dev, 0, step_dev, lr, lr_dev, stream, "mx_adamw_mix_scaled_at");
}

extern "C" int mx_adamw_mix_grouped(const mx_adamw_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                    int64_t iter, int64_t step, float lr, const float* lr_dev, void* stream) {
    return adamw_mix(c, runs, gscale_dev, iter, nullptr, step, nullptr, lr, lr_dev, stream, "mx_adamw_mix_grouped");
}

extern "C" int mx_adamw_mix_grouped_at(const mx_adamw_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                       const int64_t* iter_dev, int64_t n_iters, const int64_t* step_dev, float lr,
                                       const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev && step_dev, "mx_adamw_mix_grouped_at: null iteration or step counter");
    return adamw_mix(c, runs, gscale_dev, n_iters, iter_dev, 0, step_dev, lr, lr_dev, stream, "mx_adamw_mix_grouped_at");
}
