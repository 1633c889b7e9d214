// lion_mix.hip -- the Lion update of every local worker fused into the mixing round (fp32 rows,
// local-only groups): one launch per training iteration instead of n optimizer steps + one mix.
//
// Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") steps every weight by
// +-lr along the sign of an interpolation of gradient and momentum, with decoupled weight decay: one
// state array, no sqrt, no division, no bias correction and no step counter.  Each row's x, g and m
// elements are read once and the update is applied on the way into LDS, every line one fp32 rounding
// (-ffp-contract=off, explicit fmas):
//     decay = fmaf(-lr, wd, 1)                            once per launch
//     x1 = (wd != 0) ? fmul(x, decay) : x                 decoupled decay, as AdamW's
//     dm = fsub(g, m)
//     c  = fmaf(omb1, dm, m)                              (1 - beta1) g + beta1 m in lerp form
//     x' = c > 0 ? fsub(x1, lr) : c < 0 ? fadd(x1, lr) : c == 0 ? x1 : NaN
//     m' = fmaf(omb2, dm, m)                              (1 - beta2) g + beta2 m
// omb1 / omb2 are the fp32 roundings of the fp64 values 1 - beta.  A zero direction (either zero)
// leaves x1 bit for bit, -0.0 included; a NaN direction gives a NaN of any payload.  The round of
// sgd_mix.hip then runs on the staged x' values: per output row the partners' columns in ascending
// matching order, the self term last, every step one __builtin_fmaf.  Rows the plan record does not
// read and write (degree 0 outside idle mode 1), and every row of a round whose flags are all zero, get
// x' stored as it is: an all-zero round is the Lion step alone, not a no-op.
//
// Traffic per element: read x, g, m, write x, m = 20 bytes (24 when the gradients are zeroed): the
// bytes of SGD with momentum.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  m is read and written by the same lane only, so it is
// stored when its chunk is staged; so are the zeros over g with zero_grads.  No receive slots:
// n_slots == n_local; a device counter outside the schedule, or a record with the peer-reads bit, makes
// the launch write nothing.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<LionMix, ...>).
#include "lion_update.h"

namespace {
using namespace mx::fused;

// x, g and m as fp32; 16-byte accesses only where x, g and m of the (segment, row) are all 16-byte aligned
struct LionMix {
    using Hyper = LionHyper;
    using State = LionState;
    struct Tabs {
        float* const* x;
        float* const* g;
        float* const* m;
    };
    struct Lane {
        F4 X[kB], G[kB], Mv[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.x[gq.base + k]) && al16(tb.g[gq.base + k]) && al16(tb.m[gq.base + k]);
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
        return lion_chunk<GROUPED>(ln.X[t], grad_of(ln.G[t], h, k), ln.Mv[t], c, gq, st, h);
    }
    template <int SP>
    static __device__ __forceinline__ void keep(const Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec, const Hyper& h) {
        store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, ln.Mv[t]);
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, F4{0.0f, 0.0f, 0.0f, 0.0f});
    }
    template <int SP>
    static __device__ __forceinline__ void finish(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                  const F4& acc) {
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
    }
};

Tune g_tune;

int lion_mix(const mx_lion_mix_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
             const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->x_ptrs_dev && c->g_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(c->m_ptrs_dev, "%s: null momentum table (Lion always carries momentum)", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: x read + written, g read (+ zeroed), m read + written
    const int bpe = 4 * (5 + (c->zero_grads ? 1 : 0));
    const LionHyper h{lr, c->wd, c->omb1, c->omb2, lr_dev, gscale, c->zero_grads != 0};
    return dispatch<LionMix>(g_tune, r, bpe, h, runs, c->x_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev);
}
}  // namespace

extern "C" int mx_lion_mix_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_lion_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_lion_mix_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_lion_mix_set(const char* key, int value) { return g_tune.set("mx_lion_mix_set", key, value); }

extern "C" int mx_lion_mix_get(const char* key) { return g_tune.get("mx_lion_mix_get", key); }

extern "C" int mx_lion_mix(const mx_lion_mix_call* c, int64_t iter, float lr, const float* lr_dev, void* stream) {
    return lion_mix(c, nullptr, nullptr, iter, nullptr, lr, lr_dev, stream, "mx_lion_mix");
}

extern "C" int mx_lion_mix_scaled(const mx_lion_mix_call* c, const float* gscale_dev, int64_t iter, float lr,
                                  const float* lr_dev, void* stream) {
    return lion_mix(c, nullptr, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_lion_mix_scaled");
}

extern "C" int mx_lion_mix_at(const mx_lion_mix_call* c, const int64_t* iter_dev, int64_t n_iters, float lr,
                              const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_lion_mix_at: null iteration counter");
    return lion_mix(c, nullptr, nullptr, n_iters, iter_dev, lr, lr_dev, stream, "mx_lion_mix_at");
}

extern "C" int mx_lion_mix_scaled_at(const mx_lion_mix_call* c, const float* gscale_dev, const int64_t* iter_dev,
                                     int64_t n_iters, float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_lion_mix_scaled_at: null iteration counter");
    return lion_mix(c, nullptr, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_lion_mix_scaled_at");
}

extern "C" int mx_lion_mix_grouped(const mx_lion_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                   int64_t iter, float lr, const float* lr_dev, void* stream) {
    return lion_mix(c, runs, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_lion_mix_grouped");
}

extern "C" int mx_lion_mix_grouped_at(const mx_lion_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                      const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                                      void* stream) {
    MX_CHECK(iter_dev, "mx_lion_mix_grouped_at: null iteration counter");
    return lion_mix(c, runs, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_lion_mix_grouped_at");
}
