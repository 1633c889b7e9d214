// sgd_mix_bf16.hip -- mixed-precision SGD fused into the mixing round: bfloat16 models and gradients,
// fp32 master weights and momentum (local-only groups).  One launch per training iteration.
//
// sgd_mix.hip's launch for models held in bfloat16.  The optimizer state that has to keep small updates
// (lr * d is usually below half a bf16 ulp of the weight) is an fp32 master row; the master rows are what
// the round mixes, so nothing is lost to bf16 rounding between rounds, and the bf16 model row is the
// rounded image of the master, rewritten by every launch.  Per (segment, row) four arrays:
//     w  fp32 master      read and written in place
//     g  bf16 gradient    read; overwritten with zeros when zero_grads
//     m  fp32 momentum    read and written; absent when mom == 0
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (torch.optim.SGD, dampening 0, on the fp32 masters):
//     g32 = f32(g)                                        exact widening, bits << 16
//     d   = (wd != 0) ? fmaf(wd, w, g32) : g32
//     m   = fadd(fmul(mom, m), d)            [mom != 0]   two roundings (-ffp-contract=off)
//     d   = nesterov ? fmaf(mom, m, d) : m   [mom != 0]
//     w'  = fmaf(-lr, d, w)
//     w   = the round of sgd_mix.hip on the w' values: per output row the partners' columns in ascending
//           matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//           leaves alone, and every row of an all-zero round, keeps w' as it is
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// p is written for every row in every launch that runs, rows the round leaves alone included: their w
// changed by the SGD step.  A device counter outside the schedule, or a plan record with the peer-reads
// bit, makes the launch a complete no-op.  Nothing is written at or past a row's length in any array.
//
// Traffic per element: read w (4), g (2), m (4), write w (4), m (4), p (2) = 20 bytes (22 when the
// gradients are zeroed, 10 / 12 without momentum) against 64 for the unfused op sequence.
//
// A lane holds 4 elements: 16-byte accesses on w and m, 8-byte accesses on g and p.  Alignment rule: the
// vector path is taken where w and m of the (segment, row) are 16-byte aligned, g and p are 8-byte
// aligned and the 4 elements are in range; everything else goes element by element (4-byte / 2-byte
// accesses), zero-filled past the end.
//
// In place: a tile's w' of every row is parked in LDS as fp32 (barrier) before any w row of it is stored,
// and different work items never share a column.  m is read and written by the same lane only, so it is
// stored when its chunk is staged; so are the zeros over g.  Because every row is read in every round,
// the first loads are issued before the plan record is looked at.  No receive slots: n_slots == n_local.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<SgdMixBf16<MOM>, ...>).
#include "sgd_update.h"

namespace {
using namespace mx::fused;

// w and m as fp32, g and p as bf16; wide accesses only where the (segment, row)'s w and m are 16-byte and
// g and p 8-byte aligned
template <bool MOM>
struct SgdMixBf16 {
    using Hyper = SgdHyper;
    using State = SgdState;
    struct Tabs {
        float* const* w;
        uint16_t* const* g;
        float* const* m;
        uint16_t* const* p;
    };
    struct Lane {
        F4 X[kB], Mv[kB];
        U2 G[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        bool v = al16(tb.w[gq.base + k]) && al8(tb.g[gq.base + k]) && al8(tb.p[gq.base + k]);
        if constexpr (MOM) v = v && al16(tb.m[gq.base + k]);
        return v;
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        ln.X[t] = load_chunk<NT>(tb.w[gq.base + k], c, gq.lim, vec);
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

int sgd_mix_bf16(const mx_sgd_mix_bf16_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                 const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->w_ptrs_dev && c->g_ptrs_dev && c->p_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK((c->mom != 0.0f) == (c->m_ptrs_dev != nullptr), "%s: the momentum table is given exactly when mom != 0",
             who);
    MX_CHECK(c->mom != 0.0f || !c->nesterov, "%s: nesterov needs momentum", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    const bool mom = c->mom != 0.0f;
    // bytes the round moves: w read + written, g read (+ zeroed), p written, m read + written
    const int bpe = 12 + (mom ? 8 : 0) + (c->zero_grads ? 2 : 0);
    const SgdHyper h{lr, c->wd, c->mom, lr_dev, gscale, c->nesterov != 0, c->zero_grads != 0};
    return mom ? dispatch<SgdMixBf16<true>>(g_tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev,
                                            c->p_ptrs_dev)
               : dispatch<SgdMixBf16<false>>(g_tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev,
                                             c->p_ptrs_dev);
}
}  // namespace

extern "C" int mx_sgd_mix_bf16_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_sgd_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_sgd_mix_bf16_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_sgd_mix_bf16_set(const char* key, int value) {
    return g_tune.set("mx_sgd_mix_bf16_set", key, value);
}

extern "C" int mx_sgd_mix_bf16_get(const char* key) { return g_tune.get("mx_sgd_mix_bf16_get", key); }

extern "C" int mx_sgd_mix_bf16(const mx_sgd_mix_bf16_call* c, int64_t iter, float lr, const float* lr_dev,
                               void* stream) {
    return sgd_mix_bf16(c, nullptr, nullptr, iter, nullptr, lr, lr_dev, stream, "mx_sgd_mix_bf16");
}

extern "C" int mx_sgd_mix_bf16_scaled(const mx_sgd_mix_bf16_call* c, const float* gscale_dev, int64_t iter, float lr,
                                      const float* lr_dev, void* stream) {
    return sgd_mix_bf16(c, nullptr, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_sgd_mix_bf16_scaled");
}

extern "C" int mx_sgd_mix_bf16_at(const mx_sgd_mix_bf16_call* c, const int64_t* iter_dev, int64_t n_iters, float lr,
                                  const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_sgd_mix_bf16_at: null iteration counter");
    return sgd_mix_bf16(c, nullptr, nullptr, n_iters, iter_dev, lr, lr_dev, stream, "mx_sgd_mix_bf16_at");
}

extern "C" int mx_sgd_mix_bf16_scaled_at(const mx_sgd_mix_bf16_call* c, const float* gscale_dev,
                                         const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                                         void* stream) {
    MX_CHECK(iter_dev, "mx_sgd_mix_bf16_scaled_at: null iteration counter");
    return sgd_mix_bf16(c, nullptr, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_sgd_mix_bf16_scaled_at");
}

extern "C" int mx_sgd_mix_bf16_grouped(const mx_sgd_mix_bf16_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                       int64_t iter, float lr, const float* lr_dev, void* stream) {
    return sgd_mix_bf16(c, runs, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_sgd_mix_bf16_grouped");
}

extern "C" int mx_sgd_mix_bf16_grouped_at(const mx_sgd_mix_bf16_call* c, const mx_param_runs* runs,
                                          const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                                          const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_sgd_mix_bf16_grouped_at: null iteration counter");
    return sgd_mix_bf16(c, runs, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_sgd_mix_bf16_grouped_at");
}
