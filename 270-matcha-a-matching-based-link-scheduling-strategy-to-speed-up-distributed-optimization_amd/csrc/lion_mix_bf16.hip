// lion_mix_bf16.hip -- mixed-precision Lion fused into the mixing round: bfloat16 models and gradients,
// fp32 master weights, momentum in fp32 or in bfloat16 (local-only groups).  One launch per training
// iteration.
//
// lion_mix.hip's launch for models held in bfloat16, with sgd_mix_bf16.hip's load and store sides.  The
// fp32 master rows are what the optimizer updates and the round mixes, so nothing is lost to bf16
// rounding between rounds; the bf16 model row is the rounded image of the master, rewritten by every
// launch.  Per (segment, row) four arrays:
//     w  fp32 master      read and written in place
//     g  bf16 gradient    read; overwritten with zeros when zero_grads
//     m  momentum         read and written: fp32, or bf16 when the record's m_bf16 is set
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (lion_mix.hip's on the fp32 masters; every line one fp32 rounding):
//     g32 = f32(g)                                        exact widening, bits << 16
//     m32 = m, or f32(m) for a bf16 momentum              exact widening
//     decay = fmaf(-lr, wd, 1)                            once per launch
//     w1 = (wd != 0) ? fmul(w, decay) : w
//     dm = fsub(g32, m32)
//     c  = fmaf(omb1, dm, m32)
//     w' = c > 0 ? fsub(w1, lr) : c < 0 ? fadd(w1, lr) : c == 0 ? w1 : NaN
//     m' = fmaf(omb2, dm, m32);  a bf16 momentum stores bf16_rne(m'), rounded once at the store
//     w   = the round of sgd_mix.hip on the w' values: per output row the partners' columns in ascending
//           matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//           leaves alone, and every row of an all-zero round, keeps w' as it is
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// p is written for every row in every launch that runs, rows the round leaves alone included: their w
// changed by the Lion step.  A device counter outside the schedule, or a plan record with the peer-reads
// bit, makes the launch a complete no-op.  Nothing is written at or past a row's length in any array.
//
// Traffic per element, fp32 momentum: read w (4), g (2), m (4), write w (4), m (4), p (2) = 20 bytes (22
// when the gradients are zeroed); bf16 momentum: 16 (18).
//
// A lane holds 4 elements: 16-byte accesses on w (and an fp32 m), 8-byte accesses on g, p and a bf16 m.
// Alignment rule: the vector path is taken where w of the (segment, row) is 16-byte aligned, m is aligned
// to its own access (16 bytes fp32, 8 bytes bf16), g and p are 8-byte aligned and the 4 elements are in
// range; everything else goes element by element (4-byte / 2-byte accesses), zero-filled past the end.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<LionMixBf16<MB16>, ...>).
#include "lion_update.h"

namespace {
using namespace mx::fused;

// w as fp32, g and p as bf16, m as fp32 (MB16 = false) or bf16 (MB16 = true: held in flight as its 8
// bytes, widened for the update and rounded once on the way back)
template <bool MB16>
struct LionMixBf16 {
    using Hyper = LionHyper;
    using State = LionState;
    using MT = std::conditional_t<MB16, uint16_t, float>;
    using MC = std::conditional_t<MB16, U2, F4>;
    struct Tabs {
        float* const* w;
        uint16_t* const* g;
        MT* const* m;
        uint16_t* const* p;
    };
    struct Lane {
        F4 X[kB];
        MC Mv[kB];
        U2 G[kB];
    };
    static __device__ __forceinline__ bool vec_of(const Tabs& tb, const Geo& gq, int k) {
        const bool v = al16(tb.w[gq.base + k]) && al8(tb.g[gq.base + k]) && al8(tb.p[gq.base + k]);
        if constexpr (MB16) return v && al8(tb.m[gq.base + k]);
        else return v && al16(tb.m[gq.base + k]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        ln.X[t] = load_chunk<NT>(tb.w[gq.base + k], c, gq.lim, vec);
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

int lion_mix_bf16(const mx_lion_mix_bf16_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                  const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->w_ptrs_dev && c->g_ptrs_dev && c->p_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(c->m_ptrs_dev, "%s: null momentum table (Lion always carries momentum)", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    const bool mb16 = c->m_bf16 != 0;
    // bytes the round moves: w read + written, g read (+ zeroed), p written, m read + written
    const int bpe = 12 + (mb16 ? 4 : 8) + (c->zero_grads ? 2 : 0);
    const LionHyper h{lr, c->wd, c->omb1, c->omb2, lr_dev, gscale, c->zero_grads != 0};
    return mb16 ? dispatch<LionMixBf16<true>>(g_tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev,
                                              reinterpret_cast<uint16_t* const*>(c->m_ptrs_dev), c->p_ptrs_dev)
                : dispatch<LionMixBf16<false>>(g_tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev,
                                               reinterpret_cast<float* const*>(c->m_ptrs_dev), c->p_ptrs_dev);
}
}  // namespace

extern "C" int mx_lion_mix_bf16_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_lion_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_lion_mix_bf16_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_lion_mix_bf16_set(const char* key, int value) {
    return g_tune.set("mx_lion_mix_bf16_set", key, value);
}

extern "C" int mx_lion_mix_bf16_get(const char* key) { return g_tune.get("mx_lion_mix_bf16_get", key); }

extern "C" int mx_lion_mix_bf16(const mx_lion_mix_bf16_call* c, int64_t iter, float lr, const float* lr_dev,
                                void* stream) {
    return lion_mix_bf16(c, nullptr, nullptr, iter, nullptr, lr, lr_dev, stream, "mx_lion_mix_bf16");
}

extern "C" int mx_lion_mix_bf16_scaled(const mx_lion_mix_bf16_call* c, const float* gscale_dev, int64_t iter, float lr,
                                       const float* lr_dev, void* stream) {
    return lion_mix_bf16(c, nullptr, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_lion_mix_bf16_scaled");
}

extern "C" int mx_lion_mix_bf16_at(const mx_lion_mix_bf16_call* c, const int64_t* iter_dev, int64_t n_iters, float lr,
                                   const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_lion_mix_bf16_at: null iteration counter");
    return lion_mix_bf16(c, nullptr, nullptr, n_iters, iter_dev, lr, lr_dev, stream, "mx_lion_mix_bf16_at");
}

extern "C" int mx_lion_mix_bf16_scaled_at(const mx_lion_mix_bf16_call* c, const float* gscale_dev,
                                          const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                                          void* stream) {
    MX_CHECK(iter_dev, "mx_lion_mix_bf16_scaled_at: null iteration counter");
    return lion_mix_bf16(c, nullptr, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_lion_mix_bf16_scaled_at");
}

extern "C" int mx_lion_mix_bf16_grouped(const mx_lion_mix_bf16_call* c, const mx_param_runs* runs,
                                        const float* gscale_dev, int64_t iter, float lr, const float* lr_dev,
                                        void* stream) {
    return lion_mix_bf16(c, runs, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_lion_mix_bf16_grouped");
}

extern "C" int mx_lion_mix_bf16_grouped_at(const mx_lion_mix_bf16_call* c, const mx_param_runs* runs,
                                           const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                                           const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_lion_mix_bf16_grouped_at: null iteration counter");
    return lion_mix_bf16(c, runs, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_lion_mix_bf16_grouped_at");
}
