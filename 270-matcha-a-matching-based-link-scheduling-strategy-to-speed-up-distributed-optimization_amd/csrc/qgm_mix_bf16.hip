// qgm_mix_bf16.hip -- mixed-precision quasi-global momentum fused into the mixing round: bfloat16 models
// and gradients, fp32 master weights and an fp32 momentum buffer (local-only groups).  One launch per
// training iteration.
//
// qgm_mix.hip's launch for models held in bfloat16, with sgd_mix_bf16.hip's arrays.  Per (segment, row):
//     w   fp32 master           read and written in place
//     g   bf16 gradient         read; overwritten with zeros when zero_grads
//     mh  fp32 buffer           the quasi-global momentum: read, and written after the round
//     p   bf16 model row        WRITE ONLY: never read
// Arithmetic contract: qgm_mix.hip's lines on w with g32 = f32(g) (exact widening, bits << 16), every line
// one fp32 rounding:
//     lr_r = fmul(lr, scale_r)
//     d    = (wd_r != 0) ? fmaf(wd_r, w, g32) : g32
//     m    = fadd(fmul(beta, mh), d)
//     s    = nesterov ? fmaf(beta, m, d) : m
//     w'   = fmaf(-lr_r, s, w)
//     y    = the round of sgd_mix.hip on the w' values; a row the plan record leaves alone, and every row
//            of an all-zero round, keeps y = w'
//     q    = fmul(fsub(w, y), fdiv(1.0f, lr_r))           w: the master BEFORE this launch
//     mh'  = (lr_r != 0) ? fmaf(omu, fsub(q, mh), mh) : mh
//     w    = y;   p = bf16_rne(y)                         ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// p is written for every row in every launch that runs.  A device counter outside the schedule, or a plan
// record with the peer-reads bit, makes the launch a complete no-op, the buffer included.  Nothing is read
// or written at or past a row's length in any array.
//
// Traffic per element: read w (4), g (2), mh (4), write w (4), mh (4), p (2) = 20 bytes (22 when the
// gradients are zeroed): the bytes of mixed-precision SGD with momentum.  The finish side re-reads w and mh
// moments after the workgroup staged their lines; that re-read is NOT free (the step measures
// behind mixed-precision SGD with momentum, less so with w and mh staged with plain loads than with nt loads).
//
// A lane holds 4 elements: 16-byte accesses on w and mh, 8-byte accesses on g and p.  Alignment rule, on
// the staging and the finish side alike: the vector path is taken where w and mh of the (segment, row) are
// 16-byte aligned, g and p are 8-byte aligned and the 4 elements are in range; everything else goes element
// by element (4-byte / 2-byte accesses), zero-filled past the end.
//
// In place: as qgm_mix.hip.  The staging lane stores only the zeros over g; the lane that finishes a (row,
// chunk) reloads w and mh of its own 4 columns with plain loads, stores mh', then y and p.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<QgmMixBf16<NESTEROV, PLAIN>, ...>).
#include "qgm_update.h"

namespace {
using namespace mx::fused;

// w and mh as fp32, g and p as bf16; wide accesses only where the (segment, row)'s w and mh are 16-byte and
// g and p 8-byte aligned.  PLAIN: w and mh are staged with plain loads where the launch streams (knob
// "stage_plain", the default)
template <bool NESTEROV, bool PLAIN = false>
struct QgmMixBf16 {
    static constexpr bool kAfterMix = true;
    using Hyper = QgmHyper;
    using State = QgmState;
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
        return al16(tb.w[gq.base + k]) && al8(tb.g[gq.base + k]) && al8(tb.p[gq.base + k]) && al16(tb.m[gq.base + k]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load(Lane& ln, int t, const Tabs& tb, const Geo& gq, int k, int64_t c,
                                                bool vec) {
        constexpr bool XNT = NT && !PLAIN;
        ln.X[t] = load_chunk<XNT>(tb.w[gq.base + k], c, gq.lim, vec);
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
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, U2{0u, 0u});
    }
    template <bool GROUPED, int SP>
    static __device__ __forceinline__ void after_mix(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                     const F4& acc, const State& st,
                                                     const GroupedIf<Hyper, GROUPED>& h) {
        const F4 w = load_chunk<false>(tb.w[gq.base + k], c, gq.lim, vec);     // the master before this launch
        const F4 mh = load_chunk<false>(tb.m[gq.base + k], c, gq.lim, vec);
        store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, qgm_buf_chunk<GROUPED>(w, acc, mh, c, gq, st, h));
        store_chunk<SP>(tb.w[gq.base + k], c, gq.lim, vec, acc);
        store_chunk<SP>(tb.p[gq.base + k], c, gq.lim, vec, pack4(acc));         // the model row: bf16 of the stored w
    }
};

Tune g_tune;
int g_stage_plain = 1;     // "stage_plain": 1 = w and mh staged with plain loads (see QgmMixBf16); 0 = with nt loads, as g

int qgm_mix_bf16(const mx_qgm_mix_bf16_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
                 const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->w_ptrs_dev && c->g_ptrs_dev && c->p_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(c->m_ptrs_dev, "%s: null buffer table (quasi-global momentum always carries its buffer)", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: w read + written, g read (+ zeroed), p written, mh read + written
    const int bpe = 20 + (c->zero_grads ? 2 : 0);
    const QgmHyper h{lr, c->wd, c->beta, c->omu, lr_dev, gscale, c->zero_grads != 0};
#define MX_QGM(N, P)                                                                                           \
    dispatch<QgmMixBf16<N, P>>(g_tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev, c->p_ptrs_dev)
    if (c->nesterov) return g_stage_plain ? MX_QGM(true, true) : MX_QGM(true, false);
    return g_stage_plain ? MX_QGM(false, true) : MX_QGM(false, false);
#undef MX_QGM
}
}  // namespace

extern "C" int mx_qgm_mix_bf16_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_qgm_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_qgm_mix_bf16_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_qgm_mix_bf16_set(const char* key, int value) {
    if (key && !strcmp(key, "stage_plain")) {
        MX_CHECK(value == 0 || value == 1, "mx_qgm_mix_bf16_set: stage_plain %d", value);
        g_stage_plain = value;
        return MX_OK;
    }
    return g_tune.set("mx_qgm_mix_bf16_set", key, value);
}

extern "C" int mx_qgm_mix_bf16_get(const char* key) {
    if (key && !strcmp(key, "stage_plain")) return g_stage_plain;
    return g_tune.get("mx_qgm_mix_bf16_get", key);
}

extern "C" int mx_qgm_mix_bf16(const mx_qgm_mix_bf16_call* c, int64_t iter, float lr, const float* lr_dev,
                               void* stream) {
    return qgm_mix_bf16(c, nullptr, nullptr, iter, nullptr, lr, lr_dev, stream, "mx_qgm_mix_bf16");
}

extern "C" int mx_qgm_mix_bf16_scaled(const mx_qgm_mix_bf16_call* c, const float* gscale_dev, int64_t iter, float lr,
                                      const float* lr_dev, void* stream) {
    return qgm_mix_bf16(c, nullptr, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_qgm_mix_bf16_scaled");
}

extern "C" int mx_qgm_mix_bf16_at(const mx_qgm_mix_bf16_call* c, const int64_t* iter_dev, int64_t n_iters, float lr,
                                  const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_qgm_mix_bf16_at: null iteration counter");
    return qgm_mix_bf16(c, nullptr, nullptr, n_iters, iter_dev, lr, lr_dev, stream, "mx_qgm_mix_bf16_at");
}

extern "C" int mx_qgm_mix_bf16_scaled_at(const mx_qgm_mix_bf16_call* c, const float* gscale_dev,
                                         const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                                         void* stream) {
    MX_CHECK(iter_dev, "mx_qgm_mix_bf16_scaled_at: null iteration counter");
    return qgm_mix_bf16(c, nullptr, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_qgm_mix_bf16_scaled_at");
}

extern "C" int mx_qgm_mix_bf16_grouped(const mx_qgm_mix_bf16_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                       int64_t iter, float lr, const float* lr_dev, void* stream) {
    return qgm_mix_bf16(c, runs, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_qgm_mix_bf16_grouped");
}

extern "C" int mx_qgm_mix_bf16_grouped_at(const mx_qgm_mix_bf16_call* c, const mx_param_runs* runs,
                                          const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                                          const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_qgm_mix_bf16_grouped_at: null iteration counter");
    return qgm_mix_bf16(c, runs, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_qgm_mix_bf16_grouped_at");
}
