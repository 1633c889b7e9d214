// qgm_mix.hip -- quasi-global momentum (QG-DSGDm: Lin et al., ICML 2021, "Quasi-Global Momentum:
// Accelerating Decentralized Deep Learning on Heterogeneous Data") fused into the mixing round (fp32 rows,
// local-only groups): one launch per training iteration applies every worker's local step, mixes the
// updated rows and feeds each worker's momentum buffer with the displacement of its row AFTER the round.
//
// A worker's buffer mh follows (x_t - x_{t+1}) / lr, the direction its neighbourhood actually moved, not
// its own shard's gradient; it costs no extra communication.  Per row and column, every line one fp32
// rounding (-ffp-contract=off, explicit fmas); g is widened and clip-scaled by grad_of, (wd_r, scale_r) are
// the run's pair (the launch's wd and 1.0 when ungrouped):
//     lr_r = fmul(lr, scale_r)
//     d    = (wd_r != 0) ? fmaf(wd_r, x, g) : g
//     m    = fadd(fmul(beta, mh), d)                      mh is read only here; m is never stored
//     s    = nesterov ? fmaf(beta, m, d) : m
//     x'   = fmaf(-lr_r, s, x)
//     y    = the round of sgd_mix.hip on the x' values: per output row the partners' columns in ascending
//            matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//            leaves alone, and every row of an all-zero round, keeps y = x'
//     rl   = fdiv(1.0f, lr_r)                             once per launch, or per run when grouped
//     q    = fmul(fsub(x, y), rl)                         x: the value the row held BEFORE this launch
//     mh'  = (lr_r != 0) ? fmaf(omu, fsub(q, mh), mh) : mh
//     x    = y
// omu is the fp32 rounding of the fp64 value 1 - mu.  An all-zero round is the local step plus the buffer
// update, not a no-op.  lr_r == 0 (lr = 0, or a run of scale 0) leaves mh bit for bit while x is still
// mixed.  q amplifies the rounding of x by 1 / lr: that is the algorithm's, in any fp32 implementation.
//
// Traffic per element: read x, g, mh, write x, mh = 20 bytes (24 when the gradients are zeroed): the bytes
// of SGD with momentum.  The buffer update needs x and mh again after the round; they are re-read by the
// lane that finishes the (row, chunk), moments after the workgroup staged the same lines.  That re-read is NOT
// free: the step measures well behind the SGD-momentum step of the same bytes, less so with x and mh staged
// with plain loads than with nt loads (which cache level serves it has not been counted).
//
// In place: the staging lane loads x, g and mh, parks x' in LDS and stores ONLY the zeros over g; it never
// stores mh.  After the barrier the lane that finishes a (row, chunk) reloads x and mh of its own 4 columns
// with plain loads, computes q and mh', stores mh' and then y.  No other lane writes either address in this
// launch, and the row's own x is stored only by this lane, after its reload; different work items never
// share a column.  The finish side honours the alignment rule too: 16-byte accesses only where x, g and mh
// of the (segment, row) are all 16-byte aligned and the chunk is in range, per element elsewhere; nothing
// is read or written at or past a row's length.
//
// No receive slots: n_slots == n_local; a device counter outside the schedule, or a record with the
// peer-reads bit, makes the launch write nothing, the buffer included.
//
// The row kernel, its mixing walk and the host side are fused_round.h's; this file is the policy that
// kernel is instantiated with (kernel traces show it as fused_round_rows<QgmMix<NESTEROV, PLAIN>, ...>).
#include "qgm_update.h"

namespace {
using namespace mx::fused;

// x, g and mh as fp32; 16-byte accesses only where x, g and mh of the (segment, row) are all 16-byte
// aligned.  PLAIN: x and mh are staged with plain loads where the launch streams (knob "stage_plain", the
// default), so that the finish side's reload finds more of their lines cached
template <bool NESTEROV, bool PLAIN = false>
struct QgmMix {
    static constexpr bool kAfterMix = true;
    using Hyper = QgmHyper;
    using State = QgmState;
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
        constexpr bool XNT = NT && !PLAIN;
        ln.X[t] = load_chunk<XNT>(tb.x[gq.base + k], c, gq.lim, vec);
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
        if (h.zero_grads) store_chunk<SP>(tb.g[gq.base + k], c, gq.lim, vec, F4{0.0f, 0.0f, 0.0f, 0.0f});
    }
    template <bool GROUPED, int SP>
    static __device__ __forceinline__ void after_mix(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                     const F4& acc, const State& st,
                                                     const GroupedIf<Hyper, GROUPED>& h) {
        const F4 x = load_chunk<false>(tb.x[gq.base + k], c, gq.lim, vec);     // the row before this launch
        const F4 mh = load_chunk<false>(tb.m[gq.base + k], c, gq.lim, vec);
        store_chunk<SP>(tb.m[gq.base + k], c, gq.lim, vec, qgm_buf_chunk<GROUPED>(x, acc, mh, c, gq, st, h));
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
    }
};

Tune g_tune;
int g_stage_plain = 1;     // "stage_plain": 1 = x and mh staged with plain loads (see QgmMix); 0 = with nt loads, as g

int qgm_mix(const mx_qgm_mix_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
            const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->x_ptrs_dev && c->g_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev,
             "%s: null pointer", who);
    Round r;
    if (const int rc = check_round(c, iter, iter_dev, stream, who, &r)) return rc;
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK(c->m_ptrs_dev, "%s: null buffer table (quasi-global momentum always carries its buffer)", who);
    if (const int rc = check_runs(runs, who)) return rc;
    if (c->total_tiles <= 0) return MX_OK;
    // bytes the round moves: x read + written, g read (+ zeroed), mh read + written
    const int bpe = 4 * (5 + (c->zero_grads ? 1 : 0));
    const QgmHyper h{lr, c->wd, c->beta, c->omu, lr_dev, gscale, c->zero_grads != 0};
#define MX_QGM(N, P) dispatch<QgmMix<N, P>>(g_tune, r, bpe, h, runs, c->x_ptrs_dev, c->g_ptrs_dev, c->m_ptrs_dev)
    if (c->nesterov) return g_stage_plain ? MX_QGM(true, true) : MX_QGM(true, false);
    return g_stage_plain ? MX_QGM(false, true) : MX_QGM(false, false);
#undef MX_QGM
}
}  // namespace

extern "C" int mx_qgm_mix_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_qgm_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    return layout("mx_qgm_mix_layout", seg_len_host, nseg, n_slots, tile_off_host);
}

extern "C" int mx_qgm_mix_set(const char* key, int value) {
    if (key && !strcmp(key, "stage_plain")) {
        MX_CHECK(value == 0 || value == 1, "mx_qgm_mix_set: stage_plain %d", value);
        g_stage_plain = value;
        return MX_OK;
    }
    return g_tune.set("mx_qgm_mix_set", key, value);
}

extern "C" int mx_qgm_mix_get(const char* key) {
    if (key && !strcmp(key, "stage_plain")) return g_stage_plain;
    return g_tune.get("mx_qgm_mix_get", key);
}

extern "C" int mx_qgm_mix(const mx_qgm_mix_call* c, int64_t iter, float lr, const float* lr_dev, void* stream) {
    return qgm_mix(c, nullptr, nullptr, iter, nullptr, lr, lr_dev, stream, "mx_qgm_mix");
}

extern "C" int mx_qgm_mix_scaled(const mx_qgm_mix_call* c, const float* gscale_dev, int64_t iter, float lr,
                                 const float* lr_dev, void* stream) {
    return qgm_mix(c, nullptr, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_qgm_mix_scaled");
}

extern "C" int mx_qgm_mix_at(const mx_qgm_mix_call* c, const int64_t* iter_dev, int64_t n_iters, float lr,
                             const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_qgm_mix_at: null iteration counter");
    return qgm_mix(c, nullptr, nullptr, n_iters, iter_dev, lr, lr_dev, stream, "mx_qgm_mix_at");
}

extern "C" int mx_qgm_mix_scaled_at(const mx_qgm_mix_call* c, const float* gscale_dev, const int64_t* iter_dev,
                                    int64_t n_iters, float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_qgm_mix_scaled_at: null iteration counter");
    return qgm_mix(c, nullptr, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_qgm_mix_scaled_at");
}

extern "C" int mx_qgm_mix_grouped(const mx_qgm_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                  int64_t iter, float lr, const float* lr_dev, void* stream) {
    return qgm_mix(c, runs, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_qgm_mix_grouped");
}

extern "C" int mx_qgm_mix_grouped_at(const mx_qgm_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                     const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                                     void* stream) {
    MX_CHECK(iter_dev, "mx_qgm_mix_grouped_at: null iteration counter");
    return qgm_mix(c, runs, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_qgm_mix_grouped_at");
}
