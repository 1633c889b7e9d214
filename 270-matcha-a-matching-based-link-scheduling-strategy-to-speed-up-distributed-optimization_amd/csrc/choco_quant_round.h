// choco_quant_round.h -- the one-launch quantized ChocoSGD round as one kernel over a storage form and a step
// policy, and its host side: what choco_quant_round.hip (fp32 models: Fp32Io), choco_quant_round_bf16.hip
// (bfloat16 models and gradients over fp32 x, x_hat, s and m: Bf16Io) and the AdamW forms
// (choco_quant_adamw_round.h: AdamStep) share.  The design is at the head of choco_quant_round.hip, the
// mixed-precision contract at the head of choco_quant_round_bf16.hip.  A form says how g is held and widened and
// whether an image of the final x is written; everything between the widening and the x store is the same
// instructions in both, so x, x_hat, s, m and the norms are the same bits for gradients of the same values.  A step
// says what happens between "x and x_hat are loaded" and "x' is known"; the schedule lookup, the quantizer, the
// barrier and the apply phase exist once, in quant_round.
#pragma once
#include "choco_quant.h"
#include "mx_common.h"
#include "sgd_update.h"

namespace mx {
namespace choco {
namespace qround {
using namespace mx::choco::quant;
using mx::fused::SgdHyper;
using mx::fused::SgdState;
using mx::fused::U2;

constexpr int kItems = 16;                // (row, bucket) items of a tile
constexpr int kIPW = kItems / kWV;        // items a wave owns: 4
constexpr int kMaxRows = kItems;
static_assert(kBucket == 64 * 4, "a lane owns 4 consecutive columns of an item");

// the scalars of a launch as one record, the arrays as __restrict__ kernel parameters (as ApplyDims)
struct RoundDims {
    int64_t ld, P, norm_ld, tiles;
    int64_t round, n_iters, words;        // the round (host counter), or with iter_dev the schedule's length
    uint32_t seed_mix;                    // mix32(u32(seed))
    int n_local, M, row_base, bshift;     // 1 << bshift buckets of a row per tile
    float alpha, g;
};

// 4 columns of a row from column c: one 16-byte access, or (rows off a 16-byte boundary, the bucket that holds
// P) element by element with +0 / nothing at and past P
template <bool NT>
__device__ __forceinline__ F4 load_q(const float* p, int64_t c, bool vec, int64_t P) {
    if (vec) return ld4<NT>(p + c);
    F4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < P) v[t] = ld1(p + c + t);
    return v;
}
template <bool NT>
__device__ __forceinline__ void store_q(const F4& v, float* p, int64_t c, bool vec, int64_t P) {
    if (vec) {
        st4<NT>(v, p + c);
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < P) *(GPtr<float>)(p + c + t) = v[t];
}
// the same 4 columns of a bfloat16 row: one 8-byte access, or 2-byte accesses under the same rule
template <bool NT>
__device__ __forceinline__ U2 load_q(const uint16_t* p, int64_t c, bool vec, int64_t P) {
    if (vec) return mx::fused::ld8<NT>(p + c);
    U2 v = {0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < P) v[t >> 1] |= ld2(p + c + t) << (16 * (t & 1));
    return v;
}
template <bool NT>
__device__ __forceinline__ void store_q(const U2& v, uint16_t* p, int64_t c, bool vec, int64_t P) {
    if (vec) {
        mx::fused::st8<NT ? mx::kStoreNt : mx::kStorePlain>(p + c, v);
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < P) st2(p + c + t, v[t >> 1] >> (16 * (t & 1)));
}

// the storage forms.  GT / GC: the gradient's element and a lane's 4 of them, al_g: a row of them takes the
// form's wide access (16 bytes, 8 bytes); kImage: the launch writes p = bf16_rne(x) wherever it writes x
struct Fp32Io {
    using GT = float;
    using GC = F4;
    static constexpr bool kImage = false;
    static __device__ __forceinline__ GC zero() { return F4{0.0f, 0.0f, 0.0f, 0.0f}; }
    static __device__ __forceinline__ bool al_g(const GT* g) { return al16(g); }
};
struct Bf16Io {
    using GT = uint16_t;
    using GC = U2;
    static constexpr bool kImage = true;
    static __device__ __forceinline__ GC zero() { return U2{0u, 0u}; }
    static __device__ __forceinline__ bool al_g(const GT* g) { return mx::fused::al8(g); }
};

// the kernel's last argument: the step's constants and in a form with an image p: a member, not a parameter of
// its own, so the fp32 kernel's argument block is what it was before there was a second form
template <class H, bool IMAGE>
struct Tail {
    H h;
};
template <class H>
struct Tail<H, true> {
    H h;
    uint16_t* p;
};
template <class IO, class H>
Tail<H, IO::kImage> make_tail(const H& h, uint16_t* p) {
    if constexpr (IO::kImage) return {h, p};
    else return {h};
}

// message item `it` of LDS image (cw, un) applied to a lane's four columns
template <int BITS, bool OWN>
__device__ __forceinline__ void apply_item(const uint32_t (*cw)[64], const float* un, int it, int lane, float w, F4& sv,
                                           F4& hv) {
    const uint32_t wd = cw[it][lane];
    const float unit = un[it];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float se = sv[c], he = hv[c];                                // (a vector's element binds to no reference)
        upd<BITS, OWN>(se, he, w, unit, wd >> (8 * c));
        sv[c] = se;
        if constexpr (OWN) hv[c] = he;
    }
}

// x and, in a form with an image, its rounded image next to it: packed from the registers that hold x
template <class IO, bool NT, class TL>
__device__ __forceinline__ void store_x(const F4& xv, float* x, const TL& tl, int64_t off, int64_t c, bool vec,
                                        int64_t P) {
    store_q<NT>(xv, x + off, c, vec, P);
    if constexpr (IO::kImage) store_q<NT>(mx::fused::pack4(xv), tl.p + off, c, vec, P);
}

// A step policy is a struct of types and static functions (fused_round.h's idiom); it supplies
//   Hyper, State, no_step, setup   the launch's constants, "this launch does nothing", what a launch derives
//   kSteps                         false: the round alone, an inactive round of the schedule writes nothing
//   Held<IO>, clear, hold          what of a wave's four items stays in flight across the tile, loaded with x and
//                                  x_hat before the first use (SGD: g and m)
//   Stream<IO>, load               what of one item streams (AdamW: g, m, v): two sets alternate, item q + 1's
//                                  loads are issued before item q's update
//   al                             the item's alignment conjunction so far, and the step's arrays' part of it
//   step                           x to x' in a lane's four columns, then the stores: the state rows, the zeros over g
// (StepBase: nothing held, nothing streamed, no part in the alignment -- a step overrides what it has)
//   given, check, kernel           the host side: its pointers, its argument checks, its instantiation
// The state rows (m; m and v) are the kernel's own __restrict__ parameters, one per element of the pack F.
// NoStep keeps SgdStep's argument block (g, m and SgdHyper, unused): the round alone is launched as it always was.
template <class IO, class Step, int BITS, bool NT, class... F>
__global__ __launch_bounds__(kTPB) void quant_round(float* __restrict__ x, typename IO::GT* __restrict__ g,
                                                    F* __restrict__... rows, float* __restrict__ xh,
                                                    float* __restrict__ s, float* __restrict__ norms,
                                                    const int32_t* __restrict__ rec_in,
                                                    const int64_t* __restrict__ iter_dev, RoundDims a,
                                                    Tail<typename Step::Hyper, IO::kImage> tl) {
    const typename Step::Hyper& h = tl.h;
    __shared__ uint32_t codes[2][kItems][64];                        // one byte per column, a word per lane
    __shared__ float units[2][kItems];                               // fmul(norm, c) of each item
    // round_rec's rules (choco_round.h), except that under a step an inactive round of the schedule still steps
    int64_t rnd = a.round;
    const int32_t* __restrict__ rec = rec_in;
    bool on = true;
    if (iter_dev) {
        rnd = *iter_dev;
        if (rnd < 0 || rnd >= a.n_iters) return;                     // outside the schedule: nothing, no step either
        rec = rec_in + rnd * a.words;
        on = rec[0] != 0;
    }
    if (rec[1] != 0 || (rec[2] & 2)) return;                         // receive slots, peer reads: not this kernel's
    if (!Step::kSteps && !on) return;
    typename Step::State st;
    if (Step::no_step(st, h)) return;                                // (AdamW: an optimizer step below 1) nothing
    Step::setup(st, h);                                              // -lr / the bias corrections, lr from lr_dev
    const uint32_t kr = mix32(a.seed_mix ^ (uint32_t)rnd);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t* deg = rec + mx::kPlanHeader;
    const int bmask = (1 << a.bshift) - 1;
    const F4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    int par = 0;
    for (int64_t w = blockIdx.x; w < a.tiles; w += gridDim.x, par ^= 1) {
        // the wave's items: row, first column of the lane, live (a row of the group, a bucket below P), vec
        int64_t off[kIPW], col[kIPW];
        bool live[kIPW], vec[kIPW];
        F4 xv[kIPW], hv[kIPW];
        typename Step::template Held<IO> hd;
        typename Step::template Stream<IO> sm[2];
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            const int64_t b0 = ((w << a.bshift) + (i & bmask)) * kBucket;
            off[q] = (int64_t)r * a.ld;
            col[q] = b0 + lane * 4;
            live[q] = r < a.n_local && b0 < a.P;
            vec[q] = Step::template al<IO>(
                b0 + kBucket <= a.P && al16(x + off[q]) && al16(xh + off[q]) && al16(s + off[q]), g, rows..., off[q]);
            if constexpr (IO::kImage) vec[q] = vec[q] && mx::fused::al8(tl.p + off[q]);
            xv[q] = hv[q] = zero;
            Step::template clear<IO>(hd, q);
            if (live[q]) {
                xv[q] = load_q<NT>(x + off[q], col[q], vec[q], a.P);
                hv[q] = load_q<NT>(xh + off[q], col[q], vec[q], a.P);
                Step::template hold<IO, NT>(hd, q, g, rows..., off[q], col[q], vec[q], a.P);
            }
        }
        // what a step streams alternates between two sets: item q + 1's loads are issued before item q's update, and
        // an item's set is free again as soon as its state rows and the zeros over g are stored
        if (live[0]) sm[0] = Step::template load<IO, NT>(g, rows..., off[0], col[0], vec[0], a.P);
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            if (q + 1 < kIPW && live[q + 1])
                sm[(q + 1) & 1] = Step::template load<IO, NT>(g, rows..., off[q + 1], col[q + 1], vec[q + 1], a.P);
            if (!live[q]) continue;                                  // wave-uniform
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            if constexpr (Step::kSteps) {
                Step::template step<IO, NT>(xv[q], hd, q, sm[q & 1], st, h, g, rows..., off[q], col[q], vec[q], a.P);
                if (!on) {                                           // no active matching: the step alone
                    store_x<IO, NT>(xv[q], x, tl, off[q], col[q], vec[q], a.P);
                    continue;
                }
            }
            float d[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                d[t] = __fsub_rn(xv[q][t], hv[q][t]);
                if (!vec[q] && col[q] + t >= a.P) d[t] = 0.0f;       // past P: +0 to the norm, a zero code
            }
            const uint32_t key = mix32(kr ^ (uint32_t)(a.row_base + r));
            float norm;
            uint32_t word = quant_pass<BITS>(d, key + (uint32_t)col[q], norm);
            if constexpr (BITS == 4)                                 // nibble t to byte t
                word = (word & 0xfu) | (word & 0xf0u) << 4 | (word & 0xf00u) << 8 | (word & 0xf000u) << 12;
            codes[par][i][lane] = word;
            if (lane == 0) {
                units[par][i] = __fmul_rn(norm, Lv<BITS>::c);
                if (norms) *(GPtr<float>)(norms + (int64_t)r * a.norm_ld + (col[q] >> 8)) = norm;
            }
        }
        if (!on) continue;                                           // kernel-uniform
        __syncthreads();
        // phase 2: the step's lanes are gone, so s of all four items fits beside x' and x_hat
        F4 sv[kIPW];
#pragma unroll
        for (int q = 0; q < kIPW; ++q)
            if (live[q]) sv[q] = load_q<NT>(s + off[q], col[q], vec[q], a.P);
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            if (!live[q]) continue;
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            const int b = i & bmask;
            const int dg = deg[r];                                   // active partners of the row
            const float sw = __int_as_float(deg[a.n_local + r]);     // the record's self weight
            const int32_t* src = deg + 2 * a.n_local + r * a.M;      // their rows, ascending matching
            for (int e = 0; e < dg; ++e)                             // (the mask: no index leaves the LDS image)
                apply_item<BITS, false>(codes[par], units[par], ((src[e] << a.bshift) + b) & (kItems - 1), lane,
                                        a.alpha, sv[q], hv[q]);
            apply_item<BITS, true>(codes[par], units[par], i, lane, sw, sv[q], hv[q]);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                xv[q][c] = __builtin_fmaf(-a.g, hv[q][c], __builtin_fmaf(a.g, sv[q][c], xv[q][c]));
            store_x<IO, NT>(xv[q], x, tl, off[q], col[q], vec[q], a.P);
            store_q<NT>(sv[q], s + off[q], col[q], vec[q], a.P);
            store_q<NT>(hv[q], xh + off[q], col[q], vec[q], a.P);
        }
    }
}

template <class IO, class Step, class... F>
auto pick(int bits, bool nt) {
    return bits == 4 ? (nt ? quant_round<IO, Step, 4, true, F...> : quant_round<IO, Step, 4, false, F...>)
                     : (nt ? quant_round<IO, Step, 8, true, F...> : quant_round<IO, Step, 8, false, F...>);
}

// what a step inherits: nothing held, nothing streamed, no part in the alignment
struct StepBase {
    struct None {};
    template <class IO>
    using Held = None;
    template <class IO>
    using Stream = None;
    template <class IO, class... A>
    static __device__ __forceinline__ bool al(bool base, A...) { return base; }
    template <class IO>
    static __device__ __forceinline__ void clear(None&, int) {}
    template <class IO, bool NT, class... A>
    static __device__ __forceinline__ void hold(None&, int, A...) {}
    template <class IO, bool NT, class... A>
    static __device__ __forceinline__ None load(A...) { return {}; }
};

struct NoStep : StepBase {
    using Hyper = SgdHyper;
    struct State {};
    static constexpr bool kSteps = false;
    static __device__ __forceinline__ bool no_step(State&, const Hyper&) { return false; }
    static __device__ __forceinline__ void setup(State&, const Hyper&) {}
    template <class IO, bool NT, class... A>
    static __device__ __forceinline__ void step(A...) {}
    static bool given(const Hyper&, const void*, const float*) { return true; }
    static int check(const char*, const Hyper&, const float*) { return MX_OK; }
    template <class IO, class... F>
    static auto kernel(const Hyper&, int bits, bool nt) { return pick<IO, NoStep, F...>(bits, nt); }
};

// torch.optim.SGD's step (sgd_update.h): g, and with MOM m, of all four items held in flight with x and x_hat
template <bool MOM>
struct SgdStep : StepBase {
    using Hyper = SgdHyper;
    using State = SgdState;
    template <class IO>
    struct Held {
        typename IO::GC g[kIPW];
        F4 m[kIPW];
    };
    static constexpr bool kSteps = true;
    static __device__ __forceinline__ bool no_step(State& st, const Hyper& h) { return mx::fused::sgd_no_step(st, h); }
    static __device__ __forceinline__ void setup(State& st, const Hyper& h) { mx::fused::sgd_setup(st, h); }
    template <class IO>
    static __device__ __forceinline__ bool al(bool base, const typename IO::GT* g, const float* m, int64_t off) {
        return base && IO::al_g(g + off) && (!MOM || al16(m + off));
    }
    template <class IO>
    static __device__ __forceinline__ void clear(Held<IO>& hd, int q) {
        hd.m[q] = F4{0.0f, 0.0f, 0.0f, 0.0f};
        hd.g[q] = IO::zero();
    }
    template <class IO, bool NT>
    static __device__ __forceinline__ void hold(Held<IO>& hd, int q, const typename IO::GT* g, const float* m,
                                                int64_t off, int64_t c, bool vec, int64_t P) {
        hd.g[q] = load_q<NT>(g + off, c, vec, P);
        if constexpr (MOM) hd.m[q] = load_q<NT>(m + off, c, vec, P);
    }
    template <class IO, bool NT>
    static __device__ __forceinline__ void step(F4& xv, Held<IO>& hd, int q, None&, const State& st, const Hyper& h,
                                                typename IO::GT* g, float* m, int64_t off, int64_t c, bool vec,
                                                int64_t P) {
        xv = mx::fused::sgd4<MOM>(xv, mx::fused::widen4(hd.g[q]), hd.m[q], st.nlr, h);
        if constexpr (MOM) store_q<NT>(hd.m[q], m + off, c, vec, P);
        if (h.zero_grads) store_q<NT>(IO::zero(), g + off, c, vec, P);
    }
};
// its host side, and its name in round_launch: momentum picks the policy
struct Sgd {
    using Hyper = SgdHyper;
    static bool given(const Hyper&, const void* g, const float*) { return g != nullptr; }
    static int check(const char* who, const Hyper& h, const float* m) {
        MX_CHECK((h.mom != 0.0f) == (m != nullptr), "%s: the momentum rows are given exactly when momentum != 0", who);
        MX_CHECK(h.mom != 0.0f || !h.nesterov, "%s: nesterov needs momentum", who);
        return MX_OK;
    }
    template <class IO, class... F>
    static auto kernel(const Hyper& h, int bits, bool nt) {
        return h.mom != 0.0f ? pick<IO, SgdStep<true>, F...>(bits, nt) : pick<IO, SgdStep<false>, F...>(bits, nt);
    }
};

// the geometry of a launch, whatever its step: what every entry point checks of its shape, then the tile class,
// the plan record and the persistent grid
struct RoundGeo {
    RoundDims dims;
    const int32_t* rec;
    unsigned grid;
    bool nt;
};
inline int round_geo(const char* who, int64_t ld, int n_local, int64_t P, int bits, const int32_t* plan_dev,
                     int64_t iter, const int64_t* iter_dev, int M, float alpha, float gamma, int64_t seed,
                     int row_base, const float* norms, int64_t norm_ld, RoundGeo* out) {
    MX_CHECK(bits == 4 || bits == 8, "%s: bits=%d (4 or 8)", who, bits);
    MX_CHECK(n_local >= 1 && n_local <= kMaxRows, "%s: n_local=%d (1-%d rows; more take the two launches)", who,
             n_local, kMaxRows);
    MX_CHECK(P >= 1 && (n_local == 1 || ld >= P) && M >= 1 && row_base >= 0, "%s: P=%lld ld=%lld M=%d row_base=%d",
             who, (long long)P, (long long)ld, M, row_base);
    MX_CHECK(!norms || norm_ld >= n_buckets(P), "%s: norm_ld=%lld < %lld buckets", who, (long long)norm_ld,
             (long long)n_buckets(P));
    int bshift = 4;                                                  // 16 / row class buckets of a row per tile
    while ((kItems >> bshift) < n_local) --bshift;
    const int64_t tiles = (n_buckets(P) + (1 << bshift) - 1) >> bshift;
    const int64_t words = mx::plan_words(n_local, M);
    out->rec = iter_dev ? plan_dev : plan_dev + iter * words;        // with iter_dev: iter = n_iters
    out->dims = RoundDims{ld, P, norm_ld, tiles, iter, iter, words, mix32((uint32_t)seed), n_local, M, row_base,
                          bshift, alpha, gamma};
    const int64_t target = mx::choco::g_quant_round_grid > 0
                               ? (int64_t)mx::choco::g_quant_round_grid
                               : (int64_t)mx::cu_count() * mx::choco::g_quant_round_blocks_per_cu;
    out->grid = (unsigned)(tiles < target ? tiles : target);
    // the existing rule: several workers' rows are far larger than the Infinity Cache, one row's are not
    out->nt = n_local > 1;
    return MX_OK;
}

// the SGD entry points' arguments as the step's constants
inline SgdHyper sgd_hyper(float lr, const float* lr_dev, float wd, float mom, int nesterov, int zero_grads) {
    return {lr, wd, mom, lr_dev, nullptr, nesterov != 0, zero_grads != 0};
}

// what every entry point checks alike, then the launch: the step's pointers and argument checks are the step's,
// a form with an image has p, the step's state rows come last (m; m and v)
template <class IO, class Step, class... F>
int round_launch(const char* who, float* x, typename IO::GT* g, float* xhat, float* s, uint16_t* p, int64_t ld,
                 int n_local, int64_t P, int bits, const int32_t* plan_dev, int64_t iter, const int64_t* iter_dev,
                 int M, float alpha, float gamma, int64_t seed, int row_base, float* norms, int64_t norm_ld,
                 const typename Step::Hyper& h, void* stream, F*... rows) {
    MX_CHECK(x && xhat && s && plan_dev && (!IO::kImage || p) && Step::given(h, g, rows...), "%s: null pointer", who);
    if (const int rc = Step::check(who, h, rows...)) return rc;
    RoundGeo geo;
    if (const int rc = round_geo(who, ld, n_local, P, bits, plan_dev, iter, iter_dev, M, alpha, gamma, seed, row_base,
                                 norms, norm_ld, &geo))
        return rc;
    hipLaunchKernelGGL((Step::template kernel<IO, F...>(h, bits, geo.nt)), dim3(geo.grid), dim3(kTPB), 0,
                       mx::as_stream(stream), x, g, rows..., xhat, s, norms, geo.rec, iter_dev, geo.dims,
                       make_tail<IO>(h, p));
    MX_LAUNCH_CHECK();
    return MX_OK;
}

}  // namespace qround
}  // namespace choco
}  // namespace mx
