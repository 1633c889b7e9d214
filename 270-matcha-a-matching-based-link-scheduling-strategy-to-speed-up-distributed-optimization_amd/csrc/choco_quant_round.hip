// choco_quant_round.hip -- a whole ChocoSGD round of the bucketed stochastic quantizer (choco_quant.hip) in ONE
// launch, for 1-16 worker rows that all live on this GPU, optionally with torch.optim.SGD's step on the way in.
//
// A quantized value depends on its own 256-column bucket alone (the norm is per bucket, the random number a
// hash of (seed, round, row, column)), so a workgroup that holds one column tile of ALL rows can quantize every
// row's part of the tile and apply the round from on-chip codes: the messages never reach memory.  x, x_hat and
// s are read and written once each, 24 bytes per parameter (+ 1/64 for the optional norms), where
// mx_choco_quant_compress + mx_choco_quant_apply move 8 + bits/8 + 24 + (deg + 1) bits/8 and more.
//
// mx_choco_quant_round     = quant_compress + quant_apply on the same values: the SAME BITS in x, x_hat and s,
//                            and the same norms (the same lane columns, the same butterfly)
// mx_choco_quant_sgd_round = mx_choco_sgd_step, then that round, on x' from the registers (sgd_update.h)
//
// Work item: a tile of 16 (row, bucket) items, the same buckets of every row: with n_local rounded up to the
// row class rc = 1, 2, 4, 8, 16 a tile is 16 / rc buckets = 256 (16 / rc) columns of each row.  256 threads;
// item i = (row i / (16 / rc), bucket i % (16 / rc)); wave w owns items 4w .. 4w + 3, a lane 4 consecutive
// columns of each.  A persistent grid only decides WHO computes a tile.
// Phase 1 (per wave, its items): x and x_hat (and g, m) by 16-byte loads, all items' loads issued before the
//   first use; x' = sgd(x, g, m) with m' and the zeros over g stored at once; d = fsub(x', x_hat); quant_pass
//   gives the bucket's norm and the lane's four codes; the codes go to LDS one byte per column (a 32-bit word a
//   lane), unit = fmul(norm, c) too; lane 0 writes the norm to `norms` when given.  x' and x_hat stay in
//   registers.
// ONE barrier: the tile is quantized completely before any of its columns is written, and no other workgroup
//   touches those columns, so the round runs in place.  The LDS image alternates between two buffers, which
//   makes the barrier of the next tile the only other ordering a workgroup needs.
// Phase 2 (the same wave, the same items): s by a 16-byte load; the row's partners from the plan record in
//   ascending matching order, each one 32-bit LDS word of codes and one unit; then the own message (s += sw q,
//   x_hat += q); x = fmaf(-gamma, x_hat, fmaf(gamma, s, x')); three 16-byte stores.
// Items whose row is off a 16-byte boundary or whose bucket holds P take the same registers through
// per-element loads and stores (+0 at and past P); nothing is written at or past P.
// No atomics, no workspace, no finish launch.  The plan must be all-local: a record with receive slots
// (n_remote != 0) or the peer-reads bit lives in device memory, so it is the launch that refuses it -- it
// writes nothing.
#include "choco_quant.h"
#include "mx_common.h"
#include "sgd_update.h"

namespace mx {
namespace choco {
int g_quant_round_blocks_per_cu = 4;      // mx_choco_quant_set "round_blocks_per_cu"
int g_quant_round_grid = 0;               // "round_grid": > 0 is the exact grid (tests: few workgroups, many tiles)
}  // namespace choco
}  // namespace mx

namespace {
using namespace mx::choco::quant;
using mx::fused::SgdHyper;
using mx::fused::SgdState;

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

template <int BITS, bool STEP, bool MOM, bool NT>
__global__ __launch_bounds__(kTPB) void quant_round(float* __restrict__ x, float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ xh,
                                                    float* __restrict__ s, float* __restrict__ norms,
                                                    const int32_t* __restrict__ rec_in,
                                                    const int64_t* __restrict__ iter_dev, RoundDims a, SgdHyper h) {
    static_assert(STEP || !MOM, "momentum belongs to the step");
    __shared__ uint32_t codes[2][kItems][64];                        // one byte per column, a word per lane
    __shared__ float units[2][kItems];                               // fmul(norm, c) of each item
    // round_rec's rules (choco_round.h), except that under STEP an inactive round of the schedule still steps
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
    if (!STEP && !on) return;
    SgdState st{0.0f};
    if constexpr (STEP) mx::fused::sgd_setup(st, h);                 // -lr, from lr_dev when given
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
        F4 xv[kIPW], hv[kIPW], gv[kIPW], mv[kIPW];
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            const int64_t b0 = ((w << a.bshift) + (i & bmask)) * kBucket;
            off[q] = (int64_t)r * a.ld;
            col[q] = b0 + lane * 4;
            live[q] = r < a.n_local && b0 < a.P;
            vec[q] = b0 + kBucket <= a.P && al16(x + off[q]) && al16(xh + off[q]) && al16(s + off[q]);
            if constexpr (STEP) vec[q] = vec[q] && al16(g + off[q]) && (!MOM || al16(m + off[q]));
            xv[q] = hv[q] = gv[q] = mv[q] = zero;
            if (live[q]) {
                xv[q] = load_q<NT>(x + off[q], col[q], vec[q], a.P);
                hv[q] = load_q<NT>(xh + off[q], col[q], vec[q], a.P);
                if constexpr (STEP) gv[q] = load_q<NT>(g + off[q], col[q], vec[q], a.P);
                if constexpr (MOM) mv[q] = load_q<NT>(m + off[q], col[q], vec[q], a.P);
            }
        }
#pragma unroll
        for (int q = 0; q < kIPW; ++q) {
            if (!live[q]) continue;                                  // wave-uniform
            const int i = wave * kIPW + q;
            const int r = i >> a.bshift;
            if constexpr (STEP) {
                xv[q] = mx::fused::sgd4<MOM>(xv[q], gv[q], mv[q], st.nlr, h);
                if constexpr (MOM) store_q<NT>(mv[q], m + off[q], col[q], vec[q], a.P);
                if (h.zero_grads) store_q<NT>(zero, g + off[q], col[q], vec[q], a.P);
                if (!on) {                                           // no active matching: the step alone
                    store_q<NT>(xv[q], x + off[q], col[q], vec[q], a.P);
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
            store_q<NT>(xv[q], x + off[q], col[q], vec[q], a.P);
            store_q<NT>(sv[q], s + off[q], col[q], vec[q], a.P);
            store_q<NT>(hv[q], xh + off[q], col[q], vec[q], a.P);
        }
    }
}

template <int BITS, bool STEP, bool MOM>
auto pick_nt(bool nt) { return nt ? quant_round<BITS, STEP, MOM, true> : quant_round<BITS, STEP, MOM, false>; }
template <bool STEP, bool MOM>
auto pick(int bits, bool nt) { return bits == 4 ? pick_nt<4, STEP, MOM>(nt) : pick_nt<8, STEP, MOM>(nt); }

// what the four entry points check alike, then the launch; STEP with g / m and the hyperparameters
template <bool STEP>
int round_launch(const char* who, float* x, float* g, float* m, float* xhat, float* s, int64_t ld, int n_local,
                 int64_t P, int bits, const int32_t* plan_dev, int64_t iter, const int64_t* iter_dev, int M,
                 float alpha, float gamma, int64_t seed, int row_base, float* norms, int64_t norm_ld, float lr,
                 const float* lr_dev, float wd, float mom, int nesterov, int zero_grads, void* stream) {
    MX_CHECK(x && xhat && s && plan_dev && (!STEP || g), "%s: null pointer", who);
    MX_CHECK(bits == 4 || bits == 8, "%s: bits=%d (4 or 8)", who, bits);
    MX_CHECK(n_local >= 1 && n_local <= kMaxRows, "%s: n_local=%d (1-%d rows; more take the two launches)", who,
             n_local, kMaxRows);
    MX_CHECK(P >= 1 && (n_local == 1 || ld >= P) && M >= 1 && row_base >= 0, "%s: P=%lld ld=%lld M=%d row_base=%d",
             who, (long long)P, (long long)ld, M, row_base);
    if constexpr (STEP) {
        MX_CHECK((mom != 0.0f) == (m != nullptr), "%s: the momentum rows are given exactly when momentum != 0", who);
        MX_CHECK(mom != 0.0f || !nesterov, "%s: nesterov needs momentum", who);
    }
    MX_CHECK(!norms || norm_ld >= n_buckets(P), "%s: norm_ld=%lld < %lld buckets", who, (long long)norm_ld,
             (long long)n_buckets(P));
    int bshift = 4;                                                  // 16 / row class buckets of a row per tile
    while ((kItems >> bshift) < n_local) --bshift;
    const int64_t tiles = (n_buckets(P) + (1 << bshift) - 1) >> bshift;
    const int64_t words = mx::plan_words(n_local, M);
    const int32_t* rec = iter_dev ? plan_dev : plan_dev + iter * words;   // with iter_dev: iter = n_iters
    const RoundDims dims{ld, P, norm_ld, tiles, iter, iter, words, mix32((uint32_t)seed), n_local, M, row_base,
                         bshift, alpha, gamma};
    const SgdHyper h{lr, wd, mom, lr_dev, nullptr, nesterov != 0, zero_grads != 0};
    const int64_t target = mx::choco::g_quant_round_grid > 0
                               ? (int64_t)mx::choco::g_quant_round_grid
                               : (int64_t)mx::cu_count() * mx::choco::g_quant_round_blocks_per_cu;
    // the existing rule: several workers' rows are far larger than the Infinity Cache, one row's are not
    const bool nt = n_local > 1;
    const auto kern = !STEP ? pick<false, false>(bits, nt)
                            : mom != 0.0f ? pick<STEP, STEP>(bits, nt) : pick<STEP, false>(bits, nt);
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles < target ? tiles : target)), dim3(kTPB), 0, mx::as_stream(stream), x,
                       g, m, xhat, s, norms, rec, iter_dev, dims, h);
    MX_LAUNCH_CHECK();
    return MX_OK;
}
}  // namespace

extern "C" int mx_choco_quant_round(float* x, float* xhat, float* s, int64_t ld, int n_local, int64_t P, int bits,
                                    const int32_t* plan_dev, int64_t iter, int M, float alpha, float gamma,
                                    int64_t seed, int row_base, float* norms, int64_t norm_ld, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_round: iter < 0");
    return round_launch<false>("mx_choco_quant_round", x, nullptr, nullptr, xhat, s, ld, n_local, P, bits, plan_dev,
                               iter, nullptr, M, alpha, gamma, seed, row_base, norms, norm_ld, 0.0f, nullptr, 0.0f,
                               0.0f, 0, 0, stream);
}

extern "C" int mx_choco_quant_round_at(float* x, float* xhat, float* s, int64_t ld, int n_local, int64_t P, int bits,
                                       const int32_t* plan_dev, const int64_t* iter_dev, int64_t n_iters, int M,
                                       float alpha, float gamma, int64_t seed, int row_base, float* norms,
                                       int64_t norm_ld, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_round_at: bad iteration counter");
    return round_launch<false>("mx_choco_quant_round_at", x, nullptr, nullptr, xhat, s, ld, n_local, P, bits,
                               plan_dev, n_iters, iter_dev, M, alpha, gamma, seed, row_base, norms, norm_ld, 0.0f,
                               nullptr, 0.0f, 0.0f, 0, 0, stream);
}

extern "C" int mx_choco_quant_sgd_round(float* x, float* g, float* m, float* xhat, float* s, int64_t ld, int n_local,
                                        int64_t P, int bits, const int32_t* plan_dev, int64_t iter, int M,
                                        float alpha, float gamma, int64_t seed, int row_base, float* norms,
                                        int64_t norm_ld, float lr, const float* lr_dev, float weight_decay,
                                        float momentum, int nesterov, int zero_grads, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_sgd_round: iter < 0");
    return round_launch<true>("mx_choco_quant_sgd_round", x, g, m, xhat, s, ld, n_local, P, bits, plan_dev, iter,
                              nullptr, M, alpha, gamma, seed, row_base, norms, norm_ld, lr, lr_dev, weight_decay,
                              momentum, nesterov, zero_grads, stream);
}

extern "C" int mx_choco_quant_sgd_round_at(float* x, float* g, float* m, float* xhat, float* s, int64_t ld,
                                           int n_local, int64_t P, int bits, const int32_t* plan_dev,
                                           const int64_t* iter_dev, int64_t n_iters, int M, float alpha, float gamma,
                                           int64_t seed, int row_base, float* norms, int64_t norm_ld, float lr,
                                           const float* lr_dev, float weight_decay, float momentum, int nesterov,
                                           int zero_grads, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_sgd_round_at: bad iteration counter");
    return round_launch<true>("mx_choco_quant_sgd_round_at", x, g, m, xhat, s, ld, n_local, P, bits, plan_dev,
                              n_iters, iter_dev, M, alpha, gamma, seed, row_base, norms, norm_ld, lr, lr_dev,
                              weight_decay, momentum, nesterov, zero_grads, stream);
}
