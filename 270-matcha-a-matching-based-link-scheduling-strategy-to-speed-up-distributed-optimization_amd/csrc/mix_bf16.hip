// mix_bf16.hip -- the mixing round of mix.hip for worker rows held in bfloat16 (local-only groups).
//
// Same contract as mix_kernel_rows (decenCommunicator.prepare_comm_buffer / averaging / reset_model,
// communicator.py:87-131): per output row the partners' columns are accumulated in ascending
// matching order, the self term last, every step one __builtin_fmaf in fp32 -- but the rows are
// 16-bit: every input is widened exactly (bits << 16) and the fp32 chain is rounded to bfloat16 ONCE,
// to nearest even, at the store.  (The reference handed bf16 tensors would round after every
// partner: recv_buffer.add_(alpha, recv_tmp), communicator.py:92-122; one rounding of an fp32 chain
// is the stated contract here)
//
// Traffic per round = 2 * n_active * P * 2 bytes: half of the fp32 round's.
//
// A tile is staged in LDS as raw bf16 (16-byte chunks of 8 elements, so a tile holds twice the
// columns of an fp32 tile in the same LDS bytes) and widened when a partner walk reads it.  Each
// wave takes whole (row, 512-column pass) items: per partner one ds_read_b128, 8 widenings and 8
// FMAs per lane; per item one packed convert per element pair and one 16-byte store per lane.
// The in-place rule of mix_kernel_rows holds: a tile is staged completely (loads in registers, parked
// in LDS, barrier) before any row of it is written, and different work items never share a column.
//
// No receive slots: n_slots == n_local, the plan's n_remote is 0 and its peer-reads bit is never
// set (the host entry points refuse anything else).
#include "fused_host.h"
#include "mx_common.h"
#include "row_walk.h"

#include <cstdlib>

namespace {
using namespace mx::rows;
constexpr int kTPB = 256;
constexpr int kWV = kTPB / 64;

typedef float F2 __attribute__((ext_vector_type(2)));
typedef __bf16 B2 __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ U4 ld16(const uint16_t* p) {
    const GPtr<const U4> g = (GPtr<const U4>)(p);
    if constexpr (NT) return __builtin_nontemporal_load(g);
    else return *g;
}
template <bool NT>
__device__ __forceinline__ void st16(uint16_t* p, const U4& v) {
    const GPtr<U4> g = (GPtr<U4>)(p);
    if constexpr (NT) __builtin_nontemporal_store(v, g);
    else *g = v;
}

// one lane's chunk of 8 elements at column c of `row`: a 16-byte load when the row pointer is
// 16-byte aligned and the chunk is in range, else 2-byte loads zero-filled from `lim` on
template <bool NT>
__device__ __forceinline__ U4 load_chunk(const uint16_t* row, int64_t c, int64_t lim) {
    if (al16(row) && c + 8 <= lim) return ld16<NT>(row + c);
    U4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t lo = (c + 2 * t < lim) ? ld2(row + c + 2 * t) : 0u;
        const uint32_t hi = (c + 2 * t + 1 < lim) ? ld2(row + c + 2 * t + 1) : 0u;
        v[t] = lo | (hi << 16);
    }
    return v;
}

template <bool NT>
__device__ __forceinline__ void store_chunk(uint16_t* row, int64_t c, int64_t lim, const U4& v) {
    if (al16(row) && c + 8 <= lim) {
        st16<NT>(row + c, v);
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (c + 2 * t < lim) st2(row + c + 2 * t, v[t] & 0xFFFFu);
        if (c + 2 * t + 1 < lim) st2(row + c + 2 * t + 1, v[t] >> 16);
    }
}

// the one rounding: fp32 -> bf16, to nearest even (v_cvt_pk_bf16_f32; NaN stays NaN)
__device__ __forceinline__ U4 pack8(const float (&a)[8]) {
    U4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const F2 f = {a[2 * t], a[2 * t + 1]};
        v[t] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, B2));
    }
    return v;
}

// the round's plan record into LDS; returns the mask of rows read and written (degree > 0, or every
// row of an active round in idle mode 1), 0 when the round has no active matching
template <int NS>
__device__ __forceinline__ uint64_t load_plan(PlanLds<NS>& sp, const int32_t* plan, int64_t iter, int n_local, int M) {
    if (iter < 0) return 0;                      // block-uniform
    copy_plan(sp, plan, iter, n_local, M);
    if (sp.w[0] == 0) return 0;
    return local_need(sp, n_local);
}

// NS slots x TW columns per work item; a layout tile (mx_mix_bf16_tile) is `split` work items.
template <int NS, int TW, bool NT>
__global__ __launch_bounds__(kTPB) void mix_bf16_rows(uint16_t* const* __restrict__ seg_ptrs,
                                                      const int64_t* __restrict__ seg_len,
                                                      const int64_t* __restrict__ tile_off, int nseg,
                                                      int64_t total_tiles, int split, int n_slots,
                                                      const int32_t* __restrict__ plan, int64_t iter,
                                                      const int64_t* __restrict__ iter_dev, int n_local, int M,
                                                      float alpha, uint64_t hint) {
    constexpr int C8 = TW / 8;            // 16-byte chunks per slot per work item
    constexpr int NQ = TW / 512;          // 512-column passes per row
    constexpr int NI = NS * NQ;           // items per work item (<= 64: one per lane of wave 0)
    constexpr int E = NS * C8 / kTPB;     // chunks staged per lane
    static_assert(NQ >= 1 && NI <= 64 && NI % kWV == 0 && E >= 1 && E * kTPB == NS * C8 && C8 % 64 == 0,
                  "bf16 row kernel geometry");
    __shared__ U4 lds[NS * C8];
    __shared__ PlanLds<NS> sp;
    __shared__ int32_t wl[kWV][NI / kWV];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total_work = total_tiles * split;
    const int64_t niter = total_work > blockIdx.x ? (total_work - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (niter == 0) return;                  // block-uniform, before any barrier

    struct Geo {
        uint16_t* const* ptrs;
        int64_t col0, lim;
    };
    auto geo = [&](int64_t work) {
        const int64_t tile = work / split;
        int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (tile_off[mid] <= tile) lo = mid; else hi = mid;
        }
        Geo gq;
        gq.ptrs = seg_ptrs + (int64_t)lo * n_slots;
        gq.col0 = (tile - tile_off[lo]) * ((int64_t)TW * split) + (work % split) * TW;
        gq.lim = seg_len[lo];
        return gq;
    };
    U4 R[E];
    auto stage_mask = [&](const Geo& gq, uint64_t mask) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int k = (wave * 64 + kTPB * j) / C8;              // wave-uniform slot
            if ((mask >> k) & 1ull) {
                const int64_t c = gq.col0 + (int64_t)((wave * 64 + kTPB * j) % C8 + lane) * 8;
                R[j] = load_chunk<NT>(gq.ptrs[k], c, gq.lim);
            }
        }
    };
    const uint64_t local_mask = n_local >= 64 ? ~0ull : (1ull << n_local) - 1;
    // the hinted rows' loads fly while the plan record is fetched (a wrong hint costs time, never
    // bits: the record decides what is parked, mixed and stored)
    Geo cur = geo(blockIdx.x);
    stage_mask(cur, hint & local_mask);
    const uint64_t need = load_plan<NS>(sp, plan, round_of(iter, iter_dev), n_local, M);
    if (need == 0) return;                   // all flags zero: no row is written
    const Plan pv = view(sp, n_local);

    // the rows of `need` are dealt, by weight degree + 1
    if (wave == 0)
        deal<NQ, NI, kWV>(wl, lane, [&](int r) { return (r < n_local && ((need >> r) & 1ull)) ? pv.deg[r] + 1 : 0; });
    const uint64_t rest = need & ~(hint & local_mask);
    if (rest) stage_mask(cur, rest);
    __syncthreads();
    const int nmy = count(wl[wave]);

    auto mix_tile = [&](const Geo& g) {
        auto finish = [&](int it, float (&acc)[8]) {
            const int r = it / NQ;
            const int col = (it % NQ) * 64 + lane;
            fma8(acc, pv.sw[r], lds[r * C8 + col]);                 // the self term, last
            store_chunk<NT>(g.ptrs[r], g.col0 + (int64_t)col * 8, g.lim, pack8(acc));
        };
        walk<Bf16, NQ, C8>(lds, wl[wave], nmy, lane, pv.src, M, alpha, [&](int r) { return pv.deg[r]; }, finish);
    };
    for (int64_t i = 0; i < niter; ++i) {
        if (i) __syncthreads();              // every wave is done reading the previous tile
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int k = (wave * 64 + kTPB * j) / C8;
            if ((need >> k) & 1ull) lds[k * C8 + (wave * 64 + kTPB * j) % C8 + lane] = R[j];
        }
        __syncthreads();                     // the tile is staged completely before any row is written
        Geo nxt = cur;
        if (i + 1 < niter) {                 // next work item's loads fly while this one is mixed
            nxt = geo(blockIdx.x + (i + 1) * gridDim.x);
            stage_mask(nxt, need);
        }
        mix_tile(cur);
        cur = nxt;
    }
}

using mx::fused::Cls;    // slot class, layout tile (columns), work-item width

// twice the columns of the fp32 classes in the same LDS bytes; 8 / 16 slots are worked in
// 1024-column halves of a 2048-column layout tile (16 / 32 KB of LDS per workgroup)
Cls pick(int n_slots) {
    if (n_slots < 1) return {0, 0, 0};
    if (n_slots <= 8) return {8, 2048, 1024};
    if (n_slots <= 16) return {16, 2048, 1024};
    if (n_slots <= 32) return {32, 1024, 1024};
    if (n_slots <= 64) return {64, 512, 512};
    return {0, 0, 0};
}

// the knobs of the fused rounds (fused_host.h) without store_policy, and split: 8 / 16 slots, work items
// per 2048-column layout tile, 1 / 2 / 4 (0 = the default, 2)
mx::fused::Tune g_tune;
int g_split = 0;

template <int NS, int TW, bool NT>
int launch(uint16_t* const* seg_ptrs, const int64_t* seg_len, const int64_t* tile_off, int nseg, int64_t total_tiles,
           int split, int n_slots, const int32_t* plan, int64_t iter, const int64_t* iter_dev, int n_local, int M,
           float alpha, uint64_t hint, hipStream_t st) {
    bool flat = false;
    const int64_t grid = g_tune.grid_of(NS, total_tiles * split, &flat);
    size_t pad = 0;
    if (flat && g_tune.wgpc > 0) {
        static const int stat = [] {                           // static LDS of this instantiation
            hipFuncAttributes fa{};
            return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(mix_bf16_rows<NS, TW, NT>)) == hipSuccess
                       ? (int)fa.sharedSizeBytes : 0;
        }();
        pad = mx::lds_cap_pad(stat, g_tune.wgpc);
    }
    hipLaunchKernelGGL((mix_bf16_rows<NS, TW, NT>), dim3((unsigned)grid), dim3(kTPB), pad, st, seg_ptrs, seg_len,
                       tile_off, nseg, total_tiles, split, n_slots, plan, iter, iter_dev, n_local, M, alpha, hint);
    MX_LAUNCH_CHECK();
    return MX_OK;
}

int gossip_mix_bf16(uint16_t* const* seg_ptrs, const int64_t* seg_len, const int64_t* tile_off, int nseg,
                    int64_t total_tiles, int n_slots, const int32_t* plan, int64_t iter, const int64_t* iter_dev,
                    int n_local, int M, float alpha, void* stream, uint64_t hint) {
    MX_CHECK(seg_ptrs && seg_len && tile_off && plan, "mx_gossip_mix_bf16: null pointer");
    MX_CHECK(nseg >= 1 && n_local >= 1, "mx_gossip_mix_bf16: nseg=%d n_local=%d", nseg, n_local);
    MX_CHECK(n_slots == n_local, "mx_gossip_mix_bf16: n_slots=%d != n_local=%d (bf16 rows have no receive slots)",
             n_slots, n_local);
    MX_CHECK(n_slots <= 64, "mx_gossip_mix_bf16: n_slots=%d exceeds 64", n_slots);
    MX_CHECK(M >= 1 && M <= kMaxM, "mx_gossip_mix_bf16: M=%d outside [1, %d]", M, kMaxM);
    MX_CHECK(iter >= 0, "mx_gossip_mix_bf16: iter < 0");
    if (total_tiles <= 0) return MX_OK;
    const Cls c = pick(n_slots);
    const int split = (c.ns <= 16 && g_split > 0) ? g_split : c.tile / c.tw;
    hipStream_t st = mx::as_stream(stream);
    const bool nt = g_tune.streaming(total_tiles, c.tile, n_slots, 2);
#define MX_B16(N, TW)                                                                                             \
    (nt ? launch<N, TW, true>(seg_ptrs, seg_len, tile_off, nseg, total_tiles, split, n_slots, plan, iter, iter_dev, \
                              n_local, M, alpha, hint, st)                                                        \
        : launch<N, TW, false>(seg_ptrs, seg_len, tile_off, nseg, total_tiles, split, n_slots, plan, iter,        \
                               iter_dev, n_local, M, alpha, hint, st))
    switch (c.ns) {
        case 8: return split == 1 ? MX_B16(8, 2048) : split == 4 ? MX_B16(8, 512) : MX_B16(8, 1024);
        case 16: return split == 1 ? MX_B16(16, 2048) : split == 4 ? MX_B16(16, 512) : MX_B16(16, 1024);
        case 32: return MX_B16(32, 1024);
        default: return MX_B16(64, 512);
    }
#undef MX_B16
}
}  // namespace

extern "C" int mx_mix_bf16_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    MX_CHECK(seg_len_host && tile_off_host && nseg >= 1, "mx_mix_bf16_layout: bad arguments");
    const int tile = mx_mix_bf16_tile(n_slots);
    MX_CHECK(tile > 0, "mx_mix_bf16_layout: n_slots=%d outside [1, 64]", n_slots);
    return mx::tile_prefix("mx_mix_bf16_layout", tile, seg_len_host, nseg, tile_off_host);
}

extern "C" int mx_mix_bf16_set(const char* key, int value) {
    MX_CHECK(key, "mx_mix_bf16_set: null key");
    if (!strcmp(key, "split")) {
        MX_CHECK(value == 0 || value == 1 || value == 2 || value == 4, "mx_mix_bf16_set: split %d", value);
        g_split = value;
        return MX_OK;
    }
    MX_CHECK(strcmp(key, "store_policy"), "mx_mix_bf16_set: unknown key '%s'", key);
    return g_tune.set("mx_mix_bf16_set", key, value);
}

extern "C" int mx_mix_bf16_get(const char* key) {
    if (!key) return MX_ERR_INVALID;
    if (!strcmp(key, "split")) return g_split;
    MX_CHECK(strcmp(key, "store_policy"), "mx_mix_bf16_get: unknown key '%s'", key);
    return g_tune.get("mx_mix_bf16_get", key);
}

extern "C" int mx_gossip_mix_bf16_packed(const mx_mix_call* c, int64_t iter, void* stream) {
    MX_CHECK(c, "mx_gossip_mix_bf16_packed: null call record");
    MX_CHECK(!c->need_host || (iter >= 0 && iter < c->n_iters),
             "mx_gossip_mix_bf16_packed: iter %lld outside [0, %lld)", (long long)iter, (long long)c->n_iters);
    return gossip_mix_bf16(reinterpret_cast<uint16_t* const*>(c->seg_ptrs_dev), c->seg_len_dev, c->tile_off_dev,
                           c->nseg, c->total_tiles, c->n_slots, c->plan_dev, iter, nullptr, c->n_local, c->M,
                           c->alpha, stream, c->need_host ? c->need_host[iter] : 0);
}

extern "C" int mx_gossip_mix_bf16_at(uint16_t* const* seg_ptrs_dev, const int64_t* seg_len_dev,
                                     const int64_t* tile_off_dev, const uint8_t* seg_vec_dev, int nseg,
                                     int64_t total_tiles, int n_slots, const int32_t* plan_dev,
                                     const int64_t* iter_dev, int64_t n_iters, int n_local, int M, float alpha,
                                     void* stream) {
    (void)seg_vec_dev;                       // alignment is tested per row pointer in the kernel
    MX_CHECK(iter_dev, "mx_gossip_mix_bf16_at: null iteration counter");
    return gossip_mix_bf16(seg_ptrs_dev, seg_len_dev, tile_off_dev, nseg, total_tiles, n_slots, plan_dev, n_iters,
                           iter_dev, n_local, M, alpha, stream, 0);
}
