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
#include "mx_common.h"

#include <cstdlib>

namespace {
constexpr int kTPB = 256;
constexpr int kMaxM = 32;
constexpr int kWV = kTPB / 64;

typedef uint32_t U4 __attribute__((ext_vector_type(4)));      // 8 bf16: one 16-byte access
typedef float F2 __attribute__((ext_vector_type(2)));
typedef __bf16 B2 __attribute__((ext_vector_type(2)));

// global (not flat) accesses: counted on vmcnt only, so the LDS waits of the partner walk do not
// drain the HBM stream (see mix.hip)
template <typename T>
using GPtr = __attribute__((address_space(1))) T*;

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
__device__ __forceinline__ uint32_t ld2(const uint16_t* p) { return *(GPtr<const uint16_t>)(p); }
__device__ __forceinline__ void st2(uint16_t* p, uint32_t v) { *(GPtr<uint16_t>)(p) = (uint16_t)v; }
__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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

// acc[0..7] = fmaf(w, f32(x[0..7]), acc[0..7]); f32() is the exact widening bits << 16
__device__ __forceinline__ void fma8(float (&a)[8], float w, const U4& x) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        a[2 * t] = __builtin_fmaf(w, __builtin_bit_cast(float, x[t] << 16), a[2 * t]);
        a[2 * t + 1] = __builtin_fmaf(w, __builtin_bit_cast(float, x[t] & 0xFFFF0000u), a[2 * t + 1]);
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

template <int NS>
struct PlanLds {
    int32_t w[mx::kPlanHeader + 2 * NS + NS * kMaxM];
};

// The round to mix: `iter`, or with iter_dev (graph-replayable launches) the device counter
// *iter_dev, `iter` then being the schedule length; outside [0, length) the launch is a no-op.
__device__ __forceinline__ int64_t round_of(int64_t iter, const int64_t* iter_dev) {
    if (!iter_dev) return iter;
    const int64_t v = *iter_dev;
    return (v >= 0 && v < iter) ? v : -1;
}

// the round's plan record into LDS; returns the mask of rows read and written (degree > 0, or every
// row of an active round in idle mode 1), 0 when the round has no active matching
template <int NS>
__device__ __forceinline__ uint64_t load_plan(PlanLds<NS>& sp, const int32_t* plan, int64_t iter, int n_local, int M) {
    if (iter < 0) return 0;                      // block-uniform
    const int64_t W = mx::plan_words(n_local, M);
    const int32_t* rec = plan + iter * W;
    for (int i = threadIdx.x; i < W; i += blockDim.x) sp.w[i] = rec[i];
    __syncthreads();
    if (sp.w[0] == 0) return 0;
    const bool idle = (sp.w[2] & 1) != 0;
    const int32_t* deg = sp.w + mx::kPlanHeader;
    uint64_t need = 0;
    for (int r = 0; r < n_local; ++r)
        if (deg[r] > 0 || idle) need |= 1ull << r;
    return need;
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
    const int32_t* deg = sp.w + mx::kPlanHeader;
    const float* sw = reinterpret_cast<const float*>(deg + n_local);
    const int32_t* src = deg + 2 * n_local;

    // deal the items (row r, pass q) = r * NQ + q to the waves: wave 0 ranks them by weight
    // (degree + 1), snake order over the waves
    if (wave == 0) {
        const int r = lane / NQ;
        const int w = (lane < NI && r < n_local && ((need >> r) & 1ull)) ? deg[r] + 1 : 0;
        int rank = 0;
        for (int j = 0; j < NI; ++j) {
            const int wj = __builtin_amdgcn_readlane(w, j);
            rank += (wj > w) || (wj == w && j < lane);
        }
        const int round = rank / kWV, within = rank % kWV;
        if (lane < NI) wl[(round & 1) ? kWV - 1 - within : within][round] = w > 0 ? lane : -1;
    }
    const uint64_t rest = need & ~(hint & local_mask);
    if (rest) stage_mask(cur, rest);
    __syncthreads();
    // ranks grow along a wave's list, so its unused (-1) entries form a suffix
    int nmy = 0;
    while (nmy < NI / kWV && wl[wave][nmy] >= 0) ++nmy;
    nmy = __builtin_amdgcn_readfirstlane(nmy);

    auto mix_tile = [&](const Geo& g) {
        auto finish = [&](int it, float (&acc)[8]) {
            const int r = it / NQ;
            const int col = (it % NQ) * 64 + lane;
            fma8(acc, sw[r], lds[r * C8 + col]);                    // the self term, last
            store_chunk<NT>(g.ptrs[r], g.col0 + (int64_t)col * 8, g.lim, pack8(acc));
        };
        int p = 0;
        for (; p + 1 < nmy; p += 2) {            // two items interleaved
            const int ia = __builtin_amdgcn_readfirstlane(wl[wave][p]);
            const int ib = __builtin_amdgcn_readfirstlane(wl[wave][p + 1]);
            const int ra = ia / NQ, rb = ib / NQ;
            const int ca = (ia % NQ) * 64 + lane, cb = (ib % NQ) * 64 + lane;
            const int da = deg[ra], db = deg[rb];
            const int dmin = da < db ? da : db;
            float a[8], b[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) a[t] = b[t] = 0.0f;
            int e = 0;
            for (; e < dmin; ++e) {
                const int sa = __builtin_amdgcn_readfirstlane(src[ra * M + e]);
                const int sb = __builtin_amdgcn_readfirstlane(src[rb * M + e]);
                const U4 xa = lds[sa * C8 + ca];
                const U4 xb = lds[sb * C8 + cb];
                fma8(a, alpha, xa);
                fma8(b, alpha, xb);
            }
            for (int ea = e; ea < da; ++ea)
                fma8(a, alpha, lds[__builtin_amdgcn_readfirstlane(src[ra * M + ea]) * C8 + ca]);
            for (int eb = e; eb < db; ++eb)
                fma8(b, alpha, lds[__builtin_amdgcn_readfirstlane(src[rb * M + eb]) * C8 + cb]);
            finish(ia, a);
            finish(ib, b);
        }
        if (p < nmy) {
            const int ia = __builtin_amdgcn_readfirstlane(wl[wave][p]);
            const int ra = ia / NQ, ca = (ia % NQ) * 64 + lane;
            float a[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) a[t] = 0.0f;
            for (int e = 0; e < deg[ra]; ++e)
                fma8(a, alpha, lds[__builtin_amdgcn_readfirstlane(src[ra * M + e]) * C8 + ca]);
            finish(ia, a);
        }
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

struct Cls {
    int ns, tile, tw;    // slot class, layout tile (columns), work-item width
};

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

struct Tune {
    int nontemporal = 2;   // 1 / 0: streaming hints on / off; 2 = auto (off for rounds of 32-320 MB, as mix.hip)
    int wgpc = 0;          // 8 / 16 slots, flat grid: workgroups per CU cap (dynamic LDS); 0 = as many as fit
    int blocks_per_cu = 2; // persistent grids (32 / 64 slots, or more work items than flat_small x the grid)
    int flat_small = 256;  // 8 / 16 slots: one workgroup per work item up to flat_small x CUs x blocks_per_cu items
    int grid = 0;          // > 0: exact persistent grid size (tests: few workgroups looping over many work items)
    int split = 0;         // 8 / 16 slots: work items per 2048-column layout tile, 1 / 2 / 4 (0 = the default, 2)
};
Tune g_tune;

int cu_count() {
    static int v = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 256;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 256;
        return n > 0 ? n : 256;
    }();
    return v;
}

template <int NS, int TW, bool NT>
int launch(uint16_t* const* seg_ptrs, const int64_t* seg_len, const int64_t* tile_off, int nseg, int64_t total_tiles,
           int split, int n_slots, const int32_t* plan, int64_t iter, const int64_t* iter_dev, int n_local, int M,
           float alpha, uint64_t hint, hipStream_t st) {
    const int64_t work = total_tiles * split;
    const int64_t target = g_tune.grid > 0 ? (int64_t)g_tune.grid : (int64_t)cu_count() * g_tune.blocks_per_cu;
    const bool flat = NS <= 16 && g_tune.grid == 0 && g_tune.flat_small > 0 &&
                      work <= (int64_t)g_tune.flat_small * target;
    int64_t grid = flat ? work : (work < target ? work : target);
    if (grid < 1) grid = 1;
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
    const int split = (c.ns <= 16 && g_tune.split > 0) ? g_tune.split : c.tile / c.tw;
    hipStream_t st = mx::as_stream(stream);
    const int64_t ws = total_tiles * (int64_t)c.tile * n_slots * 2;
    const bool nt = g_tune.nontemporal == 2 ? (ws <= ((int64_t)32 << 20) || ws > ((int64_t)320 << 20))
                                            : g_tune.nontemporal != 0;
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
    tile_off_host[0] = 0;
    for (int s = 0; s < nseg; ++s) {
        MX_CHECK(seg_len_host[s] >= 0, "mx_mix_bf16_layout: negative length");
        tile_off_host[s + 1] = tile_off_host[s] + (seg_len_host[s] + tile - 1) / tile;
    }
    return MX_OK;
}

extern "C" int mx_mix_bf16_set(const char* key, int value) {
    MX_CHECK(key, "mx_mix_bf16_set: null key");
    if (!strcmp(key, "nontemporal")) {
        g_tune.nontemporal = value == 2 ? 2 : (value ? 1 : 0);
    } else if (!strcmp(key, "wgpc")) {
        MX_CHECK(value >= 0 && value <= 32, "mx_mix_bf16_set: wgpc %d", value);
        g_tune.wgpc = value;
    } else if (!strcmp(key, "blocks_per_cu")) {
        MX_CHECK(value >= 1 && value <= 64, "mx_mix_bf16_set: blocks_per_cu %d", value);
        g_tune.blocks_per_cu = value;
    } else if (!strcmp(key, "flat_small")) {
        MX_CHECK(value >= 0 && value <= 4096, "mx_mix_bf16_set: flat_small %d", value);
        g_tune.flat_small = value;
    } else if (!strcmp(key, "grid")) {
        MX_CHECK(value >= 0 && value <= 65536, "mx_mix_bf16_set: grid %d", value);
        g_tune.grid = value;
    } else if (!strcmp(key, "split")) {
        MX_CHECK(value == 0 || value == 1 || value == 2 || value == 4, "mx_mix_bf16_set: split %d", value);
        g_tune.split = value;
    } else {
        MX_CHECK(false, "mx_mix_bf16_set: unknown key '%s'", key);
    }
    return MX_OK;
}

extern "C" int mx_mix_bf16_get(const char* key) {
    if (!key) return MX_ERR_INVALID;
    if (!strcmp(key, "nontemporal")) return g_tune.nontemporal;
    if (!strcmp(key, "wgpc")) return g_tune.wgpc;
    if (!strcmp(key, "blocks_per_cu")) return g_tune.blocks_per_cu;
    if (!strcmp(key, "flat_small")) return g_tune.flat_small;
    if (!strcmp(key, "split")) return g_tune.split;
    if (!strcmp(key, "grid")) return g_tune.grid;
    mx::set_error("mx_mix_bf16_get: unknown key '%s'", key);
    return MX_ERR_INVALID;
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
