// sgd_mix.hip -- the SGD update of every local worker fused into the mixing round (fp32 rows,
// local-only groups): one launch per training iteration instead of n optimizer steps + one mix.
//
// The reference's iteration (train_mpi.py:131-142) runs optimizer.step(), optimizer.zero_grad(),
// communicator.communicate(model).  Here each row's x, g and m elements are read once, torch.optim.SGD's
// update (dampening 0) is applied on the way into LDS
//     d  = (wd != 0) ? fmaf(wd, x, g) : g                 g.add(p, alpha=wd)
//     m  = fadd(fmul(mom, m), d)           [mom != 0]     buf.mul_(mom).add_(d_p): two roundings
//     d  = nesterov ? fmaf(mom, m, d) : m  [mom != 0]
//     x' = fmaf(-lr, d, x)                                p.add_(d_p, alpha=-lr)
// and the round of mix.hip's mix_kernel_rows (decenCommunicator.prepare_comm_buffer / averaging /
// reset_model, communicator.py:87-131) then runs on the staged x' values: per output row the partners'
// columns in ascending matching order, the self term last, every step one __builtin_fmaf.  Rows the plan
// record does not read and write (degree 0 outside idle mode 1), and every row of a round whose flags
// are all zero, get x' stored as it is: an all-zero round is the SGD step alone, not a no-op.
//
// Traffic per element: read x, g, m, write x, m = 20 bytes (24 when the gradients are zeroed, 12 / 16
// without momentum) against 52 for the torch op sequence followed by the mixing round.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  m is read and written by the same lane only, so it is
// stored when its chunk is staged; so are the zeros over g with zero_grads.  Because every row is read
// in every round, the first loads are issued before the plan record is looked at.
//
// No receive slots: n_slots == n_local, the plan's n_remote is 0; a record with the peer-reads bit
// makes the launch write nothing (the bit lives on the device; see mx_sgd_mix in the header).
#include "mx_common.h"

#include <cstdlib>
#include <type_traits>

namespace {
constexpr int kTPB = 256;
constexpr int kMaxM = 32;
constexpr int kWV = kTPB / 64;
// 16-byte chunks of x, g and m a lane has in flight at once: 2 keeps the 8-row kernel at 68 VGPRs (7 waves per
// SIMD) and measured 3 % faster on the headline shape than 4 (94 VGPRs, 5 waves)
constexpr int kB = 2;

typedef float F4 __attribute__((ext_vector_type(4)));

// global (not flat) accesses: counted on vmcnt only, so the LDS waits of the partner walk do not
// drain the HBM stream (see mix.hip)
template <typename T>
using GPtr = __attribute__((address_space(1))) T*;

template <bool NT>
__device__ __forceinline__ F4 ld16(const float* p) {
    const GPtr<const F4> g = (GPtr<const F4>)(p);
    if constexpr (NT) return __builtin_nontemporal_load(g);
    else return *g;
}
template <bool NT>
__device__ __forceinline__ void st16(float* p, const F4& v) {
    const GPtr<F4> g = (GPtr<F4>)(p);
    if constexpr (NT) __builtin_nontemporal_store(v, g);
    else *g = v;
}
__device__ __forceinline__ float ld4(const float* p) { return *(GPtr<const float>)(p); }
__device__ __forceinline__ void st4(float* p, float v) { *(GPtr<float>)(p) = v; }
__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one lane's chunk of 4 elements at column c of `row`: a 16-byte access when the (segment, row)'s
// pointers are all 16-byte aligned (`vec`) and the chunk is in range, else 4-byte accesses,
// zero-filled from `lim` on; nothing is ever stored at or past `lim`
template <bool NT>
__device__ __forceinline__ F4 load_chunk(const float* row, int64_t c, int64_t lim, bool vec) {
    if (vec && c + 4 <= lim) return ld16<NT>(row + c);
    F4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = (c + t < lim) ? ld4(row + c + t) : 0.0f;
    return v;
}
template <bool NT>
__device__ __forceinline__ void store_chunk(float* row, int64_t c, int64_t lim, bool vec, const F4& v) {
    if (vec && c + 4 <= lim) {
        st16<NT>(row + c, v);
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < lim) st4(row + c + t, v[t]);
}

__device__ __forceinline__ void fma4(F4& a, float w, const F4& x) {
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = __builtin_fmaf(w, x[t], a[t]);
}

// the clip factor of the row (mx_*_scaled): g' = fmul(gscale[r], g), before anything else in the update
__device__ __forceinline__ F4 scale4(const F4& g, float s) {
    F4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = s * g[t];
    return v;
}

struct Hyper {
    float lr, wd, mom;
    const float* lr_dev;   // non-NULL: the learning rate, read when the kernel runs
    const float* gscale;   // non-NULL: float [n_local], row r's gradient is multiplied by gscale[r] (wave-uniform: a scalar load)
    int nesterov, zero_grads;
};

// torch.optim.SGD's update of one chunk (dampening 0); the momentum line always runs, with no
// first-step case: from a zero buffer fadd(fmul(mom, 0), d) == d under IEEE ==
template <bool MOM>
__device__ __forceinline__ F4 sgd4(const F4& x, const F4& g, F4& m, float nlr, const Hyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float d = h.wd != 0.0f ? __builtin_fmaf(h.wd, x[t], g[t]) : g[t];
        if constexpr (MOM) {
            const float scaled = h.mom * m[t];          // separately rounded (-ffp-contract=off)
            m[t] = scaled + d;
            d = h.nesterov ? __builtin_fmaf(h.mom, m[t], d) : m[t];
        }
        out[t] = __builtin_fmaf(nlr, d, x[t]);
    }
    return out;
}

// Per-parameter-group launches (mx_sgd_mix_grouped): the columns of a segment are cut into runs that
// each carry their own weight decay and learning-rate scale (mx_param_runs; the tables are read when
// the kernel runs).  Element of run r: lr_r = fmul(lr, s_r), then the update above with wd -> wd_r and
// lr -> lr_r.  The ungrouped instantiations carry none of this: their argument block is Hyper alone.
struct Runs {
    const int32_t* off;    // int32 [nseg + 1]: segment s owns runs [off[s], off[s + 1])
    const int64_t* end;    // int64 [nruns]: exclusive end column within the segment, ascending
    const float* wd;       // float [nruns]
    const float* scale;    // float [nruns]
};
struct HyperG : Hyper {
    Runs rn;
};
template <bool GROUPED>
using HyperOf = std::conditional_t<GROUPED, HyperG, Hyper>;

// sgd4's update of one element with the run's own decay and (negated) learning rate
template <bool MOM>
__device__ __forceinline__ float sgd1(float x, float g, float& m, float nlr, float wd, const Hyper& h) {
    float d = wd != 0.0f ? __builtin_fmaf(wd, x, g) : g;
    if constexpr (MOM) {
        const float scaled = h.mom * m;
        m = scaled + d;
        d = h.nesterov ? __builtin_fmaf(h.mom, m, d) : m;
    }
    return __builtin_fmaf(nlr, d, x);
}

// a chunk that lies in one run (the whole work item does): the run's constants are scalars
template <bool MOM>
__device__ __forceinline__ F4 sgd4_run(const F4& x, const F4& g, F4& m, float nlr, float wd, const Hyper& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float mt = MOM ? m[t] : 0.0f;
        out[t] = sgd1<MOM>(x[t], g[t], mt, nlr, wd, h);
        if constexpr (MOM) m[t] = mt;
    }
    return out;
}

// a chunk of a work item that holds a run boundary: every element walks forward from the work item's
// first run `r` to its own (a chunk may span four runs) and derives its constants itself.  The walk
// stops at the segment's last run, so columns at or past the segment's length (zero-filled, never
// stored) read inside the tables.
template <bool MOM>
__device__ __forceinline__ F4 sgd4_walk(const F4& x, const F4& g, F4& m, int64_t c, int r, int rhi, float lr,
                                        const HyperG& h) {
    F4 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        while (r + 1 < rhi && h.rn.end[r] <= c + t) ++r;
        const float lr_r = lr * h.rn.scale[r];                       // one rounding; scale 1.0 gives lr
        float mt = MOM ? m[t] : 0.0f;
        out[t] = sgd1<MOM>(x[t], g[t], mt, -lr_r, h.rn.wd[r], h);
        if constexpr (MOM) m[t] = mt;
    }
    return out;
}

template <int NS>
struct PlanLds {
    int32_t w[mx::kPlanHeader + 2 * NS + NS * kMaxM];
};

// The round to run: `iter`, or with iter_dev (graph-replayable launches) the device counter
// *iter_dev, `iter` then being the schedule length; outside [0, length) the launch is a no-op.
__device__ __forceinline__ int64_t round_of(int64_t iter, const int64_t* iter_dev) {
    if (!iter_dev) return iter;
    const int64_t v = *iter_dev;
    return (v >= 0 && v < iter) ? v : -1;
}

// NS rows x TW columns per work item; a layout tile (mx_sgd_mix_tile) is `split` work items.
// GROUPED: per-run weight decay and learning-rate scale (see Runs above).
template <int NS, int TW, bool NT, bool MOM, bool GROUPED>
__global__ __launch_bounds__(kTPB) void sgd_mix_rows(float* const* __restrict__ x_ptrs,
                                                     float* const* __restrict__ g_ptrs,
                                                     float* const* __restrict__ m_ptrs,
                                                     const int64_t* __restrict__ seg_len,
                                                     const int64_t* __restrict__ tile_off, int nseg,
                                                     int64_t total_tiles, int split,
                                                     const int32_t* __restrict__ plan, int64_t iter,
                                                     const int64_t* __restrict__ iter_dev, int n_local, int M,
                                                     float alpha, HyperOf<GROUPED> h) {
    constexpr int C4 = TW / 4;            // 16-byte chunks per row per work item
    constexpr int NQ = TW / 256;          // 256-column passes per row
    constexpr int NI = NS * NQ;           // items per work item (<= 64: one per lane of wave 0)
    constexpr int E = NS * C4 / kTPB;     // chunks staged per lane
    static_assert(NQ >= 1 && NI <= 64 && NI % kWV == 0 && E % kB == 0 && E * kTPB == NS * C4 && C4 % 64 == 0,
                  "sgd row kernel geometry");
    __shared__ F4 lds[NS * C4];
    __shared__ PlanLds<NS> sp;
    __shared__ int32_t wl[kWV][NI / kWV];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total_work = total_tiles * split;
    const int64_t niter = total_work > blockIdx.x ? (total_work - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (niter == 0) return;                  // block-uniform, before any barrier

    struct Geo {
        int64_t base, col0, lim;             // base: the segment's row of the pointer tables
        // GROUPED only: the first run that ends past col0, the end of the segment's runs, whether that
        // run covers the whole work item, and its pair
        int r0, rhi;
        bool uni;
        float wd, scale;
    };
    auto geo = [&](int64_t work) {
        const int64_t tile = work / split;
        int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (tile_off[mid] <= tile) lo = mid; else hi = mid;
        }
        Geo gq;
        gq.base = (int64_t)lo * n_local;
        gq.col0 = (tile - tile_off[lo]) * ((int64_t)TW * split) + (work % split) * TW;
        gq.lim = seg_len[lo];
        gq.r0 = gq.rhi = 0;
        gq.uni = true;
        gq.wd = gq.scale = 0.0f;
        if constexpr (GROUPED) {
            int a = h.rn.off[lo], b = h.rn.off[lo + 1];
            gq.rhi = b;
            while (a < b) {                  // wave-uniform: the first run with end > col0
                const int mid = (a + b) >> 1;
                if (h.rn.end[mid] <= gq.col0) a = mid + 1; else b = mid;
            }
            gq.r0 = a < gq.rhi ? a : gq.rhi - 1;             // a work item wholly past the segment's length
            const int64_t last = gq.col0 + TW < gq.lim ? gq.col0 + TW : gq.lim;
            gq.uni = h.rn.end[gq.r0] >= last;
            gq.wd = h.rn.wd[gq.r0];
            gq.scale = h.rn.scale[gq.r0];
        }
        return gq;
    };
    // 16-byte accesses only where x, g and m of the (segment, row) are all 16-byte aligned
    auto vec_of = [&](const Geo& gq, int r) {
        bool v = al16(x_ptrs[gq.base + r]) && al16(g_ptrs[gq.base + r]);
        if constexpr (MOM) v = v && al16(m_ptrs[gq.base + r]);
        return v;
    };
    F4 X[kB], G[kB], Mv[kB];
    auto issue = [&](const Geo& gq, int j0) {
#pragma unroll
        for (int t = 0; t < kB; ++t) {
            const int at = wave * 64 + kTPB * (j0 + t);
            const int k = at / C4;                                   // wave-uniform row
            if (k < n_local) {
                const int64_t c = gq.col0 + (int64_t)(at % C4 + lane) * 4;
                const bool vec = vec_of(gq, k);
                X[t] = load_chunk<NT>(x_ptrs[gq.base + k], c, gq.lim, vec);
                G[t] = load_chunk<NT>(g_ptrs[gq.base + k], c, gq.lim, vec);
                if constexpr (MOM) Mv[t] = load_chunk<NT>(m_ptrs[gq.base + k], c, gq.lim, vec);
            }
        }
    };
    // the first chunks' loads fly while the round and its plan record are fetched: every row is read
    // in every round, so they wait for nothing
    Geo cur = geo(blockIdx.x);
    issue(cur, 0);
    const int64_t rnd = round_of(iter, iter_dev);
    if (rnd < 0) return;                     // counter outside the schedule: nothing is written
    {
        const int64_t W = mx::plan_words(n_local, M);
        const int32_t* rec = plan + rnd * W;
        for (int i = tid; i < W; i += kTPB) sp.w[i] = rec[i];
    }
    __syncthreads();
    if (sp.w[2] & 2) return;                 // peer-reads record: not this kernel's (nothing is written)
    const bool active = sp.w[0] != 0;
    const bool idle = (sp.w[2] & 1) != 0;
    const int32_t* deg = sp.w + mx::kPlanHeader;
    const float* sw = reinterpret_cast<const float*>(deg + n_local);
    const int32_t* src = deg + 2 * n_local;
    // rows that get the FMA chain (degree > 0, or every row of an active round in idle mode 1); every
    // other row stores x' as it is
    auto mixes = [&](int r) { return active && (deg[r] > 0 || idle); };
    auto degree = [&](int r) { return mixes(r) ? deg[r] : 0; };
    // GROUPED: the launch's learning rate; the parked work item's -lr_r is derived in park from its own
    // Geo, never from the prefetched one's
    const float nlr = -(h.lr_dev ? *h.lr_dev : h.lr);

    // deal the items (row r, pass q) = r * NQ + q to the waves: wave 0 ranks them by weight
    // (degree + 1), snake order over the waves
    if (wave == 0) {
        const int r = lane / NQ;
        const int w = (lane < NI && r < n_local) ? degree(r) + 1 : 0;
        int rank = 0;
        for (int j = 0; j < NI; ++j) {
            const int wj = __builtin_amdgcn_readlane(w, j);
            rank += (wj > w) || (wj == w && j < lane);
        }
        const int round = rank / kWV, within = rank % kWV;
        if (lane < NI) wl[(round & 1) ? kWV - 1 - within : within][round] = w > 0 ? lane : -1;
    }
    __syncthreads();
    // ranks grow along a wave's list, so its unused (-1) entries form a suffix
    int nmy = 0;
    while (nmy < NI / kWV && wl[wave][nmy] >= 0) ++nmy;
    nmy = __builtin_amdgcn_readfirstlane(nmy);

    // the update of the chunks in flight: x' parked in LDS, m (and the zeros over g) stored
    auto park = [&](const Geo& gq, int j0) {
#pragma unroll
        for (int t = 0; t < kB; ++t) {
            const int at = wave * 64 + kTPB * (j0 + t);
            const int k = at / C4;
            if (k < n_local) {
                const int64_t c = gq.col0 + (int64_t)(at % C4 + lane) * 4;
                const bool vec = vec_of(gq, k);
                const F4 g = h.gscale ? scale4(G[t], h.gscale[k]) : G[t];
                if constexpr (GROUPED) {
                    lds[at + lane] = gq.uni ? sgd4_run<MOM>(X[t], g, Mv[t], -(-nlr * gq.scale), gq.wd, h)
                                            : sgd4_walk<MOM>(X[t], g, Mv[t], c, gq.r0, gq.rhi, -nlr, h);
                } else {
                    lds[at + lane] = sgd4<MOM>(X[t], g, Mv[t], nlr, h);
                }
                if constexpr (MOM) store_chunk<NT>(m_ptrs[gq.base + k], c, gq.lim, vec, Mv[t]);
                if (h.zero_grads) store_chunk<NT>(g_ptrs[gq.base + k], c, gq.lim, vec, F4{0.0f, 0.0f, 0.0f, 0.0f});
            }
        }
    };
    auto mix_tile = [&](const Geo& g) {
        auto finish = [&](int it, F4& acc) {
            const int r = it / NQ;
            const int col = (it % NQ) * 64 + lane;
            const F4 self = lds[r * C4 + col];
            if (mixes(r)) fma4(acc, sw[r], self);                    // the self term, last
            else acc = self;                                         // x' as it is
            store_chunk<NT>(x_ptrs[g.base + r], g.col0 + (int64_t)col * 4, g.lim, vec_of(g, r), acc);
        };
        int p = 0;
        for (; p + 1 < nmy; p += 2) {            // two items interleaved
            const int ia = __builtin_amdgcn_readfirstlane(wl[wave][p]);
            const int ib = __builtin_amdgcn_readfirstlane(wl[wave][p + 1]);
            const int ra = ia / NQ, rb = ib / NQ;
            const int ca = (ia % NQ) * 64 + lane, cb = (ib % NQ) * 64 + lane;
            const int da = degree(ra), db = degree(rb);
            const int dmin = da < db ? da : db;
            F4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
            int e = 0;
            for (; e < dmin; ++e) {
                const int sa = __builtin_amdgcn_readfirstlane(src[ra * M + e]);
                const int sb = __builtin_amdgcn_readfirstlane(src[rb * M + e]);
                const F4 xa = lds[sa * C4 + ca];
                const F4 xb = lds[sb * C4 + cb];
                fma4(a, alpha, xa);
                fma4(b, alpha, xb);
            }
            for (int ea = e; ea < da; ++ea)
                fma4(a, alpha, lds[__builtin_amdgcn_readfirstlane(src[ra * M + ea]) * C4 + ca]);
            for (int eb = e; eb < db; ++eb)
                fma4(b, alpha, lds[__builtin_amdgcn_readfirstlane(src[rb * M + eb]) * C4 + cb]);
            finish(ia, a);
            finish(ib, b);
        }
        if (p < nmy) {
            const int ia = __builtin_amdgcn_readfirstlane(wl[wave][p]);
            const int ra = ia / NQ, ca = (ia % NQ) * 64 + lane;
            const int da = degree(ra);
            F4 a = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int e = 0; e < da; ++e)
                fma4(a, alpha, lds[__builtin_amdgcn_readfirstlane(src[ra * M + e]) * C4 + ca]);
            finish(ia, a);
        }
    };
    for (int64_t i = 0; i < niter; ++i) {
        if (i) __syncthreads();              // every wave is done reading the previous tile
        park(cur, 0);
        for (int j0 = kB; j0 < E; j0 += kB) {
            issue(cur, j0);
            park(cur, j0);
        }
        __syncthreads();                     // every row's x' is staged before any x row is written
        Geo nxt = cur;
        if (i + 1 < niter) {                 // the next work item's first loads fly while this one is mixed
            nxt = geo(blockIdx.x + (i + 1) * gridDim.x);
            issue(nxt, 0);
        }
        mix_tile(cur);
        cur = nxt;
    }
}

struct Cls {
    int ns, tile, tw;    // row class, layout tile (columns), work-item width
};

// the LDS bytes of mix_bf16.hip's classes: 8 / 16 rows are worked in 512-column halves of a
// 1024-column layout tile (16 / 32 KB of LDS per workgroup)
Cls pick(int n_slots) {
    if (n_slots < 1) return {0, 0, 0};
    if (n_slots <= 8) return {8, 1024, 512};
    if (n_slots <= 16) return {16, 1024, 512};
    if (n_slots <= 32) return {32, 512, 512};
    if (n_slots <= 64) return {64, 256, 256};
    return {0, 0, 0};
}

struct Tune {
    int nontemporal = 2;   // 1 / 0: streaming hints on / off; 2 = auto (off for rounds moving 32-320 MB, as mix.hip)
    int wgpc = 0;          // 8 / 16 rows, flat grid: workgroups per CU cap (dynamic LDS); 0 = as many as fit
    int blocks_per_cu = 2; // persistent grids (32 / 64 rows, or more work items than flat_small x the grid)
    int flat_small = 256;  // 8 / 16 rows: one workgroup per work item up to flat_small x CUs x blocks_per_cu items
    int grid = 0;          // > 0: exact persistent grid size (tests: few workgroups looping over many work items)
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

struct Args {
    const mx_sgd_mix_call* c;
    int64_t iter;
    const int64_t* iter_dev;
    Hyper h;
    Runs rn;
    hipStream_t st;
};

template <int NS, int TW, bool NT, bool MOM, bool GROUPED>
int launch(const Args& a) {
    const mx_sgd_mix_call* c = a.c;
    const int split = pick(c->n_local).tile / TW;
    const int64_t work = c->total_tiles * split;
    const int64_t target = g_tune.grid > 0 ? (int64_t)g_tune.grid : (int64_t)cu_count() * g_tune.blocks_per_cu;
    const bool flat = NS <= 16 && g_tune.grid == 0 && g_tune.flat_small > 0 &&
                      work <= (int64_t)g_tune.flat_small * target;
    int64_t grid = flat ? work : (work < target ? work : target);
    if (grid < 1) grid = 1;
    size_t pad = 0;
    if (flat && g_tune.wgpc > 0) {
        static const int stat = [] {                           // static LDS of this instantiation
            hipFuncAttributes fa{};
            return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(sgd_mix_rows<NS, TW, NT, MOM, GROUPED>)) == hipSuccess
                       ? (int)fa.sharedSizeBytes : 0;
        }();
        pad = mx::lds_cap_pad(stat, g_tune.wgpc);
    }
    HyperOf<GROUPED> hy;
    static_cast<Hyper&>(hy) = a.h;
    if constexpr (GROUPED) hy.rn = a.rn;
    hipLaunchKernelGGL((sgd_mix_rows<NS, TW, NT, MOM, GROUPED>), dim3((unsigned)grid), dim3(kTPB), pad, a.st, c->x_ptrs_dev,
                       c->g_ptrs_dev, c->m_ptrs_dev, c->seg_len_dev, c->tile_off_dev, c->nseg, c->total_tiles, split,
                       c->plan_dev, a.iter, a.iter_dev, c->n_local, c->M, c->alpha, hy);
    MX_LAUNCH_CHECK();
    return MX_OK;
}

int sgd_mix(const mx_sgd_mix_call* c, const mx_param_runs* runs, const float* gscale, int64_t iter,
            const int64_t* iter_dev, float lr, const float* lr_dev, void* stream, const char* who) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->x_ptrs_dev && c->g_ptrs_dev && c->seg_len_dev && c->tile_off_dev && c->plan_dev,
             "%s: null pointer", who);
    MX_CHECK(c->nseg >= 1 && c->n_local >= 1, "%s: nseg=%d n_local=%d", who, c->nseg, c->n_local);
    MX_CHECK(c->n_slots == c->n_local, "%s: n_slots=%d != n_local=%d (every partner must be a local row)", who,
             c->n_slots, c->n_local);
    MX_CHECK(c->n_local <= 64, "%s: n_local=%d exceeds 64", who, c->n_local);
    MX_CHECK(c->M >= 1 && c->M <= kMaxM, "%s: M=%d outside [1, %d]", who, c->M, kMaxM);
    MX_CHECK(iter >= 0, "%s: iter < 0", who);
    MX_CHECK((c->mom != 0.0f) == (c->m_ptrs_dev != nullptr), "%s: the momentum table is given exactly when mom != 0",
             who);
    MX_CHECK(c->mom != 0.0f || !c->nesterov, "%s: nesterov needs momentum", who);
    MX_CHECK(!runs || (runs->run_off_dev && runs->run_end_dev && runs->wd_dev && runs->lr_scale_dev && runs->nruns >= 1),
             "%s: parameter runs with a null table or nruns < 1", who);
    if (c->total_tiles <= 0) return MX_OK;
    const Cls cl = pick(c->n_local);
    const bool mom = c->mom != 0.0f;
    // bytes the round moves: x read + written, g read (+ zeroed), m read + written
    const int64_t ws = c->total_tiles * (int64_t)cl.tile * c->n_local * 4 * (3 + (mom ? 2 : 0) + (c->zero_grads ? 1 : 0));
    const bool nt = g_tune.nontemporal == 2 ? (ws <= ((int64_t)32 << 20) || ws > ((int64_t)320 << 20))
                                            : g_tune.nontemporal != 0;
    const Args a{c, iter, iter_dev, Hyper{lr, c->wd, c->mom, lr_dev, gscale, c->nesterov != 0, c->zero_grads != 0},
                 runs ? Runs{runs->run_off_dev, runs->run_end_dev, runs->wd_dev, runs->lr_scale_dev} : Runs{},
                 mx::as_stream(stream)};
#define MX_SGD_G(N, TW, G)                                                                         \
    (nt ? (mom ? launch<N, TW, true, true, G>(a) : launch<N, TW, true, false, G>(a))               \
        : (mom ? launch<N, TW, false, true, G>(a) : launch<N, TW, false, false, G>(a)))
#define MX_SGD(N, TW) (runs ? MX_SGD_G(N, TW, true) : MX_SGD_G(N, TW, false))
    switch (cl.ns) {
        case 8: return MX_SGD(8, 512);
        case 16: return MX_SGD(16, 512);
        case 32: return MX_SGD(32, 512);
        default: return MX_SGD(64, 256);
    }
#undef MX_SGD
#undef MX_SGD_G
}
}  // namespace

extern "C" int mx_sgd_mix_tile(int n_slots) { return pick(n_slots).tile; }

extern "C" int mx_sgd_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    MX_CHECK(seg_len_host && tile_off_host && nseg >= 1, "mx_sgd_mix_layout: bad arguments");
    const int tile = mx_sgd_mix_tile(n_slots);
    MX_CHECK(tile > 0, "mx_sgd_mix_layout: n_slots=%d outside [1, 64]", n_slots);
    tile_off_host[0] = 0;
    for (int s = 0; s < nseg; ++s) {
        MX_CHECK(seg_len_host[s] >= 0, "mx_sgd_mix_layout: negative length");
        tile_off_host[s + 1] = tile_off_host[s] + (seg_len_host[s] + tile - 1) / tile;
    }
    return MX_OK;
}

extern "C" int mx_sgd_mix_set(const char* key, int value) {
    MX_CHECK(key, "mx_sgd_mix_set: null key");
    if (!strcmp(key, "nontemporal")) {
        g_tune.nontemporal = value == 2 ? 2 : (value ? 1 : 0);
    } else if (!strcmp(key, "wgpc")) {
        MX_CHECK(value >= 0 && value <= 32, "mx_sgd_mix_set: wgpc %d", value);
        g_tune.wgpc = value;
    } else if (!strcmp(key, "blocks_per_cu")) {
        MX_CHECK(value >= 1 && value <= 64, "mx_sgd_mix_set: blocks_per_cu %d", value);
        g_tune.blocks_per_cu = value;
    } else if (!strcmp(key, "flat_small")) {
        MX_CHECK(value >= 0 && value <= 4096, "mx_sgd_mix_set: flat_small %d", value);
        g_tune.flat_small = value;
    } else if (!strcmp(key, "grid")) {
        MX_CHECK(value >= 0 && value <= 65536, "mx_sgd_mix_set: grid %d", value);
        g_tune.grid = value;
    } else {
        MX_CHECK(false, "mx_sgd_mix_set: unknown key '%s'", key);
    }
    return MX_OK;
}

extern "C" int mx_sgd_mix_get(const char* key) {
    if (!key) return MX_ERR_INVALID;
    if (!strcmp(key, "nontemporal")) return g_tune.nontemporal;
    if (!strcmp(key, "wgpc")) return g_tune.wgpc;
    if (!strcmp(key, "blocks_per_cu")) return g_tune.blocks_per_cu;
    if (!strcmp(key, "flat_small")) return g_tune.flat_small;
    if (!strcmp(key, "grid")) return g_tune.grid;
    mx::set_error("mx_sgd_mix_get: unknown key '%s'", key);
    return MX_ERR_INVALID;
}

extern "C" int mx_sgd_mix(const mx_sgd_mix_call* c, int64_t iter, float lr, const float* lr_dev, void* stream) {
    return sgd_mix(c, nullptr, nullptr, iter, nullptr, lr, lr_dev, stream, "mx_sgd_mix");
}

extern "C" int mx_sgd_mix_scaled(const mx_sgd_mix_call* c, const float* gscale_dev, int64_t iter, float lr,
                                 const float* lr_dev, void* stream) {
    return sgd_mix(c, nullptr, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_sgd_mix_scaled");
}

extern "C" int mx_sgd_mix_at(const mx_sgd_mix_call* c, const int64_t* iter_dev, int64_t n_iters, float lr,
                             const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_sgd_mix_at: null iteration counter");
    return sgd_mix(c, nullptr, nullptr, n_iters, iter_dev, lr, lr_dev, stream, "mx_sgd_mix_at");
}

extern "C" int mx_sgd_mix_scaled_at(const mx_sgd_mix_call* c, const float* gscale_dev, const int64_t* iter_dev,
                                    int64_t n_iters, float lr, const float* lr_dev, void* stream) {
    MX_CHECK(iter_dev, "mx_sgd_mix_scaled_at: null iteration counter");
    return sgd_mix(c, nullptr, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_sgd_mix_scaled_at");
}

extern "C" int mx_sgd_mix_grouped(const mx_sgd_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                  int64_t iter, float lr, const float* lr_dev, void* stream) {
    return sgd_mix(c, runs, gscale_dev, iter, nullptr, lr, lr_dev, stream, "mx_sgd_mix_grouped");
}

extern "C" int mx_sgd_mix_grouped_at(const mx_sgd_mix_call* c, const mx_param_runs* runs, const float* gscale_dev,
                                     const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                                     void* stream) {
    MX_CHECK(iter_dev, "mx_sgd_mix_grouped_at: null iteration counter");
    return sgd_mix(c, runs, gscale_dev, n_iters, iter_dev, lr, lr_dev, stream, "mx_sgd_mix_grouped_at");
}
