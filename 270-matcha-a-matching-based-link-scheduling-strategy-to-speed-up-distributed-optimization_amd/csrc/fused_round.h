// fused_round.h -- the scaffold the fused optimizer rounds share (sgd_mix.hip, adamw_mix.hip, lion_mix.hip,
// qgm_mix.hip and the _bf16 file of each): one row kernel that stages a work item's updated rows in LDS and
// runs the mixing round on them, the host side that picks its class, grid and streaming mode, the two
// storage forms and the definition of a family's entry points.
//
// A family supplies a compile-time policy type `Update` and nothing else:
//     Hyper                 the launch's argument block (fields lr, lr_dev, gscale, zero_grads and its own)
//     Tabs                  its pointer tables, one `T* const*` per array, in kernel-argument order
//     Lane                  what a lane keeps in flight: kB chunks of every array it reads
//     State                 what a launch (and, grouped, a work item) derives from Hyper
//     vec_of(tb, gq, k)     the alignment rule of the (segment, row): true = wide accesses
//     load<NT>(...)         issues the loads of chunk t into Lane
//     no_step(st, h)        launch-uniform: true = no such optimizer step, the launch writes nothing
//     setup(st, h)          the per-launch constants
//     begin_item<G>(...)    the per-work-item constants of a grouped launch
//     update<G>(...)        the optimizer update of chunk t in registers: returns x' for LDS
//     keep<SP>(...)         stores the state the lane owns and, with zero_grads, the zeros over g
//     finish<SP>(...)       stores a mixed chunk (and, bf16 families, its rounded image)
// (SP: the store policy, mx::StorePolicy -- its 16-byte stores; the 8-byte bf16 stores are plain or nt)
// One optional hook, for an optimizer whose state follows the MIXED row (quasi-global momentum, qgm_mix.hip):
//     kAfterMix = true      a static constexpr flag of the policy; the kernel then calls
//     after_mix<G, SP>(tb, geo, r, c, vec, acc, st, h)   in place of finish: the mixed chunk together with the
//                           launch state and the (grouped) argument block; the work item's own Geo resolves
//                           the run, as sgd_chunk does
// Everything a policy decides is decided at compile time; the kernel has no run-time branch on the family.
// Policies without the flag compile to exactly what they did without the hook.
//
// An optimizer's two families (fp32 rows; bf16 rows over fp32 masters) differ only in storage, so each
// optimizer writes ONE policy template over a storage form (Fp32Form, Bf16Form, and gradient tracking's
// Bf16GradForm and Fp32GradForm: at the end of this file) in its *_update.h, beside its arithmetic and its one host function template.  A form supplies
//     GT, GC                the gradient's element and chunk type (float / F4, uint16_t / U2)
//     PTab                  the type of the last member `p` of every Tabs: the bf16 model rows' table (fp32: empty)
//     zero()                the chunk stored over g
//     al(tb, gq, k)         its share of the alignment rule: g (and p) of the (segment, row)
//     store<SP>(...)        the store of a mixed chunk: x, or the master and p = pack4(acc)
//     kBytes                the bytes per element the round moves on x, g (and p)
//     tables(c), run<U>(..) which fields of the call record are its tables, and dispatch with them in
//                           kernel-argument order: x, g, the optimizer's state tables (, p)
// A policy's Tabs names the mixed fp32 row `x` in both forms (the master `w` of a bf16 call record).  The
// kernel is instantiated with NAMED policies, one line each in the family's .hip file
// (template <bool MOM> struct SgdMixBf16 : SgdRows<Bf16Form, MOM> {};), so kernel traces and resource tables
// show the family.  MX_FUSED_FAMILY, also at the end, defines a family's knobs and its ten entry points.
// A new optimizer is one policy template, two named policies and two MX_FUSED_FAMILY lines: nothing in this
// file changes.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  State arrays are read and written by the same lane only, so
// they are stored when their chunk is staged.  Because every row is read in every round, the first loads
// are issued before the round, the step and the plan record are looked at; every return happens before
// any store and is taken by the whole block.
#pragma once
#include "fused_host.h"
#include "mx_common.h"
#include "row_walk.h"

#include <type_traits>

namespace mx {
namespace fused {
// the access helpers and the fp32 chunk the families use too; the kernel names the rest as rows::
using rows::al16;
using rows::F4;
using rows::fma4;
using rows::GPtr;
using rows::kMaxM;
using rows::ld2;
using rows::st2;

constexpr int kTPB = 256;
constexpr int kWV = kTPB / 64;
// 16-byte chunks of every array a lane has in flight at once: 2 keeps the 8-row SGD kernel at 68 VGPRs
// (7 waves per SIMD) and measured 3 % faster on the headline shape than 4 (94 VGPRs, 5 waves); for AdamW
// it is 32 VGPRs of loads in flight (the bf16 families hold g in 2 registers, not 4)
constexpr int kB = 2;

typedef float F2 __attribute__((ext_vector_type(2)));
typedef __bf16 B2 __attribute__((ext_vector_type(2)));
typedef uint32_t U2 __attribute__((ext_vector_type(2)));      // 4 bf16: one 8-byte access

template <bool NT>
__device__ __forceinline__ F4 ld16(const float* p) {
    const GPtr<const F4> g = (GPtr<const F4>)(p);
    if constexpr (NT) return __builtin_nontemporal_load(g);
    else return *g;
}
template <int SP>
__device__ __forceinline__ void st16(float* p, const F4& v) {
    mx::store16<SP>(reinterpret_cast<F4*>(p), v);
}
template <bool NT>
__device__ __forceinline__ U2 ld8(const uint16_t* p) {
    const GPtr<const U2> g = (GPtr<const U2>)(p);
    if constexpr (NT) return __builtin_nontemporal_load(g);
    else return *g;
}
// 8-byte stores never take a write-through policy (narrow sc1 stores cost 2.7x per byte): nt or plain
template <int SP>
__device__ __forceinline__ void st8(uint16_t* p, const U2& v) {
    const GPtr<U2> g = (GPtr<U2>)(p);
    if constexpr (SP != mx::kStorePlain) __builtin_nontemporal_store(v, g);
    else *g = v;
}
__device__ __forceinline__ float ld4(const float* p) { return *(GPtr<const float>)(p); }
__device__ __forceinline__ void st4(float* p, float v) { *(GPtr<float>)(p) = v; }
__device__ __forceinline__ bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// one lane's chunk of 4 elements at column c of `row`: one wide access on the vector path (`vec`: the
// family's alignment rule holds for the (segment, row)) when the chunk is in range, else one access per
// element, zero-filled from `lim` on; nothing is ever stored at or past `lim`
template <bool NT>
__device__ __forceinline__ F4 load_chunk(const float* row, int64_t c, int64_t lim, bool vec) {
    if (vec && c + 4 <= lim) return ld16<NT>(row + c);
    F4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = (c + t < lim) ? ld4(row + c + t) : 0.0f;
    return v;
}
template <int SP>
__device__ __forceinline__ void store_chunk(float* row, int64_t c, int64_t lim, bool vec, const F4& v) {
    if (vec && c + 4 <= lim) {
        st16<SP>(row + c, v);
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < lim) st4(row + c + t, v[t]);
}
template <bool NT>
__device__ __forceinline__ U2 load_chunk(const uint16_t* row, int64_t c, int64_t lim, bool vec) {
    if (vec && c + 4 <= lim) return ld8<NT>(row + c);
    U2 v;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t lo = (c + 2 * t < lim) ? ld2(row + c + 2 * t) : 0u;
        const uint32_t hi = (c + 2 * t + 1 < lim) ? ld2(row + c + 2 * t + 1) : 0u;
        v[t] = lo | (hi << 16);
    }
    return v;
}
template <int SP>
__device__ __forceinline__ void store_chunk(uint16_t* row, int64_t c, int64_t lim, bool vec, const U2& v) {
    if (vec && c + 4 <= lim) {
        st8<SP>(row + c, v);
        return;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (c + 2 * t < lim) st2(row + c + 2 * t, v[t] & 0xFFFFu);
        if (c + 2 * t + 1 < lim) st2(row + c + 2 * t + 1, v[t] >> 16);
    }
}

// f32() of 4 bf16: the exact widening bits << 16 (an fp32 chunk is its own widening)
__device__ __forceinline__ F4 widen4(const U2& g) {
    F4 v;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        v[2 * t] = __builtin_bit_cast(float, g[t] << 16);
        v[2 * t + 1] = __builtin_bit_cast(float, g[t] & 0xFFFF0000u);
    }
    return v;
}
__device__ __forceinline__ F4 widen4(const F4& g) { return g; }

// the one rounding: fp32 -> bf16, to nearest even (v_cvt_pk_bf16_f32; NaN stays NaN)
__device__ __forceinline__ U2 pack4(const F4& a) {
    U2 v;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const F2 f = {a[2 * t], a[2 * t + 1]};
        v[t] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, B2));
    }
    return v;
}

// the clip factor of the row (mx_*_scaled): g' = fmul(gscale[r], f32(g)), before anything else in the update
__device__ __forceinline__ F4 scale4(const F4& g, float s) {
    F4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = s * g[t];
    return v;
}
// row k's gradient chunk as the update sees it: widened, and scaled where the launch has clip factors
template <class G, class H>
__device__ __forceinline__ F4 grad_of(const G& g, const H& h, int k) {
    return h.gscale ? scale4(widen4(g), h.gscale[k]) : widen4(g);
}

// Per-parameter-group launches (mx_*_grouped): the columns of a segment are cut into runs that each
// carry their own weight decay and learning-rate scale (mx_param_runs; the tables are read when the
// kernel runs).  Element of run r: lr_r = fmul(lr, s_r), then the family's update with wd -> wd_r and
// lr -> lr_r.  The ungrouped instantiations carry none of this: their argument block is Hyper alone.
struct Runs {
    const int32_t* off;    // int32 [nseg + 1]: segment s owns runs [off[s], off[s + 1])
    const int64_t* end;    // int64 [nruns]: exclusive end column within the segment, ascending
    const float* wd;       // float [nruns]
    const float* scale;    // float [nruns]
};
template <class Hyper>
struct Grouped : Hyper {
    Runs rn;
};
template <class Hyper, bool GROUPED>
using GroupedIf = std::conditional_t<GROUPED, Grouped<Hyper>, Hyper>;
template <class Update, bool GROUPED>
using HyperOf = GroupedIf<typename Update::Hyper, GROUPED>;

// the optional hook: a policy that declares `static constexpr bool kAfterMix = true` gets after_mix, not finish
template <class Update, class = void>
struct AfterMix : std::false_type {};
template <class Update>
struct AfterMix<Update, std::void_t<decltype(Update::kAfterMix)>> : std::bool_constant<Update::kAfterMix> {};

// where a work item lies
struct Geo {
    int64_t base, col0, lim;             // base: the segment's row of the pointer tables
    // GROUPED only: the first run that ends past col0, the end of the segment's runs, whether that
    // run covers the whole work item, and its pair
    int r0, rhi;
    bool uni;
    float wd, scale;
};

// NS rows x TW columns per work item; a layout tile (mx_*_tile) is `split` work items.
// GROUPED: per-run weight decay and learning-rate scale (see Runs above).  SP: the store policy of the
// 16-byte stores (mx::StorePolicy; the loads follow NT).  T...: Update::Tabs' members.
template <class Update, int NS, int TW, bool NT, bool GROUPED, int SP, class... T>
__global__ __launch_bounds__(kTPB) void fused_round_rows(T __restrict__... tabs,
                                                         const int64_t* __restrict__ seg_len,
                                                         const int64_t* __restrict__ tile_off, int nseg,
                                                         int64_t total_tiles, int split,
                                                         const int32_t* __restrict__ plan, int64_t iter,
                                                         const int64_t* __restrict__ iter_dev, int n_local, int M,
                                                         float alpha, HyperOf<Update, GROUPED> h) {
    constexpr int C4 = TW / 4;            // 4-element chunks per row per work item
    constexpr int NQ = TW / 256;          // 256-column passes per row
    constexpr int NI = NS * NQ;           // items per work item (<= 64: one per lane of wave 0)
    constexpr int E = NS * C4 / kTPB;     // chunks staged per lane
    static_assert(NQ >= 1 && NI <= 64 && NI % kWV == 0 && E % kB == 0 && E * kTPB == NS * C4 && C4 % 64 == 0,
                  "fused row kernel geometry");
    __shared__ F4 lds[NS * C4];
    __shared__ rows::PlanLds<NS> sp;
    __shared__ int32_t wl[kWV][NI / kWV];
    const typename Update::Tabs tb{tabs...};
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total_work = total_tiles * split;
    const int64_t niter = total_work > blockIdx.x ? (total_work - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (niter == 0) return;                  // block-uniform, before any barrier

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
    typename Update::Lane ln;
    auto issue = [&](const Geo& gq, int j0) {
#pragma unroll
        for (int t = 0; t < kB; ++t) {
            const int at = wave * 64 + kTPB * (j0 + t);
            const int k = at / C4;                                   // wave-uniform row
            if (k < n_local) {
                const int64_t c = gq.col0 + (int64_t)(at % C4 + lane) * 4;
                Update::template load<NT>(ln, t, tb, gq, k, c, Update::vec_of(tb, gq, k));
            }
        }
    };
    // the first chunks' loads fly while the round and its plan record are fetched: every row is read
    // in every round, so they wait for nothing
    Geo cur = geo(blockIdx.x);
    issue(cur, 0);
    const int64_t rnd = rows::round_of(iter, iter_dev);
    if (rnd < 0) return;                     // counter outside the schedule: nothing is written
    typename Update::State st;
    if (Update::no_step(st, h)) return;      // no such optimizer step: nothing is written
    rows::copy_plan<NS, kTPB>(sp, plan, rnd, n_local, M);
    if (sp.w[2] & 2) return;                 // peer-reads record: not this kernel's (nothing is written)
    const bool active = sp.w[0] != 0;
    const bool idle = (sp.w[2] & 1) != 0;
    const rows::Plan pv = rows::view(sp, n_local);
    // rows that get the FMA chain (degree > 0, or every row of an active round in idle mode 1); every
    // other row stores x' as it is
    auto mixes = [&](int r) { return active && (pv.deg[r] > 0 || idle); };
    auto degree = [&](int r) { return mixes(r) ? pv.deg[r] : 0; };
    Update::setup(st, h);

    // every row is dealt, by weight degree + 1
    if (wave == 0) rows::deal<NQ, NI, kWV>(wl, lane, [&](int r) { return r < n_local ? degree(r) + 1 : 0; });
    __syncthreads();
    const int nmy = rows::count(wl[wave]);

    // the update of the chunks in flight: x' parked in LDS, the lane's state (and the zeros over g) stored
    auto park = [&](const Geo& gq, int j0) {
#pragma unroll
        for (int t = 0; t < kB; ++t) {
            const int at = wave * 64 + kTPB * (j0 + t);
            const int k = at / C4;
            if (k < n_local) {
                const int64_t c = gq.col0 + (int64_t)(at % C4 + lane) * 4;
                const bool vec = Update::vec_of(tb, gq, k);
                lds[at + lane] = Update::template update<GROUPED>(ln, t, k, c, gq, st, h);
                Update::template keep<SP>(ln, t, tb, gq, k, c, vec, h);
            }
        }
    };
    // the mixing walk: partners in ascending matching order, the self term last, one __builtin_fmaf per step
    auto mix_tile = [&](const Geo& g) {
        auto finish = [&](int it, F4& acc) {
            const int r = it / NQ;
            const int col = (it % NQ) * 64 + lane;
            const F4 self = lds[r * C4 + col];
            if (mixes(r)) fma4(acc, pv.sw[r], self);                    // the self term, last
            else acc = self;                                         // x' as it is
            if constexpr (AfterMix<Update>::value)
                Update::template after_mix<GROUPED, SP>(tb, g, r, g.col0 + (int64_t)col * 4, Update::vec_of(tb, g, r),
                                                        acc, st, h);
            else
                Update::template finish<SP>(tb, g, r, g.col0 + (int64_t)col * 4, Update::vec_of(tb, g, r), acc);
        };
        rows::walk<rows::Fp32, NQ, C4>(lds, wl[wave], nmy, lane, pv.src, M, alpha, degree, finish);
    };
    for (int64_t i = 0; i < niter; ++i) {
        if (i) __syncthreads();              // every wave is done reading the previous tile
        // the parked work item's constants come from its own Geo (`cur`), never the prefetched one's
        Update::template begin_item<GROUPED>(st, cur, h);
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

// ---------------------------------------------------------------- host side (fused_host.h, fused_round.cpp)

// the launch-independent fields every call record carries, and what the entry point adds
struct Round {
    const int64_t* seg_len;
    const int64_t* tile_off;
    const int32_t* plan;
    int64_t total_tiles;
    int nseg, n_local, M;
    float alpha;
    int64_t iter;
    const int64_t* iter_dev;
    hipStream_t stream;
};

// the checks common to the four call records (`who`: the entry point called; the family has looked at
// the record's pointers), then the record's Round
template <class Call>
int check_round(const Call* c, int64_t iter, const int64_t* iter_dev, void* stream, const char* who, Round* r) {
    MX_CHECK(c->nseg >= 1 && c->n_local >= 1, "%s: nseg=%d n_local=%d", who, c->nseg, c->n_local);
    MX_CHECK(c->n_slots == c->n_local, "%s: n_slots=%d != n_local=%d (every partner must be a local row)", who,
             c->n_slots, c->n_local);
    MX_CHECK(c->n_local <= 64, "%s: n_local=%d exceeds 64", who, c->n_local);
    MX_CHECK(c->M >= 1 && c->M <= kMaxM, "%s: M=%d outside [1, %d]", who, c->M, kMaxM);
    *r = Round{c->seg_len_dev, c->tile_off_dev, c->plan_dev, c->total_tiles, c->nseg, c->n_local, c->M, c->alpha,
               iter, iter_dev, mx::as_stream(stream)};
    return MX_OK;
}
// the last check of every family, after its own (the order of the checks decides which of two faults is
// reported)
inline int check_runs(const mx_param_runs* runs, const char* who) {
    MX_CHECK(!runs || (runs->run_off_dev && runs->run_end_dev && runs->wd_dev && runs->lr_scale_dev && runs->nruns >= 1),
             "%s: parameter runs with a null table or nruns < 1", who);
    return MX_OK;
}

template <class Update, int NS, int TW, bool NT, bool GROUPED, int SP = NT ? mx::kStoreNt : mx::kStorePlain, class... T>
int launch(const Tune& tune, const Round& r, const typename Update::Hyper& h, const mx_param_runs* runs, T... tabs) {
    const auto kernel = fused_round_rows<Update, NS, TW, NT, GROUPED, SP, T...>;
    const int split = pick(r.n_local).tile / TW;
    bool flat = false;
    const int64_t grid = tune.grid_of(NS, r.total_tiles * split, &flat);
    size_t pad = 0;
    if (flat && tune.wgpc > 0) {
        static const int stat = [kernel] {                     // static LDS of this instantiation
            hipFuncAttributes fa{};
            return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) == hipSuccess ? (int)fa.sharedSizeBytes
                                                                                                   : 0;
        }();
        pad = mx::lds_cap_pad(stat, tune.wgpc);
    }
    HyperOf<Update, GROUPED> hy;
    static_cast<typename Update::Hyper&>(hy) = h;
    if constexpr (GROUPED) hy.rn = Runs{runs->run_off_dev, runs->run_end_dev, runs->wd_dev, runs->lr_scale_dev};
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kTPB), pad, r.stream, tabs..., r.seg_len, r.tile_off, r.nseg,
                       r.total_tiles, split, r.plan, r.iter, r.iter_dev, r.n_local, r.M, r.alpha, hy);
    MX_LAUNCH_CHECK();
    return MX_OK;
}

// the instantiation of a checked call: row class x streaming mode x grouped (runs != NULL), and for the
// streaming launches of the 8- and 16-row classes the store policy; bytes_per_elem: what the round moves
// per (row, column)
template <class Update, class... T>
int dispatch(const Tune& tune, const Round& r, int bytes_per_elem, const typename Update::Hyper& h,
             const mx_param_runs* runs, T... tabs) {
    const Cls cls = pick(r.n_local);
    const bool nt = tune.streaming(r.total_tiles, cls.tile, r.n_local, bytes_per_elem);
    const int pol = tune.policy(nt, r.total_tiles, cls.tile, r.n_local, bytes_per_elem);
#define MX_FUSED_POL(N, TW, P)                                                                                \
    (runs ? launch<Update, N, TW, true, true, P>(tune, r, h, runs, tabs...)                                  \
          : launch<Update, N, TW, true, false, P>(tune, r, h, runs, tabs...))
#define MX_FUSED_S(N, TW)                                                                                     \
    (pol == mx::kStoreSc1 ? MX_FUSED_POL(N, TW, mx::kStoreSc1)                                                \
                          : pol == mx::kStoreSc1Nt ? MX_FUSED_POL(N, TW, mx::kStoreSc1Nt) : MX_FUSED(N, TW))
#define MX_FUSED(N, TW)                                                                                       \
    (runs ? (nt ? launch<Update, N, TW, true, true>(tune, r, h, runs, tabs...)                              \
                : launch<Update, N, TW, false, true>(tune, r, h, runs, tabs...))                             \
          : (nt ? launch<Update, N, TW, true, false>(tune, r, h, runs, tabs...)                             \
                : launch<Update, N, TW, false, false>(tune, r, h, runs, tabs...)))
    switch (cls.ns) {
        case 8: return MX_FUSED_S(8, 512);
        case 16: return MX_FUSED_S(16, 512);
        case 32: return MX_FUSED(32, 512);
        default: return MX_FUSED(64, 256);
    }
#undef MX_FUSED
#undef MX_FUSED_S
#undef MX_FUSED_POL
}

// ---------------------------------------------------------------- the storage forms

// The helpers index the tables as the policies do, tb.g[gq.base + k] at every use: with the index computed
// once by the caller the bf16 kernels came out different (profiles/fused_forms_refactor.md).

// fp32 rows: x, g and the optimizer's state all fp32, 16-byte accesses
struct NoTable {};
struct Fp32Form {
    using GT = float;
    using GC = F4;
    using PTab = NoTable;
    static constexpr int kBytes = 12;      // x read + written, g read
    static __device__ __forceinline__ GC zero() { return F4{0.0f, 0.0f, 0.0f, 0.0f}; }
    template <class Tabs>
    static __device__ __forceinline__ bool al(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.g[gq.base + k]);
    }
    template <int SP, class Tabs>
    static __device__ __forceinline__ void store(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                 const F4& acc) {
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
    }
    template <class Call>
    static bool tables(const Call* c) {
        return c->x_ptrs_dev && c->g_ptrs_dev;
    }
    template <class Update, class Call, class... S>
    static int run(const Tune& tune, const Round& r, int bpe, const typename Update::Hyper& h, const mx_param_runs* runs,
                   const Call* c, S... state) {
        return dispatch<Update>(tune, r, bpe, h, runs, c->x_ptrs_dev, c->g_ptrs_dev, state...);
    }
};

// bf16 rows over fp32 masters: the master w (a policy's `x`) and the state fp32, the gradient g and the
// model row p bf16 in 8-byte accesses; p is write only, the rounded image of every master chunk stored
struct Bf16Form {
    using GT = uint16_t;
    using GC = U2;
    using PTab = uint16_t* const*;
    static constexpr int kBytes = 12;      // w read + written, g read, p written
    static __device__ __forceinline__ GC zero() { return U2{0u, 0u}; }
    template <class Tabs>
    static __device__ __forceinline__ bool al(const Tabs& tb, const Geo& gq, int k) {
        return al8(tb.g[gq.base + k]) && al8(tb.p[gq.base + k]);
    }
    template <int SP, class Tabs>
    static __device__ __forceinline__ void store(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                 const F4& acc) {
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
        store_chunk<SP>(tb.p[gq.base + k], c, gq.lim, vec, pack4(acc));         // the model row: bf16 of the stored w
    }
    template <class Call>
    static bool tables(const Call* c) {
        return c->w_ptrs_dev && c->g_ptrs_dev && c->p_ptrs_dev;
    }
    template <class Update, class Call, class... S>
    static int run(const Tune& tune, const Round& r, int bpe, const typename Update::Hyper& h, const mx_param_runs* runs,
                   const Call* c, S... state) {
        return dispatch<Update>(tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev, state..., c->p_ptrs_dev);
    }
};

// The two forms of gradient tracking (gt_update.h), whose second gossiped array is an fp32 row that is no
// model: its track launch mixes the tracker (no bf16 image to write), its mixed-precision step launch reads
// the tracker where the others read a bf16 gradient.

// fp32 mixed row with no model row, bf16 gradient in 8-byte accesses: Fp32Form's tables and store, Bf16Form's g
struct Bf16GradForm {
    using GT = uint16_t;
    using GC = U2;
    using PTab = NoTable;
    static constexpr int kBytes = 10;      // x read + written, g read
    static __device__ __forceinline__ GC zero() { return U2{0u, 0u}; }
    template <class Tabs>
    static __device__ __forceinline__ bool al(const Tabs& tb, const Geo& gq, int k) {
        return al8(tb.g[gq.base + k]);
    }
    template <int SP, class Tabs>
    static __device__ __forceinline__ void store(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                 const F4& acc) {
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
    }
    template <class Call>
    static bool tables(const Call* c) {
        return c->x_ptrs_dev && c->g_ptrs_dev;
    }
    template <class Update, class Call, class... S>
    static int run(const Tune& tune, const Round& r, int bpe, const typename Update::Hyper& h, const mx_param_runs* runs,
                   const Call* c, S... state) {
        return dispatch<Update>(tune, r, bpe, h, runs, c->x_ptrs_dev, c->g_ptrs_dev, state...);
    }
};

// bf16 rows over fp32 masters with an fp32 "gradient" in 16-byte accesses: Bf16Form's tables and store,
// Fp32Form's g
struct Fp32GradForm {
    using GT = float;
    using GC = F4;
    using PTab = uint16_t* const*;
    static constexpr int kBytes = 14;      // w read + written, g read, p written
    static __device__ __forceinline__ GC zero() { return F4{0.0f, 0.0f, 0.0f, 0.0f}; }
    template <class Tabs>
    static __device__ __forceinline__ bool al(const Tabs& tb, const Geo& gq, int k) {
        return al16(tb.g[gq.base + k]) && al8(tb.p[gq.base + k]);
    }
    template <int SP, class Tabs>
    static __device__ __forceinline__ void store(const Tabs& tb, const Geo& gq, int k, int64_t c, bool vec,
                                                 const F4& acc) {
        store_chunk<SP>(tb.x[gq.base + k], c, gq.lim, vec, acc);
        store_chunk<SP>(tb.p[gq.base + k], c, gq.lim, vec, pack4(acc));         // the model row: bf16 of the stored w
    }
    template <class Call>
    static bool tables(const Call* c) {
        return c->w_ptrs_dev && c->g_ptrs_dev && c->p_ptrs_dev;
    }
    template <class Update, class Call, class... S>
    static int run(const Tune& tune, const Round& r, int bpe, const typename Update::Hyper& h, const mx_param_runs* runs,
                   const Call* c, S... state) {
        return dispatch<Update>(tune, r, bpe, h, runs, c->w_ptrs_dev, c->g_ptrs_dev, state..., c->p_ptrs_dev);
    }
};

}  // namespace fused
}  // namespace mx

// ---------------------------------------------------------------- a family's entry points

// MX_FUSED_FAMILY(name, TUNE, S, round): the knobs of family `name` (its own TUNE instance: mx::fused::Tune,
// or a type derived from it whose set / get know further keys) and its ten entry points, as
// include/matcha_gossip.h declares them.  `round` is the optimizer's host function template instantiated
// with the family's named policy: round(tune, c, runs, gscale, iter, iter_dev, [step, step_dev,] lr, lr_dev,
// stream, who).  S is MX_WITH_STEP for an optimizer with a step counter (AdamW), else MX_NO_STEP.
#define MX_NO_STEP(...)
#define MX_WITH_STEP(...) __VA_ARGS__
#define MX_FUSED_FAMILY(name, TUNE, S, ...)                                                                            \
    namespace {                                                                                                        \
    TUNE g_tune;                                                                                                       \
    }                                                                                                                  \
    extern "C" int mx_##name##_tile(int n_slots) { return mx::fused::pick(n_slots).tile; }                             \
    extern "C" int mx_##name##_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {    \
        return mx::fused::layout("mx_" #name "_layout", seg_len_host, nseg, n_slots, tile_off_host);                   \
    }                                                                                                                  \
    extern "C" int mx_##name##_set(const char* key, int value) { return g_tune.set("mx_" #name "_set", key, value); }  \
    extern "C" int mx_##name##_get(const char* key) { return g_tune.get("mx_" #name "_get", key); }                    \
    extern "C" int mx_##name(const mx_##name##_call* c, int64_t iter, S(int64_t step, ) float lr, const float* lr_dev, \
                             void* stream) {                                                                           \
        return __VA_ARGS__(g_tune, c, nullptr, nullptr, iter, nullptr, S(step, nullptr, ) lr, lr_dev, stream,          \
                           "mx_" #name);                                                                               \
    }                                                                                                                  \
    extern "C" int mx_##name##_scaled(const mx_##name##_call* c, const float* gscale_dev, int64_t iter,                \
                                      S(int64_t step, ) float lr, const float* lr_dev, void* stream) {                 \
        return __VA_ARGS__(g_tune, c, nullptr, gscale_dev, iter, nullptr, S(step, nullptr, ) lr, lr_dev, stream,       \
                           "mx_" #name "_scaled");                                                                     \
    }                                                                                                                  \
    extern "C" int mx_##name##_grouped(const mx_##name##_call* c, const mx_param_runs* runs, const float* gscale_dev,  \
                                       int64_t iter, S(int64_t step, ) float lr, const float* lr_dev, void* stream) {  \
        return __VA_ARGS__(g_tune, c, runs, gscale_dev, iter, nullptr, S(step, nullptr, ) lr, lr_dev, stream,          \
                           "mx_" #name "_grouped");                                                                    \
    }                                                                                                                  \
    extern "C" int mx_##name##_at(const mx_##name##_call* c, const int64_t* iter_dev, int64_t n_iters,                 \
                                  S(const int64_t* step_dev, ) float lr, const float* lr_dev, void* stream) {          \
        MX_CHECK(iter_dev S(&& step_dev), "mx_" #name "_at: null iteration" S(" or step") " counter");                 \
        return __VA_ARGS__(g_tune, c, nullptr, nullptr, n_iters, iter_dev, S(0, step_dev, ) lr, lr_dev, stream,        \
                           "mx_" #name "_at");                                                                         \
    }                                                                                                                  \
    extern "C" int mx_##name##_scaled_at(const mx_##name##_call* c, const float* gscale_dev, const int64_t* iter_dev,  \
                                         int64_t n_iters, S(const int64_t* step_dev, ) float lr, const float* lr_dev,  \
                                         void* stream) {                                                               \
        MX_CHECK(iter_dev S(&& step_dev), "mx_" #name "_scaled_at: null iteration" S(" or step") " counter");          \
        return __VA_ARGS__(g_tune, c, nullptr, gscale_dev, n_iters, iter_dev, S(0, step_dev, ) lr, lr_dev, stream,     \
                           "mx_" #name "_scaled_at");                                                                  \
    }                                                                                                                  \
    extern "C" int mx_##name##_grouped_at(const mx_##name##_call* c, const mx_param_runs* runs,                        \
                                          const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters,           \
                                          S(const int64_t* step_dev, ) float lr, const float* lr_dev, void* stream) {  \
        MX_CHECK(iter_dev S(&& step_dev), "mx_" #name "_grouped_at: null iteration" S(" or step") " counter");         \
        return __VA_ARGS__(g_tune, c, runs, gscale_dev, n_iters, iter_dev, S(0, step_dev, ) lr, lr_dev, stream,        \
                           "mx_" #name "_grouped_at");                                                                 \
    }
