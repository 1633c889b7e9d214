// slowmo.hip -- the SlowMo outer step (Wang, Tantia, Ballas, Rabbat, ICLR 2020: "SlowMo: Improving
// Communication-Efficient Distributed SGD with Slow Momentum") for workers held as rows of one arena: the
// exact average of the n rows, the slow momentum on the averaged displacement and the broadcast of the new
// common point, in ONE streaming pass.  Per column, every line one fp32 rounding (-ffp-contract=off; the
// fmas are explicit):
//     s    = the sum of the n rows' values in mx_mean_rows' order (row_sum.h; order 0 the binomial tree,
//            1 rank order)
//     mean = fdiv(s, (float)n)                     the bits mx_mean_rows_to gives for the same rows and order
//     rl   = fdiv(1, lr);  al = fmul(alpha, lr)    once per launch
//     q    = fmul(fsub(a, mean), rl)
//     u'   = fmaf(beta, u, q)
//     a'   = fmaf(-al, u', a)
//     every row x_r = a';  a = a';  u = u'
//     mixed precision: the rows are the fp32 masters and every p_r = bf16_rne(a') (p is write only; NaN
//     stays NaN)
// a (the anchor: the common point of the last outer step) and u (the slow momentum) are fp32 [count], one
// pair per group.  lr is the argument or, with lr_dev, read when the kernel runs; a learning rate of exactly
// 0 read there makes the launch a complete no-op (rl would be Inf, as qgm_buf1's lr_r != 0 rule).
//
// Every lane reads its columns of all n rows, a and u before it writes anything in those columns, and no two
// lanes share a column: in place is safe, as in mean_tile_kernel.  Nothing is read or written at or past
// `count` in any array.
//
// Row classes.  Up to 8 rows: mean_tile_kernel's geometry -- one workgroup per 512-column tile, the rows'
// (and a's and u's) 2 KB pieces staged in LDS with 16-byte loads, each wave load 1 KB of one array, all of
// them issued before anything else; then both halves of the workgroup compute the column and share the
// stores (rows h, h + 2, ...; a by half 0, u by half 1).  Large rounds run at `wgpc` workgroups per CU
// (dynamic LDS cap), the mean kernel's measured best.  9..64 rows: one lane holds its columns of every
// row in registers, 16 bytes a lane up to 16 rows, 8 up to 32, 4 up to 64 (consensus.hip's widths).
// Wide accesses (16 bytes on rows, a and u, 8 on p in the widest class) where every pointer is aligned that
// far, ld % 4 == 0 and the chunk is in range; per element for the last count % 4 columns and for unaligned
// tables.  The bits do not depend on the class, the widths or a knob.
#include "fused_round.h"
#include "row_sum.h"

#include <cmath>

namespace {
using namespace mx::fused;       // F4, F2, B2, U2, GPtr, ld4, st4, st2, st8, st16, load_chunk, store_chunk, pack4

template <int W>
using FV = float __attribute__((ext_vector_type(W)));

// the launch's arguments: the call record's fields, the learning rate and whether the wide accesses are legal
struct Args {
    float* rows;
    float* a;
    float* u;
    uint16_t* p;
    int64_t ld, p_ld, count;
    const float* lr_dev;
    float lr, alpha, beta;
    int n, vec;
};

// one lane's W columns at column c of `row`: one wide access on the vector path when they are in range,
// else one access per element, zero-filled from `lim` on
template <int W>
__device__ __forceinline__ FV<W> load_cols(const float* row, int64_t c, int64_t lim, bool vec) {
    if constexpr (W == 4) {
        return load_chunk<true>(row, c, lim, vec);
    } else {
        if (vec && c + W <= lim) return __builtin_nontemporal_load((GPtr<const FV<W>>)(row + c));
        FV<W> v;
#pragma unroll
        for (int t = 0; t < W; ++t) v[t] = (c + t < lim) ? ld4(row + c + t) : 0.0f;
        return v;
    }
}
// only whole 16-byte stores take the policy SP; the narrower wide stores are non-temporal, element stores plain
template <int SP, int W>
__device__ __forceinline__ void store_cols(float* row, int64_t c, int64_t lim, bool vec, const FV<W>& v) {
    if constexpr (W == 4) {
        store_chunk<SP>(row, c, lim, vec, v);
    } else {
        if (vec && c + W <= lim) {
            __builtin_nontemporal_store(v, (GPtr<FV<W>>)(row + c));
            return;
        }
#pragma unroll
        for (int t = 0; t < W; ++t)
            if (c + t < lim) st4(row + c + t, v[t]);
    }
}
// the model row's image of the same columns: bf16, rounded once to nearest even
template <int SP, int W>
__device__ __forceinline__ void store_image(uint16_t* row, int64_t c, int64_t lim, bool vec, const FV<W>& v) {
    if constexpr (W == 4) {
        store_chunk<SP>(row, c, lim, vec, pack4(v));
    } else {
        const F2 f = {v[0], W == 2 ? v[W - 1] : 0.0f};
        const uint32_t b = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, B2));
        if (W == 2 && vec && c + 2 <= lim) {
            __builtin_nontemporal_store(b, (GPtr<uint32_t>)(row + c));
            return;
        }
        if (c < lim) st2(row + c, b & 0xFFFFu);
        if (W == 2 && c + 1 < lim) st2(row + c + 1, b >> 16);
    }
}

// the launch's learning rate, and what is derived from it once
struct Rates {
    float lr, rl, nal;       // lr; fdiv(1, lr); -fmul(alpha, lr)
};
__device__ __forceinline__ Rates rates_of(const Args& g) {
    Rates r;
    r.lr = g.lr_dev ? *g.lr_dev : g.lr;
    r.rl = __fdiv_rn(1.0f, r.lr);
    r.nal = -(g.alpha * r.lr);
    return r;
}

// the column arithmetic after the sum `s`: the new momentum and the new common point
template <int W>
__device__ __forceinline__ void outer_update(const FV<W>& s, float size, const FV<W>& a, const FV<W>& u, const Rates& r,
                                             float beta, FV<W>& u2, FV<W>& a2) {
    const FV<W> mean = s / size;                 // the mean kernels' expression: one IEEE division per element
#pragma unroll
    for (int t = 0; t < W; ++t) {
        const float moved = a[t] - mean[t];
        const float q = moved * r.rl;            // separately rounded (-ffp-contract=off)
        u2[t] = __builtin_fmaf(beta, u[t], q);
        a2[t] = __builtin_fmaf(r.nal, u2[t], a[t]);
    }
}

template <int TREE, int MAXR, int W>
__device__ __forceinline__ FV<W> sum_rows(FV<W> (&v)[MAXR], int n) {
    const auto add = [&](int i, int j) { v[i] = v[i] + v[j]; };
    if constexpr (TREE) mx::rowsum::tree_order<MAXR>(n, add);
    else mx::rowsum::rank_order<MAXR>(n, add);
    return v[0];
}

constexpr int kTileRows = 8;
constexpr int kC4 = 128;                         // 16-byte vectors of a tile per array: 512 columns
constexpr int kTileLds = (kTileRows + 2) * kC4 * (int)sizeof(F4);

// up to 8 rows: arrays 0..7 of the tile are the rows, 8 is a and 9 is u
template <int TREE, bool MIXED, int SP>
__global__ __launch_bounds__(256) void slowmo_tile(const Args g) {
    __shared__ F4 lds[(kTileRows + 2) * kC4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t c0 = (int64_t)blockIdx.x * (4 * kC4);
    const bool vec = g.vec != 0;
    F4 R[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int e = wave * 64 + 256 * j;                 // wave-uniform array e / kC4
        const int k = e / kC4;
        const float* src = k < kTileRows ? g.rows + (int64_t)k * g.ld : k == kTileRows ? g.a : g.u;
        R[j] = (k >= kTileRows || k < g.n) ? load_chunk<true>(src, c0 + 4 * (e % kC4 + lane), g.count, vec) : F4(0.0f);
    }
    const Rates rt = rates_of(g);
    if (rt.lr == 0.0f) return;                             // the whole grid, before any store
#pragma unroll
    for (int j = 0; j < 5; ++j) lds[wave * 64 + 256 * j + lane] = R[j];
    __syncthreads();
    const int c = tid % kC4, h = tid / kC4;
    F4 v[kTileRows];
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) v[r] = lds[r * kC4 + c];
    const F4 a = lds[kTileRows * kC4 + c], u = lds[(kTileRows + 1) * kC4 + c];
    const F4 s = sum_rows<TREE>(v, g.n);
    F4 u2, a2;
    outer_update<4>(s, (float)g.n, a, u, rt, g.beta, u2, a2);
    const int64_t col = c0 + 4 * c;
    for (int d = h; d < g.n; d += 2) {
        store_chunk<SP>(g.rows + (int64_t)d * g.ld, col, g.count, vec, a2);
        if constexpr (MIXED) store_image<SP, 4>(g.p + (int64_t)d * g.p_ld, col, g.count, vec, a2);
    }
    if (h == 0) store_chunk<SP>(g.a, col, g.count, vec, a2);
    else store_chunk<SP>(g.u, col, g.count, vec, u2);
}

// 9..64 rows: NR bounds n; a lane holds W columns of every row
template <int NR, int W, int TREE, bool MIXED, int SP>
__global__ __launch_bounds__(256) void slowmo_rows(const Args g) {
    const int64_t col = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (col >= g.count) return;
    const bool vec = g.vec != 0;
    FV<W> v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (r < g.n) v[r] = load_cols<W>(g.rows + (int64_t)r * g.ld, col, g.count, vec);
        else v[r] = FV<W>(0.0f);
    }
    const FV<W> a = load_cols<W>(g.a, col, g.count, vec), u = load_cols<W>(g.u, col, g.count, vec);
    const Rates rt = rates_of(g);
    if (rt.lr == 0.0f) return;
    const FV<W> s = sum_rows<TREE>(v, g.n);
    FV<W> u2, a2;
    outer_update<W>(s, (float)g.n, a, u, rt, g.beta, u2, a2);
    for (int d = 0; d < g.n; ++d) {
        store_cols<SP, W>(g.rows + (int64_t)d * g.ld, col, g.count, vec, a2);
        if constexpr (MIXED) store_image<SP, W>(g.p + (int64_t)d * g.p_ld, col, g.count, vec, a2);
    }
    store_cols<SP, W>(g.a, col, g.count, vec, a2);
    store_cols<SP, W>(g.u, col, g.count, vec, u2);
}

struct Tune {
    int store_policy = mx::kStoreNt;   // the 16-byte stores: nt, or sc1 nt (the mean kernel's policy on large rounds); unmeasured here
    int wgpc = 3;                      // the tile kernel's workgroups per CU on rounds moving > 64 MB of rows (0: no cap)
};
Tune g_tune;

const mx::Knob kKnobs[] = {mx::knob_one_of("store_policy", &g_tune.store_policy, mx::kStoreNt, mx::kStoreSc1Nt,
                                           mx::kStoreSc1Nt, mx::kStoreSc1Nt),
                           mx::knob_range("wgpc", &g_tune.wgpc, 0, 16)};

// the row class of n rows: 0 the tile kernel, then 16 / 32 / 64 rows a lane
int class_of(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : 3; }

const char* const kNames[4][2][2] = {   // [class][rank order, tree][fp32, mixed]
    {{"slowmo_tile<0, false>", "slowmo_tile<0, true>"}, {"slowmo_tile<1, false>", "slowmo_tile<1, true>"}},
    {{"slowmo_rows<16, 4, 0, false>", "slowmo_rows<16, 4, 0, true>"},
     {"slowmo_rows<16, 4, 1, false>", "slowmo_rows<16, 4, 1, true>"}},
    {{"slowmo_rows<32, 2, 0, false>", "slowmo_rows<32, 2, 0, true>"},
     {"slowmo_rows<32, 2, 1, false>", "slowmo_rows<32, 2, 1, true>"}},
    {{"slowmo_rows<64, 1, 0, false>", "slowmo_rows<64, 1, 0, true>"},
     {"slowmo_rows<64, 1, 1, false>", "slowmo_rows<64, 1, 1, true>"}}};

// what every entry point refuses alike; `who` names it in the error text
int check_call(const char* who, const mx_slowmo_call* c) {
    MX_CHECK(c, "%s: null call record", who);
    MX_CHECK(c->rows && c->a && c->u, "%s: null rows, a or u", who);
    MX_CHECK(c->n_local >= 1 && c->n_local <= 64, "%s: n_local=%d outside [1, 64]", who, c->n_local);
    MX_CHECK(c->count >= 0 && c->ld >= c->count, "%s: ld=%lld < count=%lld (or count < 0)", who, (long long)c->ld,
             (long long)c->count);
    MX_CHECK(!c->p || c->p_ld >= c->count, "%s: p_ld=%lld < count=%lld", who, (long long)c->p_ld, (long long)c->count);
    MX_CHECK(c->order == 0 || c->order == 1, "%s: order %d (0 tree, 1 rank order)", who, c->order);
    MX_CHECK(std::isfinite(c->alpha) && c->alpha > 0.0f, "%s: alpha=%g is not finite and positive", who, (double)c->alpha);
    MX_CHECK(c->beta >= 0.0f && c->beta < 1.0f, "%s: beta=%g outside [0, 1)", who, (double)c->beta);
    struct Span {
        uintptr_t lo, hi;
    };
    const int64_t last = (int64_t)(c->n_local - 1);
    const Span rows = {(uintptr_t)c->rows, (uintptr_t)(c->rows + last * c->ld + c->count)};
    const Span a = {(uintptr_t)c->a, (uintptr_t)(c->a + c->count)}, u = {(uintptr_t)c->u, (uintptr_t)(c->u + c->count)};
    const uint16_t* p16 = static_cast<const uint16_t*>(c->p);
    const Span p = {(uintptr_t)p16, p16 ? (uintptr_t)(p16 + last * c->p_ld + c->count) : (uintptr_t)0};
    const auto meet = [](const Span& x, const Span& y) { return x.lo < y.hi && y.lo < x.hi; };
    MX_CHECK(!meet(a, rows) && !meet(u, rows) && !meet(a, p) && !meet(u, p) && !meet(a, u) && !meet(p, rows),
             "%s: a, u, p and the rows must not overlap", who);
    return MX_OK;
}

// 16-byte accesses on rows, a and u and the image's wide stores: every pointer aligned that far, whole vectors a row
bool vec_path(const mx_slowmo_call* c) {
    return (((uintptr_t)c->rows | (uintptr_t)c->a | (uintptr_t)c->u) & 15) == 0 && c->ld % 4 == 0 &&
           (!c->p || (((uintptr_t)c->p & 7) == 0 && c->p_ld % 4 == 0));
}

template <int TREE, bool MIXED, int SP>
void launch(int cls, const Args& g, size_t pad, hipStream_t st) {
    const auto grid = [&](int w) { return dim3((unsigned)((g.count + 256 * w - 1) / (256 * w))); };
    if (cls == 0)
        hipLaunchKernelGGL((slowmo_tile<TREE, MIXED, SP>), dim3((unsigned)((g.count + 4 * kC4 - 1) / (4 * kC4))), dim3(256),
                           pad, st, g);
    else if (cls == 1)
        hipLaunchKernelGGL((slowmo_rows<16, 4, TREE, MIXED, SP>), grid(4), dim3(256), 0, st, g);
    else if (cls == 2)
        hipLaunchKernelGGL((slowmo_rows<32, 2, TREE, MIXED, SP>), grid(2), dim3(256), 0, st, g);
    else
        hipLaunchKernelGGL((slowmo_rows<64, 1, TREE, MIXED, SP>), grid(1), dim3(256), 0, st, g);
}
template <int TREE, bool MIXED>
void launch(int cls, const Args& g, size_t pad, hipStream_t st) {
    if (g_tune.store_policy == mx::kStoreSc1Nt) launch<TREE, MIXED, mx::kStoreSc1Nt>(cls, g, pad, st);
    else launch<TREE, MIXED, mx::kStoreNt>(cls, g, pad, st);
}
}  // namespace

extern "C" int mx_slowmo_set(const char* key, int value) { return mx::knob_set("mx_slowmo_set", kKnobs, 2, key, value); }

extern "C" int mx_slowmo_get(const char* key) { return mx::knob_get("mx_slowmo_get", kKnobs, 2, key); }

extern "C" const char* mx_slowmo_kernel_name(const mx_slowmo_call* c) {
    if (check_call("mx_slowmo_kernel_name", c) != MX_OK) return "invalid";
    return kNames[class_of(c->n_local)][mx::rowsum::tree_of(c->order)][c->p ? 1 : 0];
}

extern "C" int mx_slowmo_step(const mx_slowmo_call* c, float lr, const float* lr_dev, void* stream) {
    const int rc = check_call("mx_slowmo_step", c);
    if (rc != MX_OK) return rc;
    MX_CHECK(lr_dev || (std::isfinite(lr) && lr > 0.0f), "mx_slowmo_step: lr=%g is not finite and positive", (double)lr);
    if (c->count == 0) return MX_OK;
    Args g;
    g.rows = c->rows;
    g.a = c->a;
    g.u = c->u;
    g.p = static_cast<uint16_t*>(c->p);
    g.ld = c->ld;
    g.p_ld = c->p_ld;
    g.count = c->count;
    g.lr_dev = lr_dev;
    g.lr = lr;
    g.alpha = c->alpha;
    g.beta = c->beta;
    g.n = c->n_local;
    g.vec = vec_path(c) ? 1 : 0;
    const int cls = class_of(c->n_local);
    size_t pad = cls == 0 && (int64_t)c->n_local * c->count * 4 > ((int64_t)64 << 20)
                     ? mx::lds_cap_pad(kTileLds, g_tune.wgpc) : 0;
    if (pad > (size_t)(64 * 1024 - kTileLds)) pad = 64 * 1024 - kTileLds;   // a workgroup's LDS limit (wgpc 1)
    hipStream_t st = mx::as_stream(stream);
    const bool tree = mx::rowsum::tree_of(c->order) != 0;
    if (tree) {
        if (g.p) launch<1, true>(cls, g, pad, st);
        else launch<1, false>(cls, g, pad, st);
    } else {
        if (g.p) launch<0, true>(cls, g, pad, st);
        else launch<0, false>(cls, g, pad, st);
    }
    MX_LAUNCH_CHECK();
    return MX_OK;
}
