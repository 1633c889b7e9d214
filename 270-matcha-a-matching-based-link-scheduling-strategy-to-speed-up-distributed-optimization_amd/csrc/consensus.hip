// consensus.hip -- how far apart the workers are: every worker's distance from the mean of the rows, the
// consensus distance and the norm of the mean, on the device, from ONE read of the rows:
//     s_c      = ((f64(x_0c) + f64(x_1c)) + f64(x_2c)) + ...            fp64 adds in ROW ORDER
//     m_c      = s_c / f64(n)                                           one IEEE fp64 division
//     d_rc     = f64(x_rc) - m_c                                        one fp64 subtraction
//     D_r      = sum_c d_rc^2          M = sum_c m_c^2                  fp64
//     dist[r]  = f32(sqrt(D_r))
//     stats[0] = f32(sqrt((D_0 + D_1 + ... in row order) / n))          the consensus distance
//     stats[1] = f32(sqrt(M))                                           the norm of the mean row
// bfloat16 rows are widened exactly first (bits << 16).  The arithmetic of a column is pinned -- row order,
// a true division (the multiplication by 1/n only where n is a power of two: the same bits), nothing
// reassociated -- because x - m cancels: near consensus another order of the mean moves d by far more than
// an fp64 rounding.  With m pinned every d_rc is the specification's bit for bit, and the sums over the
// columns of the non-negative d^2 and m^2 are within P * 2^-53 of exact in any order: every output is
// within 1 fp32 ulp of the specification for P <= 2^26.  Identical rows give exactly 0.0 (k * x is exact
// in fp64 for k <= 64, so m = x).
//
// Two launches, no atomics, no host step, modelled on grad_norm.hip:
//   consensus_partials   a work item is kCols columns of one segment across ALL n rows; its workgroup
//                        writes n + 1 fp64 partials to the item's own workspace slots, row r's sum of d^2
//                        to work[r * chunks + j] and the mean's sum of m^2 to work[n * chunks + j].  Each
//                        wave takes kCols / 4 columns in passes of 64 lanes x EPL columns; a lane keeps
//                        its columns of every row in registers between the sum and the deviations, so
//                        every element comes from HBM once; per lane one fma chain per row in column
//                        order, then a butterfly over the 64 lanes, then the four wave sums in wave
//                        order.  The grid is persistent and only decides WHICH workgroup computes an item,
//                        never how: the bits do not depend on it.
//   consensus_finish     one workgroup: wave v adds the partials of rows v, v + 16, ... (lane l its slots
//                        l, l + 64, ... in index order, then a butterfly), then dist[r] and the two stats,
//                        the D_r added in row order.
//
// Row classes (rows held per lane): n <= 8, <= 16, <= 32, <= 64.  A lane loads 16 bytes of a row at a time
// in the first two; the larger classes load kWords32 / kWords64 words a lane, and widen each word once per
// pass instead of keeping its fp64 value, so that the rows and the n fp64 accumulators still fit the
// register file without scratch (DESIGN 6h has the resource report and the timings behind the choice; the
// MX_CONSENSUS_* macros build the other variants).  Vector loads, non-temporal (the rows are read once and
// nothing reads them from this kernel's lines next: 10 % faster at 8 rows), where the row pointer is
// 16-byte aligned and the lane's elements are in range, per-element loads elsewhere; an element at or
// past seg_len is never loaded -- its place holds 0 in every row, which adds +0.0 to every sum.
#include "mx_common.h"
#include "row_walk.h"

#include <cmath>

#ifndef MX_CONSENSUS_WORDS32
#define MX_CONSENSUS_WORDS32 2
#endif
#ifndef MX_CONSENSUS_WORDS64
#define MX_CONSENSUS_WORDS64 1
#endif
#ifndef MX_CONSENSUS_NT
#define MX_CONSENSUS_NT 1
#endif
#ifndef MX_CONSENSUS_AGAIN
#define MX_CONSENSUS_AGAIN 32
#endif

namespace {
using namespace mx::rows;        // GPtr, al16, U4, ld2
constexpr int kTPB = 256;
constexpr int kWV = kTPB / 64;
constexpr int kCols = 4096;          // columns per work item = per workspace slot of a row (mx_consensus_cols)
constexpr int kMaxRows = 64;
constexpr int kFinTPB = 1024;        // the finishing workgroup: 16 waves, a row each at a time
constexpr int kWords32 = MX_CONSENSUS_WORDS32;   // 32-bit words a lane loads per row and pass, n in (16, 32]
constexpr int kWords64 = MX_CONSENSUS_WORDS64;   // ... n in (32, 64]
constexpr bool kStream = MX_CONSENSUS_NT != 0;   // non-temporal row loads
constexpr int kWidenAgainFrom = MX_CONSENSUS_AGAIN;   // row classes from this one on widen twice (elem<AGAIN>)

typedef uint32_t U2 __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ T gload(const void* p) {
    if constexpr (kStream)
        return __builtin_nontemporal_load((GPtr<const T>)p);
    else
        return *(GPtr<const T>)p;
}

// one lane's WD words (WD * 4 / ES elements) at column c of a row; 0 where the column is at or past lim
template <int ES, int WD>
__device__ __forceinline__ void lane_load(const void* row, int64_t c, int64_t lim, bool vec, uint32_t (&w)[WD]) {
    constexpr int EPL = WD * 4 / ES;
    const char* p = static_cast<const char*>(row) + c * ES;
    if (vec && c + EPL <= lim) {
        if constexpr (WD == 4) {
            const U4 v = gload<U4>(p);
#pragma unroll
            for (int t = 0; t < 4; ++t) w[t] = v[t];
        } else if constexpr (WD == 2) {
            const U2 v = gload<U2>(p);
            w[0] = v[0];
            w[1] = v[1];
        } else {
            w[0] = gload<uint32_t>(p);
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < WD; ++t) w[t] = 0u;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        if (c + e < lim) {
            if constexpr (ES == 4)
                w[e] = *(GPtr<const uint32_t>)(p + 4 * e);
            else
                w[e >> 1] |= ld2(reinterpret_cast<const uint16_t*>(p) + e) << (16 * (e & 1));
        }
    }
}

// element e of a lane's words, widened exactly: fp32 bits, or the bf16 in the low (even e) / high half.
// AGAIN: widen the word anew instead of keeping the fp64 value of the sum pass alive until the deviation
// pass (the empty asm hides the word from common-subexpression elimination; it emits nothing): two
// registers less per row and column held, one conversion more per element.
template <int ES, int WD, bool AGAIN = false>
__device__ __forceinline__ double elem(const uint32_t (&w)[WD], int e) {
    uint32_t u = w[ES == 4 ? e : e >> 1];
    if constexpr (AGAIN) asm volatile("" : "+v"(u));
    if constexpr (ES == 4) return (double)__builtin_bit_cast(float, u);
    return (double)__builtin_bit_cast(float, (e & 1) ? (u & 0xFFFF0000u) : (u << 16));
}

__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);      // butterfly: every lane holds the sum
    return a;
}

// ES = element size in bytes: 4 (fp32) or 2 (bfloat16 bit patterns); NR = rows of the class (n <= NR);
// WD = words a lane loads per row and pass; FULL: n == NR, known at compile time (no row guards)
template <int ES, int NR, int WD, bool FULL>
__global__ __launch_bounds__(kTPB) void consensus_partials(const void* const* __restrict__ x_ptrs,
                                                           const int64_t* __restrict__ seg_len, int nseg, int n_rows,
                                                           int64_t chunks, double* __restrict__ work) {
    constexpr int EPL = WD * 4 / ES;             // elements per lane per pass
    constexpr bool AGAIN = NR >= kWidenAgainFrom;
    const int n = FULL ? NR : n_rows;
    constexpr int WC = kCols / kWV;              // columns per wave
    constexpr int NP = WC / (64 * EPL);          // passes per wave
    static_assert(NP * 64 * EPL == WC && NP >= 1 && EPL >= 1, "consensus geometry");
    __shared__ double part[2][kWV][NR + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double dn = (double)n;
    const bool pow2 = (n & (n - 1)) == 0;
    const double inv = 1.0 / dn;                 // exact when n is a power of two: s * inv == s / dn bit for bit
    int par = 0;
    for (int64_t w = blockIdx.x; w < chunks; w += gridDim.x, par ^= 1) {
        // the item's segment: chunk w of the segments laid end to end (a chunk never spans two)
        int64_t j = w;
        int s = 0;
        int64_t lim = 0;
        for (; s < nseg; ++s) {
            lim = seg_len[s];
            const int64_t cnt = lim > 0 ? (lim + kCols - 1) / kCols : 0;
            if (j < cnt) break;
            j -= cnt;
        }
        double D[NR];
        double M = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) D[r] = 0.0;
        if (s < nseg) {                          // else: `chunks` larger than the lengths give -- an empty item
            const void* const* tab = x_ptrs + (int64_t)s * n;
            const int64_t c0 = j * kCols + (int64_t)wave * WC + (int64_t)lane * EPL;
#pragma unroll 1
            for (int q = 0; q < NP; ++q) {
                const int64_t c = c0 + (int64_t)q * 64 * EPL;
                uint32_t x[NR][WD];
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (r < n) {
                        const void* row = tab[r];
                        lane_load<ES, WD>(row, c, lim, al16(row), x[r]);
                    }
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    double sum = elem<ES, WD>(x[0], e);
#pragma unroll
                    for (int r = 1; r < NR; ++r)
                        if (r < n) sum += elem<ES, WD>(x[r], e);              // row order
                    const double m = pow2 ? sum * inv : sum / dn;
                    M = __builtin_fma(m, m, M);
#pragma unroll
                    for (int r = 0; r < NR; ++r)
                        if (r < n) {
                            const double d = elem<ES, WD, AGAIN>(x[r], e) - m;
                            D[r] = __builtin_fma(d, d, D[r]);
                        }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < n) {
                const double a = wave_sum(D[r]);
                if (lane == 0) part[par][wave][r] = a;
            }
        M = wave_sum(M);
        if (lane == 0) part[par][wave][NR] = M;
        __syncthreads();                         // one barrier per item: the slots alternate
        if (tid <= n) {
            const int k = tid < n ? tid : NR;
            double t = part[par][0][k];
#pragma unroll
            for (int v = 1; v < kWV; ++v) t += part[par][v][k];               // the waves, in wave order
            work[(int64_t)tid * chunks + w] = t;                             // slot r * chunks + w of the item
        }
    }
}

__global__ __launch_bounds__(kFinTPB) void consensus_finish(const double* __restrict__ work, int64_t chunks, int n,
                                                            float* __restrict__ dist, float* __restrict__ stats) {
    __shared__ double tot[kMaxRows + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int r = wave; r <= n; r += kFinTPB / 64) {
        const double* row = work + (int64_t)r * chunks;
        double a = 0.0;
#pragma unroll 16
        for (int64_t i = lane; i < chunks; i += 64) a += row[i];              // index order
        a = wave_sum(a);
        if (lane == 0) tot[r] = a;
    }
    __syncthreads();
    if (tid < n) dist[tid] = (float)__builtin_sqrt(tot[tid]);                // IEEE fp64 square root, one rounding
    if (tid == 0) {
        double a = tot[0];
        for (int r = 1; r < n; ++r) a += tot[r];                             // row order
        stats[0] = (float)__builtin_sqrt(a / (double)n);
        stats[1] = (float)__builtin_sqrt(tot[n]);
    }
}

struct Tune {
    int blocks_per_cu = 8;   // persistent grid of the partial pass: workgroups per CU (capped by the work items)
    int grid = 0;            // > 0: exact grid size (tests: few workgroups looping over many work items)
};
Tune g_tune;

template <int ES>
void launch_partials(const mx_consensus_call* c, int64_t grid, hipStream_t st) {
    const dim3 g((unsigned)grid), b(kTPB);
#define MX_CONS_LAUNCH(NR, WD)                                                                                  \
    do {                                                                                                        \
        if (c->n_local == NR)                                                                                   \
            hipLaunchKernelGGL((consensus_partials<ES, NR, WD, true>), g, b, 0, st, c->x_ptrs_dev,              \
                               c->seg_len_dev, c->nseg, c->n_local, c->chunks, c->work_dev);                    \
        else                                                                                                    \
            hipLaunchKernelGGL((consensus_partials<ES, NR, WD, false>), g, b, 0, st, c->x_ptrs_dev,             \
                               c->seg_len_dev, c->nseg, c->n_local, c->chunks, c->work_dev);                    \
    } while (0)
    if (c->n_local <= 8)
        MX_CONS_LAUNCH(8, 4);
    else if (c->n_local <= 16)
        MX_CONS_LAUNCH(16, 4);
    else if (c->n_local <= 32)
        MX_CONS_LAUNCH(32, kWords32);
    else
        MX_CONS_LAUNCH(64, kWords64);
#undef MX_CONS_LAUNCH
}
}  // namespace

extern "C" int mx_consensus_cols(void) { return kCols; }

extern "C" int64_t mx_consensus_layout(const int64_t* seg_len_host, int nseg, int n_local, int64_t* chunks_out) {
    if (!seg_len_host || nseg < 1 || n_local < 1 || n_local > kMaxRows) {
        mx::set_error("mx_consensus_layout: bad arguments (nseg=%d n_local=%d)", nseg, n_local);
        return MX_ERR_INVALID;
    }
    int64_t chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        if (seg_len_host[s] < 0) {
            mx::set_error("mx_consensus_layout: negative length");
            return MX_ERR_INVALID;
        }
        chunks += (seg_len_host[s] + kCols - 1) / kCols;
    }
    if (chunks_out) *chunks_out = chunks;
    return chunks * (n_local + 1) * (int64_t)sizeof(double);
}

const mx::Knob kKnobs[] = {mx::knob_range("blocks_per_cu", &g_tune.blocks_per_cu, 1, 64),
                           mx::knob_range("grid", &g_tune.grid, 0, 65536)};

extern "C" int mx_consensus_set(const char* key, int value) { return mx::knob_set("mx_consensus_set", kKnobs, 2, key, value); }

extern "C" int mx_consensus_get(const char* key) { return mx::knob_get("mx_consensus_get", kKnobs, 2, key); }

extern "C" int mx_consensus(const mx_consensus_call* c, void* stream) {
    MX_CHECK(c, "mx_consensus: null call record");
    MX_CHECK(c->x_ptrs_dev && c->seg_len_dev, "mx_consensus: null row table");
    MX_CHECK(c->dist_dev && c->stats_dev, "mx_consensus: null output");
    MX_CHECK(c->work_dev, "mx_consensus: null workspace");
    MX_CHECK(c->elem_size == 2 || c->elem_size == 4, "mx_consensus: elem_size=%d (4 = fp32, 2 = bfloat16)",
             c->elem_size);
    MX_CHECK(c->n_local >= 1 && c->n_local <= kMaxRows, "mx_consensus: n_local=%d outside [1, 64]", c->n_local);
    MX_CHECK(c->nseg >= 1 && c->chunks >= 0, "mx_consensus: nseg=%d chunks=%lld", c->nseg, (long long)c->chunks);
    hipStream_t st = mx::as_stream(stream);
    if (c->chunks > 0) {
        const int64_t target = g_tune.grid > 0 ? (int64_t)g_tune.grid : (int64_t)mx::cu_count() * g_tune.blocks_per_cu;
        const int64_t grid = c->chunks < target ? c->chunks : target;
        if (c->elem_size == 4)
            launch_partials<4>(c, grid, st);
        else
            launch_partials<2>(c, grid, st);
        MX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(consensus_finish, dim3(1), dim3(kFinTPB), 0, st, c->work_dev, c->chunks, c->n_local,
                       c->dist_dev, c->stats_dev);
    MX_LAUNCH_CHECK();
    return MX_OK;
}
