// choco_randk.hip -- ChocoSGD gossip with random sparsification (rand-k) in top-k's place.
//
// mx_choco_randk_compress = ChocoCommunicator.prepare_comm_buffer (communicator.py:175-196) with k columns of
//                           send = x - x_hat drawn at random in place of compressors.get_top_k's k largest
//
// The message has top-k's layout (mx_choco_msg_bytes: vals f32[kpad] | idx int64[k] | bnd int32[T + 1],
// index-sorted, T = ceil(P / 4096)), so mx_choco_apply, the exchange and the graph-replayable rounds consume it
// as they are.  WHICH columns travel depends on (seed, round, worker, column) alone, never on the data:
//     rk     = mix32(mix32(mix32(u32(seed)) ^ u32(round)) ^ u32(row_base + r))      the quantizer's key chain
//     o      = (u64(mix32(rk ^ 0xA5A5A5A5)) P) >> 32                                the message's offset, in [0, P)
//     bnd[t] = floor((k min(4096 t, P) + o) / P),  t = 0 .. T                       bnd[0] = 0, bnd[T] = k
//     tile t sends k_t = bnd[t + 1] - bnd[t] of its len_t columns: those with the k_t smallest rank keys
//     v(j)   = (mix32(tk + j) & 0xFFFFF000) | j,  tk = mix32(rk ^ u32(t + 1)),  0 <= j < len_t
// v is unique within a tile; equal 20 random bits order by the column, as top-k's ties do.  The rotating offset o
// makes every column travel with probability exactly k / P, also where k < T.
//     vals[i] = fsub(x[idx[i]], x_hat[idx[i]]) (x itself without an x_hat); the pad element of an odd k is +0.
//
// ONE launch for all rows, no workspace, no atomics on memory, no barrier between workgroups, no error state: a
// 256-thread workgroup per (row, tile).  Thread tid holds the keys of columns 256 s + tid, s = 0 .. 15, in
// registers -- they cost hashes, no memory.  The k_t-th smallest key is found by a two-level radix select in
// LDS: a 1024-bin histogram of bits 31..22 (LDS atomics), a workgroup scan over the bins (4 bins a thread, a wave
// scan, 4 wave totals), then the same over bits 21..12 of the threshold bin's members; what remains are keys with
// equal random bits, taken in column order.  A set of flagged columns becomes ranks in column order from the
// ballot popcounts of every (step, wave) pair -- 64 of them, scanned by one wave -- plus mbcnt inside the wave:
// once for the ties, once for the selected columns, whose rank is their place in the message.  Only the
// selected columns of x and x_hat are loaded (all of a thread's loads before its stores).  k_t = 0 stores the
// bound alone; k_t = len_t sends the tile in order without a select, from 16-byte loads on whole aligned tiles.
#include "choco_quant.h"
#include "mx_common.h"

namespace {
using namespace mx::choco::quant;        // choco_sign.h's geometry and accesses; mix32

constexpr int kSteps = kItem / kTPB;     // columns a thread holds: column 256 s + tid
constexpr int kBins = 1024;              // 10 bits per radix level
constexpr int kBPT = kBins / kTPB;       // bins a thread scans
constexpr int kPairs = kSteps * kWV;     // (step, wave) pairs, in column order
constexpr uint32_t kOffsetSalt = 0xA5A5A5A5u;
static_assert(kPairs == 64 && kBPT == 4, "one wave scans the (step, wave) table; a thread reads its bins as one uint4");

struct RandkDims {
    int64_t ld, P, k, msg_ld;
    int64_t round, n_rounds;          // the round, or with round_dev the schedule's length
    uint32_t seed_mix;                // mix32(u32(seed))
    int row_base;
};

struct Lds {
    alignas(16) uint32_t hist[kBins];
    uint32_t tab[kPairs];             // per (step, wave): flagged columns before the pair
    uint32_t wsum[kWV];
    uint32_t bin, below, total;
};

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {          // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// The bin that holds the need-th smallest (1 <= need <= the histogram's total) and the count of the bins below
// it.  The histogram is complete on entry (the caller's barrier); every thread has read its bins before the
// first barrier here, so the caller may overwrite the histogram on return.
__device__ __forceinline__ void find_bin(Lds& L, uint32_t need, uint32_t& bin, uint32_t& below) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint4 h4 = *reinterpret_cast<const uint4*>(&L.hist[kBPT * tid]);
    const uint32_t h[kBPT] = {h4.x, h4.y, h4.z, h4.w};
    const uint32_t sum = h[0] + h[1] + h[2] + h[3];
    const uint32_t inc = wave_scan(sum, lane);
    if (lane == 63) L.wsum[wave] = inc;
    __syncthreads();
    uint32_t c = inc - sum;
    for (int w = 0; w < wave; ++w) c += L.wsum[w];
#pragma unroll
    for (int i = 0; i < kBPT; ++i) {
        if (c < need && need <= c + h[i]) {              // exactly one bin of one thread
            L.bin = (uint32_t)(kBPT * tid + i);
            L.below = c;
        }
        c += h[i];
    }
    __syncthreads();
    bin = L.bin;
    below = L.below;
}

// mask: bit s set where column 256 s + tid is flagged.  Leaves in L.tab the flagged columns before every
// (step, wave) pair, in column order, and returns their total.  The rank of a flagged column is then
// L.tab[s kWV + wave] + lanes_below(__ballot(its flag)).
__device__ __forceinline__ uint32_t rank_table(Lds& L, uint32_t mask) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t b = __ballot((mask >> s) & 1u);
        if (lane == 0) L.tab[s * kWV + wave] = (uint32_t)__builtin_popcountll(b);
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t v = L.tab[lane];
        const uint32_t inc = wave_scan(v, lane);
        L.tab[lane] = inc - v;
        if (lane == 63) L.total = inc;
    }
    __syncthreads();
    return L.total;
}

__device__ __forceinline__ uint32_t rank_of(const Lds& L, uint32_t mask, int s) {
    const int wave = threadIdx.x >> 6;
    return L.tab[s * kWV + wave] + lanes_below(__ballot((mask >> s) & 1u));
}

__global__ __launch_bounds__(kTPB) void randk_compress(const float* __restrict__ x, const float* __restrict__ xh,
                                                       char* __restrict__ msgs,
                                                       const int64_t* __restrict__ round_dev, RandkDims a) {
    __shared__ Lds L;
    int64_t rnd = a.round;
    if (round_dev) {
        rnd = *round_dev;
        if (rnd < 0 || rnd >= a.n_rounds) return;                  // outside the schedule: nothing is written
    }
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int64_t t = blockIdx.x;
    const int64_t T = n_items(a.P);
    const int64_t t0 = t * kItem;
    const int len = (int)(a.P - t0 < kItem ? a.P - t0 : kItem);
    const uint32_t rk = mix32(mix32(a.seed_mix ^ (uint32_t)rnd) ^ (uint32_t)(a.row_base + r));
    const uint64_t P = (uint64_t)a.P, k = (uint64_t)a.k;
    const uint64_t o = ((uint64_t)mix32(rk ^ kOffsetSalt) * P) >> 32;
    const int64_t b0 = (int64_t)((k * (uint64_t)t0 + o) / P);               // k P + o < 2^63: P < 2^31, k <= P
    const int64_t b1 = (int64_t)((k * (uint64_t)(t0 + len) + o) / P);
    const int kt = (int)(b1 - b0);

    const int64_t kpad = (a.k + 1) / 2 * 2;
    char* m = msgs + (int64_t)r * a.msg_ld;
    GPtr<float> vals = (GPtr<float>)m + b0;
    GPtr<int64_t> idx = (GPtr<int64_t>)(m + 4 * kpad) + b0;
    GPtr<int32_t> bnd = (GPtr<int32_t>)(m + 4 * kpad + 8 * a.k);
    if (tid == 0) {
        bnd[t] = (int32_t)b0;
        if (t == T - 1) {
            bnd[T] = (int32_t)b1;                                            // = k
            if (kpad != a.k) ((GPtr<float>)m)[a.k] = 0.0f;                   // the pad element of an odd k
        }
    }
    if (kt == 0) return;                                                     // block-uniform, as every branch below
    const float* xr = x + (int64_t)r * a.ld + t0;
    const float* hr = xh ? xh + (int64_t)r * a.ld + t0 : nullptr;

    if (kt == len) {                                                         // the whole tile, in order
        if (len == kItem && al16(xr) && al16(hr)) {
#pragma unroll
            for (int q = 0; q < kItem / 4 / kTPB; ++q) {
                const int c = 4 * (q * kTPB + tid);
                const F4 u = ld4<false>(xr + c);
                const F4 v = hr ? ld4<false>(hr + c) : F4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vals[c + e] = hr ? __fsub_rn(u[e], v[e]) : u[e];
                    idx[c + e] = t0 + c + e;
                }
            }
        } else {
            for (int c = tid; c < len; c += kTPB) {
                vals[c] = hr ? __fsub_rn(ld1(xr + c), ld1(hr + c)) : ld1(xr + c);
                idx[c] = t0 + c;
            }
        }
        return;
    }

    // 0 < kt < len: the kt smallest keys of the tile
    const uint32_t tk = mix32(rk ^ (uint32_t)(t + 1));
    uint32_t r20[kSteps];                                                    // a column's 20 random bits
    uint32_t valid = 0;                                                      // bit s: column 256 s + tid < len
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const int j = s * kTPB + tid;
        r20[s] = mix32(tk + (uint32_t)j) >> 12;
        valid |= (j < len ? 1u : 0u) << s;
    }
    *reinterpret_cast<uint4*>(&L.hist[kBPT * tid]) = make_uint4(0, 0, 0, 0);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSteps; ++s)
        if ((valid >> s) & 1u) atomicAdd(&L.hist[r20[s] >> 10], 1u);
    __syncthreads();
    uint32_t bin1, below1, bin2, below2;
    find_bin(L, (uint32_t)kt, bin1, below1);
    *reinterpret_cast<uint4*>(&L.hist[kBPT * tid]) = make_uint4(0, 0, 0, 0);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSteps; ++s)
        if (((valid >> s) & 1u) && (r20[s] >> 10) == bin1) atomicAdd(&L.hist[r20[s] & (kBins - 1)], 1u);
    __syncthreads();
    find_bin(L, (uint32_t)kt - below1, bin2, below2);
    const uint32_t thr = (bin1 << 10) | bin2;                                // the threshold's random bits
    const uint32_t ties = (uint32_t)kt - below1 - below2;                    // of its columns, the first `ties`

    uint32_t sel = 0, eq = 0;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        sel |= (r20[s] < thr ? 1u : 0u) << s;
        eq |= (r20[s] == thr ? 1u : 0u) << s;
    }
    sel &= valid;
    eq &= valid;
    rank_table(L, eq);
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint32_t rank = rank_of(L, eq, s);
        if (((eq >> s) & 1u) && rank < ties) sel |= 1u << s;
    }
    __syncthreads();                                                         // the table is written again
    rank_table(L, sel);                                                      // its total is kt

    float u[kSteps], v[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        u[s] = v[s] = 0.0f;
        if ((sel >> s) & 1u) {
            const int j = s * kTPB + tid;
            u[s] = ld1(xr + j);
            if (hr) v[s] = ld1(hr + j);
        }
    }
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint32_t rank = rank_of(L, sel, s);
        if (((sel >> s) & 1u) && rank < (uint32_t)kt) {                     // (always: the selection's total is kt)
            vals[rank] = hr ? __fsub_rn(u[s], v[s]) : u[s];
            idx[rank] = t0 + s * kTPB + tid;
        }
    }
}
}  // namespace

extern "C" int mx_choco_randk_compress(const float* x, const float* x_hat, int64_t ld, int nrows, int64_t P, int64_t k,
                                       void* msgs, int64_t msg_ld_bytes, int64_t seed, int64_t round,
                                       const int64_t* round_dev, int64_t n_rounds, int row_base, void* stream) {
    MX_CHECK(x && msgs, "mx_choco_randk_compress: null pointer");
    MX_CHECK(P >= 1 && P < (int64_t)1 << 31 && k >= 1 && k <= P && nrows >= 1 && nrows <= 65535 &&
                 (nrows == 1 || ld >= P) && row_base >= 0,
             "mx_choco_randk_compress: P=%lld (1 .. 2^31 - 1) k=%lld nrows=%d ld=%lld row_base=%d", (long long)P,
             (long long)k, nrows, (long long)ld, row_base);
    MX_CHECK((uintptr_t)msgs % 8 == 0 &&
                 (nrows == 1 || (msg_ld_bytes >= mx_choco_msg_bytes(P, k) && msg_ld_bytes % 8 == 0)),
             "mx_choco_randk_compress: msg_ld %lld or an unaligned buffer", (long long)msg_ld_bytes);
    MX_CHECK(!round_dev || n_rounds >= 0, "mx_choco_randk_compress: bad round counter");
    const RandkDims dims{ld, P, k, msg_ld_bytes, round, n_rounds, mix32((uint32_t)seed), row_base};
    hipLaunchKernelGGL(randk_compress, dim3((unsigned)n_items(P), nrows), dim3(kTPB), 0, mx::as_stream(stream), x,
                       x_hat, static_cast<char*>(msgs), round_dev, dims);
    MX_LAUNCH_CHECK();
    return MX_OK;
}
