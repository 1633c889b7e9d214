// choco_quant.hip -- ChocoSGD gossip with the bucketed stochastic quantizer (QSGD's qsgd_s, rescaled to a
// contraction as the ChocoSGD paper does) at 4 or 8 bits per element.
//
// mx_choco_quant_compress = ChocoCommunicator.prepare_comm_buffer (communicator.py:175-196) with the dense
//                           quantized message of send = x - x_hat in place of compressors.get_top_k
// mx_choco_quant_apply    = ChocoCommunicator.averaging (communicator.py:200-230) on those messages
//
// B = 256 columns make a bucket; s = 2^(bits-1) - 1 levels; tau = 1 + min(B / s^2, sqrt(B) / s);
// c = f32(1 / (s tau)).  Per bucket b of a row, with d = x - x_hat (one fp32 subtraction; x itself without an
// x_hat; +0 at and past P):
//     N2     = sum f64(d) f64(d)                      exact products, fp64 sum
//     norm   = f32(sqrt_f64(N2))                      stored in the message
//     inv    = norm == 0 ? 0 : f32(s) / norm          one correctly rounded fp32 division
//     xi[c]  = f32(mix32(key + u32(c)) >> 8) 2^-24    24 random bits, exact, in [0, 1)
//     v      = fadd(fmul(|d[c]|, inv), xi[c])
//     level  = v >= 1 ? min(s, floor(v)) : 0          a NaN v gives 0; the clamp catches s + 0.99999994 -> s + 1
//     neg    = d[c] < 0                               false for +0, -0 and NaN
//     q[c]   = fmul(f32(level), fmul(norm, c)), the sign bit flipped where neg
// key = mix32(mix32(mix32(u32(seed)) ^ u32(round)) ^ u32(row_base + r)): a message is a pure function of
// (seed, round, the row's index in the whole group, the row's values).
// A message slot (mx_choco_quant_msg_bytes(P, bits) = 64 + 64 ceil(nb / 16) + 32 bits nb, nb = ceil(P / 256)):
// int64 P at 16, int32 bits at 24, int32 256 at 28, zeros elsewhere up to 64; fp32 norm[nb] zero-padded to a
// multiple of 64 bytes; the codes (neg << (bits - 1) | level) up to the end of the last bucket, zero at and
// past P -- 8 bits: column c is byte c; 4 bits: nibble c & 1 of byte c >> 1.  A 4096-column tile starts at a
// 64-byte boundary of both arrays.
//
// Compress, ONE streaming launch: no LDS, no barrier, no workspace, no atomics.  A work item is kItem columns
// of one row on a persistent grid; a wave covers one bucket per pass (four passes an item), a lane 4
// consecutive columns (one 16-byte load of x and of x_hat, all passes' loads issued first).  Per pass: the
// lane's four squares added in column order, a 64-lane butterfly (DPP inside a 16-lane row, two cross-row
// exchanges), norm / inv / unit wave-uniform, four hashes, the codes packed in registers -- 8 bits: one 32-bit
// store a lane, 256 contiguous bytes a wave; 4 bits: lane pairs combine by a DPP row shift and the even lane
// stores.  Lane 0 stores the norm.  The grid only decides WHICH workgroup computes an item; whole aligned
// items and the per-element path (tails, rows off a 16-byte boundary) give every lane the same columns in the
// same order, so a norm depends on the bucket's values alone.
//
// Apply, sign_apply's shape: one launch over (row, 4096-column tile); a wave's 64 quads of a pass are one
// bucket, so a message's norm is wave-uniform and a lane reads one 32-bit (16-bit) word of codes per quad.
// NaN and Inf need no special case: they make norm NaN or Inf, so every q of THAT bucket is NaN.
// The quantizer itself (Lv, mix32, wave_sum, quant_pass, upd) lives in choco_quant.h, shared with the one-launch
// round of choco_quant_round.hip.
#include <type_traits>

#include "choco_quant.h"
#include "choco_round.h"
#include "mx_common.h"
#include "row_walk.h"

namespace {
using namespace mx::choco::quant;   // choco_sign.h's geometry and accesses; Lv, mix32, quant_pass, upd
using mx::choco::round_rec;

constexpr int kBPI = kItem / kBucket;          // buckets (= norms) per work item / apply tile: 16
static_assert(kBPI * sizeof(float) == 64 && kBPI == kWV * kNP, "a tile's norms are 64 bytes, one bucket a pass");

struct QuantDims {
    int64_t ld, P, msg_ld, chunks;
    int64_t round, n_rounds;          // the round, or with round_dev the schedule's length
    uint32_t seed_mix;                // mix32(u32(seed))
    int nrows, row_base;
};

template <int BITS, bool NT>
__global__ __launch_bounds__(kTPB) void quant_compress(const float* __restrict__ x, const float* __restrict__ xh,
                                                       char* __restrict__ msgs,
                                                       const int64_t* __restrict__ round_dev, QuantDims a) {
    int64_t rnd = a.round;
    if (round_dev) {
        rnd = *round_dev;
        if (rnd < 0 || rnd >= a.n_rounds) return;                  // outside the schedule: nothing is written
    }
    const uint32_t kr = mix32(a.seed_mix ^ (uint32_t)rnd);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total = a.chunks * a.nrows;
    const int64_t nb = n_buckets(a.P);
    const int64_t coff = codes_off(a.P);
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int r = (int)(w / a.chunks);
        const int64_t j = w % a.chunks;
        const float* xr = x + (int64_t)r * a.ld;
        const float* hr = xh ? xh + (int64_t)r * a.ld : nullptr;
        char* m = msgs + (int64_t)r * a.msg_ld;
        const uint32_t key = mix32(kr ^ (uint32_t)(a.row_base + r));
        if (j == 0 && tid < kHeader / 4) {                           // the row's first item writes the header
            const uint32_t hv = tid == 4 ? (uint32_t)a.P : tid == 5 ? (uint32_t)((uint64_t)a.P >> 32)
                              : tid == 6 ? (uint32_t)BITS : tid == 7 ? (uint32_t)kBucket : 0u;
            ((GPtr<uint32_t>)m)[tid] = hv;
        }
        const int64_t c0 = j * kItem + (int64_t)wave * (kItem / kWV) + lane * 4;
        float d[kNP][4];
        if (al16(xr) && al16(hr) && (j + 1) * kItem <= a.P) {        // a whole item of aligned rows (block-uniform)
            F4 u[kNP], v[kNP];
#pragma unroll
            for (int q = 0; q < kNP; ++q) {
                u[q] = ld4<NT>(xr + c0 + q * kPass);
                v[q] = hr ? ld4<NT>(hr + c0 + q * kPass) : F4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int q = 0; q < kNP; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) d[q][t] = hr ? __fsub_rn(u[q][t], v[q][t]) : u[q][t];
        } else {
#pragma unroll
            for (int q = 0; q < kNP; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int64_t c = c0 + q * kPass + t;
                    d[q][t] = 0.0f;                                // past P: +0 to the norm, a zero code
                    if (c < a.P) d[q][t] = hr ? __fsub_rn(ld1(xr + c), ld1(hr + c)) : ld1(xr + c);
                }
        }
        const int64_t b0 = j * kBPI + wave * kNP;                    // the wave's first bucket
#pragma unroll
        for (int q = 0; q < kNP; ++q) {
            const int64_t col = c0 + q * kPass;
            float norm;
            uint32_t word = quant_pass<BITS>(d[q], key + (uint32_t)col, norm);
            // the norms of a tile's 16 buckets, the empty ones of the last tile (+0) included: the padding
            if (lane == 0) ((GPtr<float>)(m + kHeader))[b0 + q] = norm;
            if (b0 + q < nb) {                                       // wave-uniform; codes end with the last bucket
                GPtr<uint32_t> codes = (GPtr<uint32_t>)(m + coff);
                if constexpr (BITS == 8) {
                    codes[col >> 2] = word;
                } else {
                    word |= row_up<1>(word) << 16;                   // the odd lane's 4 nibbles above the even lane's
                    if ((lane & 1) == 0) codes[col >> 3] = word;
                }
            }
        }
    }
}

// The launch arguments of the apply kernel: the scalars as one record, the arrays as __restrict__ kernel
// parameters (choco.hip's ApplyDims explains why)
struct ApplyDims {
    int64_t ld, P, msg_ld, coff;
    int64_t n_iters, words;    // round_rec's arguments, with rec_in and iter_dev
    int n_local, M;
    float alpha, g;
};

// message `slot` applied to a lane's kQ quads of whole tile t
constexpr int kQ = kItem / 4 / kTPB;          // quads per lane; quad j kTPB + tid lies in bucket j kWV + wave
template <int BITS, bool OWN>
__device__ __forceinline__ void apply_quads(const char* __restrict__ msgs, const ApplyDims& a, int slot, int64_t t,
                                            float w, F4 (&sv)[kQ], F4 (&hv)[kQ]) {
    using Word = typename std::conditional<BITS == 8, uint32_t, uint16_t>::type;
    const char* m = msgs + (int64_t)slot * a.msg_ld;
    GPtr<const float> nrm = (GPtr<const float>)(m + kHeader) + t * kBPI;
    GPtr<const Word> cw = (GPtr<const Word>)(m + a.coff) + t * (kItem / 4);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float unit[kQ];
    uint32_t wd[kQ];
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
        wd[j] = cw[j * kTPB + tid];
        unit[j] = __fmul_rn(nrm[j * kWV + wave], Lv<BITS>::c);
    }
#pragma unroll
    for (int j = 0; j < kQ; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float se = sv[j][c], he = hv[j][c];                          // (a vector's element binds to no reference)
            upd<BITS, OWN>(se, he, w, unit[j], wd[j] >> (BITS * c));
            sv[j][c] = se;
            if constexpr (OWN) hv[j][c] = he;
        }
}

// the same for one element at column c of the row (partial tiles, rows off a 16-byte boundary)
template <int BITS, bool OWN>
__device__ __forceinline__ void apply_one(const char* __restrict__ msgs, const ApplyDims& a, int slot, int64_t c,
                                          float w, float& sv, float& hv) {
    const char* m = msgs + (int64_t)slot * a.msg_ld;
    const float unit = __fmul_rn(*((GPtr<const float>)(m + kHeader) + (c >> 8)), Lv<BITS>::c);
    GPtr<const uint8_t> cb = (GPtr<const uint8_t>)(m + a.coff);
    const uint32_t code = BITS == 8 ? cb[c] : (uint32_t)cb[c >> 1] >> (4 * (c & 1));
    upd<BITS, OWN>(sv, hv, w, unit, code);
}

// NT: non-temporal accesses (mx_choco_quant_set "apply_nt", -1 = auto: with several rows only)
template <int BITS, bool NT>
__global__ __launch_bounds__(kTPB) void quant_apply(float* __restrict__ x, float* __restrict__ xh,
                                                    float* __restrict__ s, const char* __restrict__ msgs,
                                                    const int32_t* __restrict__ rec_in,
                                                    const int64_t* __restrict__ iter_dev, ApplyDims a) {
    const int32_t* __restrict__ rec = round_rec(rec_in, iter_dev, a.n_iters, a.words);
    if (!rec) return;
    const int r = blockIdx.y;
    const int64_t t = blockIdx.x;
    const int64_t t0 = t * kItem;
    const int len = (int)(a.P - t0 < kItem ? a.P - t0 : kItem);
    float* xr = x + (int64_t)r * a.ld + t0;
    float* sr = s + (int64_t)r * a.ld + t0;
    float* hr = xh + (int64_t)r * a.ld + t0;
    const int32_t* deg = rec + mx::kPlanHeader;
    const int d = deg[r];                                            // active partners of the row
    const float sw = __int_as_float(deg[a.n_local + r]);             // the record's self weight
    const int32_t* src = deg + 2 * a.n_local + r * a.M;              // their message slots, ascending matching
    const int tid = threadIdx.x;
    if (len == kItem && al16(xr) && al16(sr) && al16(hr)) {
        F4 xv[kQ], sv[kQ], hv[kQ];
#pragma unroll
        for (int j = 0; j < kQ; ++j) {
            const int o = 4 * (j * kTPB + tid);
            xv[j] = ld4<NT>(xr + o);
            sv[j] = ld4<NT>(sr + o);
            hv[j] = ld4<NT>(hr + o);
        }
        for (int e = 0; e < d; ++e) apply_quads<BITS, false>(msgs, a, src[e], t, a.alpha, sv, hv);
        apply_quads<BITS, true>(msgs, a, r, t, sw, sv, hv);
#pragma unroll
        for (int j = 0; j < kQ; ++j) {
            const int o = 4 * (j * kTPB + tid);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                xv[j][c] = __builtin_fmaf(-a.g, hv[j][c], __builtin_fmaf(a.g, sv[j][c], xv[j][c]));
            st4<NT>(xv[j], xr + o);
            st4<NT>(sv[j], sr + o);
            st4<NT>(hv[j], hr + o);
        }
        return;
    }
    for (int i = tid; i < len; i += kTPB) {
        float sv = ld1(sr + i), hv = ld1(hr + i);
        for (int e = 0; e < d; ++e) apply_one<BITS, false>(msgs, a, src[e], t0 + i, a.alpha, sv, hv);
        apply_one<BITS, true>(msgs, a, r, t0 + i, sw, sv, hv);
        *(GPtr<float>)(xr + i) = __builtin_fmaf(-a.g, hv, __builtin_fmaf(a.g, sv, ld1(xr + i)));
        *(GPtr<float>)(sr + i) = sv;
        *(GPtr<float>)(hr + i) = hv;
    }
}

int g_apply_nt = -1;          // access hints of the apply pass: -1 auto (non-temporal with several rows only), 0, 1
int g_blocks_per_cu = 8;      // persistent grid of the compress pass: workgroups per CU (capped by the work items)
int g_grid = 0;               // > 0: its exact grid size (tests: few workgroups looping over many work items)

const mx::Knob kKnobs[] = {
    mx::knob_range("apply_nt", &g_apply_nt, -1, 1),
    mx::knob_range("blocks_per_cu", &g_blocks_per_cu, 1, 64),
    mx::knob_range("grid", &g_grid, 0, 65536),
    // the one-launch round's persistent grid (choco_quant_round.hip), as the two above
    mx::knob_range("round_blocks_per_cu", &mx::choco::g_quant_round_blocks_per_cu, 1, 64),
    mx::knob_range("round_grid", &mx::choco::g_quant_round_grid, 0, 65536),
};
constexpr int kNumKnobs = sizeof(kKnobs) / sizeof(kKnobs[0]);

template <typename K4, typename K8>
auto by_bits(int bits, K4 k4, K8 k8) { return bits == 4 ? k4 : k8; }

int quant_apply_launch(const char* who, float* x, float* xhat, float* s, int64_t ld, int64_t P, int bits,
                       const void* msgs, int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev, int64_t iter,
                       const int64_t* iter_dev, int n_local, int M, float alpha, float gamma, void* stream) {
    MX_CHECK(x && xhat && s && msgs && plan_dev, "%s: null pointer", who);
    MX_CHECK(bits == 4 || bits == 8, "%s: bits=%d (4 or 8)", who, bits);
    MX_CHECK(P >= 1 && ld >= P, "%s: P=%lld ld=%lld", who, (long long)P, (long long)ld);
    MX_CHECK(n_local >= 1 && n_local <= 65535 && n_slots >= n_local && n_slots <= 65535 && M >= 1,
             "%s: n_local=%d n_slots=%d M=%d", who, n_local, n_slots, M);
    MX_CHECK(msg_ld_bytes >= mx_choco_quant_msg_bytes(P, bits) && msg_ld_bytes % 8 == 0 && (uintptr_t)msgs % 8 == 0,
             "%s: msg_ld %lld", who, (long long)msg_ld_bytes);
    const int64_t nt = n_items(P);
    MX_CHECK(nt <= 0x7fffffff, "%s: P too large", who);
    const int64_t words = mx::plan_words(n_local, M);
    const int32_t* rec = iter_dev ? plan_dev : plan_dev + iter * words;   // with iter_dev: iter = n_iters
    const ApplyDims dims{ld, P, msg_ld_bytes, codes_off(P), iter, words, n_local, M, alpha, gamma};
    const bool nt_hint = g_apply_nt < 0 ? n_local > 1 : g_apply_nt > 0;
    const auto kern = nt_hint ? by_bits(bits, quant_apply<4, true>, quant_apply<8, true>)
                              : by_bits(bits, quant_apply<4, false>, quant_apply<8, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)nt, n_local), dim3(kTPB), 0, mx::as_stream(stream), x, xhat, s,
                       static_cast<const char*>(msgs), rec, iter_dev, dims);
    MX_LAUNCH_CHECK();
    return MX_OK;
}
}  // namespace

extern "C" int64_t mx_choco_quant_msg_bytes(int64_t P, int bits) {
    if (P < 1 || (bits != 4 && bits != 8)) {
        mx::set_error("mx_choco_quant_msg_bytes: P=%lld bits=%d", (long long)P, bits);
        return MX_ERR_INVALID;
    }
    return codes_off(P) + 32 * (int64_t)bits * n_buckets(P);
}

extern "C" int mx_choco_quant_set(const char* key, int value) {
    return mx::knob_set("mx_choco_quant_set", kKnobs, kNumKnobs, key, value);
}

extern "C" int mx_choco_quant_get(const char* key) {
    return mx::knob_get("mx_choco_quant_get", kKnobs, kNumKnobs, key);
}

extern "C" int mx_choco_quant_compress(const float* x, const float* x_hat, int64_t ld, int nrows, int64_t P, int bits,
                                       void* msgs, int64_t msg_ld_bytes, int64_t seed, int64_t round,
                                       const int64_t* round_dev, int64_t n_rounds, int row_base, void* stream) {
    MX_CHECK(x && msgs, "mx_choco_quant_compress: null pointer");
    MX_CHECK(bits == 4 || bits == 8, "mx_choco_quant_compress: bits=%d (4 or 8)", bits);
    MX_CHECK(P >= 1 && nrows >= 1 && nrows <= 65535 && (nrows == 1 || ld >= P) && row_base >= 0,
             "mx_choco_quant_compress: P=%lld nrows=%d ld=%lld row_base=%d", (long long)P, nrows, (long long)ld,
             row_base);
    MX_CHECK((uintptr_t)msgs % 8 == 0 &&
                 (nrows == 1 || (msg_ld_bytes >= mx_choco_quant_msg_bytes(P, bits) && msg_ld_bytes % 8 == 0)),
             "mx_choco_quant_compress: msg_ld %lld or an unaligned buffer", (long long)msg_ld_bytes);
    MX_CHECK(!round_dev || n_rounds >= 0, "mx_choco_quant_compress: bad round counter");
    const int64_t chunks = n_items(P);
    const int64_t total = chunks * nrows;
    const int64_t target = g_grid > 0 ? (int64_t)g_grid : (int64_t)mx::cu_count() * g_blocks_per_cu;
    const QuantDims dims{ld, P, msg_ld_bytes, chunks, round, n_rounds, mix32((uint32_t)seed), nrows, row_base};
    // the rows of several workers are far larger than the Infinity Cache: non-temporal loads; one row's apply
    // pass finds part of what this pass read still on die (the sign pass's rule)
    const auto kern = nrows > 1 ? by_bits(bits, quant_compress<4, true>, quant_compress<8, true>)
                                : by_bits(bits, quant_compress<4, false>, quant_compress<8, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)(total < target ? total : target)), dim3(kTPB), 0, mx::as_stream(stream),
                       x, x_hat, static_cast<char*>(msgs), round_dev, dims);
    MX_LAUNCH_CHECK();
    return MX_OK;
}

extern "C" int mx_choco_quant_apply(float* x, float* xhat, float* s, int64_t ld, int64_t P, int bits, const void* msgs,
                                    int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev, int64_t iter,
                                    int n_local, int M, float alpha, float gamma, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_apply: iter < 0");
    return quant_apply_launch("mx_choco_quant_apply", x, xhat, s, ld, P, bits, msgs, msg_ld_bytes, n_slots, plan_dev,
                              iter, nullptr, n_local, M, alpha, gamma, stream);
}

extern "C" int mx_choco_quant_apply_at(float* x, float* xhat, float* s, int64_t ld, int64_t P, int bits,
                                       const void* msgs, int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev,
                                       const int64_t* iter_dev, int64_t n_iters, int n_local, int M, float alpha,
                                       float gamma, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_apply_at: bad iteration counter");
    return quant_apply_launch("mx_choco_quant_apply_at", x, xhat, s, ld, P, bits, msgs, msg_ld_bytes, n_slots,
                              plan_dev, n_iters, iter_dev, n_local, M, alpha, gamma, stream);
}
