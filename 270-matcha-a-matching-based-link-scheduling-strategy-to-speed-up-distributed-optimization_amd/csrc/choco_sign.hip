// choco_sign.hip -- ChocoSGD gossip with the scaled-sign (1-bit) compressor Q(v) = (|v|_1 / P) sign(v).
//
// mx_choco_sign_compress = ChocoCommunicator.prepare_comm_buffer (communicator.py:175-196) with the dense
//                          1-bit message of send = x - x_hat in place of compressors.get_top_k
// mx_choco_sign_apply    = ChocoCommunicator.averaging (communicator.py:200-230) on those messages
//
// Per row, with d = x - x_hat (one fp32 subtraction; x itself without an x_hat):
//     L      = sum_c f64(|d[c]|)                  fp64 sum of exact widenings
//     scale  = f32(L / f64(P))                    fp64 division, one rounding to fp32
//     bit c  = d[c] < 0                           false for +0, -0 and NaN: a zero difference travels as +scale
//     q[c]   = bit c ? -scale : +scale
// A message slot (mx_choco_sign_msg_bytes(P) = 64 + 8 ceil(P / 64) bytes): float32 scale at 0, float64 L at 8
// (diagnostic), int64 P at 16, zeros up to 64, then the bits -- column c is bit c & 7 of byte c >> 3, the
// padding bits past P zero.  The apply uses its own P and reads nothing of a header but `scale`; a message
// carries no index, so none can address out of range.
//
// Compress, two launches, no atomics (the shape of grad_norm.hip):
//   sign_compress   a work item is kItem columns of one row; its workgroup writes the item's packed bits and ONE
//                   fp64 partial of the sum to the item's own workspace slot work[r * chunks + j].  A lane holds 4
//                   consecutive columns per pass (one 16-byte load of x and of x_hat); the 8 lanes of 32
//                   columns combine their nibbles by DPP row shifts and the first of them stores the word.
//                   Per lane the |d| are added in column order, the passes in order, then a butterfly over
//                   the wave and the four waves in order.  The grid is persistent and only decides WHICH
//                   workgroup computes an item, never how; whole aligned items and the per-element path
//                   (tails, rows off a 16-byte boundary) give every lane the same columns in the same order.
//   sign_finish     one workgroup per row adds the row's partials in index order (a fixed tree) and writes the
//                   slot's header.
// So scale depends on the row's values and P alone.  Any fp64 order over P <= 2^26 non-negative terms is
// within P 2^-53 of the exact sum: scale is within 1 fp32 ulp of the correctly rounded value.
//
// Apply, one elementwise launch over (row, 4096-column tile): x, x_hat and s as 16-byte accesses, the plan
// record read as the top-k apply reads it, every needed message's scale (wave-uniform) and the tile's bits:
//     for each active partner j of row r, ascending matching:  s = fadd(s, fmul(f32(alpha), q_j))
//     s = fadd(s, fmul(self weight of the plan record, q_r));  x_hat = fadd(x_hat, q_r)
//     x = fmaf(g, s, x);  x = fmaf(-g, x_hat, x)
// No LDS, no barrier, no error path.  NaN and Inf need no special case: they make scale NaN or Inf, which
// the arithmetic above propagates.
#include "choco_round.h"
#include "mx_common.h"
#include "row_walk.h"

namespace {
using namespace mx::rows;        // GPtr, al16, F4
using mx::choco::round_rec;
constexpr int kTPB = 256;
constexpr int kWV = kTPB / 64;
constexpr int kItem = 4096;              // columns per work item = per workspace slot = per apply tile
constexpr int kPass = 64 * 4;            // columns a wave covers per pass
constexpr int kNP = kItem / kWV / kPass; // passes per wave: 4
constexpr int kHeader = 64;              // bytes of a slot before its bits
static_assert(kNP * kPass * kWV == kItem, "sign compress geometry");

__host__ __device__ inline int64_t n_items(int64_t P) { return (P + kItem - 1) / kItem; }
__host__ __device__ inline int64_t n_words(int64_t P) { return 2 * ((P + 63) / 64); }   // uint32 words of bits

template <bool NT>
__device__ __forceinline__ F4 ld4(const float* p) {
    if constexpr (NT) return __builtin_nontemporal_load((GPtr<const F4>)(p));
    else return *(GPtr<const F4>)(p);
}
template <bool NT>
__device__ __forceinline__ void st4(const F4& v, float* p) {
    if constexpr (NT) __builtin_nontemporal_store(v, (GPtr<F4>)(p));
    else *(GPtr<F4>)(p) = v;
}
__device__ __forceinline__ float ld1(const float* p) { return *(GPtr<const float>)(p); }

// the value of lane + N of the same 16-lane row (row_shl:N; zero past the row's end)
template <int N>
__device__ __forceinline__ uint32_t row_up(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + N, 0xf, 0xf, true);
}

// One pass of a lane: its 4 differences' magnitudes added in column order (returned), and the word of sign
// bits of the 32 columns that start at the lane's own (valid in lanes 0, 8, ... of the wave)
__device__ __forceinline__ double pass_of(const float (&d)[4], uint32_t& word) {
    double acc = 0.0;
    uint32_t v = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc += (double)__builtin_fabsf(d[t]);            // the widening is exact
        v |= (d[t] < 0.0f ? 1u : 0u) << t;               // false for +0, -0 and NaN
    }
    v |= row_up<1>(v) << 4;
    v |= row_up<2>(v) << 8;
    v |= row_up<4>(v) << 16;
    word = v;
    return acc;
}

template <bool NT>
__global__ __launch_bounds__(kTPB) void sign_compress(const float* __restrict__ x, const float* __restrict__ xh,
                                                      int64_t ld, int nrows, int64_t P, char* __restrict__ msgs,
                                                      int64_t msg_ld, int64_t chunks, double* __restrict__ work) {
    __shared__ double part[2][kWV];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total = chunks * nrows;
    const int64_t nw = n_words(P);
    int par = 0;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x, par ^= 1) {
        const int r = (int)(w / chunks);
        const int64_t j = w % chunks;
        const float* xr = x + (int64_t)r * ld;
        const float* hr = xh ? xh + (int64_t)r * ld : nullptr;
        GPtr<uint32_t> bits = (GPtr<uint32_t>)(msgs + (int64_t)r * msg_ld + kHeader);
        const int64_t c0 = j * kItem + (int64_t)wave * (kItem / kWV) + lane * 4;
        float d[kNP][4];
        if (al16(xr) && al16(hr) && (j + 1) * kItem <= P) {      // a whole item of aligned rows (block-uniform)
            F4 a[kNP], b[kNP];
#pragma unroll
            for (int q = 0; q < kNP; ++q) {
                a[q] = ld4<NT>(xr + c0 + q * kPass);
                b[q] = hr ? ld4<NT>(hr + c0 + q * kPass) : F4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int q = 0; q < kNP; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) d[q][t] = hr ? __fsub_rn(a[q][t], b[q][t]) : a[q][t];
        } else {
#pragma unroll
            for (int q = 0; q < kNP; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int64_t c = c0 + q * kPass + t;
                    d[q][t] = 0.0f;                                // past P: +0 to the sum, a zero bit
                    if (c < P) d[q][t] = hr ? __fsub_rn(ld1(xr + c), ld1(hr + c)) : ld1(xr + c);
                }
        }
        double acc[kNP];
#pragma unroll
        for (int q = 0; q < kNP; ++q) {
            uint32_t word;
            acc[q] = pass_of(d[q], word);
            const int64_t wi = (c0 + q * kPass) >> 5;              // lanes 0, 8, ...: c0 is a multiple of 32
            if ((lane & 7) == 0 && wi < nw) bits[wi] = word;       // the padding words up to 64 columns too
        }
        double s = acc[0];
#pragma unroll
        for (int q = 1; q < kNP; ++q) s += acc[q];                 // the passes, in column order
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);   // butterfly: every lane holds the wave's sum
        if (lane == 0) part[par][wave] = s;
        __syncthreads();                                           // one barrier per item: the slots alternate
        if (tid == 0) {
            double t = part[par][0];
#pragma unroll
            for (int v = 1; v < kWV; ++v) t += part[par][v];
            work[w] = t;                                           // slot r * chunks + j, whoever computed it
        }
    }
}

__global__ __launch_bounds__(kTPB) void sign_finish(const double* __restrict__ work, int64_t chunks, int64_t P,
                                                    char* __restrict__ msgs, int64_t msg_ld) {
    __shared__ double red[kTPB];
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const double* row = work + (int64_t)r * chunks;
    double a = 0.0;
#pragma unroll 8
    for (int64_t i = tid; i < chunks; i += kTPB) a += row[i];
    red[tid] = a;
    __syncthreads();
    for (int o = kTPB / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        char* h = msgs + (int64_t)r * msg_ld;
        const double L = red[0];
        *reinterpret_cast<float*>(h) = (float)(L / (double)P);     // IEEE fp64 division, then one rounding
        *reinterpret_cast<uint32_t*>(h + 4) = 0u;
        *reinterpret_cast<double*>(h + 8) = L;
        *reinterpret_cast<int64_t*>(h + 16) = P;
        for (int o = 24; o < kHeader; o += 8) *reinterpret_cast<uint64_t*>(h + o) = 0ull;
    }
}

// The launch arguments of the apply kernel: the scalars as one record, the arrays as __restrict__ kernel
// parameters (choco.hip's ApplyDims explains why)
struct SignDims {
    int64_t ld, P, msg_ld;
    int64_t n_iters, words;    // round_rec's arguments, with rec_in and iter_dev
    int n_local, M;
    float alpha, g;
};

// q = bit ? -scale : +scale
__device__ __forceinline__ float signed_scale(float scale, uint32_t bit) {
    return __uint_as_float(__float_as_uint(scale) ^ (bit << 31));
}

// one message applied to one element: s += w q, and for the row's own message x_hat += q
template <bool OWN>
__device__ __forceinline__ void upd(float& sv, float& hv, float w, float scale, uint32_t bit) {
    const float q = signed_scale(scale, bit);
    sv = __fadd_rn(sv, __fmul_rn(w, q));
    if constexpr (OWN) hv = __fadd_rn(hv, q);
}

// message `slot` applied to a lane's kQ quads of a whole tile (the tile's bits start at word w0)
constexpr int kQ = kItem / 4 / kTPB;          // quads per lane
template <bool OWN>
__device__ __forceinline__ void apply_quads(const char* __restrict__ msgs, int64_t msg_ld, int slot, int64_t w0,
                                            float w, F4 (&sv)[kQ], F4 (&hv)[kQ]) {
    const char* m = msgs + (int64_t)slot * msg_ld;
    const float scale = *(GPtr<const float>)(reinterpret_cast<const float*>(m));
    GPtr<const uint32_t> bw = (GPtr<const uint32_t>)(m + kHeader) + w0;
    const int tid = threadIdx.x;
    uint32_t wd[kQ];
#pragma unroll
    for (int j = 0; j < kQ; ++j) wd[j] = bw[(j * kTPB + tid) >> 3];      // quad q's nibble: word q / 8
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
        const uint32_t nib = wd[j] >> ((tid & 7) * 4);                    // ..., bits 4 (q % 8) on (kTPB % 8 == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float se = sv[j][c], he = hv[j][c];                          // (a vector's element binds to no reference)
            upd<OWN>(se, he, w, scale, (nib >> c) & 1u);
            sv[j][c] = se;
            if constexpr (OWN) hv[j][c] = he;
        }
    }
}

// the same for one element at column c of the row (partial tiles, rows off a 16-byte boundary)
template <bool OWN>
__device__ __forceinline__ void apply_one(const char* __restrict__ msgs, int64_t msg_ld, int slot, int64_t c, float w,
                                          float& sv, float& hv) {
    const char* m = msgs + (int64_t)slot * msg_ld;
    const float scale = *(GPtr<const float>)(reinterpret_cast<const float*>(m));
    const uint32_t byte = *((GPtr<const uint8_t>)(m + kHeader) + (c >> 3));
    upd<OWN>(sv, hv, w, scale, (byte >> (c & 7)) & 1u);
}

// NT: non-temporal accesses (mx_choco_sign_set "apply_nt", -1 = auto: with several rows only, as the top-k
// apply chooses)
template <bool NT>
__global__ __launch_bounds__(kTPB) void sign_apply(float* __restrict__ x, float* __restrict__ xh,
                                                   float* __restrict__ s, const char* __restrict__ msgs,
                                                   const int32_t* __restrict__ rec_in,
                                                   const int64_t* __restrict__ iter_dev, SignDims a) {
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
        const int64_t w0 = t * (kItem / 32);
        for (int e = 0; e < d; ++e) apply_quads<false>(msgs, a.msg_ld, src[e], w0, a.alpha, sv, hv);
        apply_quads<true>(msgs, a.msg_ld, r, w0, sw, sv, hv);
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
        for (int e = 0; e < d; ++e) apply_one<false>(msgs, a.msg_ld, src[e], t0 + i, a.alpha, sv, hv);
        apply_one<true>(msgs, a.msg_ld, r, t0 + i, sw, sv, hv);
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
};
constexpr int kNumKnobs = sizeof(kKnobs) / sizeof(kKnobs[0]);

int sign_apply_launch(float* x, float* xhat, float* s, int64_t ld, int64_t P, const void* msgs, int64_t msg_ld_bytes,
                      int n_slots, const int32_t* plan_dev, int64_t iter, const int64_t* iter_dev, int n_local, int M,
                      float alpha, float gamma, void* stream) {
    MX_CHECK(x && xhat && s && msgs && plan_dev, "mx_choco_sign_apply: null pointer");
    MX_CHECK(P >= 1 && ld >= P, "mx_choco_sign_apply: P=%lld ld=%lld", (long long)P, (long long)ld);
    MX_CHECK(n_local >= 1 && n_local <= 65535 && n_slots >= n_local && n_slots <= 65535 && M >= 1,
             "mx_choco_sign_apply: n_local=%d n_slots=%d M=%d", n_local, n_slots, M);
    MX_CHECK(msg_ld_bytes >= mx_choco_sign_msg_bytes(P) && msg_ld_bytes % 8 == 0 && (uintptr_t)msgs % 8 == 0,
             "mx_choco_sign_apply: msg_ld %lld", (long long)msg_ld_bytes);
    const int64_t nt = n_items(P);
    MX_CHECK(nt <= 0x7fffffff, "mx_choco_sign_apply: P too large");
    const int64_t words = mx::plan_words(n_local, M);
    const int32_t* rec = iter_dev ? plan_dev : plan_dev + iter * words;   // with iter_dev: iter = n_iters
    const SignDims dims{ld, P, msg_ld_bytes, iter, words, n_local, M, alpha, gamma};
    const bool nt_hint = g_apply_nt < 0 ? n_local > 1 : g_apply_nt > 0;
    const auto kern = nt_hint ? sign_apply<true> : sign_apply<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)nt, n_local), dim3(kTPB), 0, mx::as_stream(stream), x, xhat, s,
                       static_cast<const char*>(msgs), rec, iter_dev, dims);
    MX_LAUNCH_CHECK();
    return MX_OK;
}
}  // namespace

extern "C" int64_t mx_choco_sign_msg_bytes(int64_t P) {
    if (P < 1) {
        mx::set_error("mx_choco_sign_msg_bytes: P=%lld", (long long)P);
        return MX_ERR_INVALID;
    }
    return kHeader + 8 * ((P + 63) / 64);
}

extern "C" size_t mx_choco_sign_work_bytes(int64_t P, int nrows) {
    if (P < 1 || nrows < 1) {
        mx::set_error("mx_choco_sign_work_bytes: P=%lld nrows=%d", (long long)P, nrows);
        return 0;
    }
    return sizeof(double) * (size_t)n_items(P) * (size_t)nrows;
}

extern "C" int mx_choco_sign_set(const char* key, int value) {
    return mx::knob_set("mx_choco_sign_set", kKnobs, kNumKnobs, key, value);
}

extern "C" int mx_choco_sign_get(const char* key) { return mx::knob_get("mx_choco_sign_get", kKnobs, kNumKnobs, key); }

extern "C" int mx_choco_sign_compress(const float* x, const float* x_hat, int64_t ld, int nrows, int64_t P, void* msgs,
                                      int64_t msg_ld_bytes, void* work, void* stream) {
    MX_CHECK(x && msgs && work, "mx_choco_sign_compress: null pointer");
    MX_CHECK(P >= 1 && nrows >= 1 && nrows <= 65535 && (nrows == 1 || ld >= P),
             "mx_choco_sign_compress: P=%lld nrows=%d ld=%lld", (long long)P, nrows, (long long)ld);
    MX_CHECK((uintptr_t)msgs % 8 == 0 && (uintptr_t)work % 8 == 0 &&
                 (nrows == 1 || (msg_ld_bytes >= mx_choco_sign_msg_bytes(P) && msg_ld_bytes % 8 == 0)),
             "mx_choco_sign_compress: msg_ld %lld or an unaligned buffer", (long long)msg_ld_bytes);
    hipStream_t st = mx::as_stream(stream);
    const int64_t chunks = n_items(P);
    const int64_t total = chunks * nrows;
    const int64_t target = g_grid > 0 ? (int64_t)g_grid : (int64_t)mx::cu_count() * g_blocks_per_cu;
    const unsigned grid = (unsigned)(total < target ? total : target);
    // the rows of several workers are far larger than the Infinity Cache: non-temporal loads; one row's apply
    // pass finds part of what this pass read still on die (the top-k passes' rule)
    const auto kern = nrows > 1 ? sign_compress<true> : sign_compress<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTPB), 0, st, x, x_hat, ld, nrows, P, static_cast<char*>(msgs),
                       msg_ld_bytes, chunks, static_cast<double*>(work));
    MX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sign_finish, dim3((unsigned)nrows), dim3(kTPB), 0, st, static_cast<const double*>(work), chunks, P,
                       static_cast<char*>(msgs), msg_ld_bytes);
    MX_LAUNCH_CHECK();
    return MX_OK;
}

extern "C" int mx_choco_sign_apply(float* x, float* xhat, float* s, int64_t ld, int64_t P, const void* msgs,
                                   int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev, int64_t iter,
                                   int n_local, int M, float alpha, float gamma, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_sign_apply: iter < 0");
    return sign_apply_launch(x, xhat, s, ld, P, msgs, msg_ld_bytes, n_slots, plan_dev, iter, nullptr, n_local, M,
                             alpha, gamma, stream);
}

extern "C" int mx_choco_sign_apply_at(float* x, float* xhat, float* s, int64_t ld, int64_t P, const void* msgs,
                                      int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev,
                                      const int64_t* iter_dev, int64_t n_iters, int n_local, int M, float alpha,
                                      float gamma, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_sign_apply_at: bad iteration counter");
    return sign_apply_launch(x, xhat, s, ld, P, msgs, msg_ld_bytes, n_slots, plan_dev, n_iters, iter_dev, n_local, M,
                             alpha, gamma, stream);
}
