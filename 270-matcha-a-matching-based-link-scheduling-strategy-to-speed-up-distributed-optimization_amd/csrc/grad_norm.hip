// grad_norm.hip -- per-worker 2-norm of the gradient rows and the clip factor of
// torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) (error_if_nonfinite=False), on the device:
//     S_r      = sum over every segment of row r of f64(g)^2           fp64 squares, fp64 sum
//     norm[r]  = f32(sqrt(S_r))                                        fp64 square root, one rounding to fp32
//     c        = fmul(fdiv(1.0f, fadd(norm[r], 1e-6f)), max_norm)      torch's max_norm / (total_norm + 1e-6) on a
//                                                                      tensor: reciprocal() * max_norm
//     scale[r] = c > 1.0f ? 1.0f : c                                   a NaN stays a NaN
// The fused optimizer kernels multiply scale[r] into g on its way into the update (gscale_dev of the
// mx_*_mix_scaled entry points), so clipping costs this one extra read of g.
//
// Two launches, no atomics, no host step:
//   grad_norm_partials   a work item is kCols columns of one (segment, row); its workgroup writes ONE fp64
//                        partial to the item's own workspace slot work[r * chunks + j].  Each wave sums
//                        kCols / 4 columns (per lane: its elements in column order, one fma chain; then a
//                        butterfly over the 64 lanes), thread 0 adds the four wave sums in wave order.
//                        The grid is persistent and only decides WHICH workgroup computes an item, never
//                        how: the bits do not depend on it.
//   grad_norm_finish     one workgroup per row: thread t adds the row's partials t, t + 256, ... in index
//                        order, a fixed LDS tree adds the 256 sums, thread 0 writes norm and scale.
// So norm[r] depends on row r's values and lengths alone, and is the same on every launch.
//
// fp64 because the product of two fp32 values is exact in fp64 and, for P <= 2^26 elements, any
// summation order is within P * 2^-53 <= 2^-27 (relative) of the exact sum: the norm is within 1 fp32 ulp
// of the correctly rounded value whatever the tree.
//
// 16-byte loads where the (segment, row) pointer is 16-byte aligned and the lane's 4 (fp32) / 8 (bf16)
// elements are in range, per-element loads elsewhere; nothing at or past seg_len enters the sum.  Plain
// (temporal) loads: the fused launch reads the same gradient right afterwards.
#include "mx_common.h"
#include "row_walk.h"

#include <cmath>

namespace {
using namespace mx::rows;        // GPtr, al16, F4, U4
constexpr int kTPB = 256;
constexpr int kWV = kTPB / 64;
constexpr int kCols = 4096;          // columns per work item = per workspace slot (mx_grad_norm_cols)

__device__ __forceinline__ double sq(double acc, float x) {
    const double d = (double)x;
    return __builtin_fma(d, d, acc);             // the product is exact: one rounding, the sum's
}

// one lane's EPL elements at column c of a row, added to acc in column order
template <int ES>
__device__ __forceinline__ double lane_sum(const void* row, int64_t c, int64_t lim, bool vec, double acc);

template <>
__device__ __forceinline__ double lane_sum<4>(const void* row, int64_t c, int64_t lim, bool vec, double acc) {
    const float* p = static_cast<const float*>(row);
    if (vec && c + 4 <= lim) {
        const F4 v = *(GPtr<const F4>)(p + c);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = sq(acc, v[t]);
        return acc;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c + t < lim) acc = sq(acc, *(GPtr<const float>)(p + c + t));
    return acc;
}

template <>
__device__ __forceinline__ double lane_sum<2>(const void* row, int64_t c, int64_t lim, bool vec, double acc) {
    const uint16_t* p = static_cast<const uint16_t*>(row);
    if (vec && c + 8 <= lim) {
        const U4 v = *(GPtr<const U4>)(p + c);
#pragma unroll
        for (int t = 0; t < 4; ++t) {            // f32() of a bf16: the exact widening bits << 16
            acc = sq(acc, __builtin_bit_cast(float, v[t] << 16));
            acc = sq(acc, __builtin_bit_cast(float, v[t] & 0xFFFF0000u));
        }
        return acc;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (c + t < lim) acc = sq(acc, __builtin_bit_cast(float, (uint32_t)(*(GPtr<const uint16_t>)(p + c + t)) << 16));
    return acc;
}

// ES = element size in bytes: 4 (fp32) or 2 (bfloat16 bit patterns)
template <int ES>
__global__ __launch_bounds__(kTPB) void grad_norm_partials(const void* const* __restrict__ g_ptrs,
                                                           const int64_t* __restrict__ seg_len, int nseg,
                                                           int n_local, int64_t chunks, double* __restrict__ work) {
    constexpr int EPL = 16 / ES;                 // elements per lane per pass
    constexpr int WC = kCols / kWV;              // columns per wave
    constexpr int NP = WC / (64 * EPL);          // passes per wave: 4 (fp32) / 2 (bf16)
    static_assert(NP * 64 * EPL == WC && NP >= 2, "grad norm geometry");
    __shared__ double part[2][kWV];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total = chunks * n_local;
    int par = 0;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x, par ^= 1) {
        const int r = (int)(w / chunks);
        int64_t j = w % chunks;
        // the item's segment: chunk j of the row's segments laid end to end (a chunk never spans two)
        int s = 0;
        int64_t lim = 0;
        for (; s < nseg; ++s) {
            lim = seg_len[s];
            const int64_t cnt = lim > 0 ? (lim + kCols - 1) / kCols : 0;
            if (j < cnt) break;
            j -= cnt;
        }
        double acc[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) acc[q] = 0.0;
        if (s < nseg) {                          // else: `chunks` larger than the lengths give -- an empty item
            const void* row = g_ptrs[(int64_t)s * n_local + r];
            const bool vec = al16(row);
            const int64_t c0 = j * kCols + (int64_t)wave * WC + (int64_t)lane * EPL;
#pragma unroll
            for (int q = 0; q < NP; ++q) acc[q] = lane_sum<ES>(row, c0 + (int64_t)q * 64 * EPL, lim, vec, 0.0);
        }
        double a = acc[0];
#pragma unroll
        for (int q = 1; q < NP; ++q) a += acc[q];                    // the passes, in column order
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);  // butterfly: every lane holds the wave's sum
        if (lane == 0) part[par][wave] = a;
        __syncthreads();                         // one barrier per item: the slots alternate
        if (tid == 0) {
            double t = part[par][0];
#pragma unroll
            for (int v = 1; v < kWV; ++v) t += part[par][v];
            work[w] = t;                         // slot r * chunks + j of the item, whoever computed it
        }
    }
}

__global__ __launch_bounds__(kTPB) void grad_norm_finish(const double* __restrict__ work, int64_t chunks,
                                                         float max_norm, float* __restrict__ norm,
                                                         float* __restrict__ scale) {
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
        const float nr = (float)__builtin_sqrt(red[0]);              // IEEE fp64 square root, then one rounding
        const float rcp = __fdiv_rn(1.0f, nr + 1e-6f);               // Tensor.__rtruediv__: reciprocal() * max_norm
        const float c = rcp * max_norm;
        norm[r] = nr;
        scale[r] = c > 1.0f ? 1.0f : c;                              // NaN > 1 is false: a NaN stays a NaN
    }
}

struct Tune {
    int blocks_per_cu = 8;   // persistent grid of the partial pass: workgroups per CU (capped by the work items)
    int grid = 0;            // > 0: exact grid size (tests: few workgroups looping over many work items)
};
Tune g_tune;
}  // namespace

extern "C" int mx_grad_norm_cols(void) { return kCols; }

extern "C" int64_t mx_grad_norm_layout(const int64_t* seg_len_host, int nseg, int n_local, int64_t* chunks_out) {
    if (!seg_len_host || nseg < 1 || n_local < 1 || n_local > 64) {
        mx::set_error("mx_grad_norm_layout: bad arguments (nseg=%d n_local=%d)", nseg, n_local);
        return MX_ERR_INVALID;
    }
    int64_t chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        if (seg_len_host[s] < 0) {
            mx::set_error("mx_grad_norm_layout: negative length");
            return MX_ERR_INVALID;
        }
        chunks += (seg_len_host[s] + kCols - 1) / kCols;
    }
    if (chunks_out) *chunks_out = chunks;
    return chunks * n_local * (int64_t)sizeof(double);
}

const mx::Knob kKnobs[] = {mx::knob_range("blocks_per_cu", &g_tune.blocks_per_cu, 1, 64),
                           mx::knob_range("grid", &g_tune.grid, 0, 65536)};

extern "C" int mx_grad_norm_set(const char* key, int value) { return mx::knob_set("mx_grad_norm_set", kKnobs, 2, key, value); }

extern "C" int mx_grad_norm_get(const char* key) { return mx::knob_get("mx_grad_norm_get", kKnobs, 2, key); }

extern "C" int mx_grad_norm(const mx_grad_norm_call* c, void* stream) {
    MX_CHECK(c, "mx_grad_norm: null call record");
    MX_CHECK(c->g_ptrs_dev && c->seg_len_dev, "mx_grad_norm: null gradient table");
    MX_CHECK(c->norm_dev && c->scale_dev, "mx_grad_norm: null output");
    MX_CHECK(c->work_dev, "mx_grad_norm: null workspace");
    MX_CHECK(c->elem_size == 2 || c->elem_size == 4, "mx_grad_norm: elem_size=%d (4 = fp32, 2 = bfloat16)",
             c->elem_size);
    MX_CHECK(c->n_local >= 1 && c->n_local <= 64, "mx_grad_norm: n_local=%d outside [1, 64]", c->n_local);
    MX_CHECK(c->nseg >= 1 && c->chunks >= 0, "mx_grad_norm: nseg=%d chunks=%lld", c->nseg, (long long)c->chunks);
    MX_CHECK(c->max_norm > 0.0f && std::isfinite(c->max_norm), "mx_grad_norm: max_norm must be positive and finite");
    hipStream_t st = mx::as_stream(stream);
    const int64_t total = c->chunks * c->n_local;
    if (total > 0) {
        const int64_t target = g_tune.grid > 0 ? (int64_t)g_tune.grid : (int64_t)mx::cu_count() * g_tune.blocks_per_cu;
        const int64_t grid = total < target ? total : target;
        if (c->elem_size == 4)
            hipLaunchKernelGGL(grad_norm_partials<4>, dim3((unsigned)grid), dim3(kTPB), 0, st, c->g_ptrs_dev,
                               c->seg_len_dev, c->nseg, c->n_local, c->chunks, c->work_dev);
        else
            hipLaunchKernelGGL(grad_norm_partials<2>, dim3((unsigned)grid), dim3(kTPB), 0, st, c->g_ptrs_dev,
                               c->seg_len_dev, c->nseg, c->n_local, c->chunks, c->work_dev);
        MX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(grad_norm_finish, dim3((unsigned)c->n_local), dim3(kTPB), 0, st, c->work_dev, c->chunks,
                       c->max_norm, c->norm_dev, c->scale_dev);
    MX_LAUNCH_CHECK();
    return MX_OK;
}
