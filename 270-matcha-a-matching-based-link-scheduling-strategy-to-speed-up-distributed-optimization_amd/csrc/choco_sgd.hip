// choco_sgd.hip -- torch.optim.SGD's step fused into the ChocoSGD round, in front of the compressor.
//
// A ChocoSGD iteration is optimizer.step() + zero_grad() (train_mpi.py:131-142), then prepare_comm_buffer
// (communicator.py:175-196) on the updated parameters, then averaging.  The scaled-sign compress pass
// (choco_sign.hip) already streams x and x_hat once; here the update runs on x on the way into that pass:
//     x', m' = sgd(x, g, m)          sgd_update.h's sgd4 / sgd1: torch.optim.SGD, dampening 0
//     g      = +0                    under zero_grads
//     d      = fsub(x', x_hat)       from the registers; bits and the fp64 partial as sign_compress
// mx_choco_sign_sgd_compress = that launch + sign_finish: 28.125 bytes per parameter with momentum and
//                              zero_grads (x, g, m, x_hat in; x, m, g out; 1/8 for the bits) where the torch
//                              sequence and the compress pass move about 44 + 8.125
// mx_choco_sgd_step          = the same kernel with the compress half compiled out (no x_hat, no bits, no sum,
//                              no LDS, no barrier): top-k groups before their selection launches, and rounds
//                              with no active matching, where the local step still happens
//
// The work split is sign_compress's, exactly: a work item is 4096 columns of one row, 256 threads, each wave
// 4 passes of 256 columns, a lane 4 consecutive columns per pass, a persistent grid that only decides WHO
// computes an item.  The |d| are added in sign_compress's order (lane columns, passes, butterfly over the
// wave, four waves, one partial per item to work[r * chunks + j]), so the scale sign_finish writes is the SAME
// BITS mx_choco_sign_compress writes when run on x'.
// The loads of kFly passes (x, g, m, x_hat: 4 kFly 16-byte values per lane) are issued before the first of them
// is used; the updated values are stored as soon as they exist and only the differences live to the tail.
// With iter_dev the launch returns before touching anything when the counter is outside [0, n_iters):
// VirtualWorkerGroup.sgd_device_round's contract, no SGD step either.
#include "choco_sign.h"
#include "mx_common.h"
#include "sgd_update.h"

namespace {
using namespace mx::choco::sign;    // the geometry, ld4 / st4 / ld1, pass_of; GPtr, al16, F4
using mx::fused::SgdHyper;
using mx::fused::SgdState;
constexpr int kFly = 2;             // passes whose loads are in flight together (the register figures)
static_assert(kNP % kFly == 0, "passes in flight");

__device__ __forceinline__ void st1(float* p, float v) { *(GPtr<float>)(p) = v; }

// the scalars of a launch as one record, the arrays as __restrict__ kernel parameters (as SignDims)
struct StepDims {
    int64_t ld, P, msg_ld, chunks, n_iters;
    int nrows;
};

template <bool MOM, bool NT, bool COMPRESS>
__global__ __launch_bounds__(kTPB) void sgd_compress(float* __restrict__ x, float* __restrict__ g,
                                                     float* __restrict__ m, const float* __restrict__ xh,
                                                     char* __restrict__ msgs, double* __restrict__ work,
                                                     const int64_t* __restrict__ iter_dev, StepDims a, SgdHyper h) {
    if (iter_dev) {                                      // a counter outside the schedule: no step, nothing written
        const int64_t v = *iter_dev;
        if (v < 0 || v >= a.n_iters) return;
    }
    SgdState st;
    mx::fused::sgd_setup(st, h);                         // -lr, from lr_dev when given
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t total = a.chunks * a.nrows;
    const F4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    int par = 0;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x, par ^= 1) {
        const int r = (int)(w / a.chunks);
        const int64_t j = w % a.chunks;
        float* xr = x + (int64_t)r * a.ld;
        float* gr = g + (int64_t)r * a.ld;
        float* mr = MOM ? m + (int64_t)r * a.ld : nullptr;
        const float* hr = COMPRESS ? xh + (int64_t)r * a.ld : nullptr;
        const int64_t c0 = j * kItem + (int64_t)wave * (kItem / kWV) + lane * 4;
        float d[kNP][4];                                 // x' - x_hat; dead without COMPRESS
        // a whole item of aligned rows (block-uniform; al16(nullptr) holds)
        if (al16(xr) && al16(gr) && al16(mr) && al16(hr) && (j + 1) * kItem <= a.P) {
#pragma unroll
            for (int q0 = 0; q0 < kNP; q0 += kFly) {
                F4 xv[kFly], gv[kFly], mv[kFly], hv[kFly];
#pragma unroll
                for (int u = 0; u < kFly; ++u) {
                    const int64_t c = c0 + (q0 + u) * kPass;
                    xv[u] = ld4<NT>(xr + c);
                    gv[u] = ld4<NT>(gr + c);
                    mv[u] = MOM ? ld4<NT>(mr + c) : zero;
                    hv[u] = COMPRESS ? ld4<NT>(hr + c) : zero;
                }
#pragma unroll
                for (int u = 0; u < kFly; ++u) {
                    const int64_t c = c0 + (q0 + u) * kPass;
                    const F4 xn = mx::fused::sgd4<MOM>(xv[u], gv[u], mv[u], st.nlr, h);
                    st4<NT>(xn, xr + c);
                    if constexpr (MOM) st4<NT>(mv[u], mr + c);
                    if (h.zero_grads) st4<NT>(zero, gr + c);
                    if constexpr (COMPRESS) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) d[q0 + u][t] = __fsub_rn(xn[t], hv[u][t]);
                    }
                }
            }
        } else {                                         // tails, rows off a 16-byte boundary: the same columns per lane
#pragma unroll
            for (int q = 0; q < kNP; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int64_t c = c0 + q * kPass + t;
                    d[q][t] = 0.0f;                      // past P: +0 to the sum, a zero bit
                    if (c < a.P) {
                        float me = MOM ? ld1(mr + c) : 0.0f;
                        const float xn = mx::fused::sgd1<MOM>(ld1(xr + c), ld1(gr + c), me, st.nlr, h.wd, h);
                        st1(xr + c, xn);
                        if constexpr (MOM) st1(mr + c, me);
                        if (h.zero_grads) st1(gr + c, 0.0f);
                        if constexpr (COMPRESS) d[q][t] = __fsub_rn(xn, ld1(hr + c));
                    }
                }
        }
        if constexpr (COMPRESS) {                        // sign_compress's tail, in its order
            __shared__ double part[2][kWV];
            GPtr<uint32_t> bits = (GPtr<uint32_t>)(msgs + (int64_t)r * a.msg_ld + kHeader);
            const int64_t nw = n_words(a.P);
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
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);   // butterfly over the wave
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
}

// what both entry points check alike, then the launch; COMPRESS with xh / msgs / work
template <bool COMPRESS>
int step_launch(const char* who, float* x, float* g, float* m, const float* xh, int64_t ld, int nrows, int64_t P,
                void* msgs, int64_t msg_ld_bytes, void* work, float lr, const float* lr_dev, float wd, float mom,
                int nesterov, int zero_grads, const int64_t* iter_dev, int64_t n_iters, void* stream) {
    MX_CHECK(x && g && (!COMPRESS || (xh && msgs && work)), "%s: null pointer", who);
    MX_CHECK((mom != 0.0f) == (m != nullptr), "%s: the momentum rows are given exactly when momentum != 0", who);
    MX_CHECK(mom != 0.0f || !nesterov, "%s: nesterov needs momentum", who);
    MX_CHECK(P >= 1 && nrows >= 1 && nrows <= 65535 && (nrows == 1 || ld >= P), "%s: P=%lld nrows=%d ld=%lld", who,
             (long long)P, nrows, (long long)ld);
    MX_CHECK(!iter_dev || n_iters >= 0, "%s: bad iteration counter", who);
    if constexpr (COMPRESS)
        MX_CHECK((uintptr_t)msgs % 8 == 0 && (uintptr_t)work % 8 == 0 &&
                     (nrows == 1 || (msg_ld_bytes >= mx_choco_sign_msg_bytes(P) && msg_ld_bytes % 8 == 0)),
                 "%s: msg_ld %lld or an unaligned buffer", who, (long long)msg_ld_bytes);
    hipStream_t st = mx::as_stream(stream);
    const int64_t chunks = n_items(P);
    const StepDims dims{ld, P, msg_ld_bytes, chunks, n_iters, nrows};
    const SgdHyper h{lr, wd, mom, lr_dev, nullptr, nesterov != 0, zero_grads != 0};
    // the compress pass's own rule: several workers' rows are far larger than the Infinity Cache
    const bool nt = nrows > 1;
    const auto kern = mom != 0.0f ? (nt ? sgd_compress<true, true, COMPRESS> : sgd_compress<true, false, COMPRESS>)
                                  : (nt ? sgd_compress<false, true, COMPRESS> : sgd_compress<false, false, COMPRESS>);
    hipLaunchKernelGGL(kern, dim3(mx::choco::sign_grid(chunks * nrows)), dim3(kTPB), 0, st, x, g, m, xh,
                       static_cast<char*>(msgs), static_cast<double*>(work), iter_dev, dims, h);
    MX_LAUNCH_CHECK();
    if constexpr (COMPRESS)
        return mx::choco::sign_finish_launch(static_cast<const double*>(work), chunks, P, static_cast<char*>(msgs),
                                             msg_ld_bytes, nrows, st);
    return MX_OK;
}
}  // namespace

extern "C" int mx_choco_sign_sgd_compress(float* x, float* g, float* m, const float* x_hat, int64_t ld, int nrows,
                                          int64_t P, void* msgs, int64_t msg_ld_bytes, void* work, float lr,
                                          const float* lr_dev, float weight_decay, float momentum, int nesterov,
                                          int zero_grads, const int64_t* iter_dev, int64_t n_iters, void* stream) {
    return step_launch<true>("mx_choco_sign_sgd_compress", x, g, m, x_hat, ld, nrows, P, msgs, msg_ld_bytes, work, lr,
                             lr_dev, weight_decay, momentum, nesterov, zero_grads, iter_dev, n_iters, stream);
}

extern "C" int mx_choco_sgd_step(float* x, float* g, float* m, int64_t ld, int nrows, int64_t P, float lr,
                                 const float* lr_dev, float weight_decay, float momentum, int nesterov,
                                 int zero_grads, const int64_t* iter_dev, int64_t n_iters, void* stream) {
    return step_launch<false>("mx_choco_sgd_step", x, g, m, nullptr, ld, nrows, P, nullptr, 0, nullptr, lr, lr_dev,
                              weight_decay, momentum, nesterov, zero_grads, iter_dev, n_iters, stream);
}
