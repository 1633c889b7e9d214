// choco_quant_round_bf16.hip -- the one-launch quantized ChocoSGD round (choco_quant_round.hip) for models held in
// bfloat16: bfloat16 gradients in, bfloat16 model rows out, everything the algorithm accumulates in fp32.  1-16
// local rows, bits 4 or 8, one launch per training iteration.
//
// A Choco update x += gamma (s - deg x_hat) is usually below half a bf16 ulp of the weight, as an SGD update is,
// so x (the master rows), x_hat, s and the momentum stay fp32; only what the models touch is bf16.  Per row:
//     x, x_hat, s  fp32   read and written in place
//     g            bf16   read; overwritten with bf16 zeros when zero_grads       (the sgd forms)
//     m            fp32   read and written; absent when momentum == 0             (the sgd forms)
//     p            bf16   the model row, WRITE ONLY: never read
// All arrays share the one leading dimension ld, counted in elements.
// Arithmetic contract:
//     g32     = f32(g)                       the exact widening, bits << 16
//     x', m'  = sgd_update.h on (x, g32, m)  exactly as mx_choco_quant_sgd_round computes them
//     the quantizer and the round on x', x_hat, s are choco_quant_round.hip's: the same lane columns, the same
//     butterfly, the same hash keys -- x, x_hat, s, m and the norms are THE SAME BITS mx_choco_quant_round /
//     mx_choco_quant_sgd_round give for gradients equal to the widened ones
//     p       = bf16_rne(x)                  ONE rounding, to nearest even, of the value stored to x
//                                            (v_cvt_pk_bf16_f32; NaN stays NaN, payload unspecified)
// p is written for every column below P of every local row in which x is written; nothing is written at or past
// P in any array.  A round with no active matching is, with the step, the step alone -- it still writes
// p = bf16_rne(x'), m' and the zeros over g -- and without the step writes nothing.  A counter outside the
// schedule, a plan record with receive slots or with the peer-reads bit: the launch writes nothing.
//
// Traffic per parameter: g 2 + 2, m 8, x 8, x_hat 8, s 8, p 2 = 38 bytes (30 without momentum, 26 without the
// step) where the fp32 launch moves 40 (32, 24) and an unfused wrapper around it (widen g, the fp32 launch, cast
// x to p, zero g) about 54.
//
// This kernel's own: a lane still owns 4 consecutive columns of an item, which is one 8-byte access on g and p
// and stays 16 bytes on the fp32 arrays.  The vector path of an item needs g and p 8-byte aligned on top of the
// fp32 arrays' 16; rows off those boundaries and the bucket that holds P take the per-element path (2-byte
// accesses on g and p) with the same registers.  g is held in flight as its 2 registers and widened at its
// first use, after all of the wave's loads (x, x_hat, g, m of its four items) are issued.  p is packed from the
// registers that hold the final x and stored next to the x store.  LDS use, the single barrier per tile, the
// double-buffered code image, the persistent grid and its knobs ("round_blocks_per_cu", "round_grid") are the
// fp32 kernel's: the kernel is choco_quant_round.h's quant_round over Bf16Io.
#include "choco_quant_round.h"

namespace {
using namespace mx::choco::qround;
float* const kNoRows = nullptr;           // the round alone: no state rows
}  // namespace

extern "C" int mx_choco_quant_round_bf16(float* x, float* xhat, float* s, uint16_t* p, int64_t ld, int n_local,
                                         int64_t P, int bits, const int32_t* plan_dev, int64_t iter, int M, float alpha,
                                         float gamma, int64_t seed, int row_base, float* norms, int64_t norm_ld,
                                         void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_round_bf16: iter < 0");
    return round_launch<Bf16Io, NoStep>("mx_choco_quant_round_bf16", x, nullptr, xhat, s, p, ld, n_local, P, bits,
                                        plan_dev, iter, nullptr, M, alpha, gamma, seed, row_base, norms, norm_ld, {},
                                        stream, kNoRows);
}

extern "C" int mx_choco_quant_round_bf16_at(float* x, float* xhat, float* s, uint16_t* p, int64_t ld, int n_local,
                                            int64_t P, int bits, const int32_t* plan_dev, const int64_t* iter_dev,
                                            int64_t n_iters, int M, float alpha, float gamma, int64_t seed,
                                            int row_base, float* norms, int64_t norm_ld, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_round_bf16_at: bad iteration counter");
    return round_launch<Bf16Io, NoStep>("mx_choco_quant_round_bf16_at", x, nullptr, xhat, s, p, ld, n_local, P, bits,
                                        plan_dev, n_iters, iter_dev, M, alpha, gamma, seed, row_base, norms, norm_ld,
                                        {}, stream, kNoRows);
}

extern "C" int mx_choco_quant_sgd_round_bf16(float* x, uint16_t* g, float* m, float* xhat, float* s, uint16_t* p,
                                             int64_t ld, int n_local, int64_t P, int bits, const int32_t* plan_dev,
                                             int64_t iter, int M, float alpha, float gamma, int64_t seed, int row_base,
                                             float* norms, int64_t norm_ld, float lr, const float* lr_dev,
                                             float weight_decay, float momentum, int nesterov, int zero_grads,
                                             void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_sgd_round_bf16: iter < 0");
    return round_launch<Bf16Io, Sgd>(
        "mx_choco_quant_sgd_round_bf16", x, g, xhat, s, p, ld, n_local, P, bits, plan_dev, iter, nullptr, M, alpha,
        gamma, seed, row_base, norms, norm_ld, sgd_hyper(lr, lr_dev, weight_decay, momentum, nesterov, zero_grads),
        stream, m);
}

extern "C" int mx_choco_quant_sgd_round_bf16_at(float* x, uint16_t* g, float* m, float* xhat, float* s, uint16_t* p,
                                                int64_t ld, int n_local, int64_t P, int bits, const int32_t* plan_dev,
                                                const int64_t* iter_dev, int64_t n_iters, int M, float alpha,
                                                float gamma, int64_t seed, int row_base, float* norms, int64_t norm_ld,
                                                float lr, const float* lr_dev, float weight_decay, float momentum,
                                                int nesterov, int zero_grads, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_sgd_round_bf16_at: bad iteration counter");
    return round_launch<Bf16Io, Sgd>(
        "mx_choco_quant_sgd_round_bf16_at", x, g, xhat, s, p, ld, n_local, P, bits, plan_dev, n_iters, iter_dev, M,
        alpha, gamma, seed, row_base, norms, norm_ld,
        sgd_hyper(lr, lr_dev, weight_decay, momentum, nesterov, zero_grads), stream, m);
}
