// choco_quant_adamw_round_bf16.hip -- the one-launch AdamW + quantized ChocoSGD round (choco_quant_adamw_round.hip)
// for models held in bfloat16: bfloat16 gradients in, bfloat16 model rows out, everything the optimizer and the
// algorithm accumulate in fp32.  Per row:
//     x, x_hat, s          fp32   read and written in place
//     exp_avg, exp_avg_sq  fp32   read and written in place
//     g                    bf16   read; overwritten with bf16 zeros when zero_grads
//     p                    bf16   the model row, WRITE ONLY: never read
// All arrays share the one leading dimension ld, counted in elements.
// Arithmetic contract:
//     g32         = f32(g)                          the exact widening, bits << 16
//     x', m', v'  = adam_update.h on (x, g32, m, v) exactly as mx_choco_quant_adamw_round computes them
//     the quantizer and the round are choco_quant_round.hip's -- x, x_hat, s, m, v and the norms are THE SAME BITS
//     mx_choco_quant_adamw_round gives for gradients equal to the widened ones
//     p           = bf16_rne(x)                     ONE rounding, to nearest even, of the value stored to x
// p is written wherever x is, the step-alone launch of a round with no active matching included; nothing is
// written at or past P in any array.  The no-op rules are the fp32 launch's.
//
// Traffic per parameter: g 2 + 2, m 8, v 8, x 8, x_hat 8, s 8, p 2 = 46 bytes where the fp32 launch moves 48.
//
// The kernel is choco_quant_round.h's quant_round over Bf16Io under AdamStep: a lane still owns 4 consecutive
// columns of an item, one 8-byte access on g and p and 16 bytes on the fp32 arrays; the vector path needs g and p
// 8-byte aligned on top of the fp32 arrays' 16, everything else goes element by element (2-byte accesses on g and
// p).  g streams as its 2 registers and is widened at its use; p is packed from the registers that hold the final x.
#include "choco_quant_adamw_round.h"

using namespace mx::choco::qround;

extern "C" int mx_choco_quant_adamw_round_bf16(float* x, uint16_t* g, float* m, float* v, float* xhat, float* s,
                                               uint16_t* p, int64_t ld, int n_local, int64_t P, int bits,
                                               const int32_t* plan_dev, int64_t iter, int M, float alpha,
                                               float gamma, int64_t seed, int row_base, float* norms,
                                               int64_t norm_ld, float lr, const float* lr_dev, float omb1,
                                               float beta2, float omb2, float eps, float weight_decay,
                                               int decoupled, int zero_grads, const float* bias_dev, int64_t n_bias,
                                               int64_t step, const int64_t* step_dev, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_adamw_round_bf16: iter < 0");
    return round_launch<Bf16Io, AdamStep>(
        "mx_choco_quant_adamw_round_bf16", x, g, xhat, s, p, ld, n_local, P, bits, plan_dev, iter, nullptr, M,
        alpha, gamma, seed, row_base, norms, norm_ld,
        adam_hyper(lr, lr_dev, omb1, beta2, omb2, eps, weight_decay, decoupled, zero_grads, bias_dev, n_bias, step,
                   step_dev),
        stream, m, v);
}

extern "C" int mx_choco_quant_adamw_round_bf16_at(float* x, uint16_t* g, float* m, float* v, float* xhat, float* s,
                                                  uint16_t* p, int64_t ld, int n_local, int64_t P, int bits,
                                                  const int32_t* plan_dev, const int64_t* iter_dev, int64_t n_iters,
                                                  int M, float alpha, float gamma, int64_t seed, int row_base,
                                                  float* norms, int64_t norm_ld, float lr, const float* lr_dev,
                                                  float omb1, float beta2, float omb2, float eps,
                                                  float weight_decay, int decoupled, int zero_grads,
                                                  const float* bias_dev, int64_t n_bias, int64_t step,
                                                  const int64_t* step_dev, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_adamw_round_bf16_at: bad iteration counter");
    return round_launch<Bf16Io, AdamStep>(
        "mx_choco_quant_adamw_round_bf16_at", x, g, xhat, s, p, ld, n_local, P, bits, plan_dev, n_iters, iter_dev, M,
        alpha, gamma, seed, row_base, norms, norm_ld,
        adam_hyper(lr, lr_dev, omb1, beta2, omb2, eps, weight_decay, decoupled, zero_grads, bias_dev, n_bias, step,
                   step_dev),
        stream, m, v);
}
