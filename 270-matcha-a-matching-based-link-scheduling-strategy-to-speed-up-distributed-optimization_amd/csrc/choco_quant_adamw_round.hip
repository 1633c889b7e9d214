// choco_quant_adamw_round.hip -- torch.optim.AdamW's (or Adam's) step of every worker, then a whole ChocoSGD round
// of the bucketed stochastic quantizer, in ONE launch: the one-launch round of choco_quant_round.hip with the
// update of adamw_mix.hip on the way into the quantizer.  1-16 worker rows on this GPU, bits 4 or 8.
//
// mx_choco_quant_adamw_round = adam_update.h's update of (x, g, m, v) at optimizer step t (m' and v' the bits of
//     mx_adamw_mix's, the bias corrections from the same [n_bias][2] table, lr / step from lr_dev / step_dev when
//     given), then mx_choco_quant_round on x' -- THE SAME BITS in x, x_hat, s and the norms (the same lane
//     columns, the same butterfly, the same hash keys).  decoupled = 0 is Adam with the decay as an L2 term.
//
// Traffic per parameter: x, x_hat, s, m and v read and written (40 bytes), g read and zeroed (8): 48, where the
// SGD-with-momentum iteration moves 40 and torch's AdamW in front of the round about 40 more than the round's 24.
//
// The design question is registers.  quant_round under SGD with momentum keeps x, x_hat, m and g of a wave's four
// items in flight at once (64 VGPRs of payload, 110-111 in all, 4 workgroups per CU); a fifth array would not fit
// under 128.  Here only x and x_hat of the four items are loaded up front -- they are what crosses the barrier,
// as x' and x_hat.  g, m and v STREAM: two register sets of (g, m, v) alternate over the items, item q + 1's
// three loads are issued before item q's update, and item q's set is dead once m', v' and the zeros over g are
// stored, which happens before its differences are quantized.  Payload in phase 1: 32 + 2 x 12 registers.  Phase
// 2 is the round's own (s of all four items, the partners' codes from LDS, three stores).
// The update's divisions and square root (correctly rounded, adam_update.h) sit between the loads and the
// quantizer's butterflies; nothing of them reaches memory but m' and v'.
//
// No-op rules: a counter outside the schedule, a record with receive slots or the peer-reads bit, an optimizer
// step below 1 -- the launch writes nothing.  A round of the schedule with no active matching is the step alone:
// x', m', v' and the zeros over g.  Rows off a 16-byte boundary (x, x_hat, s, g, m or v) and the bucket that
// holds P go element by element; nothing is written at or past P.  No atomics, no workspace, no second launch.
// The kernel and its host side are choco_quant_round.h's quant_round and round_launch under
// choco_quant_adamw_round.h's AdamStep; this file instantiates them for fp32 gradients and no image.
#include "choco_quant_adamw_round.h"

using namespace mx::choco::qround;

extern "C" int mx_choco_quant_adamw_round(float* x, float* g, float* m, float* v, float* xhat, float* s, int64_t ld,
                                          int n_local, int64_t P, int bits, const int32_t* plan_dev, int64_t iter,
                                          int M, float alpha, float gamma, int64_t seed, int row_base, float* norms,
                                          int64_t norm_ld, float lr, const float* lr_dev, float omb1, float beta2,
                                          float omb2, float eps, float weight_decay, int decoupled, int zero_grads,
                                          const float* bias_dev, int64_t n_bias, int64_t step,
                                          const int64_t* step_dev, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_adamw_round: iter < 0");
    return round_launch<Fp32Io, AdamStep>(
        "mx_choco_quant_adamw_round", x, g, xhat, s, nullptr, ld, n_local, P, bits, plan_dev, iter, nullptr, M,
        alpha, gamma, seed, row_base, norms, norm_ld,
        adam_hyper(lr, lr_dev, omb1, beta2, omb2, eps, weight_decay, decoupled, zero_grads, bias_dev, n_bias, step,
                   step_dev),
        stream, m, v);
}

extern "C" int mx_choco_quant_adamw_round_at(float* x, float* g, float* m, float* v, float* xhat, float* s,
                                             int64_t ld, int n_local, int64_t P, int bits, const int32_t* plan_dev,
                                             const int64_t* iter_dev, int64_t n_iters, int M, float alpha,
                                             float gamma, int64_t seed, int row_base, float* norms, int64_t norm_ld,
                                             float lr, const float* lr_dev, float omb1, float beta2, float omb2,
                                             float eps, float weight_decay, int decoupled, int zero_grads,
                                             const float* bias_dev, int64_t n_bias, int64_t step,
                                             const int64_t* step_dev, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_adamw_round_at: bad iteration counter");
    return round_launch<Fp32Io, AdamStep>(
        "mx_choco_quant_adamw_round_at", x, g, xhat, s, nullptr, ld, n_local, P, bits, plan_dev, n_iters, iter_dev, M,
        alpha, gamma, seed, row_base, norms, norm_ld,
        adam_hyper(lr, lr_dev, omb1, beta2, omb2, eps, weight_decay, decoupled, zero_grads, bias_dev, n_bias, step,
                   step_dev),
        stream, m, v);
}
