// choco_quant_round.hip -- a whole ChocoSGD round of the bucketed stochastic quantizer (choco_quant.hip) in ONE
// launch, for 1-16 worker rows that all live on this GPU, optionally with torch.optim.SGD's step on the way in.
//
// A quantized value depends on its own 256-column bucket alone (the norm is per bucket, the random number a
// hash of (seed, round, row, column)), so a workgroup that holds one column tile of ALL rows can quantize every
// row's part of the tile and apply the round from on-chip codes: the messages never reach memory.  x, x_hat and
// s are read and written once each, 24 bytes per parameter (+ 1/64 for the optional norms), where
// mx_choco_quant_compress + mx_choco_quant_apply move 8 + bits/8 + 24 + (deg + 1) bits/8 and more.
//
// mx_choco_quant_round     = quant_compress + quant_apply on the same values: the SAME BITS in x, x_hat and s,
//                            and the same norms (the same lane columns, the same butterfly)
// mx_choco_quant_sgd_round = mx_choco_sgd_step, then that round, on x' from the registers (sgd_update.h)
//
// Work item: a tile of 16 (row, bucket) items, the same buckets of every row: with n_local rounded up to the
// row class rc = 1, 2, 4, 8, 16 a tile is 16 / rc buckets = 256 (16 / rc) columns of each row.  256 threads;
// item i = (row i / (16 / rc), bucket i % (16 / rc)); wave w owns items 4w .. 4w + 3, a lane 4 consecutive
// columns of each.  A persistent grid only decides WHO computes a tile.
// Phase 1 (per wave, its items): x and x_hat (and g, m) by 16-byte loads, all items' loads issued before the
//   first use; x' = sgd(x, g, m) with m' and the zeros over g stored at once; d = fsub(x', x_hat); quant_pass
//   gives the bucket's norm and the lane's four codes; the codes go to LDS one byte per column (a 32-bit word a
//   lane), unit = fmul(norm, c) too; lane 0 writes the norm to `norms` when given.  x' and x_hat stay in
//   registers.
// ONE barrier: the tile is quantized completely before any of its columns is written, and no other workgroup
//   touches those columns, so the round runs in place.  The LDS image alternates between two buffers, which
//   makes the barrier of the next tile the only other ordering a workgroup needs.
// Phase 2 (the same wave, the same items): s by a 16-byte load; the row's partners from the plan record in
//   ascending matching order, each one 32-bit LDS word of codes and one unit; then the own message (s += sw q,
//   x_hat += q); x = fmaf(-gamma, x_hat, fmaf(gamma, s, x')); three 16-byte stores.
// Items whose row is off a 16-byte boundary or whose bucket holds P take the same registers through
// per-element loads and stores (+0 at and past P); nothing is written at or past P.
// No atomics, no workspace, no finish launch.  The plan must be all-local: a record with receive slots
// (n_remote != 0) or the peer-reads bit lives in device memory, so it is the launch that refuses it -- it
// writes nothing.
// The kernel and its host side live in choco_quant_round.h, written over a storage form and a step policy
// (NoStep, SgdStep; choco_quant_adamw_round.h adds AdamStep), because choco_quant_round_bf16.hip runs the same
// round for bfloat16 models; this file instantiates it for fp32 gradients and no image, and defines the fp32
// entry points and the two knobs.
#include "choco_quant_round.h"

namespace mx {
namespace choco {
int g_quant_round_blocks_per_cu = 4;      // mx_choco_quant_set "round_blocks_per_cu"
int g_quant_round_grid = 0;               // "round_grid": > 0 is the exact grid (tests: few workgroups, many tiles)
}  // namespace choco
}  // namespace mx

namespace {
using namespace mx::choco::qround;
float* const kNoRows = nullptr;           // the round alone: no state rows
}  // namespace

extern "C" int mx_choco_quant_round(float* x, float* xhat, float* s, int64_t ld, int n_local, int64_t P, int bits,
                                    const int32_t* plan_dev, int64_t iter, int M, float alpha, float gamma,
                                    int64_t seed, int row_base, float* norms, int64_t norm_ld, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_round: iter < 0");
    return round_launch<Fp32Io, NoStep>("mx_choco_quant_round", x, nullptr, xhat, s, nullptr, ld, n_local, P, bits,
                                        plan_dev, iter, nullptr, M, alpha, gamma, seed, row_base, norms, norm_ld, {},
                                        stream, kNoRows);
}

extern "C" int mx_choco_quant_round_at(float* x, float* xhat, float* s, int64_t ld, int n_local, int64_t P, int bits,
                                       const int32_t* plan_dev, const int64_t* iter_dev, int64_t n_iters, int M,
                                       float alpha, float gamma, int64_t seed, int row_base, float* norms,
                                       int64_t norm_ld, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_round_at: bad iteration counter");
    return round_launch<Fp32Io, NoStep>("mx_choco_quant_round_at", x, nullptr, xhat, s, nullptr, ld, n_local, P, bits,
                                        plan_dev, n_iters, iter_dev, M, alpha, gamma, seed, row_base, norms, norm_ld,
                                        {}, stream, kNoRows);
}

extern "C" int mx_choco_quant_sgd_round(float* x, float* g, float* m, float* xhat, float* s, int64_t ld, int n_local,
                                        int64_t P, int bits, const int32_t* plan_dev, int64_t iter, int M,
                                        float alpha, float gamma, int64_t seed, int row_base, float* norms,
                                        int64_t norm_ld, float lr, const float* lr_dev, float weight_decay,
                                        float momentum, int nesterov, int zero_grads, void* stream) {
    MX_CHECK(iter >= 0, "mx_choco_quant_sgd_round: iter < 0");
    return round_launch<Fp32Io, Sgd>(
        "mx_choco_quant_sgd_round", x, g, xhat, s, nullptr, ld, n_local, P, bits, plan_dev, iter, nullptr, M, alpha,
        gamma, seed, row_base, norms, norm_ld, sgd_hyper(lr, lr_dev, weight_decay, momentum, nesterov, zero_grads),
        stream, m);
}

extern "C" int mx_choco_quant_sgd_round_at(float* x, float* g, float* m, float* xhat, float* s, int64_t ld,
                                           int n_local, int64_t P, int bits, const int32_t* plan_dev,
                                           const int64_t* iter_dev, int64_t n_iters, int M, float alpha, float gamma,
                                           int64_t seed, int row_base, float* norms, int64_t norm_ld, float lr,
                                           const float* lr_dev, float weight_decay, float momentum, int nesterov,
                                           int zero_grads, void* stream) {
    MX_CHECK(iter_dev && n_iters >= 0, "mx_choco_quant_sgd_round_at: bad iteration counter");
    return round_launch<Fp32Io, Sgd>(
        "mx_choco_quant_sgd_round_at", x, g, xhat, s, nullptr, ld, n_local, P, bits, plan_dev, n_iters, iter_dev, M,
        alpha, gamma, seed, row_base, norms, norm_ld,
        sgd_hyper(lr, lr_dev, weight_decay, momentum, nesterov, zero_grads), stream, m);
}
