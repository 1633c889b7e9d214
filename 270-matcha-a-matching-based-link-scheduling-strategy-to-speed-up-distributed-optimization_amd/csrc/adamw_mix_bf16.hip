// adamw_mix_bf16.hip -- mixed-precision AdamW / Adam fused into the mixing round: bfloat16 models and
// gradients, fp32 master weights, exp_avg and exp_avg_sq (local-only groups).  One launch per training
// iteration.
//
// adamw_mix.hip's launch for models held in bfloat16, with sgd_mix_bf16.hip's load and store sides.  The
// fp32 master rows are what the optimizer updates and the round mixes, so nothing is lost to bf16
// rounding between rounds; the bf16 model row is the rounded image of the master, rewritten by every
// launch.  Per (segment, row) five arrays:
//     w  fp32 master      read and written in place
//     g  bf16 gradient    read; overwritten with zeros when zero_grads
//     m  fp32 exp_avg     read and written
//     v  fp32 exp_avg_sq  read and written
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (torch.optim.AdamW's / Adam's single-tensor update on the fp32 masters; every
// line one IEEE fp32 rounding: -ffp-contract=off, explicit fmas, correctly rounded sqrt and division,
// denormals kept):
//     g32 = f32(g)                                        exact widening, bits << 16
//     decay = fmaf(-lr, wd, 1)                            once per launch
//     w1 = (wd != 0 &&  decoupled) ? fmul(w, decay) : w
//     g1 = (wd != 0 && !decoupled) ? fmaf(wd, w, g32) : g32
//     m' = fmaf(omb1, fsub(g1, m), m)
//     v' = fmaf(omb2, fmul(g1, g1), fmul(beta2, v))
//     den = fadd(fdiv(fsqrt(v'), bc2s), eps)
//     ss  = fdiv(lr, bc1)                                 once per launch
//     w'  = fmaf(-ss, fdiv(m', den), w1)
//     w   = the round of sgd_mix.hip on the w' values: per output row the partners' columns in ascending
//           matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//           leaves alone, and every row of an all-zero round, keeps w' as it is
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// (bc1, bc2s) = (1 - beta1^t, sqrt(1 - beta2^t)) of optimizer step t come from adamw_mix.hip's host-built
// device table at entry min(t, n_bias) - 1; t is an argument or, for graph replay, a device counter.
// Nothing computes pow on the device.  The square root is __builtin_sqrtf and not __fsqrt_rn, the
// division __fdiv_rn: see the head of adamw_mix.hip.
//
// p is written for every row in every launch that runs, rows the round leaves alone included: their w
// changed by the optimizer step.  A device counter outside the schedule, a step counter below 1 and a
// plan record with the peer-reads bit each make the launch a complete no-op.  Nothing is written at or
// past a row's length in any array.
//
// Traffic per element: read w (4), g (2), m (4), v (4), write w (4), m (4), v (4), p (2) = 28 bytes (30
// when the gradients are zeroed) against 100 for the unfused op sequence.
//
// A lane holds 4 elements: 16-byte accesses on w, m and v, 8-byte accesses on g and p.  Alignment rule:
// the vector path is taken where w, m and v of the (segment, row) are 16-byte aligned, g and p are
// 8-byte aligned and the 4 elements are in range; everything else goes element by element (4-byte /
// 2-byte accesses), zero-filled past the end.
//
// In place: a tile's w' of every row is parked in LDS as fp32 (barrier) before any w row of it is stored,
// and different work items never share a column.  m and v are read and written by the same lane only, so
// they are stored when their chunk is staged; so are the zeros over g.  Because every row is read in
// every round, the first loads are issued before the plan record is looked at.  No receive slots:
// n_slots == n_local.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is adam_update.h's
// AdamRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<AdamwMixBf16, ...>) and defines the family's entry points.
#include "adam_update.h"

namespace {
using namespace mx::fused;
// w, m and v as fp32, g and p as bf16; wide accesses only where the (segment, row)'s w, m and v are
// 16-byte and g and p 8-byte aligned
struct AdamwMixBf16 : AdamRows<Bf16Form> {};
}  // namespace

MX_FUSED_FAMILY(adamw_mix_bf16, Tune, MX_WITH_STEP, adamw_round<AdamwMixBf16>)
