// adamw_mix.hip -- the AdamW / Adam update of every local worker fused into the mixing round (fp32
// rows, local-only groups): one launch per training iteration instead of n optimizer steps + one mix.
//
// Each row's x, g, m (exp_avg) and v (exp_avg_sq) elements are read once, torch.optim.AdamW's (decoupled)
// or torch.optim.Adam's (L2) single-tensor update is applied on the way into LDS, every operation one
// IEEE fp32 rounding (-ffp-contract=off, explicit fmas, correctly rounded sqrt and division)
//     decay = fmaf(-lr, wd, 1)                          once per launch
//     x1 = (wd != 0 &&  decoupled) ? fmul(x, decay) : x           p.mul_(1 - lr*wd)
//     g1 = (wd != 0 && !decoupled) ? fmaf(wd, x, g) : g           g.add(p, alpha=wd)
//     m' = fmaf(omb1, fsub(g1, m), m)                             exp_avg.lerp_(g, 1 - beta1)
//     v' = fmaf(omb2, fmul(g1, g1), fmul(beta2, v))               exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
//     den = fadd(fdiv(fsqrt(v'), bc2s), eps)
//     ss  = fdiv(lr, bc1)                               once per launch
//     x'  = fmaf(-ss, fdiv(m', den), x1)
// and the round of mix.hip's mix_kernel_rows then runs on the staged x' values exactly as in sgd_mix.hip:
// per output row the partners' columns in ascending matching order, the self term last, every step one
// __builtin_fmaf.  Rows the plan record does not read and write, and every row of a round whose flags
// are all zero, get x' stored as it is: an all-zero round is the optimizer step alone, not a no-op.
//
// (bc1, bc2s) = (1 - beta1^t, sqrt(1 - beta2^t)) of optimizer step t come from a host-built device table
// at entry min(t, n_bias) - 1 (the table ends where both are exactly 1.0f); t is an argument or, for
// graph replay, a device counter.  Nothing computes pow on the device.
//
// The square root is __builtin_sqrtf, which hipcc expands to v_sqrt_f32 on a scaled input plus the two-fma
// correction to the correctly rounded result (denormals kept: float_denorm_mode_32 = 3).  __fsqrt_rn is
// NOT used: in this ROCm's headers it is __ocml_native_sqrt_f32, the bare 1-ulp v_sqrt_f32.  The
// division is __fdiv_rn: v_div_scale / v_rcp / fma refinement / v_div_fmas / v_div_fixup.
//
// Traffic per element: read x, g, m, v, write x, m, v = 28 bytes (32 when the gradients are zeroed)
// against 88 for the torch op sequence followed by the mixing round.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  m and v are read and written by the same lane only, so
// they are stored when their chunk is staged; so are the zeros over g with zero_grads.  Because every
// row is read in every round, the first loads are issued before the plan record is looked at.
//
// No receive slots: n_slots == n_local, the plan's n_remote is 0; a record with the peer-reads bit, a
// round counter outside the schedule and a step counter below 1 each make the launch write nothing.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is adam_update.h's
// AdamRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<AdamwMix, ...>) and defines the family's entry points.
#include "adam_update.h"

namespace {
using namespace mx::fused;
// x, g, m and v as fp32; 16-byte accesses only where x, g, m and v of the (segment, row) are all 16-byte
// aligned
struct AdamwMix : AdamRows<Fp32Form> {};
}  // namespace

MX_FUSED_FAMILY(adamw_mix, Tune, MX_WITH_STEP, adamw_round<AdamwMix>)
