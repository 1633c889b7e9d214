// lion_mix.hip -- the Lion update of every local worker fused into the mixing round (fp32 rows,
// local-only groups): one launch per training iteration instead of n optimizer steps + one mix.
//
// Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") steps every weight by
// +-lr along the sign of an interpolation of gradient and momentum, with decoupled weight decay: one
// state array, no sqrt, no division, no bias correction and no step counter.  Each row's x, g and m
// elements are read once and the update is applied on the way into LDS, every line one fp32 rounding
// (-ffp-contract=off, explicit fmas):
//     decay = fmaf(-lr, wd, 1)                            once per launch
//     x1 = (wd != 0) ? fmul(x, decay) : x                 decoupled decay, as AdamW's
//     dm = fsub(g, m)
//     c  = fmaf(omb1, dm, m)                              (1 - beta1) g + beta1 m in lerp form
//     x' = c > 0 ? fsub(x1, lr) : c < 0 ? fadd(x1, lr) : c == 0 ? x1 : NaN
//     m' = fmaf(omb2, dm, m)                              (1 - beta2) g + beta2 m
// omb1 / omb2 are the fp32 roundings of the fp64 values 1 - beta.  A zero direction (either zero)
// leaves x1 bit for bit, -0.0 included; a NaN direction gives a NaN of any payload.  The round of
// sgd_mix.hip then runs on the staged x' values: per output row the partners' columns in ascending
// matching order, the self term last, every step one __builtin_fmaf.  Rows the plan record does not
// read and write (degree 0 outside idle mode 1), and every row of a round whose flags are all zero, get
// x' stored as it is: an all-zero round is the Lion step alone, not a no-op.
//
// Traffic per element: read x, g, m, write x, m = 20 bytes (24 when the gradients are zeroed): the
// bytes of SGD with momentum.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  m is read and written by the same lane only, so it is
// stored when its chunk is staged; so are the zeros over g with zero_grads.  No receive slots:
// n_slots == n_local; a device counter outside the schedule, or a record with the peer-reads bit, makes
// the launch write nothing.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is lion_update.h's
// LionRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<LionMix, ...>) and defines the family's entry points.
#include "lion_update.h"

namespace {
using namespace mx::fused;
// x, g and m as fp32; 16-byte accesses only where x, g and m of the (segment, row) are all 16-byte aligned
struct LionMix : LionRows<Fp32Form, false> {};
}  // namespace

MX_FUSED_FAMILY(lion_mix, Tune, MX_NO_STEP, lion_round<LionMix, LionMix>)
