// sgd_mix_bf16.hip -- mixed-precision SGD fused into the mixing round: bfloat16 models and gradients,
// fp32 master weights and momentum (local-only groups).  One launch per training iteration.
//
// sgd_mix.hip's launch for models held in bfloat16.  The optimizer state that has to keep small updates
// (lr * d is usually below half a bf16 ulp of the weight) is an fp32 master row; the master rows are what
// the round mixes, so nothing is lost to bf16 rounding between rounds, and the bf16 model row is the
// rounded image of the master, rewritten by every launch.  Per (segment, row) four arrays:
//     w  fp32 master      read and written in place
//     g  bf16 gradient    read; overwritten with zeros when zero_grads
//     m  fp32 momentum    read and written; absent when mom == 0
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (torch.optim.SGD, dampening 0, on the fp32 masters):
//     g32 = f32(g)                                        exact widening, bits << 16
//     d   = (wd != 0) ? fmaf(wd, w, g32) : g32
//     m   = fadd(fmul(mom, m), d)            [mom != 0]   two roundings (-ffp-contract=off)
//     d   = nesterov ? fmaf(mom, m, d) : m   [mom != 0]
//     w'  = fmaf(-lr, d, w)
//     w   = the round of sgd_mix.hip on the w' values: per output row the partners' columns in ascending
//           matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//           leaves alone, and every row of an all-zero round, keeps w' as it is
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// p is written for every row in every launch that runs, rows the round leaves alone included: their w
// changed by the SGD step.  A device counter outside the schedule, or a plan record with the peer-reads
// bit, makes the launch a complete no-op.  Nothing is written at or past a row's length in any array.
//
// Traffic per element: read w (4), g (2), m (4), write w (4), m (4), p (2) = 20 bytes (22 when the
// gradients are zeroed, 10 / 12 without momentum) against 64 for the unfused op sequence.
//
// A lane holds 4 elements: 16-byte accesses on w and m, 8-byte accesses on g and p.  Alignment rule: the
// vector path is taken where w and m of the (segment, row) are 16-byte aligned, g and p are 8-byte
// aligned and the 4 elements are in range; everything else goes element by element (4-byte / 2-byte
// accesses), zero-filled past the end.
//
// In place: a tile's w' of every row is parked in LDS as fp32 (barrier) before any w row of it is stored,
// and different work items never share a column.  m is read and written by the same lane only, so it is
// stored when its chunk is staged; so are the zeros over g.  Because every row is read in every round,
// the first loads are issued before the plan record is looked at.  No receive slots: n_slots == n_local.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is sgd_update.h's
// SgdRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<SgdMixBf16<MOM>, ...>) and defines the family's entry points.
#include "sgd_update.h"

namespace {
using namespace mx::fused;
// w and m as fp32, g and p as bf16; wide accesses only where the (segment, row)'s w and m are 16-byte and
// g and p 8-byte aligned
template <bool MOM>
struct SgdMixBf16 : SgdRows<Bf16Form, MOM> {};
}  // namespace

MX_FUSED_FAMILY(sgd_mix_bf16, Tune, MX_NO_STEP, sgd_round<SgdMixBf16>)
