// lion_mix_bf16.hip -- mixed-precision Lion fused into the mixing round: bfloat16 models and gradients,
// fp32 master weights, momentum in fp32 or in bfloat16 (local-only groups).  One launch per training
// iteration.
//
// lion_mix.hip's launch for models held in bfloat16, with sgd_mix_bf16.hip's load and store sides.  The
// fp32 master rows are what the optimizer updates and the round mixes, so nothing is lost to bf16
// rounding between rounds; the bf16 model row is the rounded image of the master, rewritten by every
// launch.  Per (segment, row) four arrays:
//     w  fp32 master      read and written in place
//     g  bf16 gradient    read; overwritten with zeros when zero_grads
//     m  momentum         read and written: fp32, or bf16 when the record's m_bf16 is set
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (lion_mix.hip's on the fp32 masters; every line one fp32 rounding):
//     g32 = f32(g)                                        exact widening, bits << 16
//     m32 = m, or f32(m) for a bf16 momentum              exact widening
//     decay = fmaf(-lr, wd, 1)                            once per launch
//     w1 = (wd != 0) ? fmul(w, decay) : w
//     dm = fsub(g32, m32)
//     c  = fmaf(omb1, dm, m32)
//     w' = c > 0 ? fsub(w1, lr) : c < 0 ? fadd(w1, lr) : c == 0 ? w1 : NaN
//     m' = fmaf(omb2, dm, m32);  a bf16 momentum stores bf16_rne(m'), rounded once at the store
//     w   = the round of sgd_mix.hip on the w' values: per output row the partners' columns in ascending
//           matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//           leaves alone, and every row of an all-zero round, keeps w' as it is
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// p is written for every row in every launch that runs, rows the round leaves alone included: their w
// changed by the Lion step.  A device counter outside the schedule, or a plan record with the peer-reads
// bit, makes the launch a complete no-op.  Nothing is written at or past a row's length in any array.
//
// Traffic per element, fp32 momentum: read w (4), g (2), m (4), write w (4), m (4), p (2) = 20 bytes (22
// when the gradients are zeroed); bf16 momentum: 16 (18).
//
// A lane holds 4 elements: 16-byte accesses on w (and an fp32 m), 8-byte accesses on g, p and a bf16 m.
// Alignment rule: the vector path is taken where w of the (segment, row) is 16-byte aligned, m is aligned
// to its own access (16 bytes fp32, 8 bytes bf16), g and p are 8-byte aligned and the 4 elements are in
// range; everything else goes element by element (4-byte / 2-byte accesses), zero-filled past the end.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is lion_update.h's
// LionRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<LionMixBf16<MB16>, ...>) and defines the family's entry points.
#include "lion_update.h"

namespace {
using namespace mx::fused;
// w as fp32, g and p as bf16, m as fp32 (MB16 = false) or bf16 (MB16 = true)
template <bool MB16>
struct LionMixBf16 : LionRows<Bf16Form, MB16> {};
}  // namespace

MX_FUSED_FAMILY(lion_mix_bf16, Tune, MX_NO_STEP, lion_round<LionMixBf16<false>, LionMixBf16<true>>)
