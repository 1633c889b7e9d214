// qgm_mix_bf16.hip -- mixed-precision quasi-global momentum fused into the mixing round: bfloat16 models
// and gradients, fp32 master weights and an fp32 momentum buffer (local-only groups).  One launch per
// training iteration.
//
// qgm_mix.hip's launch for models held in bfloat16, with sgd_mix_bf16.hip's arrays.  Per (segment, row):
//     w   fp32 master           read and written in place
//     g   bf16 gradient         read; overwritten with zeros when zero_grads
//     mh  fp32 buffer           the quasi-global momentum: read, and written after the round
//     p   bf16 model row        WRITE ONLY: never read
// Arithmetic contract: qgm_mix.hip's lines on w with g32 = f32(g) (exact widening, bits << 16), every line
// one fp32 rounding:
//     lr_r = fmul(lr, scale_r)
//     d    = (wd_r != 0) ? fmaf(wd_r, w, g32) : g32
//     m    = fadd(fmul(beta, mh), d)
//     s    = nesterov ? fmaf(beta, m, d) : m
//     w'   = fmaf(-lr_r, s, w)
//     y    = the round of sgd_mix.hip on the w' values; a row the plan record leaves alone, and every row
//            of an all-zero round, keeps y = w'
//     q    = fmul(fsub(w, y), fdiv(1.0f, lr_r))           w: the master BEFORE this launch
//     mh'  = (lr_r != 0) ? fmaf(omu, fsub(q, mh), mh) : mh
//     w    = y;   p = bf16_rne(y)                         ONE rounding, to nearest even, of the value
//                                                         stored to w; NaN stays NaN, payload unspecified
// p is written for every row in every launch that runs.  A device counter outside the schedule, or a plan
// record with the peer-reads bit, makes the launch a complete no-op, the buffer included.  Nothing is read
// or written at or past a row's length in any array.
//
// Traffic per element: read w (4), g (2), mh (4), write w (4), mh (4), p (2) = 20 bytes (22 when the
// gradients are zeroed): the bytes of mixed-precision SGD with momentum.  The finish side re-reads w and mh
// moments after the workgroup staged their lines; that re-read is NOT free (the step measures
// behind mixed-precision SGD with momentum, less so with w and mh staged with plain loads than with nt loads).
//
// A lane holds 4 elements: 16-byte accesses on w and mh, 8-byte accesses on g and p.  Alignment rule, on
// the staging and the finish side alike: the vector path is taken where w and mh of the (segment, row) are
// 16-byte aligned, g and p are 8-byte aligned and the 4 elements are in range; everything else goes element
// by element (4-byte / 2-byte accesses), zero-filled past the end.
//
// In place: as qgm_mix.hip.  The staging lane stores only the zeros over g; the lane that finishes a (row,
// chunk) reloads w and mh of its own 4 columns with plain loads, stores mh', then y and p.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is qgm_update.h's
// QgmRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<QgmMixBf16<NESTEROV, PLAIN>, ...>) and defines the family's entry points.
#include "qgm_update.h"

namespace {
using namespace mx::fused;
// w and mh as fp32, g and p as bf16; wide accesses only where the (segment, row)'s w and mh are 16-byte and
// g and p 8-byte aligned.  PLAIN: knob "stage_plain"
template <bool NESTEROV, bool PLAIN>
struct QgmMixBf16 : QgmRows<Bf16Form, NESTEROV, PLAIN> {};
}  // namespace

MX_FUSED_FAMILY(qgm_mix_bf16, QgmTune, MX_NO_STEP, qgm_round<QgmMixBf16>)
