// gt_step_bf16.hip -- the step launch of gradient tracking for models held in bfloat16: sgd_mix_bf16.hip's launch
// with the fp32 tracker in the bf16 gradient's place (local-only groups).  For fp32 rows the step launch is
// mx_sgd_mix itself over the tracker's table; this file exists because the mixed-precision kernel has to read
// an fp32 "gradient".  Per (segment, row) four arrays:
//     w  fp32 master      read and written in place
//     y  fp32 tracker     READ ONLY (the call record's g table): the track launch of the same iteration wrote it
//     m  fp32 momentum    read and written; absent when mom == 0
//     p  bf16 model row   WRITE ONLY: never read
// Arithmetic contract (torch.optim.SGD, dampening 0, on the fp32 masters, with g := y):
//     d   = (wd != 0) ? fmaf(wd, w, y) : y
//     m   = fadd(fmul(mom, m), d)            [mom != 0]   two roundings (-ffp-contract=off)
//     d   = nesterov ? fmaf(mom, m, d) : m   [mom != 0]
//     w'  = fmaf(-lr, d, w)
//     w   = the round of sgd_mix.hip on the w' values
//     p   = bf16_rne(w)                                   ONE rounding, to nearest even, of the value stored to w
// lr_dev, the parameter runs (wd_r, lr_r = fmul(lr, s_r)) and the momentum line are the SGD families'.  The
// launch never writes y: a record with zero_grads is refused, and so are clip factors (they entered the
// tracker in the track launch).  Weight decay is local: it sits here, not in the tracked gradient.  No-ops are
// the SGD families': a device counter outside the schedule or a peer-reads record writes nothing.
//
// Traffic per element: read w (4), y (4), m (4), write w (4), m (4), p (2) = 22 bytes (14 without momentum).
//
// Alignment rule: the vector path is taken where w, y and m of the (segment, row) are 16-byte aligned, p is
// 8-byte aligned and the 4 elements are in range; everything else goes element by element.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is sgd_update.h's
// SgdRows over Fp32GradForm; this file names the policy the kernel is instantiated with (kernel traces show it
// as fused_round_rows<GtStepBf16<MOM>, ...>) and defines the family's entry points.
#include "gt_update.h"

namespace {
using namespace mx::fused;
template <bool MOM>
struct GtStepBf16 : SgdRows<Fp32GradForm, MOM> {};
}  // namespace

MX_FUSED_FAMILY(gt_step_bf16, Tune, MX_NO_STEP, gt_step_round<GtStepBf16>)
