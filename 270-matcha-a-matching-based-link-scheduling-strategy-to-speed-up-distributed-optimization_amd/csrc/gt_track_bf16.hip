// gt_track_bf16.hip -- gt_track.hip's launch for gradients held in bfloat16 (the mixed-precision groups): the
// tracker and the previous gradient stay fp32, so nothing the tracker accumulates is lost to bf16 rounding, and
// the tracker has no bf16 image: there is no model row in this launch.  Per (segment, row) three arrays:
//     y   fp32 tracker            read and written in place (the call record's x table)
//     g   bf16 gradient           read; overwritten with zeros when zero_grads
//     gp  fp32 previous gradient  read and written
// Arithmetic contract: gt_track.hip's lines with
//     gs = f32(g)                 exact widening, bits << 16; then the row's clip factor where there is one
// so gp holds the widened (and clipped) gradient.  No-ops and refusals are gt_track.hip's.
//
// Traffic per element: read y (4), g (2), gp (4), write y (4), gp (4) = 18 bytes (20 when the gradients are
// zeroed).
//
// A lane holds 4 elements: 16-byte accesses on y and gp, 8-byte accesses on g.  Alignment rule: the vector path
// is taken where y and gp of the (segment, row) are 16-byte aligned, g is 8-byte aligned and the 4 elements
// are in range; everything else goes element by element (4-byte / 2-byte accesses), zero-filled past the end.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is gt_update.h's
// GtTrackRows over Bf16GradForm; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<GtTrackBf16, ...>) and defines the family's entry points.
#include "gt_update.h"

namespace {
using namespace mx::fused;
struct GtTrackBf16 : GtTrackRows<Bf16GradForm> {};
}  // namespace

MX_FUSED_FAMILY(gt_track_bf16, Tune, MX_NO_STEP, gt_track_round<GtTrackBf16>)
