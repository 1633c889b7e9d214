// gt_track.hip -- the track launch of gradient tracking (GT-DSGD) with fp32 gradients (local-only groups): every
// worker's tracker takes in the change of its gradient and the trackers are gossiped, in one launch.
//
// Gradient tracking removes the stationary error that heterogeneous shards leave in D-PSGD at a constant
// learning rate: every worker steps along a tracker y_i whose network mean is the mean of the workers' current
// gradients, not along its own gradient.  Matchings are symmetric and MATCHA's per-round matrices doubly
// stochastic, so mean_i y_i = mean_i gs_i holds after every round of a time-varying schedule.  One iteration
// is this launch and then the step launch (mx_sgd_mix with the tracker's table as its g, or mx_gt_step_bf16),
// both on the same plan record.  Per (segment, row) three arrays:
//     y   fp32 tracker            read and written in place (the call record's x table)
//     g   fp32 gradient           read; overwritten with zeros when zero_grads
//     gp  fp32 previous gradient  read and written: the value that entered the tracker one iteration ago
// Arithmetic contract, per element, every line one fp32 rounding (-ffp-contract=off):
//     gs = g, multiplied by the row's clip factor where there is one (mx_gt_track_scaled)
//     t  = fsub(gs, gp)
//     y' = fadd(y, t)
//     gp = gs                     the clip factor included: the differences telescope as the tracker saw them
//     g  = 0                      under zero_grads
//     y  = the round of sgd_mix.hip on the y' values: per output row the partners' columns in ascending
//          matching order, the self term last, every step one __builtin_fmaf; a row the plan record leaves
//          alone, and every row of an all-zero round, keeps y' as it is
// y and gp start as zeros; there is no first-step case, y' = g falls out.  No learning rate and no weight decay
// enter: weight decay is local and sits in the step launch, so this launch never reads the weights.  A device
// counter outside the schedule, or a plan record with the peer-reads bit, makes the launch a complete no-op.
// Nothing is written at or past a row's length in any array.
//
// Traffic per element: read y, g, gp, write y, gp = 20 bytes (24 when the gradients are zeroed).
//
// In place: a tile's y' of every row is parked in LDS (barrier) before any y row of it is stored.  gp and g are
// read and written by the same lane only, so they are stored when their chunk is staged.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is gt_update.h's
// GtTrackRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces
// show it as fused_round_rows<GtTrack, ...>) and defines the family's entry points.
#include "gt_update.h"

namespace {
using namespace mx::fused;
// y, g and gp as fp32; 16-byte accesses only where all three of the (segment, row) are 16-byte aligned
struct GtTrack : GtTrackRows<Fp32Form> {};
}  // namespace

MX_FUSED_FAMILY(gt_track, Tune, MX_NO_STEP, gt_track_round<GtTrack>)
