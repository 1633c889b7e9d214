// qgm_mix.hip -- quasi-global momentum (QG-DSGDm: Lin et al., ICML 2021, "Quasi-Global Momentum:
// Accelerating Decentralized Deep Learning on Heterogeneous Data") fused into the mixing round (fp32 rows,
// local-only groups): one launch per training iteration applies every worker's local step, mixes the
// updated rows and feeds each worker's momentum buffer with the displacement of its row AFTER the round.
//
// A worker's buffer mh follows (x_t - x_{t+1}) / lr, the direction its neighbourhood actually moved, not
// its own shard's gradient; it costs no extra communication.  Per row and column, every line one fp32
// rounding (-ffp-contract=off, explicit fmas); g is widened and clip-scaled by grad_of, (wd_r, scale_r) are
// the run's pair (the launch's wd and 1.0 when ungrouped):
//     lr_r = fmul(lr, scale_r)
//     d    = (wd_r != 0) ? fmaf(wd_r, x, g) : g
//     m    = fadd(fmul(beta, mh), d)                      mh is read only here; m is never stored
//     s    = nesterov ? fmaf(beta, m, d) : m
//     x'   = fmaf(-lr_r, s, x)
//     y    = the round of sgd_mix.hip on the x' values: per output row the partners' columns in ascending
//            matching order, the self term last, every step one __builtin_fmaf; a row the plan record
//            leaves alone, and every row of an all-zero round, keeps y = x'
//     rl   = fdiv(1.0f, lr_r)                             once per launch, or per run when grouped
//     q    = fmul(fsub(x, y), rl)                         x: the value the row held BEFORE this launch
//     mh'  = (lr_r != 0) ? fmaf(omu, fsub(q, mh), mh) : mh
//     x    = y
// omu is the fp32 rounding of the fp64 value 1 - mu.  An all-zero round is the local step plus the buffer
// update, not a no-op.  lr_r == 0 (lr = 0, or a run of scale 0) leaves mh bit for bit while x is still
// mixed.  q amplifies the rounding of x by 1 / lr: that is the algorithm's, in any fp32 implementation.
//
// Traffic per element: read x, g, mh, write x, mh = 20 bytes (24 when the gradients are zeroed): the bytes
// of SGD with momentum.  The buffer update needs x and mh again after the round; they are re-read by the
// lane that finishes the (row, chunk), moments after the workgroup staged the same lines.  That re-read is NOT
// free: the step measures well behind the SGD-momentum step of the same bytes, less so with x and mh staged
// with plain loads than with nt loads (which cache level serves it has not been counted).
//
// In place: the staging lane loads x, g and mh, parks x' in LDS and stores ONLY the zeros over g; it never
// stores mh.  After the barrier the lane that finishes a (row, chunk) reloads x and mh of its own 4 columns
// with plain loads, computes q and mh', stores mh' and then y.  No other lane writes either address in this
// launch, and the row's own x is stored only by this lane, after its reload; different work items never
// share a column.  The finish side honours the alignment rule too: 16-byte accesses only where x, g and mh
// of the (segment, row) are all 16-byte aligned and the chunk is in range, per element elsewhere; nothing
// is read or written at or past a row's length.
//
// No receive slots: n_slots == n_local; a device counter outside the schedule, or a record with the
// peer-reads bit, makes the launch write nothing, the buffer included.
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is qgm_update.h's
// QgmRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<QgmMix<NESTEROV, PLAIN>, ...>) and defines the family's entry points.
#include "qgm_update.h"

namespace {
using namespace mx::fused;
// x, g and mh as fp32; 16-byte accesses only where x, g and mh of the (segment, row) are all 16-byte
// aligned.  PLAIN: knob "stage_plain"
template <bool NESTEROV, bool PLAIN>
struct QgmMix : QgmRows<Fp32Form, NESTEROV, PLAIN> {};
}  // namespace

MX_FUSED_FAMILY(qgm_mix, QgmTune, MX_NO_STEP, qgm_round<QgmMix>)
