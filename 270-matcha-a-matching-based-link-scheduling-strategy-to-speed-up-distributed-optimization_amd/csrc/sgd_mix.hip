// sgd_mix.hip -- the SGD update of every local worker fused into the mixing round (fp32 rows,
// local-only groups): one launch per training iteration instead of n optimizer steps + one mix.
//
// The reference's iteration (train_mpi.py:131-142) runs optimizer.step(), optimizer.zero_grad(),
// communicator.communicate(model).  Here each row's x, g and m elements are read once, torch.optim.SGD's
// update (dampening 0) is applied on the way into LDS
//     d  = (wd != 0) ? fmaf(wd, x, g) : g                 g.add(p, alpha=wd)
//     m  = fadd(fmul(mom, m), d)           [mom != 0]     buf.mul_(mom).add_(d_p): two roundings
//     d  = nesterov ? fmaf(mom, m, d) : m  [mom != 0]
//     x' = fmaf(-lr, d, x)                                p.add_(d_p, alpha=-lr)
// and the round of mix.hip's mix_kernel_rows (decenCommunicator.prepare_comm_buffer / averaging /
// reset_model, communicator.py:87-131) then runs on the staged x' values: per output row the partners'
// columns in ascending matching order, the self term last, every step one __builtin_fmaf.  Rows the plan
// record does not read and write (degree 0 outside idle mode 1), and every row of a round whose flags
// are all zero, get x' stored as it is: an all-zero round is the SGD step alone, not a no-op.
//
// Traffic per element: read x, g, m, write x, m = 20 bytes (24 when the gradients are zeroed, 12 / 16
// without momentum) against 52 for the torch op sequence followed by the mixing round.
//
// In place: a tile's x' of every row is parked in LDS (barrier) before any x row of it is stored, and
// different work items never share a column.  m is read and written by the same lane only, so it is
// stored when its chunk is staged; so are the zeros over g with zero_grads.  Because every row is read
// in every round, the first loads are issued before the plan record is looked at.
//
// No receive slots: n_slots == n_local, the plan's n_remote is 0; a record with the peer-reads bit
// makes the launch write nothing (the bit lives on the device; see mx_sgd_mix in the header).
//
// The row kernel, its mixing walk and the host side are fused_round.h's and the policy is sgd_update.h's
// SgdRows over a storage form; this file names the policy the kernel is instantiated with (kernel traces show
// it as fused_round_rows<SgdMix<MOM>, ...>) and defines the family's entry points.
#include "sgd_update.h"

namespace {
using namespace mx::fused;
// x, g and m as fp32; 16-byte accesses only where x, g and m of the (segment, row) are all 16-byte aligned
template <bool MOM>
struct SgdMix : SgdRows<Fp32Form, MOM> {};
}  // namespace

MX_FUSED_FAMILY(sgd_mix, Tune, MX_NO_STEP, sgd_round<SgdMix>)
