// choco_round.h -- what the Choco apply kernels of both compressors (choco.hip: top-k, choco_sign.hip:
// scaled sign) share: how a launch finds its round's plan record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC__)
namespace mx {
namespace choco {

// The plan record of this round: `rec` itself, or with iter_dev (graph-replayable launches) the
// record of round *iter_dev of the plan table at `rec`; null (launch is a no-op) when that round
// is outside [0, n_iters) or has no active matching -- communicator.py:249-250 skips such rounds.
__device__ __forceinline__ const int32_t* round_rec(const int32_t* rec, const int64_t* iter_dev, int64_t n_iters,
                                                   int64_t words) {
    if (!iter_dev) return rec;
    const int64_t v = *iter_dev;
    if (v < 0 || v >= n_iters) return nullptr;
    const int32_t* r = rec + v * words;
    return r[0] ? r : nullptr;
}

}  // namespace choco
}  // namespace mx
#endif
