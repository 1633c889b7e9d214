// row_sum.h -- the order in which one column of the workers' rows is summed, shared by the mean kernels
// (exchange.cpp: mx_mean_rows / mx_mean_rows_to) and the SlowMo outer step (slowmo.hip), so that "the same
// mean" is the same code.  An order is a sequence of pairwise adds over rows held in registers; the caller
// brings the add (`add(i, j)` performs row[i] = row[i] + row[j], one fp32 rounding per element,
// -ffp-contract=off) and finds the sum in row 0.  The orders are the reference's object all-reduce
// (communicator.py:61, comm.allreduce(obj, MPI.SUM)):
//   tree_order   mpi4py's default (rc.fast_reduce): a binomial-tree reduction to rank 0 -- at mask 1, 2,
//                4, ... rank r (a multiple of 2 * mask) adds the partial sum of rank r + mask:
//                ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + ...)
//   rank_order   ((x0 + x1) + x2) + ...: mpi4py with fast_reduce off (allgather, then a left fold)
// MAXR bounds nrows at compile time so that the indices are constants (a register array); the adds a
// smaller nrows leaves out are skipped, which gives the same order for every MAXR >= nrows.
#pragma once

namespace mx {
namespace rowsum {

template <int MAXR, class Add>
__device__ __forceinline__ void tree_order(int nrows, Add add) {
#pragma unroll
    for (int m = 1; m < MAXR; m <<= 1)
#pragma unroll
        for (int r = 0; r + m < MAXR; r += 2 * m)
            if (r + m < nrows) add(r, r + m);
}

template <int MAXR, class Add>
__device__ __forceinline__ void rank_order(int nrows, Add add) {
#pragma unroll
    for (int r = 1; r < MAXR; ++r)
        if (r < nrows) add(0, r);
}

// the tree over one register array, the sum left in v[0]
template <int MAXR, class V>
__device__ __forceinline__ void tree_sum(V (&v)[MAXR], int nrows) {
    tree_order<MAXR>(nrows, [&](int i, int j) __attribute__((always_inline)) { v[i] = v[i] + v[j]; });
}

// order of the C ABI (0: the tree, 1: rank order) -> the kernels' TREE template argument
constexpr int tree_of(int order) { return order == 1 ? 0 : 1; }

}  // namespace rowsum
}  // namespace mx
