"""The SlowMo outer step's specification, restated in numpy for the tests (never the code under test):

    s    = the sum of the n rows in mx_mean_rows' order (reforder.mpi4py_sum: order 0 tree, 1 rank order)
    mean = f32(s / f32(n))
    rl   = f32(1 / lr);  al = f32(alpha * lr)                once per step
    q    = f32(f32(a - mean) * rl)
    u'   = fmaf(beta, u, q)
    a'   = fmaf(-al, u', a)
    every row = a';  a = a';  u = u';  mixed precision: every p row = rne_bf16(a')

in float32, alpha / beta / lr being the fp32 roundings of the Python floats.  A learning rate of exactly 0
leaves everything as it is (the device rule; the host paths refuse it)."""
import numpy as np

from bf16ref import rne_bf16
from reforder import mpi4py_sum
from sgdref import fmaf32

F32 = np.float32
ORDERS = {0: "tree", 1: "sequential"}


def mean_rows(rows, order):
    """The pinned-order mean of the rows ([n, P] float32): mx_mean_rows' bits."""
    rows = np.asarray(rows, F32)
    with np.errstate(all="ignore"):
        s = mpi4py_sum(list(rows), ORDERS[order])
        return (s / F32(rows.shape[0])).astype(F32)


def outer_step(rows, a, u, lr, alpha, beta, order=0):
    """One outer step: (a', u') -- every row (the fp32 masters of a mixed-precision group) becomes a'."""
    a, u = np.asarray(a, F32), np.asarray(u, F32)
    lr, alpha, beta = F32(lr), F32(alpha), F32(beta)
    if lr == 0:
        return a.copy(), u.copy()
    with np.errstate(all="ignore"):
        mean = mean_rows(rows, order)
        rl = F32(1.0) / lr
        al = alpha * lr
        q = ((a - mean).astype(F32) * rl).astype(F32)
        u2 = fmaf32(beta, u, q)
        a2 = fmaf32(-al, u2, a)
    return a2, u2


def spec_step(rows, a, u, lr, alpha, beta, order=0, mixed=False):
    """The arrays after one outer step: (rows', a', u', p') with p' the bfloat16 bit patterns of a
    mixed-precision group's model rows (None for an fp32 group).  lr == 0: nothing changes (p' None: the
    launch does not write it)."""
    rows = np.asarray(rows, F32)
    a2, u2 = outer_step(rows, a, u, lr, alpha, beta, order)
    if F32(lr) == 0:
        return rows.copy(), a2, u2, None
    out = np.broadcast_to(a2, rows.shape).copy()
    return out, a2, u2, (rne_bf16(out) if mixed else None)
