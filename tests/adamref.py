"""The fused AdamW / Adam + mixing round's specification, restated in numpy for the tests (never the
code under test):

    decay = fmaf(-lr, wd, 1)
    x1 = x * decay      if wd != 0 and decoupled     else x            AdamW: p.mul_(1 - lr*wd)
    g1 = fmaf(wd, x, g) if wd != 0 and not decoupled else g            Adam:  g.add(p, alpha=wd)
    m' = fmaf(omb1, g1 - m, m)
    v' = fmaf(omb2, g1 * g1, beta2 * v)
    den = sqrt(v') / bc2s + eps
    x'  = fmaf(-(lr / bc1), m' / den, x1)
    out = x' for a round whose flags are all zero, else O.decen_round(x', partner, flags, alpha)
          (with idle_rows="skip", rows of degree 0 put back to x')

in float32, one rounding per operation: numpy's float32 +, -, *, / and sqrt are correctly rounded, and
sgdref.fmaf32 is the exact fused multiply-add.  lr, wd, eps and beta2 are the fp32 roundings of the
Python floats, omb1 / omb2 those of the fp64 values 1 - beta1 / 1 - beta2, and (bc1, bc2s) of step
t >= 1 is row min(t, n) - 1 of bias_table(beta1, beta2) -- this file's own restatement of the table."""
import math

import numpy as np

from sgdref import F32, fmaf32

BIAS_MAX = 1 << 21


def bias_table(beta1, beta2):
    """float32 [n, 2]: row t-1 = (f32(1 - beta1**t), f32(sqrt(1 - beta2**t))) in Python floats (what
    torch.optim.Adam computes), up to and including the first row that is exactly (1, 1)."""
    out = []
    for t in range(1, BIAS_MAX + 1):
        out.append((F32(1.0 - beta1 ** t), F32(math.sqrt(1.0 - beta2 ** t))))
        if out[-1][0] == F32(1.0) and out[-1][1] == F32(1.0):
            return np.array(out, F32)
    raise ValueError("betas do not saturate")


def bias_at(table, t):
    assert t >= 1
    row = table[min(int(t), len(table)) - 1]
    return F32(row[0]), F32(row[1])


def adam_ref(x, g, m, v, t, lr, hyper, table):
    """One update of float32 arrays at optimizer step t: (x', m', v').  hyper = (beta1, beta2, eps, wd,
    decoupled), Python floats."""
    beta1, beta2, eps, wd, decoupled = hyper
    x, g, m, v = (np.asarray(a, F32) for a in (x, g, m, v))
    lr, wd, eps = F32(lr), F32(wd), F32(eps)
    omb1, omb2, b2 = F32(1.0 - beta1), F32(1.0 - beta2), F32(beta2)
    bc1, bc2s = bias_at(table, t)
    with np.errstate(all="ignore"):
        x1, g1 = x, g
        if wd != 0 and decoupled:
            x1 = x * fmaf32(-lr, wd, F32(1.0))
        if wd != 0 and not decoupled:
            g1 = fmaf32(wd, x, g)
        m2 = fmaf32(omb1, g1 - m, m)
        v2 = fmaf32(omb2, g1 * g1, b2 * v)
        den = np.sqrt(v2) / bc2s + eps
        ss = lr / bc1
        xp = fmaf32(-ss, m2 / den, x1)
    assert xp.dtype == F32 and m2.dtype == F32 and v2.dtype == F32 and den.dtype == F32
    return xp, m2, v2


def spec_round(O, x, g, m, v, t, partner, flags, alpha, lr, hyper, table, idle_rows="skip"):
    """One fused round of every worker by the specification: (x_out, m', v', x')."""
    xp, m2, v2 = adam_ref(x, g, m, v, t, lr, hyper, table)
    flags = np.asarray(flags, np.uint8)
    if not flags.any():
        return xp.copy(), m2, v2, xp
    partner = np.asarray(partner, np.int32)
    out = O.decen_round(np.ascontiguousarray(xp), partner, flags, alpha)
    if idle_rows == "skip":
        deg = (partner[flags.astype(bool)] >= 0).sum(axis=0)
        out[deg == 0] = xp[deg == 0]
    return out, m2, v2, xp
