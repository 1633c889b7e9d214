"""Per-parameter-group weight decay and learning-rate scale in the fused optimizer rounds: the
specification, restated in numpy for the tests (never the code under test).

A row's columns [0, P) are cut into runs [(start, end, wd_r, s_r), ...] that cover them in order.  With
lr the step's learning rate, every element of run r gets the existing update (sgdref.sgd_ref /
adamref.adam_ref, applied to the run's column slice) with

    lr_r = F32(lr) * F32(s_r)          one fp32 multiply
    wd   -> wd_r
    lr   -> lr_r

and everything else -- momentum, betas, eps, the bias table, nesterov, decoupled, the clip factor (one
per row, over all its runs: clipref.scale_grad before anything else), the mix of the x' values -- is
the whole row's.  The mixed-precision wrappers widen the bfloat16 gradient exactly, run the fp32
specification on the masters and round the stored master to bfloat16 once, as clipref's do."""
import numpy as np

import adamref
import bf16ref
import clipref
import sgdref

F32 = np.float32


def check_runs(runs, P):
    at = 0
    for a, b, wd, s in runs:
        assert a == at and b > a, (runs, P)
        at = b
    assert at == P, (runs, P)


def run_lr(lr, s):
    with np.errstate(all="ignore"):
        return F32(F32(lr) * F32(s))


def _grad(g, scale):
    return np.asarray(g, F32) if scale is None else clipref.scale_grad(g, scale)


def sgd_update(x, g, m, runs, lr, mom, nesterov):
    """(x', m') of float32 [n, P] arrays; m is None without momentum"""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    check_runs(runs, x.shape[1])
    xp = np.empty_like(x)
    m2 = None if F32(mom) == 0 else np.empty_like(x)
    for a, b, wd, s in runs:
        xs, ms = sgdref.sgd_ref(x[:, a:b], g[:, a:b], None if m2 is None else np.asarray(m, F32)[:, a:b],
                                run_lr(lr, s), wd, mom, nesterov)
        xp[:, a:b] = xs
        if m2 is not None:
            m2[:, a:b] = ms
    return xp, m2


def adam_update(x, g, m, v, t, runs, lr, hyper, table):
    """(x', m', v') of float32 [n, P] arrays at optimizer step t; hyper = (beta1, beta2, eps, wd, decoupled),
    its wd ignored"""
    x, g, m, v = (np.asarray(a, F32) for a in (x, g, m, v))
    check_runs(runs, x.shape[1])
    beta1, beta2, eps, _, decoupled = hyper
    xp, m2, v2 = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    for a, b, wd, s in runs:
        xp[:, a:b], m2[:, a:b], v2[:, a:b] = adamref.adam_ref(x[:, a:b], g[:, a:b], m[:, a:b], v[:, a:b], t,
                                                              run_lr(lr, s), (beta1, beta2, eps, wd, decoupled), table)
    return xp, m2, v2


def mix(O, xp, partner, flags, alpha, idle_rows="skip"):
    """the round on the x' values, as sgdref / adamref.spec_round run it"""
    flags = np.asarray(flags, np.uint8)
    if not flags.any():
        return xp.copy()
    partner = np.asarray(partner, np.int32)
    out = O.decen_round(np.ascontiguousarray(xp), partner, flags, alpha)
    if idle_rows == "skip":
        deg = (partner[flags.astype(bool)] >= 0).sum(axis=0)
        out[deg == 0] = xp[deg == 0]
    return out


def sgd_round(O, x, g, m, scale, runs, partner, flags, alpha, hyper, idle_rows="skip"):
    """hyper = (lr, mom, nesterov); scale None = no clip factor.  (x_out, m')"""
    lr, mom, nesterov = hyper
    xp, m2 = sgd_update(x, _grad(g, scale), m, runs, lr, mom, nesterov)
    return mix(O, xp, partner, flags, alpha, idle_rows), m2


def sgd_bf16_round(O, w, g_bits, m, scale, runs, partner, flags, alpha, hyper, idle_rows="skip"):
    """(w_out, m', p_bits)"""
    w_out, m2 = sgd_round(O, w, bf16ref.upcast(g_bits), m, scale, runs, partner, flags, alpha, hyper, idle_rows)
    return w_out, m2, bf16ref.rne_bf16(w_out)


def adam_round(O, x, g, m, v, t, scale, runs, partner, flags, alpha, lr, hyper, table, idle_rows="skip"):
    """(x_out, m', v')"""
    xp, m2, v2 = adam_update(x, _grad(g, scale), m, v, t, runs, lr, hyper, table)
    return mix(O, xp, partner, flags, alpha, idle_rows), m2, v2


def adam_bf16_round(O, w, g_bits, m, v, t, scale, runs, partner, flags, alpha, lr, hyper, table, idle_rows="skip"):
    """(w_out, m', v', p_bits)"""
    w_out, m2, v2 = adam_round(O, w, bf16ref.upcast(g_bits), m, v, t, scale, runs, partner, flags, alpha, lr, hyper,
                               table, idle_rows)
    return w_out, m2, v2, bf16ref.rne_bf16(w_out)
