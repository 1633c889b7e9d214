"""The fused quasi-global-momentum rounds' specification (csrc/qgm_mix.hip, csrc/qgm_mix_bf16.hip; QG-DSGDm,
Lin et al., ICML 2021), restated in numpy for the tests and never the code under test.  Every line is one
fp32 rounding:

    lr_r = f32(lr * s_r)                          scale 1.0 (ungrouped): lr itself      groupref.run_lr
    d    = fmaf(wd_r, x, g) if wd_r != 0 else g
    m    = f32(f32(beta * mh) + d)                mh: the quasi-global buffer, read only here
    s    = fmaf(beta, m, d) if nesterov else m
    x'   = fmaf(-lr_r, s, x)
    y    = x' for a round whose flags are all zero, else O.decen_round(x', partner, flags, alpha)
           (with idle_rows="skip", rows of degree 0 put back to x')                     groupref.mix
    rl   = f32(1 / lr_r)
    q    = f32(f32(x - y) * rl)                   x: the value the row held before the round
    mh'  = fmaf(omu, f32(q - mh), mh) if lr_r != 0 else mh
    x    = y

beta is rounded to fp32; omu is the fp32 rounding of the fp64 value 1 - mu; g is what the update sees:
widened from bfloat16 exactly (bf16ref.upcast) and multiplied by the row's clip factor
(clipref.scale_grad) where there is one.  The mixed-precision form runs the same lines on the fp32 masters
and rounds the stored master to bfloat16 once (p)."""
import numpy as np

import bf16ref
import clipref
import groupref
from sgdref import fmaf32

F32 = np.float32


def omu_of(mu):
    """the fp32 rounding of the fp64 value 1 - mu"""
    return F32(1.0 - float(mu))


def local_step(x, g, mh, lr_r, wd, beta, nesterov):
    """x' of float32 arrays at the run's learning rate lr_r (already an fp32) and decay wd"""
    x, g, mh = (np.asarray(a, F32) for a in (x, g, mh))
    lr_r, wd, beta = F32(lr_r), F32(wd), F32(beta)
    with np.errstate(all="ignore"):
        d = fmaf32(wd, x, g) if wd != 0 else g
        m = ((beta * mh).astype(F32) + d).astype(F32)
        s = fmaf32(beta, m, d) if nesterov else m
        return fmaf32(-lr_r, s, x)


def buffer_step(x, y, mh, lr_r, mu):
    """mh' from the row before the round (x) and after it (y)"""
    x, y, mh = (np.asarray(a, F32) for a in (x, y, mh))
    lr_r = F32(lr_r)
    if lr_r == 0:
        return mh.copy()
    with np.errstate(all="ignore"):
        rl = F32(F32(1.0) / lr_r)
        q = ((x - y).astype(F32) * rl).astype(F32)
        return fmaf32(omu_of(mu), (q - mh).astype(F32), mh)


def _runs(runs, wd, P):
    if runs is None:
        return [(0, P, wd, 1.0)]
    groupref.check_runs(runs, P)
    return runs


def spec_round(O, x, g, mh, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None):
    """One fused fp32 round of every worker: (y, mh', x').  hyper = (beta, mu, wd, nesterov); `scale` the row
    clip factors (None: none); `runs` the parameter runs [(start, end, wd_r, s_r), ...] (None: one run of
    (wd, 1.0))."""
    beta, mu, wd, nesterov = hyper
    x, mh = np.asarray(x, F32), np.asarray(mh, F32)
    g = np.asarray(g, F32) if scale is None else clipref.scale_grad(g, scale)
    runs = _runs(runs, wd, x.shape[1])
    xp = np.empty_like(x)
    for a, b, wd_r, s in runs:
        xp[:, a:b] = local_step(x[:, a:b], g[:, a:b], mh[:, a:b], groupref.run_lr(lr, s), wd_r, beta, nesterov)
    y = groupref.mix(O, xp, partner, flags, alpha, idle_rows)
    m2 = np.empty_like(x)
    for a, b, wd_r, s in runs:
        m2[:, a:b] = buffer_step(x[:, a:b], y[:, a:b], mh[:, a:b], groupref.run_lr(lr, s), mu)
    return y, m2, xp


def spec_round_bf16(O, w, g_bits, mh, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None):
    """One mixed-precision round: (w_out, mh', p_bits, w').  g_bits are bfloat16 bit patterns (uint16)."""
    y, m2, wp = spec_round(O, np.asarray(w, F32), bf16ref.upcast(g_bits), mh, partner, flags, alpha, lr, hyper,
                           idle_rows, scale, runs)
    return y, m2, bf16ref.rne_bf16(y), wp


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def eq32(got, want):
    return bool(np.array_equal(u32(got), u32(want)))
