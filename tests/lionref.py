"""The fused Lion + mixing rounds' specification (csrc/lion_mix.hip, csrc/lion_mix_bf16.hip), restated in
numpy for the tests and never the code under test.  Every line is one fp32 rounding:

    lr_r  = f32(lr * s_r)                         scale 1.0 (ungrouped): lr itself      groupref.run_lr
    decay = fmaf(-lr_r, wd_r, 1)
    x1    = f32(x * decay) if wd_r != 0 else x
    dm    = f32(g - m)
    c     = fmaf(omb1, dm, m)
    x'    = f32(x1 - lr_r) if c > 0 else f32(x1 + lr_r) if c < 0 else x1 if c == 0 else NaN
    m'    = fmaf(omb2, dm, m)
    out   = x' for a round whose flags are all zero, else O.decen_round(x', partner, flags, alpha)
            (with idle_rows="skip", rows of degree 0 put back to x')                    groupref.mix

omb1 / omb2 are the fp32 roundings of the fp64 values 1 - beta; g is what the update sees: widened from
bfloat16 exactly (bf16ref.upcast) and multiplied by the row's clip factor (clipref.scale_grad) where there
is one.  A zero c keeps x1 bit for bit.  The mixed-precision forms run the same lines on the fp32 masters
and round the stored master to bfloat16 once (p); a bfloat16 momentum is widened exactly on the way in and
rounded once, to nearest even, on the way out (bf16ref.rne_bf16)."""
import numpy as np

import bf16ref
import clipref
import groupref
from sgdref import fmaf32

F32 = np.float32


def omb(betas):
    """(omb1, omb2): the fp32 roundings of the fp64 values 1 - beta"""
    return F32(1.0 - float(betas[0])), F32(1.0 - float(betas[1]))


def lion_ref(x, g, m, lr, wd, betas):
    """The Lion update of float32 arrays: (x', m').  lr and wd are rounded to fp32 here."""
    x, g, m = (np.asarray(a, F32) for a in (x, g, m))
    lr, wd = F32(lr), F32(wd)
    omb1, omb2 = omb(betas)
    with np.errstate(all="ignore"):
        x1 = (x * fmaf32(-lr, wd, F32(1.0))).astype(F32) if wd != 0 else x
        dm = (g - m).astype(F32)
        c = fmaf32(omb1, dm, m)
        down, up = (x1 - lr).astype(F32), (x1 + lr).astype(F32)
        xp = np.where(c > 0, down, np.where(c < 0, up, np.where(c == 0, x1, F32(np.nan)))).astype(F32)
        return xp, fmaf32(omb2, dm, m)


def lion_update(x, g, m, lr, wd, betas, scale=None, runs=None):
    """(x', m') of float32 [n, P] arrays with the row clip factors `scale` (None: none) and the parameter
    runs [(start, end, wd_r, s_r), ...] (None: one run of (wd, 1.0))"""
    x, m = np.asarray(x, F32), np.asarray(m, F32)
    g = np.asarray(g, F32) if scale is None else clipref.scale_grad(g, scale)
    if runs is None:
        return lion_ref(x, g, m, lr, wd, betas)
    groupref.check_runs(runs, x.shape[1])
    xp, m2 = np.empty_like(x), np.empty_like(x)
    for a, b, wd_r, s in runs:
        xp[:, a:b], m2[:, a:b] = lion_ref(x[:, a:b], g[:, a:b], m[:, a:b], groupref.run_lr(lr, s), wd_r, betas)
    return xp, m2


def spec_round(O, x, g, m, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None):
    """One fused fp32 round of every worker: (x_out, m', x').  hyper = (beta1, beta2, wd)."""
    b1, b2, wd = hyper
    xp, m2 = lion_update(x, g, m, lr, wd, (b1, b2), scale, runs)
    return groupref.mix(O, xp, partner, flags, alpha, idle_rows), m2, xp


def spec_round_bf16(O, w, g_bits, m, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None,
                    m_bf16=False):
    """One mixed-precision round: (w_out, m', p_bits, w').  g_bits are bfloat16 bit patterns (uint16); m is
    float32, or with m_bf16 bfloat16 bit patterns in and out."""
    m32 = bf16ref.upcast(m) if m_bf16 else np.asarray(m, F32)
    w_out, m2, wp = spec_round(O, np.asarray(w, F32), bf16ref.upcast(g_bits), m32, partner, flags, alpha, lr, hyper,
                               idle_rows, scale, runs)
    return w_out, (bf16ref.rne_bf16(m2) if m_bf16 else m2), bf16ref.rne_bf16(w_out), wp


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def eq32(got, want):
    return bool(np.array_equal(u32(got), u32(want)))
