"""Global-norm gradient clipping in the fused optimizer rounds: the specification, restated in numpy for
the tests (never the code under test).  Per worker row r, torch.nn.utils.clip_grad_norm_'s 2-norm form
(error_if_nonfinite=False):

    norm[r]  = f32(sqrt(sum_c f64(g[r, c])^2))              fp64 squares, fp64 sum, fp64 root, one rounding
    c        = (1 / (norm[r] + f32(1e-6))) * f32(max_norm)  three fp32 roundings: torch evaluates its
                                                            max_norm / (total_norm + 1e-6) on a tensor as
                                                            reciprocal() * max_norm (Tensor.__rtruediv__)
    scale[r] = 1.0 if c > 1.0 else c                        a NaN stays a NaN
    g'       = scale[r] * g                                 one fp32 multiply, before anything else in the update

and the update then sees g' wherever it saw g (the L2 term, m, v, momentum).  For bfloat16 gradients
g is widened exactly first (bf16ref.upcast) and g' stays fp32 -- it is never rounded back -- so the
mixed-precision wrappers below run the fp32 specifications (sgdref / adamref) on the masters and round
the result to bfloat16 once (bf16ref.rne_bf16), as sgdbf16ref / adambf16ref do after their own widening
(those two take bfloat16 bit patterns, which g' no longer is).

The summation order of the norm is free: any fp64 order over P <= 2^26 non-negative terms is within
P * 2^-53 of the exact sum, so a conforming norm is within 1 fp32 ulp of grad_norm_ref."""
import math

import numpy as np

import adamref
import bf16ref
import sgdref

F32 = np.float32


def grad_norm_ref(g):
    """float32 [n]: the 2-norm of every row of a float32 [n, P] array (math.fsum: the exactly rounded
    fp64 sum of the exact fp64 squares)."""
    g = np.asarray(g, F32)
    out = np.empty(g.shape[0], F32)
    with np.errstate(all="ignore"):
        for r in range(g.shape[0]):
            sq = g[r].astype(np.float64) ** 2
            if not np.isfinite(sq).all():
                s = float(sq.sum())                        # Inf or NaN whatever the order
            else:
                s = math.fsum(sq.tolist()) if sq.size <= (1 << 16) else float(np.sum(sq))   # pairwise: ~1e-15
            out[r] = F32(np.sqrt(np.float64(s)))
    return out


def grad_norm_ref_bf16(g_bits):
    return grad_norm_ref(bf16ref.upcast(g_bits))


def clip_scale_ref(norm, max_norm):
    """float32 [n]: the clip factor of float32 norms, torch's expression in fp32."""
    norm = np.asarray(norm, F32)
    with np.errstate(all="ignore"):
        c = ((F32(1.0) / (norm + F32(1e-6))).astype(F32) * F32(max_norm)).astype(F32)
    return np.where(c > F32(1.0), F32(1.0), c).astype(F32)


def ulp_diff(a, b):
    """distance in fp32 steps between finite non-negative float32 values (their bit patterns are ordered)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def scale_grad(g, scale):
    """g' = scale[r] * g: one fp32 multiply per element"""
    with np.errstate(all="ignore"):
        out = (np.asarray(scale, F32)[:, None] * np.asarray(g, F32)).astype(F32)
    assert out.dtype == F32
    return out


def sgd_round(O, x, g, m, scale, partner, flags, alpha, hyper, idle_rows="skip"):
    """sgdref.spec_round on the pre-scaled gradient: (x_out, m', x')"""
    return sgdref.spec_round(O, x, scale_grad(g, scale), m, partner, flags, alpha, hyper, idle_rows)


def sgd_bf16_round(O, w, g_bits, m, scale, partner, flags, alpha, hyper, idle_rows="skip"):
    """the mixed-precision round on the pre-scaled widened gradient: (w_out, m', p_bits, w')"""
    w_out, m2, wp = sgdref.spec_round(O, np.asarray(w, F32), scale_grad(bf16ref.upcast(g_bits), scale), m, partner,
                                      flags, alpha, hyper, idle_rows)
    return w_out, m2, bf16ref.rne_bf16(w_out), wp


def adam_round(O, x, g, m, v, t, scale, partner, flags, alpha, lr, hyper, table, idle_rows="skip"):
    """adamref.spec_round on the pre-scaled gradient: (x_out, m', v', x')"""
    return adamref.spec_round(O, x, scale_grad(g, scale), m, v, t, partner, flags, alpha, lr, hyper, table, idle_rows)


def adam_bf16_round(O, w, g_bits, m, v, t, scale, partner, flags, alpha, lr, hyper, table, idle_rows="skip"):
    """the mixed-precision round on the pre-scaled widened gradient: (w_out, m', v', p_bits, w')"""
    w_out, m2, v2, wp = adamref.spec_round(O, np.asarray(w, F32), scale_grad(bf16ref.upcast(g_bits), scale), m, v, t,
                                           partner, flags, alpha, lr, hyper, table, idle_rows)
    return w_out, m2, v2, bf16ref.rne_bf16(w_out), wp
