"""The fused SGD + mixing round's specification, restated in numpy for the tests (never the code
under test):

    d  = fmaf(wd, x, g) if wd != 0 else g
    m  = f32(f32(mom * m) + d);  d = fmaf(mom, m, d) if nesterov else m        [mom != 0]
    x' = fmaf(-lr, d, x)
    out = x' for a round whose flags are all zero, else O.decen_round(x', partner, flags, alpha)
          (with idle_rows="skip", rows of degree 0 put back to x')

in float32, lr / wd / mom being the fp32 roundings of the Python floats.  fmaf32 is an exact fused
multiply-add: numpy has none, and rounding the fp64 value of a*b + c to fp32 rounds twice."""
from fractions import Fraction

import numpy as np

F32 = np.float32
_TWO128 = Fraction(2) ** 128


def _frac(v):
    """the value a finite float stands for; +-Inf as the float after the largest finite one (+-2^128,
    an even mantissa): what IEEE rounding to nearest compares against at the overflow boundary"""
    v = float(v)
    if np.isinf(v):
        return _TWO128 if v > 0 else -_TWO128
    return Fraction(v)


def _nearest(exact, cands):
    """the float32 among `cands` nearest to the exact value, ties to the even mantissa"""
    best = None
    for c in cands:
        key = (abs(_frac(c) - exact), int(np.array(c, F32).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def fmaf32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding, elementwise.  s = f64(a) * f64(b) + f64(c) (the product
    is exact in fp64) and r = f32(s); wherever f32 of either fp64 neighbour of s differs from r, s sits
    on an fp32 rounding boundary and the fp64 rounding may have put it on the wrong side: there the exact
    value (fractions.Fraction) picks the upper neighbour, the lower neighbour or r."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        r = s.astype(F32)
        up = np.nextafter(s, np.inf).astype(F32)
        dn = np.nextafter(s, -np.inf).astype(F32)
    amb = np.isfinite(s) & ((up.view(np.uint32) != r.view(np.uint32)) | (dn.view(np.uint32) != r.view(np.uint32)))
    r = np.array(r, F32)
    for i in np.argwhere(amb):
        i = tuple(i)
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        if exact != Fraction(float(s[i])):
            r[i] = _nearest(exact, (dn[i], r[i], up[i]))
    return r


def fmaf_fraction(a, b, c):
    """One finite triple by exact arithmetic alone: the float32 nearest a*b + c, ties to even (the
    check of fmaf32 in tests/test_sgd_ref.py).  Candidates: the fp32 below and above the exact value."""
    a, b, c = F32(a), F32(b), F32(c)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        with np.errstate(all="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))      # the sign of an exact zero
    with np.errstate(over="ignore"):
        near = F32(float(exact)) if abs(exact) < _TWO128 else F32(np.inf if exact > 0 else -np.inf)
        cands = (np.nextafter(near, F32(-np.inf)), near, np.nextafter(near, F32(np.inf)))
    got = _nearest(exact, cands)
    if got == 0:                                  # underflow to zero keeps the exact value's sign
        return F32(-0.0) if exact < 0 else F32(0.0)
    return F32(got)


def sgd_ref(x, g, m, lr, wd, mom, nesterov):
    """torch.optim.SGD's update (dampening 0) of float32 arrays: (x', m'); m is None without momentum.
    The momentum line always runs (a zero buffer on the first step)."""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    lr, wd, mom = F32(lr), F32(wd), F32(mom)
    with np.errstate(all="ignore"):
        d = fmaf32(wd, x, g) if wd != 0 else g
        if mom != 0:
            m = (mom * np.asarray(m, F32)).astype(F32) + d
            d = fmaf32(mom, m, d) if nesterov else m
        return fmaf32(-lr, d, x), m


def spec_round(O, x, g, m, partner, flags, alpha, hyper, idle_rows="skip"):
    """One fused round of every worker by the specification: (x_out, m', x').  hyper = (lr, wd, mom,
    nesterov)."""
    lr, wd, mom, nesterov = hyper
    xp, m2 = sgd_ref(x, g, m, lr, wd, mom, nesterov)
    flags = np.asarray(flags, np.uint8)
    if not flags.any():
        return xp.copy(), m2, xp
    partner = np.asarray(partner, np.int32)
    out = O.decen_round(np.ascontiguousarray(xp), partner, flags, alpha)
    if idle_rows == "skip":
        deg = (partner[flags.astype(bool)] >= 0).sum(axis=0)
        out[deg == 0] = xp[deg == 0]
    return out, m2, xp


def is_nan32(a):
    return (np.asarray(a, F32).view(np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def same_f32(got, want):
    """uint32-exact where `want` is not a NaN, a NaN of any payload where it is."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    wn = is_nan32(want)
    return bool(np.array_equal(is_nan32(got), wn) and
                np.array_equal(got.view(np.uint32)[~wn], want.view(np.uint32)[~wn]))
