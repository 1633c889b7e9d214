"""The consensus distance of a set of worker rows: the specification, restated in numpy for the tests (never
the code under test).  For n rows (1 <= n <= 64) of P columns, float32 (bfloat16 bit patterns are widened
exactly first, bf16ref.upcast):

    s_c      = ((f64(x_0c) + f64(x_1c)) + f64(x_2c)) + ...      fp64 adds in ROW ORDER
    m_c      = s_c / f64(n)                                     one IEEE fp64 division
    d_rc     = f64(x_rc) - m_c                                  one fp64 subtraction
    D_r      = sum_c d_rc^2          M = sum_c m_c^2            fp64, any order over the columns
    dist[r]  = f32(sqrt(D_r))
    stats[0] = f32(sqrt((D_0 + D_1 + ... in row order) / n))    the consensus distance
    stats[1] = f32(sqrt(M))                                     the norm of the mean row

The arithmetic of a column is pinned -- row order, a true division, nothing reassociated -- because x - m
cancels: near consensus another order of the mean changes d by far more than an fp64 rounding.  With the
mean pinned every conforming implementation has the same d_rc bit for bit, and the sums over the columns of
non-negative terms differ by at most P * 2^-53 relative between any two orders (each squared term carries
one more rounding of 2^-53 where it is not fused into the sum): every output is within 1 fp32 ulp of this
file for P <= 2^26.  Exact consequences: identical rows give exactly 0.0 (k * x is exact in fp64 for
k <= 64, so (n * x) / n = x); a NaN or Inf anywhere in a column makes its mean, hence every dist and both
stats, non-finite."""
import math

import numpy as np

import bf16ref

F32, F64 = np.float32, np.float64


def _colsum(v):
    """the fp64 sum of a non-negative fp64 vector: exactly rounded (math.fsum) up to 2^21 terms, numpy's
    pairwise sum (~1e-15) beyond, as clipref.grad_norm_ref; Inf or NaN whatever the order"""
    if not np.isfinite(v).all():
        return float(v.sum())
    return math.fsum(v.tolist()) if v.size <= (1 << 21) else float(np.sum(v))


def consref(x):
    """(dist float32 [n], stats float32 [2]) of a float32 [n, P] array"""
    x = np.asarray(x, F32)
    n = x.shape[0]
    assert x.ndim == 2 and 1 <= n <= 64
    with np.errstate(all="ignore"):
        x64 = x.astype(F64)
        s = x64[0].copy()
        for r in range(1, n):
            s = s + x64[r]                                 # row order
        m = s / F64(n)
        D = []
        for r in range(n):
            d = x64[r] - m
            D.append(_colsum(d * d))
        M = _colsum(m * m)
        total = D[0]
        for r in range(1, n):
            total = total + D[r]                           # row order
        dist = np.sqrt(np.asarray(D, F64)).astype(F32)
        stats = np.array([np.sqrt(F64(total) / F64(n)), np.sqrt(F64(M))], F64).astype(F32)
    return dist, stats


def consref_bf16(bits):
    return consref(bf16ref.upcast(bits))


KINDS = ("spread", "noise", "ulps")


def make_rows(rng, n, P, kind, elem=4):
    """the tests' inputs, [n, P] float32 (elem 4) or bfloat16 bit patterns as uint16 (elem 2): 'spread' rows of
    different magnitudes; 'noise' a shared base plus 1e-4 noise; 'ulps' a shared base with random single-ulp
    bumps of the element type (near consensus: the case a reordered mean fails)"""
    if kind == "spread":
        x = (rng.standard_normal((n, P)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(F32)
        return x if elem == 4 else bf16ref.rne_bf16(x)
    base = rng.standard_normal(P).astype(F32)
    if kind == "noise":
        x = (base[None] + 1e-4 * rng.standard_normal((n, P))).astype(F32)
        return x if elem == 4 else bf16ref.rne_bf16(x)
    assert kind == "ulps"
    bump = rng.integers(-1, 2, (n, P))
    if elem == 4:
        return (base.view(np.int32)[None] + bump.astype(np.int32)).view(F32)
    return (bf16ref.rne_bf16(base).astype(np.int32)[None] + bump).astype(np.uint16)
