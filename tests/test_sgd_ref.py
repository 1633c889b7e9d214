"""tests/sgdref.py checked on the CPU: the exact float32 fma the specification of the fused SGD +
mixing round rests on, and its SGD lines against torch.optim.SGD."""
from fractions import Fraction

import numpy as np
import pytest

from sgdref import F32, fmaf32, fmaf_fraction, sgd_ref

HYPERS = {"H0": (0.0, 0.0, False), "H1": (5e-4, 0.9, False), "H2": (5e-4, 0.9, True)}   # wd, mom, nesterov


def _bits(v):
    return int(np.array(v, F32).view(np.uint32))


def test_adversarial_triple_rounds_once():
    """a*b = 2^-24 - 2^-64 sits just below the tie between 1 + 2^-23 and 1 + 2^-22 when added to
    c = 1 + 2^-23; the fp64 sum rounds onto the tie, which then rounds to even (up)."""
    a = F32((1 + 2.0 ** -20) * 2.0 ** -12)
    b = F32((1 - 2.0 ** -20) * 2.0 ** -12)
    c = F32(1 + 2.0 ** -23)
    assert Fraction(float(a)) * Fraction(float(b)) == Fraction(2) ** -24 - Fraction(2) ** -64
    naive = F32(np.float64(a) * np.float64(b) + np.float64(c))
    assert _bits(naive) == 0x3F800002
    assert _bits(fmaf32(a, b, c)) == 0x3F800001
    assert _bits(fmaf_fraction(a, b, c)) == 0x3F800001
    assert _bits(fmaf32(-a, b, -c)) == 0xBF800001


def test_fmaf32_against_fractions():
    rng = np.random.default_rng(7)
    n = 2000
    # exponents spread so products and addends meet at every alignment, cancellations included
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-24, 24, n)).astype(F32)
    c[::7] = -(a[::7] * b[::7])                      # near-cancellation: the fp32 product's rounding error is left
    tiny, big = F32(2.0 ** -149), F32(3.4028235e38)
    planted = [(tiny, F32(0.5), F32(0.0)), (tiny, F32(0.5), tiny), (tiny, F32(1.5), tiny), (tiny, tiny, F32(0.0)),
               (-tiny, tiny, F32(0.0)), (F32(2.0 ** -75), F32(2.0 ** -75), F32(2.0 ** -149)),
               (F32(2.0 ** -126), F32(0.75), F32(2.0 ** -149)), (F32(1e-42), F32(3.0), F32(-3e-41)),
               (big, F32(1.0), big), (big, F32(1 + 2.0 ** -23), F32(0.0)), (big, F32(1.0), F32(2.0 ** 103)),
               (big, F32(1.0), F32(2.0 ** 102)), (big, F32(1.0), F32(2.0 ** 103) * F32(1 - 2.0 ** -24)),
               (-big, F32(2.0), big), (big, F32(-1.0), F32(-2.0 ** 103)), (F32(0.0), F32(-1.0), F32(0.0)),
               (F32(-0.0), F32(1.0), F32(-0.0)), (F32(1.0), F32(1.0), F32(-1.0))]
    a = np.concatenate([a, np.array([p[0] for p in planted], F32)])
    b = np.concatenate([b, np.array([p[1] for p in planted], F32)])
    c = np.concatenate([c, np.array([p[2] for p in planted], F32)])
    got = fmaf32(a, b, c)
    want = np.array([fmaf_fraction(a[i], b[i], c[i]) for i in range(a.size)], F32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, [(a[i], b[i], c[i], got[i], want[i]) for i in bad[:5]]
    assert np.isinf(got[n + 8]) and np.isinf(got[n + 10]) and np.isfinite(got[n + 11])   # the overflow boundary
    assert _bits(got[n + 3]) == 0 and _bits(got[n + 4]) == 0x80000000                      # signed underflow
    # non-finite operands go the IEEE way
    assert np.isnan(fmaf32(F32(np.inf), F32(0.0), F32(1.0))) and np.isnan(fmaf32(F32(np.nan), F32(1.0), F32(1.0)))
    assert fmaf32(F32(np.inf), F32(2.0), F32(1.0)) == np.inf and fmaf32(F32(1.0), F32(2.0), F32(-np.inf)) == -np.inf


@pytest.mark.parametrize("name", sorted(HYPERS))
def test_sgd_ref_against_torch(name):
    """Two steps of torch.optim.SGD on CPU tensors, x and g uniform in [-1, 1), lr 0.1.  torch may
    round a + alpha*b twice where the specification fuses (three ops per step), and from the second
    step on the two run the same ops on inputs that differ: |fl(u) - fl(v)| <= |u - v| + ulp.  With
    eps = 2^-24 (half an ulp below 2; the Nesterov direction stays below 4): after step one x differs
    by <= 3 eps and m by <= eps; in step two d by <= 1.01 eps, m by <= 0.9 + 1.01 + 1 + 2 < 5 eps, the
    Nesterov direction by <= 0.9 * 5 + 1.01 + 4 < 10 eps and x by <= 3 + 0.1 * 10 + 2 = 6 eps -- all
    within 2^-20 = 16 eps, where a wrong coefficient or sign shows at 1e-4 or more."""
    torch = pytest.importorskip("torch")
    wd, mom, nesterov = HYPERS[name]
    rng = np.random.default_rng(3)
    P = 4097
    x = rng.uniform(-1, 1, P).astype(F32)
    p = torch.nn.Parameter(torch.from_numpy(x.copy()))
    opt = torch.optim.SGD([p], lr=0.1, momentum=mom, weight_decay=wd, nesterov=nesterov, dampening=0)
    m = np.zeros(P, F32) if mom else None
    for step in range(2):
        g = rng.uniform(-1, 1, P).astype(F32)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        x, m = sgd_ref(x, g, m, 0.1, wd, mom, nesterov)
        dx = float(np.abs(p.detach().numpy().astype(np.float64) - x).max())
        print(f"{name} step {step}: max |x - torch| = {dx:.3e}")
        assert dx <= 2.0 ** -20
        if mom:
            buf = opt.state[p]["momentum_buffer"].numpy()
            dm = float(np.abs(buf.astype(np.float64) - m).max())
            print(f"{name} step {step}: max |m - torch| = {dm:.3e}")
            assert dm <= 2.0 ** -20
    assert np.abs(x).max() < 2 and (m is None or np.abs(m).max() < 2)
