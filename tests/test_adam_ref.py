"""tests/adamref.py checked on the CPU against torch.optim.AdamW / torch.optim.Adam, and the package's
bias-correction table (adam_bias_table) against adamref's own restatement of it."""
import numpy as np
import pytest

from adamref import adam_ref, bias_table
from sgdref import F32

# beta1, beta2, eps, wd, decoupled
HYPERS = {"adamw": (0.9, 0.999, 1e-8, 1e-2, True), "adam_l2": (0.9, 0.999, 1e-8, 5e-4, False),
          "adam_plain": (0.9, 0.999, 1e-8, 0.0, False)}
_TABLES = {}


def _table(b1, b2):
    if (b1, b2) not in _TABLES:
        _TABLES[(b1, b2)] = bias_table(b1, b2)
    return _TABLES[(b1, b2)]


@pytest.mark.parametrize("name", sorted(HYPERS))
def test_adam_ref_against_torch(name):
    """5 steps on 8 x 4097, x uniform in [-1, 1), g ~ 0.01 N(0, 1), lr 1e-3: |x - torch| <= 2^-22.
    The specification is torch's single-tensor algorithm up to the rounding order of a few ops (torch
    may round a lerp or an addcdiv twice where the specification fuses); a prototype measured 2^-23 =
    one ulp of values in [0.5, 1), and the bound leaves one more bit for another torch build's
    rounding order.  The per-step update is ~ lr = 1e-3, so a wrong coefficient, sign or bias
    correction shows at 1e-4 or more.  exp_avg and exp_avg_sq (|m| < 0.1, v < 0.01) are held to the
    same absolute bound."""
    torch = pytest.importorskip("torch")
    b1, b2, eps, wd, decoupled = HYPERS[name]
    rng = np.random.default_rng(11)
    n, P, lr = 8, 4097, 1e-3
    x = rng.uniform(-1, 1, (n, P)).astype(F32)
    m, v = np.zeros((n, P), F32), np.zeros((n, P), F32)
    p = torch.nn.Parameter(torch.from_numpy(x.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    table = _table(b1, b2)
    for step in range(1, 6):
        g = (0.01 * rng.standard_normal((n, P))).astype(F32)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        x, m, v = adam_ref(x, g, m, v, step, lr, HYPERS[name], table)
        st = opt.state[p]
        for what, ours, theirs in (("x", x, p.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            d = float(np.abs(theirs.numpy().astype(np.float64) - ours).max())
            print(f"{name} step {step}: max |{what} - torch| = {d:.3e} ({d * 2 ** 23:.2f} x 2^-23)")
            assert d <= 2.0 ** -22, (what, step)
    assert np.abs(x).max() < 1.01


@pytest.mark.parametrize("betas,length", [((0.9, 0.999), 16628), ((0.9, 0.95), 325), ((0.5, 0.5), None)])
def test_bias_table_matches_restatement(pkg, betas, length):
    got = pkg.adam_bias_table(*betas)
    want = _table(*betas)
    assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 2
    assert got.shape == want.shape
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32))
    if length is not None:
        assert len(got) == length
    assert got[-1, 0] == 1.0 and got[-1, 1] == 1.0
    assert not (got[:-1] == 1.0).all(axis=1).any()          # it stops at the FIRST saturated row
    assert (np.diff(got, axis=0) >= 0).all()                 # both columns non-decreasing
    assert got[0, 0] == np.float32(1.0 - betas[0]) and 0 < got[0, 1] < 1


def test_bias_table_refuses_betas_that_do_not_saturate(pkg):
    with pytest.raises(ValueError):
        pkg.adam_bias_table(0.9, 1.0 - 2.0 ** -24)
    with pytest.raises(ValueError):
        pkg.adam_bias_table(0.9, 1.0)
