"""tests/rowtopos.py's tables are what tests/test_gpu_row_classes.py takes them for (no GPU): matchings,
the stated degrees, the plan contract's partner order, and -- the condition that keeps the GPU comparisons
from being vacuous -- specifications that stay finite on them: with ALPHA = 1/64 a round is a convex
combination, so no NaN or Inf arises and every output element is compared bit for bit."""
import numpy as np
import pytest

import adambf16ref
import adamref
import bf16ref
import sgdbf16ref
import sgdref
from planref import py_plan
from rowtopos import ALPHA, M_MAX, N_ALL, cases, degrees, flag_rounds, round_robin, single, star, table

F32 = np.float32
LR = 1e-2
SGD_HYPER = (5e-4, 0.9, True)                      # tests/test_gpu_clip_fused.py's
ADAM_HYPER = (0.8, 0.95, 1e-6, 5e-4, False)


@pytest.mark.parametrize("n,name", cases(N_ALL))
def test_matchings_are_involutions(n, name):
    partner = table(name, n)
    assert partner.dtype == np.int32 and partner.shape[1] == n and 1 <= partner.shape[0] <= M_MAX
    for row in partner:
        for i, j in enumerate(row):
            assert j == -1 or (0 <= j < n and j != i and row[j] == i)


@pytest.mark.parametrize("n", N_ALL)
def test_degrees_as_stated(n):
    if n == 1:
        assert single().tolist() == [[-1]]
        assert not (round_robin(1) >= 0).any()
        return
    rr = round_robin(n)
    assert rr.shape == (M_MAX, n)
    deg = degrees(rr, np.ones(M_MAX, np.uint8))
    if n % 2 == 0:
        assert (deg == M_MAX).all()                # every round is a perfect matching
    else:                                          # one bye per cycle of n rounds
        byes = M_MAX - deg
        assert byes.min() >= M_MAX // n and byes.max() <= -(-M_MAX // n)
        assert int(byes.sum()) == M_MAX            # one worker sits out every matching
    if n >= 33:
        assert deg.min() >= 31
    period = n + (n & 1) - 1                       # rounds of the circle method; cycling repeats them
    first = [tuple(row) for row in rr[:min(period, M_MAX)]]
    assert len(set(first)) == len(first)
    for g in range(period, M_MAX):
        assert np.array_equal(rr[g], rr[g - period])
    for i in range(n):                             # within one cycle a row meets every other worker once
        met = [int(row[i]) for row in rr[:min(period, M_MAX)] if row[i] >= 0]
        assert len(set(met)) == len(met)
    st = star(n)
    M = min(M_MAX, n - 1)
    assert st.shape == (M, n)
    deg = degrees(st, np.ones(M, np.uint8))
    assert deg[0] == M and (deg[1:M + 1] == 1).all() and (deg[M + 1:] == 0).all()
    assert (n > 33) == bool((deg == 0).any())


@pytest.mark.parametrize("n,name", cases(N_ALL))
def test_plan_contract_matches_direct_count(n, name):
    partner = table(name, n)
    for f in flag_rounds(partner, n):
        active, n_remote, src, sw, _ = py_plan(f, partner, 0, n, ALPHA)
        assert active == int(f.any()) and n_remote == 0
        deg = degrees(partner, f) if f.any() else np.zeros(n, np.int64)
        for r in range(n):
            direct = [int(partner[g, r]) for g in range(partner.shape[0]) if f[g] and partner[g, r] >= 0]
            assert src[r] == direct and len(direct) == deg[r]
            assert sw[r] == F32(1.0 - deg[r] * ALPHA) and sw[r] >= 0.5


def test_flag_rounds():
    for n, name in cases(N_ALL):
        partner = table(name, n)
        f = flag_rounds(partner, 3)
        M = partner.shape[0]
        assert f.shape == (4, M) and f.dtype == np.uint8
        assert f[0].all() and f[1].any() and f[2].sum() == 1 and not f[3].any()
        pairs = (partner >= 0).sum(axis=1)
        assert pairs[int(np.argmax(f[2]))] == pairs.min()


@pytest.mark.parametrize("n,name", cases(N_ALL))
def test_bf16_spec_stays_finite(O, n, name):
    partner = table(name, n)
    rng = np.random.default_rng([n, len(name)])
    for idle in ("skip", "canonical"):
        X = bf16ref.random_bits(rng, (n, 129), specials=False)
        for k, f in enumerate(flag_rounds(partner, n)):
            Y = bf16ref.spec_round(O, X, partner, f, ALPHA, idle)
            assert np.isfinite(bf16ref.upcast(Y)).all()
            if k == 0 and n > 1:                   # (later rounds of two workers mix two equal rows)
                assert not np.array_equal(Y, X)    # the round did something
            X = Y


@pytest.mark.parametrize("n,name", cases(N_ALL))
def test_fused_specs_stay_finite(O, n, name):
    partner = table(name, n)
    flags = flag_rounds(partner, n)[[0, 1, 3]]
    P = 33
    rng = np.random.default_rng([n, len(name), 1])
    X = rng.standard_normal((n, P)).astype(F32)
    Gs = [(0.01 * rng.standard_normal((n, P))).astype(F32) for _ in range(3)]
    wd, mom, nest = SGD_HYPER
    table_ = adamref.bias_table(*ADAM_HYPER[:2])
    z = np.zeros((n, P), F32)
    sx, sm = X, z
    bx, bm = X, z
    ax, am, av = X, z, z
    cx, cm, cv = X, z, z
    for it in range(3):
        G, f = Gs[it], flags[it]
        Gb = bf16ref.rne_bf16(G)
        sx, sm, _ = sgdref.spec_round(O, sx, G, sm, partner, f, ALPHA, (LR, wd, mom, nest))
        bx, bm, bp, _ = sgdbf16ref.spec_round(O, bx, Gb, bm, partner, f, ALPHA, (LR, wd, mom, nest))
        ax, am, av, _ = adamref.spec_round(O, ax, G, am, av, it + 1, partner, f, ALPHA, LR, ADAM_HYPER, table_)
        cx, cm, cv, cp, _ = adambf16ref.spec_round(O, cx, Gb, cm, cv, it + 1, partner, f, ALPHA, LR, ADAM_HYPER,
                                                   table_)
        for a in (sx, sm, bx, bm, ax, am, av, cx, cm, cv, bf16ref.upcast(bp), bf16ref.upcast(cp)):
            assert np.isfinite(a).all(), (n, name, it)
