"""The scaled-sign specification (tests/signref.py) against itself, on the CPU: the scale against a plain
mean of magnitudes, the bits against d < 0, the conventions for zeros and NaN, and a convergence sanity run."""
import numpy as np

import signref
from clipref import ulp_diff

F32 = np.float32


def test_scale_is_the_mean_magnitude_and_bits_are_the_signs():
    rng = np.random.default_rng(3)
    for P in (1, 7, 64, 65, 1000, 4097):
        d = rng.standard_normal(P).astype(F32)
        scale, bits = signref.sign_message(d)
        assert scale.dtype == F32 and bits.dtype == np.uint8 and bits.size == (P + 7) // 8
        assert ulp_diff(scale, F32(np.abs(d).astype(np.float64).mean())) <= 1, P
        assert np.array_equal(signref.unpack(bits, P), d < 0), P
        pad = np.unpackbits(bits, bitorder="little")[P:]
        assert not pad.any(), P                              # padding bits zero
        q = signref.dense(scale, signref.unpack(bits, P))
        assert np.array_equal(q, np.where(d < 0, -scale, scale).astype(F32))
    assert signref.msg_bytes(1) == 72 and signref.msg_bytes(64) == 72 and signref.msg_bytes(65) == 80
    assert signref.msg_bytes(4097) == 64 + 8 * 65


def test_zeros_and_nan_travel_as_plus_scale():
    d = np.array([0.0, -0.0, np.nan, -1.0, 2.0, -np.float32(1e-42)], F32)
    d[2] = np.array([0xFFC00001], np.uint32).view(F32)[0]        # a NaN with the sign bit set is still not < 0
    scale, bits = signref.sign_message(d)
    assert np.array_equal(signref.unpack(bits, d.size), [False, False, False, True, False, True])
    assert np.isnan(scale)
    d[2] = 0.0
    scale, _ = signref.sign_message(d)
    assert scale == F32((1.0 + 2.0 + float(F32(1e-42))) / 6.0)
    scale, _ = signref.sign_message(np.array([np.inf, -1.0], F32))
    assert np.isinf(scale) and scale > 0
    scale, bits = signref.sign_message(np.zeros(5, F32))
    assert scale == 0 and not np.signbit(scale) and not bits.any()


def test_round_without_active_matching_applies_the_own_message():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((2, 9)).astype(F32)
    XH, S = np.zeros_like(X), np.zeros_like(X)
    X0 = X.copy()
    sc, neg = signref.sign_round(X, XH, S, [[1, 0]], [0], 0.5, 0.25)
    q = np.stack([signref.dense(sc[i], neg[i]) for i in range(2)])
    assert np.array_equal(XH, q) and np.array_equal(S, q)      # self weight 1
    # x + g s - g x_hat with s == x_hat: x again, up to the two fmas' roundings (half an ulp of |x| < 8 each)
    assert np.abs(X - X0).max() <= 2.0 ** -21
    sc2, _ = signref.sign_round(X.copy(), XH.copy(), S.copy(), [[1, 0]], [1], 0.5, 0.25, scale=[3.0, 4.0])
    assert sc2.tolist() == [3.0, 4.0]


def _ring8():
    """a ring of 8 as two perfect matchings"""
    a = [i + 1 if i % 2 == 0 else i - 1 for i in range(8)]                  # 0-1, 2-3, 4-5, 6-7
    b = [(i - 1) % 8 if i % 2 == 0 else (i + 1) % 8 for i in range(8)]      # 1-2, 3-4, 5-6, 7-0
    return [a, b]


def test_convergence_on_a_ring_of_eight():
    """Ring of 8 (two perfect matchings, both active), alpha = 1/3, gamma = 0.1, P = 1000, standard-normal
    rows (seed 0), 200 rounds: the consensus distance falls below a tenth of its start (measured: 0.026 of
    it) and the mean row does not move (measured: 7e-6 in max-norm)."""
    partner = _ring8()
    for i in range(8):
        for m in range(2):
            assert partner[m][partner[m][i]] == i
    X = np.random.default_rng(0).standard_normal((8, 1000)).astype(F32)
    XH, S = np.zeros_like(X), np.zeros_like(X)
    d0, mean0 = signref.consensus_distance(X), X.astype(np.float64).mean(0)
    for _ in range(200):
        signref.sign_round(X, XH, S, partner, [1, 1], 1 / 3, 0.1)
    ratio = signref.consensus_distance(X) / d0
    drift = np.abs(X.astype(np.float64).mean(0) - mean0).max()
    print(f"consensus distance ratio {ratio:.4f}, mean drift {drift:.2e}")
    assert ratio < 0.1
    assert drift < 1e-3
