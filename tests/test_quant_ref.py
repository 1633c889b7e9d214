"""tests/quantref.py against hand-computed cases: the clamp bucket, the packing, the slot, a convergence run"""
import numpy as np
import pytest

import quantref
from signref import consensus_distance
from test_choco_sign_ref import _ring8

F32 = np.float32
BITS = pytest.mark.parametrize("bits", [4, 8])


@BITS
def test_one_nonzero_element_has_level_s_for_every_xi(bits):
    """|d| inv = s exactly, so v is in [s, s + 1) and rounds up to s + 1 for xi = 0.99999994: the clamp holds it"""
    s, c = quantref.consts(bits)
    assert (s, float(c)) == {4: (7, float(F32(1 / (7 * (1 + 16 / 7))))), 8: (127, float(F32(1 / (127 * (1 + 256 / 127 ** 2)))))}[bits]
    d = np.zeros(300, F32)
    d[5], d[290] = -3.0, 2.0 ** -100
    for rnd in range(50):
        norm, code, q = quantref.quantize(d, bits, 1, rnd, 2)
        assert norm.tolist() == [3.0, 2.0 ** -100]
        want = np.zeros(512, np.uint8)
        want[5], want[290] = s | (1 << (bits - 1)), s
        assert np.array_equal(code, want)
        assert q[5] == -F32(s) * (F32(3.0) * c) and q[290] == F32(s) * (F32(2.0 ** -100) * c) and not q[:5].any()
    assert F32(s) + F32(1 - 2.0 ** -24) == s + 1                              # the largest xi: the sum rounds up


@BITS
def test_packing_and_slot(bits):
    code = (np.arange(512) * 37 % (1 << bits)).astype(np.uint8)
    packed = quantref.pack(code, bits)
    assert packed.size == 512 * bits // 8 and np.array_equal(quantref.unpack(packed, bits), code)
    assert bits == 8 or packed[0] == code[0] | code[1] << 4                    # 4 bits: the even column low
    assert [quantref.msg_bytes(P, bits) for P in (1, 256, 257, 4096, 4097)] == \
        [128 + 32 * bits * nb + 64 * (nb > 16) for nb in (1, 1, 2, 16, 17)]
    sl = quantref.slot(300, bits, np.array([3.0, 1.0], F32), code)
    assert sl.size == 128 + 64 * bits and sl[16] == 44 and sl[17] == 1 and sl[24] == bits and sl[29] == 1
    assert np.array_equal(sl[64:72].view(F32), [3.0, 1.0]) and not sl[72:128].any() and np.array_equal(sl[128:], packed)


@BITS
def test_convergence_on_a_ring_of_eight(bits):
    """200 rounds: below 0.01 of the start (a float64-state simulation gave 8e-5 at 4 bits, 2e-4 at 8); no drift"""
    X = np.random.default_rng(0).standard_normal((8, 1000)).astype(F32)
    XH, S = np.zeros_like(X), np.zeros_like(X)
    d0, mean0 = consensus_distance(X), X.astype(np.float64).mean(0)
    for t in range(200):
        quantref.quant_round(X, XH, S, _ring8(), [1, 1], 1 / 3, 0.2, bits, 0, t)
    ratio = consensus_distance(X) / d0
    assert ratio < 0.01
    assert np.abs(X.astype(np.float64).mean(0) - mean0).max() < 1e-3
