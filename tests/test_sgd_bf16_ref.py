"""tests/sgdbf16ref.py (the mixed-precision fused round's specification) on hand-computed cases, and the
new C ABI's host-only parts (tile, layout; the call record's layout is checked in tests/test_native_abi.py)
-- no GPU."""
import importlib

import numpy as np

import bf16ref
import sgdbf16ref


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def _b(bits):
    return np.array(bits, np.uint16)


def test_tie_rounds_to_even_at_the_bf16_store():
    """lr = 1, g = -2^-8 (bf16 0xBB80): w' = w + 2^-8, half a bf16 ulp of [1, 2).
    w = 1.0        -> w' = 0x3F808000, a tie between 0x3F80 (even) and 0x3F81: p = 0x3F80
    w = 1 + 2^-7   -> w' = 0x3F818000, a tie between 0x3F81 and 0x3F82 (even): p = 0x3F82"""
    w = _f([0x3F800000, 0x3F810000])
    wp, m, p = sgdbf16ref.sgd_only(w, _b([0xBB80, 0xBB80]), None, (1.0, 0.0, 0.0, False))
    assert m is None
    assert sgdbf16ref.u32(wp).tolist() == [0x3F808000, 0x3F818000]
    assert p.tolist() == [0x3F80, 0x3F82]


def test_master_low_bits_survive_a_step():
    """w = 1 + 2^-23 (0x3F800001), the same step: w' = 0x3F808001 keeps the low bit -- and that bit
    decides the store: just above the tie, p = 0x3F81 where the master 1.0 gave 0x3F80."""
    wp, _, p = sgdbf16ref.sgd_only(_f([0x3F800001]), _b([0xBB80]), None, (1.0, 0.0, 0.0, False))
    assert sgdbf16ref.u32(wp).tolist() == [0x3F808001] and p.tolist() == [0x3F81]
    # 2^-12 steps from 1.0: below half a bf16 ulp each, all kept by the master
    w = _f([0x3F800000])
    for k in range(1, 4):
        w, _, p = sgdbf16ref.sgd_only(w, _b([0x3F80]), None, (2.0 ** -12, 0.0, 0.0, False))
        assert float(w[0]) == 1.0 - k * 2.0 ** -12 and p.tolist() == [0x3F80]


def test_momentum_and_weight_decay_by_hand():
    """w = 2, g = 1 (0x3F80), m = 4, lr = 0.5, wd = 0.25, mom = 0.5 (all exact):
    d = 0.25 * 2 + 1 = 1.5;  m = 0.5 * 4 + 1.5 = 3.5;  nesterov: d = 0.5 * 3.5 + 1.5 = 3.25
    w' = 2 - 0.5 * 3.5 = 0.25 (0x3E80), with Nesterov 2 - 0.5 * 3.25 = 0.375 (0x3EC0)"""
    for nesterov, want_w, want_p in ((False, 0.25, 0x3E80), (True, 0.375, 0x3EC0)):
        wp, m, p = sgdbf16ref.sgd_only(np.float32([2.0]), _b([0x3F80]), np.float32([4.0]), (0.5, 0.25, 0.5, nesterov))
        assert float(wp[0]) == want_w and float(m[0]) == 3.5 and p.tolist() == [want_p]


def test_round_composes_the_fp32_round_and_one_rounding(O):
    """two workers, one matching, alpha = 0.25 (selfweight 0.75), no SGD motion (g = 0, wd = 0):
    w = (1 + 2^-8, 3) -> row 0 = 0.25 * 3 + 0.75 * (1 + 2^-8) = 1.5 + 3 * 2^-10 (exact in fp32),
    which is below half a bf16 ulp (2^-8) above 1.5: p = bf16(1.5) = 0x3FC0."""
    partner = np.array([[1, 0]], np.int32)
    w = np.array([[1 + 2.0 ** -8], [3.0]], np.float32)
    g = np.zeros((2, 1), np.uint16)
    out, m, p, wp = sgdbf16ref.spec_round(O, w, g, None, partner, [1], 0.25, (0.1, 0.0, 0.0, False))
    assert sgdbf16ref.eq32(wp, w) and float(out[0, 0]) == 1.5 + 3 * 2.0 ** -10 and int(p[0, 0]) == 0x3FC0
    assert float(bf16ref.upcast(p)[0, 0]) != float(out[0, 0])          # p is not the master
    # an all-zero round is the SGD step alone
    out0, _, p0, wp0 = sgdbf16ref.spec_round(O, w, g, None, partner, [0], 0.25, (0.1, 0.0, 0.0, False))
    assert sgdbf16ref.eq32(out0, wp0) and np.array_equal(p0, bf16ref.rne_bf16(w))


def test_abi_tile_and_layout(pkg):
    L = pkg.lib
    assert L.mx_sgd_mix_bf16_tile(64) > 0 and L.mx_sgd_mix_bf16_tile(65) == 0 and L.mx_sgd_mix_bf16_tile(0) == 0
    for n in (1, 8, 9, 16, 17, 32, 33, 64):
        assert L.mx_sgd_mix_bf16_tile(n) == L.mx_sgd_mix_tile(n)
    T = L.mx_sgd_mix_bf16_tile(3)
    seg = np.array([5, T + 3], np.int64)
    off = np.full(3, -1, np.int64)
    assert L.mx_sgd_mix_bf16_layout(seg.ctypes.data, 2, 3, off.ctypes.data) == 0
    assert off.tolist() == [0, 1, 3]
    assert L.mx_sgd_mix_bf16_layout(seg.ctypes.data, 2, 65, off.ctypes.data) == pkg._lib.MX_ERR_INVALID
    # the knobs exist, start at the fp32 kernel's defaults and refuse unknown names
    E = importlib.import_module(pkg.__name__ + ".engine")
    assert E.sgd_mix_bf16_tuning() == {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0}
    assert L.mx_sgd_mix_bf16_set(b"no_such_knob", 1) == pkg._lib.MX_ERR_INVALID
    assert L.mx_sgd_mix_bf16_get(b"no_such_knob") == pkg._lib.MX_ERR_INVALID
