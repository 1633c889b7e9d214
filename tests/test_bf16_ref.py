"""bfloat16 rows, host side: the tests' round-to-nearest-even helper pinned to torch's CPU cast, and
the new C entry points' geometry and refusals (nothing here needs a GPU)."""
import ctypes

import numpy as np
import pytest

from bf16ref import is_nan16, rne_bf16, upcast

torch = pytest.importorskip("torch")


def _torch_bits(f):
    return torch.from_numpy(np.ascontiguousarray(f)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _f32(words):
    return np.array(words, np.uint32).view(np.float32)


def _check(f):
    got, want = rne_bf16(f), _torch_bits(f)
    nan = np.isnan(f)
    assert np.array_equal(got[~nan], want[~nan])
    assert is_nan16(got[nan]).all() and is_nan16(want[nan]).all()
    assert not is_nan16(got[~nan]).any()


def test_rne_helper_matches_torch_on_random_patterns():
    rng = np.random.default_rng(20261019)
    f = rng.integers(0, 1 << 32, 1_200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.isnan(f).sum() > 1000                       # NaN inputs are part of the sample
    _check(f)


def test_rne_helper_ties_overflow_and_specials():
    ties = _f32([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001])
    assert rne_bf16(ties).tolist() == [0x3F80, 0x3F82, 0x3F80, 0x3F81]   # to even, to even, down, up
    edge = _f32([0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0xFF7F8000])
    assert rne_bf16(edge).tolist() == [0x7F80, 0x7F7F, 0x7F80, 0xFF80]   # +Inf, max, +Inf, -Inf
    sub = _f32([0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807F8000, 0x00400000, 0x80000001])
    zeros_inf = _f32([0x00000000, 0x80000000, 0x7F800000, 0xFF800000])
    assert rne_bf16(zeros_inf).tolist() == [0x0000, 0x8000, 0x7F80, 0xFF80]
    nans = _f32([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFF8000, 0xFFFF8000, 0x7FFFFFFF, 0xFFFFFFFF])
    assert is_nan16(rne_bf16(nans)).all()                 # the bare integer formula would give -0 / +0 here
    _check(np.concatenate([ties, edge, sub, zeros_inf, nans]))


def test_upcast_is_exact_and_round_trips():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    f = upcast(bits)
    assert np.array_equal(f.view(np.uint32), bits.astype(np.uint32) << 16)
    back = rne_bf16(f)
    keep = ~is_nan16(bits)
    assert np.array_equal(back[keep], bits[keep]) and is_nan16(back[~keep]).all()


NEW_SYMBOLS = ("mx_mix_bf16_tile", "mx_mix_bf16_layout", "mx_gossip_mix_bf16_packed", "mx_gossip_mix_bf16_at")


def test_bf16_symbols_exported(pkg):
    so = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name
        assert name in pkg._lib.SIGNATURES, name


def _tile(n_slots):
    """twice the fp32 classes' columns (1024 / 1024 / 512 / 256) in the same LDS bytes"""
    for cap, tile in ((8, 2048), (16, 2048), (32, 1024), (64, 512)):
        if 1 <= n_slots <= cap:
            return tile
    return 0


def test_bf16_tile_and_layout(pkg):
    L = pkg.lib
    lens = np.array([0, 1, 511, 512, 513, 2048, 2049, 5, 6149], np.int64)
    for ns in (1, 8, 9, 16, 33, 64):
        tile = _tile(ns)
        assert L.mx_mix_bf16_tile(ns) == tile and tile > 0
        off = np.zeros(len(lens) + 1, np.int64)
        assert L.mx_mix_bf16_layout(lens.ctypes.data, len(lens), ns, off.ctypes.data) == 0
        assert off.tolist() == np.concatenate([[0], np.cumsum(-(-lens // tile))]).tolist()
    assert L.mx_mix_bf16_tile(65) == 0 and L.mx_mix_bf16_tile(0) == 0
    off = np.zeros(len(lens) + 1, np.int64)
    assert L.mx_mix_bf16_layout(lens.ctypes.data, len(lens), 65, off.ctypes.data) == -1
    assert b"65" in L.mx_last_error()


def test_bf16_mix_refuses_before_launching(pkg):
    """n_slots > 64, M > 32 and n_slots != n_local come back as MX_ERR_INVALID with a message; the
    pointers are fake device addresses, so a launch would not go unnoticed."""
    L, E = pkg.lib, pkg.engine
    fake = 1 << 40

    def packed(n_slots, n_local, M):
        c = E.MixCall(fake, fake, fake, fake, fake, 4, 1, n_slots, n_local, M, 0.25, 0, None, 0)
        return L.mx_gossip_mix_bf16_packed(ctypes.addressof(c), 0, None)

    assert packed(65, 65, 5) == -1 and b"exceeds 64" in L.mx_last_error()
    assert packed(8, 8, 33) == -1 and b"M=33" in L.mx_last_error()
    assert packed(9, 8, 5) == -1 and b"receive slots" in L.mx_last_error()
    assert L.mx_gossip_mix_bf16_packed(None, 0, None) == -1
    at = L.mx_gossip_mix_bf16_at
    assert at(fake, fake, fake, fake, 1, 4, 9, fake, fake, 10, 8, 5, 0.25, None) == -1
    assert b"receive slots" in L.mx_last_error()
    assert at(fake, fake, fake, fake, 1, 4, 8, fake, None, 10, 8, 5, 0.25, None) == -1
    assert b"counter" in L.mx_last_error()
    assert L.mx_mix_bf16_set(b"nope", 1) == -1 and L.mx_mix_bf16_get(b"nope") == -1
    # the fused rounds' store_policy is no knob of the bf16 mixing round
    assert L.mx_mix_bf16_set(b"store_policy", 1) == -1 and L.mx_mix_bf16_get(b"store_policy") == -1
    assert L.mx_mix_bf16_get(b"nontemporal") == 2 and L.mx_mix_bf16_get(b"wgpc") >= 0
