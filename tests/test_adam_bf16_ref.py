"""tests/adambf16ref.py (the mixed-precision fused AdamW round's specification) on a closed-form case and
against torch.optim.AdamW / Adam on fp32 masters fed g.float(), and the new C ABI's host-only parts (tile,
layout, knobs; the call record's layout is checked in tests/test_native_abi.py) -- no GPU."""
import importlib

import numpy as np
import pytest

import adambf16ref
import bf16ref
from adamref import bias_table
from sgdref import F32

# beta1, beta2, eps, wd, decoupled
HYPERS = {"adamw": (0.9, 0.999, 1e-8, 1e-2, True), "adam_l2": (0.9, 0.999, 1e-8, 5e-4, False),
          "adam_plain": (0.9, 0.999, 1e-8, 0.0, False)}
_TABLES = {}


def _table(b1, b2):
    if (b1, b2) not in _TABLES:
        _TABLES[(b1, b2)] = bias_table(b1, b2)
    return _TABLES[(b1, b2)]


def accumulation_spec(steps=64):
    """betas (0.9, 0.999), eps 1e-8, wd 0, lr = 2^-12, master 1.0, gradient bf16(1.0), the optimizer
    step alone: [(w, p_bits)] after each of `steps` steps, by the specification."""
    hyper = (0.9, 0.999, 1e-8, 0.0, True)
    table = _table(0.9, 0.999)
    w, m, v = np.ones(1, F32), np.zeros(1, F32), np.zeros(1, F32)
    g = np.array([0x3F80], np.uint16)
    out = []
    for t in range(1, steps + 1):
        w, m, v, p = adambf16ref.adam_only(w, g, m, v, t, 2.0 ** -12, hyper, table)
        out.append((float(w[0]), int(p[0])))
    return out


def test_small_updates_accumulate_in_the_master():
    """With a constant gradient Adam's bias-corrected step is lr * 1 / (1 + eps) = 2^-12 up to a few
    parts in 2^-24 of itself, far below half an ulp (2^-25) of a master in [0.5, 1): every step takes
    exactly 2^-12 off the master.  p = bf16_rne(w) stays 0x3F80 through step 8 (w = 1 - 2^-9 is the tie
    between 0x3F7F and 0x3F80 and goes to the even 0x3F80), is 0x3F7F at step 9 and 0x3F7C
    (0.984375 = 1 - 2^-6) at step 64.  A pure-bf16 recurrence, which re-rounds the weight every step,
    holds 1.0 for ever: bf16(1 - 2^-12) = 1.0."""
    seq = accumulation_spec(64)
    for t, (w, p) in enumerate(seq, 1):
        assert w == 1.0 - t * 2.0 ** -12, t
        assert p == (0x3F80 if t <= 8 else bf16ref.rne_bf16(np.float32([w]))[0]), t
    assert seq[8][1] == 0x3F7F and seq[63][1] == 0x3F7C and seq[63][0] == 0.984375
    assert bf16ref.rne_bf16(np.float32([1.0 - 2.0 ** -12]))[0] == 0x3F80


@pytest.mark.parametrize("name", sorted(HYPERS))
def test_spec_against_torch_on_fp32_masters(name):
    """5 steps of torch.optim.AdamW / Adam on CPU fp32 masters fed g.float(), 8 x 4097, masters uniform
    in [-1, 1), bf16 gradients ~ 0.01 N(0, 1), lr 1e-3: |w - torch| <= 2^-22, tests/test_adam_ref.py's
    bound (g.float() is exact, so the master arithmetic is the fp32 specification's).  p equals torch's
    .to(torch.bfloat16) of the SPECIFICATION's masters exactly: one rounding to nearest even."""
    torch = pytest.importorskip("torch")
    b1, b2, eps, wd, decoupled = HYPERS[name]
    rng = np.random.default_rng(12)
    n, P, lr = 8, 4097, 1e-3
    w = rng.uniform(-1, 1, (n, P)).astype(F32)
    m, v = np.zeros((n, P), F32), np.zeros((n, P), F32)
    param = torch.nn.Parameter(torch.from_numpy(w.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    table = _table(b1, b2)
    for step in range(1, 6):
        g = bf16ref.rne_bf16((0.01 * rng.standard_normal((n, P))).astype(F32))
        gbf = torch.from_numpy(g.view(np.int16).copy()).view(torch.bfloat16)
        param.grad = gbf.float()
        opt.step()
        w, m, v, p = adambf16ref.adam_only(w, g, m, v, step, lr, HYPERS[name], table)
        d = float(np.abs(param.detach().numpy().astype(np.float64) - w).max())
        print(f"{name} step {step}: max |w - torch| = {d:.3e} ({d * 2 ** 23:.2f} x 2^-23)")
        assert d <= 2.0 ** -22, step
        cast = torch.from_numpy(w.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(p, cast), step
    assert np.abs(w).max() < 1.01
    assert not np.array_equal(adambf16ref.u32(bf16ref.upcast(p)), adambf16ref.u32(w))   # p is not the master


def test_abi_tile_layout_and_knobs(pkg):
    L, INVALID = pkg.lib, pkg._lib.MX_ERR_INVALID
    assert [L.mx_adamw_mix_bf16_tile(n) for n in (8, 16, 32, 64, 65)] == [1024, 1024, 512, 256, 0]
    assert L.mx_adamw_mix_bf16_tile(0) == 0
    for n in (1, 8, 9, 16, 17, 32, 33, 64):
        assert L.mx_adamw_mix_bf16_tile(n) == L.mx_adamw_mix_tile(n)
    T = L.mx_adamw_mix_bf16_tile(3)
    seg = np.array([5, T + 3], np.int64)
    off = np.full(3, -1, np.int64)
    assert L.mx_adamw_mix_bf16_layout(seg.ctypes.data, 2, 3, off.ctypes.data) == 0
    assert off.tolist() == [0, 1, 3]
    assert L.mx_adamw_mix_bf16_layout(seg.ctypes.data, 2, 65, off.ctypes.data) == INVALID
    # the knobs: the fp32 kernel's defaults, a set / get round trip, independent of the other kernels'
    E = importlib.import_module(pkg.__name__ + ".engine")
    default = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0}
    assert E.adamw_mix_bf16_tuning() == default
    try:
        E.set_adamw_mix_bf16_tuning(nontemporal=0, wgpc=5, blocks_per_cu=4, flat_small=7, grid=3)
        assert E.adamw_mix_bf16_tuning() == {"nontemporal": 0, "wgpc": 5, "blocks_per_cu": 4, "flat_small": 7,
                                             "grid": 3}
        assert E.adamw_mix_tuning() == default and E.sgd_mix_bf16_tuning() == default
    finally:
        E.set_adamw_mix_bf16_tuning(**default)
    assert E.adamw_mix_bf16_tuning() == default
    assert L.mx_adamw_mix_bf16_set(b"wgpc", 33) == INVALID
    assert L.mx_adamw_mix_bf16_set(b"no_such_knob", 1) == INVALID
    assert L.mx_adamw_mix_bf16_get(b"no_such_knob") == INVALID
    # a null call record is refused before anything touches a device
    assert L.mx_adamw_mix_bf16(None, 0, 1, 1e-3, None, None) == INVALID
    assert L.mx_adamw_mix_bf16_at(None, None, 1, None, 1e-3, None, None) == INVALID
