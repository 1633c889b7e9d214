"""tests/lionref.py against exact arithmetic, the Lion call records against the header, and attach_lion's
argument errors -- none of it needs a GPU."""
import ctypes
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import lionref
from conftest import ROOT
from sgdref import fmaf_fraction
from test_native_abi import _Addr, _Engine, _header_fields

F32 = np.float32
NZ = F32(-0.0)


def _mul(a, b):
    return fmaf_fraction(a, b, NZ)               # a * b + (-0): the product's own sign survives an exact zero


def _sub(a, b):
    return fmaf_fraction(F32(1.0), a, -F32(b))


def _exact_lion(x, g, m, lr, wd, betas):
    """one finite element by fractions.Fraction alone: every line the float32 nearest its exact value"""
    lr, wd = F32(lr), F32(wd)
    omb1, omb2 = F32(1.0 - float(betas[0])), F32(1.0 - float(betas[1]))
    x1 = _mul(x, fmaf_fraction(-lr, wd, F32(1.0))) if wd != 0 else F32(x)
    dm = _sub(g, m)
    c = fmaf_fraction(omb1, dm, m)
    sign = Fraction(float(omb1)) * Fraction(float(dm)) + Fraction(float(m))          # the sign of the exact direction
    assert (c > 0) == (sign > 0) or c == 0       # rounding keeps the sign (it may underflow to a zero)
    if c > 0:
        xp = _sub(x1, lr)
    elif c < 0:
        xp = fmaf_fraction(F32(1.0), x1, lr)
    else:
        xp = x1
    return xp, fmaf_fraction(omb2, dm, m)


@pytest.mark.parametrize("hyper", [(0.9, 0.99, 0.0), (0.9, 0.99, 1e-2), (0.95, 0.98, 0.1)])
def test_lion_ref_is_exactly_rounded(hyper):
    b1, b2, wd = hyper
    rng = np.random.default_rng(int(1000 * b1))
    n = 300
    x = rng.standard_normal(n).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(F32)
    m = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(F32)
    g[:30] = 0.0                                 # c exactly zero: g = m = 0 ...
    m[:30] = 0.0
    x[5:10] = NZ                                 # ... under x = -0.0 too
    g[25:30] = NZ                                # a gradient of -0.0: dm = -0, c = fmaf(omb1, -0, 0) = +0
    g[30:40] = m[30:40]                          # g = m != 0: dm = +0, c = m, m' = m
    x[40:45] = NZ                                # x = -0.0 on a non-zero direction
    lr = 3e-4
    xp, m2 = lionref.lion_ref(x, g, m, lr, wd, (b1, b2))
    zero_c = 0
    for i in range(n):
        ex, em = _exact_lion(x[i], g[i], m[i], lr, wd, (b1, b2))
        assert F32(xp[i]).view(np.uint32) == F32(ex).view(np.uint32), (i, x[i], g[i], m[i], xp[i], ex)
        assert F32(m2[i]).view(np.uint32) == F32(em).view(np.uint32), (i, x[i], g[i], m[i], m2[i], em)
        if g[i] == 0 and m[i] == 0:
            zero_c += 1
            x1 = x[i] if wd == 0 else _mul(x[i], fmaf_fraction(-F32(lr), F32(wd), F32(1.0)))
            assert xp[i].view(np.uint32) == F32(x1).view(np.uint32)
            if i in range(5, 10):
                assert xp[i].view(np.uint32) == 0x80000000
    assert zero_c == 30 and lionref.eq32(m2[30:40], m[30:40])
    # a zero direction keeps -0.0 with and without decay; a NaN direction gives a NaN
    keep, _ = lionref.lion_ref(np.array([NZ]), np.array([0.0]), np.array([0.0]), lr, wd, (b1, b2))
    assert keep.view(np.uint32)[0] == 0x80000000
    bad, mb = lionref.lion_ref(np.array([1.0]), np.array([np.nan]), np.array([0.0]), lr, wd, (b1, b2))
    assert np.isnan(bad[0]) and np.isnan(mb[0])


def test_grouped_clipped_and_bf16_forms_compose():
    """the run and clip forms are lion_ref on slices of the scaled gradient; the bf16 momentum is widened
    and rounded once"""
    import bf16ref
    rng = np.random.default_rng(3)
    n, P = 3, 40
    x, g, m = (rng.standard_normal((n, P)).astype(F32) for _ in range(3))
    scale = np.array([1.0, 0.25, 0.5], F32)
    runs = [(0, 7, 0.0, 1.0), (7, 8, 0.1, 0.5), (8, 40, 0.01, 0.0)]
    xp, m2 = lionref.lion_update(x, g, m, 1e-3, 0.3, (0.9, 0.99), scale, runs)
    gs = (scale[:, None] * g).astype(F32)
    for a, b, wd, s in runs:
        ex, em = lionref.lion_ref(x[:, a:b], gs[:, a:b], m[:, a:b], F32(F32(1e-3) * F32(s)), wd, (0.9, 0.99))
        assert lionref.eq32(xp[:, a:b], ex) and lionref.eq32(m2[:, a:b], em)
    assert lionref.eq32(xp[:, 8:], x[:, 8:] * F32(1.0))              # lr_scale 0: decay 1, step 0
    mb = bf16ref.rne_bf16(m)
    gb = bf16ref.rne_bf16(g)
    flags = np.zeros(2, np.uint8)
    w_out, mo, p, wp = lionref.spec_round_bf16(None, x, gb, mb, np.zeros((2, n), np.int32), flags, 0.5, 1e-3,
                                               (0.9, 0.99, 0.0), m_bf16=True)
    ex, em = lionref.lion_ref(x, bf16ref.upcast(gb), bf16ref.upcast(mb), 1e-3, 0.0, (0.9, 0.99))
    assert lionref.eq32(w_out, ex) and lionref.eq32(wp, ex) and mo.dtype == np.uint16
    assert np.array_equal(mo, bf16ref.rne_bf16(em)) and np.array_equal(p, bf16ref.rne_bf16(ex))


LION_RECORDS = {"mx_lion_mix_call": ("LionMixCall", 96), "mx_lion_mix_bf16_call": ("LionBf16Call", 104)}


@pytest.mark.parametrize("struct", sorted(LION_RECORDS))
def test_lion_call_struct_layout_matches_header(pkg, tmp_path, struct):
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, LION_RECORDS[struct][0])
    fields = [f for f, _ in cls._fields_]
    assert fields == _header_fields(struct)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "matcha_gossip.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({struct}));\n'
                   + "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want and got[0] == LION_RECORDS[struct][1]


@pytest.mark.parametrize("family,m_bf16", [("LionLayout", None), ("LionBf16Layout", False), ("LionBf16Layout", True)])
def test_lion_call_records_are_packed_as_specified(pkg, family, m_bf16):
    """layout.call(engine, ...) of the two Lion layouts over distinct fake addresses, as test_native_abi's
    check of the other four: every pointer table in its own field, the engine's geometry, fp32 roundings
    with omb1 / omb2 rounded from the fp64 1 - beta, flags 0 or 1 for any truthy input."""
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, family)
    fam = cls.family
    assert fam is E.FAMILIES["lion", "Bf16" in family] and not fam.adam and fam.optional is None
    assert fam.tables == (("w", "g", "m", "p") if "Bf16" in family else ("x", "g", "m"))

    def f32(v):
        return float(F32(v))

    lay = object.__new__(cls)
    want, k = {}, 1 << 40
    for t in fam.tables + ("seg_len", "tile_off"):
        k += 1
        name = t + "_ptrs" if t in fam.tables else t
        setattr(lay, name, _Addr(k))
        want[name + "_dev"] = k
    lay.total_tiles, lay.nseg, lay.n_local, lay.n_bias, lay.bias = 77, 3, 64, 0, None
    want.update(plan_dev=_Engine._plan_ptr, total_tiles=77, nseg=3, n_slots=9, n_local=8, M=5, alpha=_Engine.alpha32,
                wd=f32(0.1), omb1=f32(1.0 - 0.9), omb2=f32(1.0 - 0.99), zero_grads=1)
    if m_bf16 is None:
        call = lay.call(_Engine, (0.9, 0.99), 0.1, "x")
        want.update(pad_=0)
    else:
        call = lay.call(_Engine, (0.9, 0.99), 0.1, 2, "y" if m_bf16 else "")
        want.update(m_bf16=int(m_bf16))
    assert type(call) is fam.rec
    assert {f: getattr(call, f) for f, _ in fam.rec._fields_} == want
    assert f32(1.0 - 0.99) != f32(1 - f32(0.99))                     # the roundings differ
    assert lay.call(_Engine, (0.9, 0.99), 0.1, 0).zero_grads == 0
    assert E.lion_hyper((0.9, 0.99), 0.1, True) == (f32(0.1), f32(1.0 - 0.9), f32(1.0 - 0.99), 1, 0)
    assert E.lion_hyper((0.9, 0.99), 0.1, 0, True)[3:] == (0, 1)


def test_lion_symbols_and_knobs(pkg):
    """the twenty entry points are in the ctypes table with the SGD families' signatures, and the knobs are
    the family's own"""
    S = pkg._lib.SIGNATURES
    for base, twin in (("mx_lion_mix", "mx_sgd_mix"), ("mx_lion_mix_bf16", "mx_sgd_mix_bf16")):
        for suffix in pkg.engine._FUSED_ENTRIES:
            assert S[base + suffix] == S[twin + suffix], base + suffix
        assert getattr(pkg.lib, base + "_tile")(8) == 1024 and getattr(pkg.lib, base + "_tile")(65) == 0
    E = pkg.engine
    assert E.lion_mix_tuning() == E.lion_mix_bf16_tuning() == {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2,
                                                                "flat_small": 256, "grid": 0}
    try:
        E.set_lion_mix_tuning(grid=3)
        assert E.lion_mix_tuning()["grid"] == 3 and E.lion_mix_bf16_tuning()["grid"] == 0
        assert E.sgd_mix_tuning()["grid"] == 0
    finally:
        E.set_lion_mix_tuning(grid=0)
    assert pkg.lib.mx_lion_mix(None, 0, 0.1, None, None) == pkg._lib.MX_ERR_INVALID
    assert b"mx_lion_mix:" in pkg.lib.mx_last_error()


def test_attach_lion_argument_errors(pkg):
    """attach_lion's own checks are a host function (engine.lion_arguments)"""
    import torch
    E = pkg.engine
    assert E.lion_arguments((0.9, 0.99), 0.0, torch.float32, False) == ((0.9, 0.99), 0.0, False)
    assert E.lion_arguments((0, 0.5), 1, torch.bfloat16, True) == ((0.0, 0.5), 1.0, True)
    for betas in ((1.0, 0.99), (0.9, 1.0), (-0.1, 0.99), (0.9, 1.5), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="betas"):
            E.lion_arguments(betas, 0.0, torch.float32, False)
    for wd in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="weight_decay"):
            E.lion_arguments((0.9, 0.99), wd, torch.float32, False)
    for dt in (torch.float16, torch.float64, None):
        with pytest.raises(ValueError, match="momentum_dtype"):
            E.lion_arguments((0.9, 0.99), 0.0, dt, True)
    with pytest.raises(ValueError, match="bfloat16 momentum"):
        E.lion_arguments((0.9, 0.99), 0.0, torch.bfloat16, False)
    words = E._OPTIMIZER_WORDS
    assert set(words) == {"sgd", "adamw", "lion"} and words["lion"][0] == "Lion"
    assert words["sgd"][1] == "adamw" and words["adamw"][1] == "sgd"
