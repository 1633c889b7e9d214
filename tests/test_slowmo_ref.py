"""The SlowMo outer step's numpy specification (tests/slowmoref.py) checked against facts that need no GPU, the
header's call record against the C compiler, and the entry points' refusals (nothing is launched)."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import slowmoref as S
from bf16ref import is_nan16, rne_bf16
from conftest import ROOT
from sgdref import is_nan32

F32 = np.float32


def _dyadic_rows(rng, n, P):
    """rows of multiples of n / 16: every partial sum, the sum and the mean are exact in fp32"""
    return (rng.integers(-64, 65, (n, P)) * n).astype(F32) / F32(16)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 12])
def test_beta0_alpha1_is_the_exact_average(n, order):
    """beta = 0, alpha = 1, lr a power of two, dyadic inputs whose mean is exact: a' == mean bit for bit"""
    rng = np.random.default_rng(10 * n + order)
    rows = _dyadic_rows(rng, n, 257)
    a = (rng.integers(-64, 65, 257)).astype(F32) / F32(8)
    mean = rows.astype(np.float64).mean(axis=0).astype(F32)
    assert np.array_equal(mean.astype(np.float64), rows.astype(np.float64).sum(axis=0) / n)     # exact
    for lr in (0.5, 0.125, 4.0):
        out, a2, u2, p = S.spec_step(rows, a, np.zeros(257, F32), lr, 1.0, 0.0, order)
        # -0.0 + 0.0 may differ in sign only where the mean is zero: compare values there, bits elsewhere
        nz = mean != 0
        assert np.array_equal(a2[nz].view(np.uint32), mean[nz].view(np.uint32)) and np.all(a2[~nz] == 0)
        assert np.array_equal(out, np.broadcast_to(a2, rows.shape)) and p is None
        assert np.array_equal(u2, ((a - mean) / F32(lr)).astype(F32))


def test_second_step_halves_the_first_momentum():
    """beta = 0.5: the second outer step's u is the first's halved, plus q (0.5 * u is exact, so the fma is
    one fp32 addition)"""
    rng = np.random.default_rng(3)
    n, P, lr, alpha = 8, 1000, 0.05, 0.7
    rows = rng.standard_normal((n, P)).astype(F32)
    a = rng.standard_normal(P).astype(F32)
    out1, a1, u1, _ = S.spec_step(rows, a, np.zeros(P, F32), lr, alpha, 0.5)
    assert np.array_equal(u1, ((a - S.mean_rows(rows, 0)) * (F32(1) / F32(lr))).astype(F32))      # u = 0: u' = q
    rows2 = out1 + rng.standard_normal((n, P)).astype(F32) * F32(0.01)
    _, a2, u2, _ = S.spec_step(rows2, a1, u1, lr, alpha, 0.5)
    q2 = ((a1 - S.mean_rows(rows2, 0)).astype(F32) * (F32(1) / F32(lr))).astype(F32)
    assert np.array_equal(u2.view(np.uint32), (F32(0.5) * u1 + q2).astype(F32).view(np.uint32))
    assert not np.array_equal(u2, q2)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_stays_in_its_column(bad):
    rng = np.random.default_rng(5)
    n, P = 5, 64
    rows = rng.standard_normal((n, P)).astype(F32)
    rows[3, 17] = bad
    a, u = rng.standard_normal(P).astype(F32), rng.standard_normal(P).astype(F32)
    out, a2, u2, p = S.spec_step(rows, a, u, 0.1, 1.0, 0.5, mixed=True)
    col = np.zeros(P, bool)
    col[17] = True
    for arr in (a2, u2) + tuple(out):
        assert np.array_equal(~np.isfinite(arr), col)
    assert np.array_equal(((p & 0x7F80) == 0x7F80), np.broadcast_to(col, p.shape))                # Inf or NaN in bf16
    if np.isnan(bad):
        assert is_nan32(a2)[17] and is_nan16(p)[:, 17].all()
    clean = rows.copy()
    clean[3, 17] = 0
    out0, a0, u0, p0 = S.spec_step(clean, a, u, 0.1, 1.0, 0.5, mixed=True)
    assert np.array_equal(out0[:, ~col], out[:, ~col]) and np.array_equal(u0[~col], u2[~col])
    assert np.array_equal(p0[:, ~col], p[:, ~col])


def test_zero_learning_rate_changes_nothing():
    rng = np.random.default_rng(6)
    rows, a, u = rng.standard_normal((4, 32)).astype(F32), rng.standard_normal(32).astype(F32), np.ones(32, F32)
    out, a2, u2, p = S.spec_step(rows, a, u, 0.0, 1.0, 0.5, mixed=True)
    assert np.array_equal(out, rows) and np.array_equal(a2, a) and np.array_equal(u2, u) and p is None


def test_image_is_the_rounded_common_point():
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((8, 100)).astype(F32)
    out, a2, _, p = S.spec_step(rows, rows[0], np.zeros(100, F32), 0.1, 1.0, 0.0, mixed=True)
    assert p.dtype == np.uint16 and np.array_equal(p, np.broadcast_to(rne_bf16(a2), p.shape))


def test_synced_rows_are_not_a_fixed_point_for_three_rows():
    """Documented behaviour, not a defect to work around: for n that is not a power of two the pinned-order mean
    of n identical values can differ from the value in the last place, so an outer step on a synced state
    (beta = 0, alpha = 1, lr = 1) moves some columns by an ulp; powers of two are exact fixed points in the tree
    order (in rank order only n <= 2 is: its partial sums 3 x, 5 x, ... round)."""
    rng = np.random.default_rng(8)
    x = rng.standard_normal(20000).astype(F32)
    moved = {}
    for n in (2, 3, 5, 6, 7, 8, 12, 16):
        rows = np.broadcast_to(x, (n, x.size))
        frac = {}
        for order in (0, 1):
            m = S.mean_rows(rows, order)
            frac[order] = float(np.mean(m != x))
            # n - 1 adds and a division, each within half an ulp: the standard bound n * 2^-24 * |x|
            assert np.all(np.abs(m.astype(np.float64) - x) <= n * 2.0 ** -24 * np.abs(x.astype(np.float64)))
        moved[n] = frac
    for n in (2, 8, 16):                 # the tree adds equal partial sums: every add doubles, exactly
        assert moved[n][0] == 0.0
    assert moved[2][1] == 0.0            # rank order: 3 x, 5 x, ... round, so only n <= 2 is exact there
    assert moved[8][1] > 0.05
    for n in (3, 5, 6, 7, 12):
        assert 0.05 < moved[n][0] < 0.30, (n, moved[n])
    rows = np.broadcast_to(x, (3, x.size))
    _, a2, u2, _ = S.spec_step(rows, x, np.zeros(x.size, F32), 1.0, 1.0, 0.0)
    drift = a2 != x
    assert 0.05 < drift.mean() < 0.30 and np.array_equal(drift, u2 != 0)


def _header_fields(struct):
    text = open(os.path.join(ROOT, "include", "matcha_gossip.h")).read()
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*[\s\*]", "", part.strip()) for part in decl.split(",")]
    return names


def test_call_struct_layout_matches_header(pkg, tmp_path):
    """the ctypes mirror has the header's fields, in its order, at the C compiler's offsets; sizeof == 72"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    fields = [f for f, _ in E.SlowmoCall._fields_]
    assert fields == _header_fields("mx_slowmo_call")
    assert fields == ["rows", "a", "u", "p", "ld", "p_ld", "count", "n_local", "order", "alpha", "beta"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "matcha_gossip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mx_slowmo_call));\n'
                   + "".join(f'  printf(" %zu", offsetof(mx_slowmo_call, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(E.SlowmoCall)] + [getattr(E.SlowmoCall, f).offset for f in fields]
    assert got == want and got[0] == 72
    assert "sizeof == 72" in open(os.path.join(ROOT, "include", "matcha_gossip.h")).read()


def _record(E, n=8, count=1000, ld=1024, order=0, alpha=1.0, beta=0.5, mixed=False, **over):
    """a record over fake, disjoint, aligned addresses (the refusals come before any launch or dereference)"""
    base = 1 << 30
    f = dict(rows=base, a=base + (1 << 28), u=base + (2 << 28), p=(base + (3 << 28)) if mixed else None, ld=ld,
             p_ld=ld, count=count, n_local=n, order=order, alpha=alpha, beta=beta)
    f.update(over)
    return E.SlowmoCall(*[f[k] for k, _ in E.SlowmoCall._fields_])


def test_symbols_knobs_and_kernel_names(pkg):
    E = importlib.import_module(pkg.__name__ + ".engine")
    lib = pkg.lib
    for name in ("mx_slowmo_step", "mx_slowmo_set", "mx_slowmo_get", "mx_slowmo_kernel_name"):
        assert name in pkg._lib.SIGNATURES and hasattr(lib, name)
    assert E.slowmo_tuning() == {"store_policy": 1, "wgpc": 3}
    try:
        E.set_slowmo_tuning(store_policy=3, wgpc=0)
        assert E.slowmo_tuning() == {"store_policy": 3, "wgpc": 0}
        for key, v in (("store_policy", 0), ("store_policy", 2), ("wgpc", -1), ("wgpc", 17), ("nope", 1)):
            assert lib.mx_slowmo_set(key.encode(), v) == pkg._lib.MX_ERR_INVALID
        assert lib.mx_slowmo_get(b"nope") < 0
        assert E.slowmo_tuning() == {"store_policy": 3, "wgpc": 0}
    finally:
        E.set_slowmo_tuning(store_policy=1, wgpc=3)
    names = {}
    for n in (1, 8, 9, 16, 17, 32, 33, 64):
        for order in (0, 1):
            for mixed in (False, True):
                rec = _record(E, n=n, order=order, mixed=mixed)
                names[n, order, mixed] = lib.mx_slowmo_kernel_name(ctypes.addressof(rec)).decode()
    assert names[1, 0, False] == names[8, 0, False] == "slowmo_tile<1, false>"
    assert names[8, 1, True] == "slowmo_tile<0, true>"
    assert names[9, 0, False] == names[16, 0, False] == "slowmo_rows<16, 4, 1, false>"
    assert names[17, 1, True] == names[32, 1, True] == "slowmo_rows<32, 2, 0, true>"
    assert names[33, 0, True] == names[64, 0, True] == "slowmo_rows<64, 1, 1, true>"
    bad = _record(E, n=65)
    assert lib.mx_slowmo_kernel_name(ctypes.addressof(bad)) == b"invalid"


ABI_REFUSALS = {
    "null rows": dict(rows=None),
    "null a": dict(a=None),
    "null u": dict(u=None),
    "n_local 0": dict(n=0),
    "n_local 65": dict(n=65),
    "ld < count": dict(ld=999),
    "count < 0": dict(count=-1),
    "order 2": dict(order=2),
    "order -1": dict(order=-1),
    "a in rows": dict(a=(1 << 30) + 4 * 1024 * 3),
    "u in rows": dict(u=(1 << 30) + 4 * (1024 * 7 + 999)),
    "a is u": dict(a=(1 << 30) + (2 << 28)),
    "a meets u": dict(u=(1 << 30) + (1 << 28) + 4 * 999),
    "a in p": dict(mixed=True, a=(1 << 30) + (3 << 28) + 2 * 1024),
    "u in p": dict(mixed=True, u=(1 << 30) + (3 << 28) + 2 * (1024 * 7 + 999)),
    "p_ld < count": dict(mixed=True, p_ld=999),
    "alpha 0": dict(alpha=0.0),
    "alpha < 0": dict(alpha=-1.0),
    "alpha inf": dict(alpha=float("inf")),
    "alpha nan": dict(alpha=float("nan")),
    "beta 1": dict(beta=1.0),
    "beta < 0": dict(beta=-0.1),
    "beta nan": dict(beta=float("nan")),
}


@pytest.mark.parametrize("case", sorted(ABI_REFUSALS))
def test_abi_refusals_launch_nothing(pkg, case):
    """MX_ERR_INVALID before any launch: the addresses are fake, so a launch (or a dereference) would not
    come back with a status"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    rec = _record(E, **ABI_REFUSALS[case])
    assert pkg.lib.mx_slowmo_step(ctypes.addressof(rec), 0.1, None, None) == pkg._lib.MX_ERR_INVALID, case
    assert b"mx_slowmo_step" in pkg.lib.mx_last_error()


@pytest.mark.parametrize("lr", [0.0, -0.1, float("inf"), float("nan")])
def test_abi_refuses_a_bad_host_learning_rate(pkg, lr):
    E = importlib.import_module(pkg.__name__ + ".engine")
    rec = _record(E)
    assert pkg.lib.mx_slowmo_step(ctypes.addressof(rec), lr, None, None) == pkg._lib.MX_ERR_INVALID
    assert pkg.lib.mx_slowmo_step(None, 0.1, None, None) == pkg._lib.MX_ERR_INVALID


def test_buffer_table_names_every_family(pkg):
    """the buffer strategy's table: one row per fused family; gradient tracking's tracker is not in it"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    assert set(E._SLOWMO_STATE) == set(E._GROUP_WORDS)
    assert E._SLOWMO_STATE["gt"] == E._SLOWMO_STATE["sgd"] == ("mom_arena",)
    assert E._SLOWMO_STATE["adamw"] == ("exp_avg_arena", "exp_avg_sq_arena")
    assert not any("tracker" in a or "prev" in a for v in E._SLOWMO_STATE.values() for a in v)
    assert E.SLOWMO_BUFFERS == ("maintain", "reset", "average")
