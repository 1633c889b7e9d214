"""tests/gtref.py, gradient tracking's specification, against a direct evaluation with exact arithmetic rounded once
per line, against the tracking invariant where fp32 is exact, and against the property the algorithm exists for
(it removes D-SGD's heterogeneity error); the call records against the header, the symbols, and attach_gt's
argument errors -- none of it needs a GPU."""
import ctypes
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bf16ref
import clipref
import groupref
import gtref
import sgdref
from conftest import ROOT
from lionkit import flag_kinds
from test_native_abi import _Addr, _Engine, _header_fields

F32 = np.float32
_IDX = np.arange(8)
RING8 = np.stack([_IDX ^ 1, np.where(_IDX & 1, (_IDX + 1) % 8, (_IDX - 1) % 8)]).astype(np.int32)   # ring32's construction


def _round32(exact):
    """the float32 nearest an exact Fraction, ties to even: float() rounds a Fraction correctly to fp64, and the
    two fp32 neighbours of that are compared exactly"""
    near = F32(float(exact))
    cands = (np.nextafter(near, F32(-np.inf)), near, np.nextafter(near, F32(np.inf)))
    return F32(min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(np.array(c, F32).view(np.uint32)) & 1)))


def _line(f, *arrays):
    """one line of the contract on every element: f on exact Fractions, rounded to fp32 once"""
    arrays = [np.asarray(a, F32) for a in arrays]
    out = np.empty(arrays[0].shape, F32)
    for i in np.ndindex(out.shape):
        out[i] = _round32(f(*[Fraction(float(a[i])) for a in arrays]))
    return out


def _mix_direct(v, partner, flags, alpha):
    """the round, line for line: partners in ascending matching order, the self term last, every step one fma"""
    a32 = Fraction(float(F32(alpha)))
    out = np.empty_like(v)
    for i in range(v.shape[0]):
        acc, deg = np.zeros(v.shape[1], F32), 0
        for gi in range(partner.shape[0]):
            j = partner[gi, i]
            if flags[gi] and j >= 0:
                acc = _line(lambda x, y: a32 * x + y, v[j], acc)
                deg += 1
        sw = Fraction(float(F32(1.0 - deg * float(alpha))))
        out[i] = _line(lambda x, y: sw * x + y, v[i], acc)
    return out


def test_track_and_step_equal_a_direct_evaluation(O):
    """(a) one track-and-step on random data, with momentum, Nesterov, decay, clip factors and bfloat16 gradients:
    every line of the contract evaluated exactly and rounded to fp32 once"""
    rng = np.random.default_rng(5)
    n, P, alpha, lr = 8, 16, 1.0 / 3.0, 0.05
    wd, mom = 0.01, 0.9
    fl = np.array([1, 1], np.uint8)
    x, y, gp, m = (rng.standard_normal((n, P)).astype(F32) for _ in range(4))
    gb = bf16ref.rne_bf16(rng.standard_normal((n, P)).astype(F32))
    scale = rng.uniform(0.1, 1.0, n).astype(F32)
    s = {"x": x, "y": y, "gp": gp, "m": m}
    got = gtref.spec_round(O, s, gb, RING8, fl, alpha, lr, (wd, mom, True), scale=scale, mixed=True)

    g32 = (gb.astype(np.uint32) << 16).view(F32)
    gs = _line(lambda a, b: a * b, g32, np.repeat(scale[:, None], P, 1))
    t = _line(lambda a, b: a - b, gs, gp)
    yp = _line(lambda a, b: a + b, y, t)
    y2 = _mix_direct(yp, RING8, fl, alpha)
    fwd, fmom, flr = (Fraction(float(F32(v))) for v in (wd, mom, lr))
    d = _line(lambda a, b: fwd * a + b, x, y2)
    m2 = _line(lambda a, b: a + b, _line(lambda a: fmom * a, m), d)
    d = _line(lambda a, b: fmom * a + b, m2, d)
    xp = _line(lambda a, b: -flr * a + b, d, x)
    x2 = _mix_direct(xp, RING8, fl, alpha)
    for k, want in (("gp", gs), ("yp", yp), ("y", y2), ("m", m2), ("xp", xp), ("x", x2)):
        assert gtref.eq32(got[k], want), k
    assert np.array_equal(got["p"], bf16ref.rne_bf16(x2)) and not gtref.eq32(y2, yp) and not gtref.eq32(x2, xp)
    # the fp32 form, no momentum, no decay, no clip factor: gp is g itself and the step is x - lr * y
    got = gtref.spec_round(O, {**s, "m": None}, g32, RING8, fl, alpha, lr, (0.0, 0.0, False))
    assert gtref.eq32(got["gp"], g32) and got["m"] is None and got["p"] is None
    assert gtref.eq32(got["xp"], _line(lambda a, b: -flr * a + b, got["y"], x))


@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
def test_tracking_invariant_is_exact(O, idle_rows):
    """(b) sum_i y_i == sum_i gs_i in every column after every round, idle rows skipped and all-zero rounds
    included, compared with ==.  Integer gradients in [-8, 8], alpha = 0.25 and self weights 1 - deg / 4 (1, 3/4
    or 1/2): every operation of the specification is exact.  |g - gp| <= 16, so after 6 rounds |y| < 2^7, and each
    round's dyadic weights add two fraction bits, 12 in all: 19 bits, well inside fp32's 24.  The test asserts
    that exactness against the same iteration in fp64, so it cannot pass by luck."""
    rng = np.random.default_rng(13)
    n, P, alpha = 8, 24, 0.25
    flags = flag_kinds(RING8, 6)[[0, 3, 6, 9, 10, 1]]                # 6 rounds: all zero, one matching, both, random
    assert not flags[0].any() and flags[1].sum() == 1 and flags[2].all() and flags[3].any()
    y, gp = np.zeros((n, P), F32), np.zeros((n, P), F32)
    y64 = np.zeros((n, P))
    for it, fl in enumerate(flags):
        g = rng.integers(-8, 9, (n, P)).astype(F32)
        y64p = y64 + (g.astype(np.float64) - gp)
        y, gp, yp = gtref.track(O, y, g, gp, RING8, fl, alpha, idle_rows)
        # the same round in fp64, whose 53 bits hold every intermediate exactly
        W = np.zeros((n, n))
        for gi in np.flatnonzero(fl):
            for i, j in enumerate(RING8[gi]):
                W[i, j] += alpha
        W += np.diag(1.0 - W.sum(axis=1))
        y64 = W @ y64p if fl.any() else y64p
        assert np.array_equal(yp.astype(np.float64), y64p) and np.array_equal(y.astype(np.float64), y64), f"round {it}"
        assert np.array_equal(y.astype(np.float64).sum(axis=0), g.astype(np.float64).sum(axis=0)), f"round {it}"
        assert gtref.eq32(gp, g)
    assert np.abs(y).max() > 0


def _quadratic(O, b, iters, lr, alpha, tracking):
    """max |x_i - mean b| after `iters` iterations on f_i(x) = 0.5 |x - b_i|^2 from x = 0, every matching active"""
    n, P = b.shape
    fl = np.ones(2, np.uint8)
    x = np.zeros((n, P), F32)
    s = {"x": x, "y": np.zeros((n, P), F32), "gp": np.zeros((n, P), F32), "m": None}
    for _ in range(iters):
        g = (s["x"] - b).astype(F32)
        if tracking:
            s = gtref.spec_round(O, s, g, RING8, fl, alpha, lr, (0.0, 0.0, False))
        else:
            s["x"] = sgdref.spec_round(O, s["x"], g, None, RING8, fl, alpha, (lr, 0.0, 0.0, False))[0]
    return float(np.abs(s["x"].astype(np.float64) - b.astype(np.float64).mean(axis=0)).max())


def test_tracking_removes_the_heterogeneity_error(O):
    """(c) heterogeneous quadratics on a ring of 8, alpha 1/3, lr 0.1, 200 iterations: gradient tracking ends
    within 1e-3 of D-SGD's distance from the optimum (the issue's cap).  With these exact fp32 chains and
    this seed the figures are D-SGD 0.33 and gradient tracking 5.8e-8 (the fp32 floor): a ratio of 1.7e-7, so the
    reference sits far more than the required 10x inside the cap, which the last line holds it to."""
    b = np.random.default_rng(2024).standard_normal((8, 16)).astype(F32)
    gt = _quadratic(O, b, 200, 0.1, 1.0 / 3.0, True)
    dsgd = _quadratic(O, b, 200, 0.1, 1.0 / 3.0, False)
    print(f"max|x_i - mean b|: gradient tracking {gt:.3e}, D-SGD {dsgd:.3e}, ratio {gt / dsgd:.3e}")
    assert dsgd > 0.05                                   # D-SGD really is stuck away from the optimum
    assert gt <= 1e-3 * dsgd
    assert gt <= 1e-4 * dsgd                             # ... with the 10x margin the reference must have


def test_clip_enters_the_tracker_and_runs_only_the_step(O):
    rng = np.random.default_rng(3)
    n, P, alpha = 8, 40, 0.25
    fl = np.array([1, 0], np.uint8)
    x, y, gp, m, g = (rng.standard_normal((n, P)).astype(F32) for _ in range(5))
    s = {"x": x, "y": y, "gp": gp, "m": m}
    scale = rng.uniform(0.1, 1.0, n).astype(F32)
    runs = [(0, 7, 0.0, 1.0), (7, 8, 0.1, 0.5), (8, 40, 0.01, 0.0)]
    hyper = (0.3, 0.9, False)
    a = gtref.spec_round(O, s, g, RING8, fl, alpha, 1e-2, hyper, scale=scale, runs=runs)
    b = gtref.spec_round(O, s, g, RING8, fl, alpha, 1e-2, hyper, scale=scale)
    c = gtref.spec_round(O, s, g, RING8, fl, alpha, 1e-2, hyper, runs=runs)
    assert gtref.eq32(a["gp"], clipref.scale_grad(g, scale)) and gtref.eq32(c["gp"], g)
    assert gtref.eq32(a["y"], b["y"]) and gtref.eq32(a["gp"], b["gp"])       # the runs change only the step
    assert not gtref.eq32(a["x"], b["x"]) and not gtref.eq32(a["y"], c["y"])
    xp, m2 = groupref.sgd_update(x, a["y"], m, runs, 1e-2, 0.9, False)
    assert gtref.eq32(a["xp"], xp) and gtref.eq32(a["m"], m2)
    assert gtref.eq32(a["xp"][:, 8:], x[:, 8:]) and not gtref.eq32(a["y"][:, 8:], y[:, 8:])   # lr_scale 0: x frozen, y moves
    # all-zero round: both arrays keep their primed values; idle rows under "skip" too
    z = gtref.spec_round(O, s, g, RING8, np.zeros(2, np.uint8), alpha, 1e-2, hyper)
    assert gtref.eq32(z["y"], z["yp"]) and gtref.eq32(z["x"], z["xp"]) and not gtref.eq32(z["y"], y)
    hand = np.array([[1, 0, -1], [-1, 2, 1]], np.int32)
    s3 = {k: v[:3] for k, v in s.items()}
    h = gtref.spec_round(O, s3, g[:3], hand, np.array([1, 0], np.uint8), alpha, 1e-2, hyper, "skip")
    assert gtref.eq32(h["y"][2], h["yp"][2]) and not gtref.eq32(h["y"][:2], h["yp"][:2])


def test_gt_arguments_errors(pkg):
    """(d) attach_gt's own checks are a host function (engine.gt_arguments)"""
    E = pkg.engine
    assert E.gt_arguments(0, 0, 0) == (0.0, 0.0, False) and E.gt_arguments(0.9, 1e-2, 1) == (0.9, 1e-2, True)
    for mom in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            E.gt_arguments(mom, 0.0, False)
    for wd in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="weight_decay"):
            E.gt_arguments(0.9, wd, False)
    with pytest.raises(ValueError, match="Nesterov"):
        E.gt_arguments(0.0, 0.0, True)
    words = E._GROUP_WORDS
    assert set(words) == set(E._FUSED_WORDS) | {"gt"} and {k: words[k] for k in E._FUSED_WORDS} == E._FUSED_WORDS


GT_RECORDS = {"mx_gt_track_call": ("GtTrackCall", 80), "mx_gt_track_bf16_call": ("GtTrackBf16Call", 80),
              "mx_gt_step_bf16_call": ("GtStepBf16Call", 104)}


@pytest.mark.parametrize("struct", sorted(GT_RECORDS))
def test_gt_call_struct_layout_matches_header(pkg, tmp_path, struct):
    """the ctypes mirrors have the header's fields, in its order, at the C compiler's offsets"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, GT_RECORDS[struct][0])
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
    assert got == want and got[0] == GT_RECORDS[struct][1]


def test_gt_call_records_are_packed_as_specified(pkg):
    """layout.call(engine, ...) of the three layouts over distinct fake addresses: every pointer table in its own
    field, the engine's geometry, and a step record that cannot carry zero_grads"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    for family, key, args, hyper in (
            ("GtTrackLayout", ("gt", False), ("z",), {"zero_grads": 1}),
            ("GtTrackBf16Layout", ("gt", True), (0,), {"zero_grads": 0}),
            ("GtStepBf16Layout", ("gt_step", True), (0.1, 0.9, 1),
             {"wd": float(F32(0.1)), "mom": float(F32(0.9)), "nesterov": 1, "zero_grads": 0, "pad_": 0})):
        cls = getattr(E, family)
        fam = cls.family
        assert fam is E.FAMILIES[key] and not fam.adam
        lay = object.__new__(cls)
        want, k = {}, 1 << 40
        for t in fam.tables + ("seg_len", "tile_off"):
            k += 1
            name = t + "_ptrs" if t in fam.tables else t
            setattr(lay, name, _Addr(k))
            want[name + "_dev"] = k
        lay.total_tiles, lay.nseg, lay.n_local, lay.n_bias, lay.bias = 77, 3, 64, 0, None
        want.update(plan_dev=_Engine._plan_ptr, total_tiles=77, nseg=3, n_slots=9, n_local=8, M=5, alpha=_Engine.alpha32,
                    **hyper)
        call = lay.call(_Engine, *args)
        assert type(call) is fam.rec
        assert {f: getattr(call, f) for f, _ in fam.rec._fields_} == want, family
    assert E.FAMILIES["gt", False].tables == E.FAMILIES["gt", True].tables == ("x", "g", "gp")
    assert E.FAMILIES["gt_step", True].tables == ("w", "g", "m", "p") and E.FAMILIES["gt_step", True].optional == "m"
    assert E.FUSED_LAYOUTS["gt_step", False] is E.SgdLayout          # the fp32 step launch is the SGD family's


def test_gt_symbols_and_knobs(pkg):
    """the thirty entry points are in the ctypes table with the SGD families' signatures, the knobs are each
    family's own, and the raw entry points refuse a null record"""
    S = pkg._lib.SIGNATURES
    E = pkg.engine
    for base in ("mx_gt_track", "mx_gt_track_bf16", "mx_gt_step_bf16"):
        for suffix in E._FUSED_ENTRIES:
            assert S[base + suffix] == S["mx_sgd_mix" + suffix], base + suffix
        assert getattr(pkg.lib, base + "_tile")(8) == 1024 and getattr(pkg.lib, base + "_tile")(64) == 256
        assert getattr(pkg.lib, base + "_tile")(65) == 0
    default = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0}
    assert E.gt_track_tuning() == E.gt_track_bf16_tuning() == E.gt_step_bf16_tuning() == default
    try:
        E.set_gt_track_tuning(grid=3)
        assert E.gt_track_tuning()["grid"] == 3
        assert E.gt_track_bf16_tuning() == E.gt_step_bf16_tuning() == E.sgd_mix_tuning() == default
        with pytest.raises(pkg.MXError, match="unknown key"):
            E.set_gt_step_bf16_tuning(stage_plain=1)
    finally:
        E.set_gt_track_tuning(grid=0)
    assert E.gt_track_tuning() == default
    assert pkg.lib.mx_gt_track(None, 0, 0.1, None, None) == pkg._lib.MX_ERR_INVALID
    assert b"mx_gt_track:" in pkg.lib.mx_last_error()
    assert pkg.lib.mx_gt_track_bf16_scaled_at(None, None, None, 1, 0.1, None, None) == pkg._lib.MX_ERR_INVALID
    assert pkg.lib.mx_gt_step_bf16_grouped_at(None, None, None, None, 1, 0.1, None, None) == pkg._lib.MX_ERR_INVALID
    assert b"mx_gt_step_bf16_grouped_at:" in pkg.lib.mx_last_error()


@pytest.mark.parametrize("kind", ["f32", "mp32"])
@pytest.mark.parametrize("where", ["g", "gp", "y", "x"])
def test_special_value_inputs_bound_the_nan_count(pkg, O, kind, where):
    """the GPU test's special-values inputs (gtkit.special_case) on the CPU: 11 of the 15 planted values per row
    can make a NaN, each reaches at most the 8 rows of its column through the two mixes, so y and x of the
    specification each hold at most 11 * 8 * 8 = 704 NaNs of 32,792 (below 5 %), and one of them more than 0"""
    import gtkit
    K = gtkit.KINDS[kind]
    partner, alpha = gtkit.topology(pkg, "g0")
    s, G = gtkit.special_case(K, where)
    assert s["x"].shape == (8, 4099)
    for fl in (np.ones(partner.shape[0], np.uint8), np.zeros(partner.shape[0], np.uint8)):
        want = gtkit.spec(O, K, s, G, partner, fl, alpha, gtkit.LR, "H2")
        nan = gtkit.nan_outputs(want)
        assert gtkit.NAN_BOUND == 704 and 0 < nan <= 704 < 0.05 * 8 * 4099, (kind, where, nan)
