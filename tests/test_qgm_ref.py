"""tests/qgmref.py against an fp64 transcription of the paper's five lines on exactly representable inputs and
against the rules of the contract, the QGM call records against the header, and attach_qgm's argument errors
-- none of it needs a GPU."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import bf16ref
import clipref
import groupref
import qgmref
from conftest import ROOT
from sgdref import is_nan32
from test_native_abi import _Addr, _Engine, _header_fields

F32 = np.float32
RING4 = np.array([[1, 0, 3, 2], [3, 2, 1, 0]], np.int32)         # a ring of 4 workers as two matchings


def _paper_round(x, g, mh, W, lr, beta, mu):
    """QG-DSGDm (Lin et al. 2021, Algorithm 1) in fp64, line for line:
        m      = beta * mh + g
        x_half = x - lr * m
        x_next = W x_half
        d      = (x - x_next) / lr
        mh'    = mu * mh + (1 - mu) * d"""
    m = beta * mh + g
    x_half = x - lr * m
    x_next = W @ x_half
    d = (x - x_next) / lr
    return x_next, mu * mh + (1.0 - mu) * d, x_half


def _mixing_matrix(partner, flags, alpha):
    n = partner.shape[1]
    W = np.zeros((n, n))
    for gi in np.flatnonzero(flags):
        for i, j in enumerate(partner[gi]):
            if j >= 0:
                W[i, j] += alpha
    return W + np.diag(1.0 - W.sum(axis=1))


def test_spec_equals_the_papers_lines_where_fp32_is_exact(O):
    """lr = 2^-3, beta = mu = 0.5, wd = 0, alpha = 0.25, x and g multiples of 2^-4 below 16: every
    intermediate of three carried rounds is an fp32 value, so the fp32 specification and the fp64
    transcription agree with no tolerance -- and the test asserts that exactness, so it cannot pass vacuously"""
    rng = np.random.default_rng(7)
    n, P = 4, 64
    lr, beta, mu, alpha = 2.0 ** -3, 0.5, 0.5, 0.25
    flags = np.array([[1, 1], [1, 0], [1, 1]], np.uint8)
    x = (rng.integers(-255, 256, (n, P)) / 16.0).astype(F32)
    mh = np.zeros((n, P), F32)
    x64, mh64 = x.astype(np.float64), mh.astype(np.float64)
    for it in range(3):
        g = (rng.integers(-255, 256, (n, P)) / 16.0).astype(F32)
        y, m2, xp = qgmref.spec_round(O, x, g, mh, RING4, flags[it], alpha, lr, (beta, mu, 0.0, False))
        y64, m64, xh64 = _paper_round(x64, g.astype(np.float64), mh64, _mixing_matrix(RING4, flags[it], alpha),
                                      lr, beta, mu)
        for v in (y64, m64, xh64):                   # the fp64 results are fp32 values
            assert np.array_equal(v.astype(F32).astype(np.float64), v), f"round {it}"
        assert np.array_equal(xp.astype(np.float64), xh64), f"round {it}: x'"
        assert np.array_equal(y.astype(np.float64), y64), f"round {it}: x"
        assert np.array_equal(m2.astype(np.float64), m64), f"round {it}: the buffer"
        assert np.abs(m2).max() > 0 and not np.array_equal(y, xp)
        x, mh, x64, mh64 = y, m2, y64, m64


def test_zero_learning_rate_all_zero_round_and_idle_rows(O):
    rng = np.random.default_rng(11)
    partner = np.array([[1, 0, -1], [-1, 2, 1]], np.int32)       # 3 workers; worker 2 idle under matching 0
    n, P, alpha = 3, 33, 0.25
    x, g, mh = (rng.standard_normal((n, P)).astype(F32) for _ in range(3))
    hyper = (0.9, 0.8, 0.01, True)
    # lr_r == 0: mh bit for bit, x still mixed; with wd != 0 too (the step is fmaf(-0, s, x) = x)
    y, m2, xp = qgmref.spec_round(O, x, g, mh, partner, [1, 1], alpha, 0.0, hyper)
    assert qgmref.eq32(m2, mh) and qgmref.eq32(xp, x)
    assert qgmref.eq32(y, O.decen_round(x, partner, np.array([1, 1], np.uint8), alpha)) and not qgmref.eq32(y, x)
    # an all-zero round: the local step plus the buffer update
    y, m2, xp = qgmref.spec_round(O, x, g, mh, partner, [0, 0], alpha, 0.01, hyper)
    assert qgmref.eq32(y, xp) and not qgmref.eq32(y, x)
    assert qgmref.eq32(m2, qgmref.buffer_step(x, xp, mh, F32(0.01), 0.8)) and not qgmref.eq32(m2, mh)
    assert qgmref.eq32(xp, qgmref.local_step(x, g, mh, F32(0.01), 0.01, 0.9, True))
    # without Nesterov and decay the step is x - lr * (beta * mh + g) to within its roundings
    xs = qgmref.local_step(x, g, mh, F32(0.01), 0.0, 0.9, False)
    assert np.allclose(xs, x - 0.01 * (0.9 * mh + g), rtol=1e-6, atol=1e-7)
    # idle rows: worker 2 has no partner in matching 0
    fl = np.array([1, 0], np.uint8)
    full = O.decen_round(np.ascontiguousarray(xp), partner, fl, alpha)
    y_skip, m_skip, _ = qgmref.spec_round(O, x, g, mh, partner, fl, alpha, 0.01, hyper, "skip")
    y_can, m_can, _ = qgmref.spec_round(O, x, g, mh, partner, fl, alpha, 0.01, hyper, "canonical")
    assert qgmref.eq32(y_skip[2], xp[2]) and qgmref.eq32(y_skip[:2], full[:2]) and qgmref.eq32(y_can, full)
    assert qgmref.eq32(m_skip, qgmref.buffer_step(x, y_skip, mh, F32(0.01), 0.8))
    assert qgmref.eq32(m_can, qgmref.buffer_step(x, y_can, mh, F32(0.01), 0.8))
    # a NaN gradient reaches x and the buffer
    gn = g.copy()
    gn[0, 0] = np.nan
    y, m2, _ = qgmref.spec_round(O, x, gn, mh, partner, [0, 0], alpha, 0.01, hyper)
    assert np.isnan(y[0, 0]) and np.isnan(m2[0, 0]) and np.isfinite(y[0, 1:]).all()


def test_grouped_clipped_and_bf16_forms_compose(O):
    """the run and clip forms are the ungrouped lines on slices of the scaled gradient, with the run's own lr
    in the step AND in the buffer's 1 / lr; the bf16 form widens g and rounds the stored master once"""
    rng = np.random.default_rng(3)
    partner = RING4
    n, P, alpha = 4, 40, 0.25
    fl = np.array([1, 1], np.uint8)
    x, g, mh = (rng.standard_normal((n, P)).astype(F32) for _ in range(3))
    scale = np.array([1.0, 0.25, 0.5, 0.125], F32)
    runs = [(0, 7, 0.0, 1.0), (7, 8, 0.1, 0.5), (8, 40, 0.01, 0.0)]
    hyper = (0.9, 0.7, 0.3, False)
    y, m2, xp = qgmref.spec_round(O, x, g, mh, partner, fl, alpha, 1e-3, hyper, scale=scale, runs=runs)
    gs = clipref.scale_grad(g, scale)
    assert qgmref.eq32(gs, (scale[:, None] * g).astype(F32))
    for a, b, wd, s in runs:
        lr_r = groupref.run_lr(1e-3, s)
        assert lr_r == F32(F32(1e-3) * F32(s))
        assert qgmref.eq32(xp[:, a:b], qgmref.local_step(x[:, a:b], gs[:, a:b], mh[:, a:b], lr_r, wd, 0.9, False))
        assert qgmref.eq32(m2[:, a:b], qgmref.buffer_step(x[:, a:b], y[:, a:b], mh[:, a:b], lr_r, 0.7))
    assert qgmref.eq32(y, groupref.mix(O, xp, partner, fl, alpha))
    assert qgmref.eq32(m2[:, 8:], mh[:, 8:]) and qgmref.eq32(xp[:, 8:], x[:, 8:])          # lr_scale 0: frozen
    assert not qgmref.eq32(y[:, 8:], x[:, 8:])                                             # ... but still mixed
    gb = bf16ref.rne_bf16(g)
    w_out, mo, p, wp = qgmref.spec_round_bf16(O, x, gb, mh, partner, fl, alpha, 1e-3, hyper, scale=scale, runs=runs)
    ey, em, ep = qgmref.spec_round(O, x, bf16ref.upcast(gb), mh, partner, fl, alpha, 1e-3, hyper, scale=scale, runs=runs)
    assert qgmref.eq32(w_out, ey) and qgmref.eq32(mo, em) and qgmref.eq32(wp, ep)
    assert p.dtype == np.uint16 and np.array_equal(p, bf16ref.rne_bf16(ey))


@pytest.mark.parametrize("kind", ["f32", "mp32"])
@pytest.mark.parametrize("where", ["x", "g", "m"])
def test_special_value_inputs_bound_the_nan_count(pkg, O, kind, where):
    """the GPU test's special-values inputs (qgmkit.special_case) on the CPU: 11 of the 15 planted values per
    row can make a NaN, each reaches at most the 8 rows of its column, so the specification's x holds more
    than 0 and at most 11 * 8 * 8 = 704 NaNs of 32,792 (below 5 %)"""
    import qgmkit
    K = qgmkit.KINDS[kind]
    partner, alpha = qgmkit.topology(pkg, "g0")
    s, G = qgmkit.special_case(K, where)
    planted = is_nan32(qgmkit.g32(K, G) if where == "g" else s[where]) | \
        ~np.isfinite(qgmkit.g32(K, G) if where == "g" else s[where])
    assert s["x"].shape == (8, 4099) and 9 * 8 <= int(planted.sum()) <= 11 * 8
    for fl in (np.ones(partner.shape[0], np.uint8), np.zeros(partner.shape[0], np.uint8)):
        want = qgmkit.spec(O, K, s, G, partner, fl, alpha, qgmkit.LR, "H1")
        nan = qgmkit.nan_outputs(want)
        assert qgmkit.NAN_BOUND == 704 and 0 < nan <= 704 < 0.05 * 8 * 4099, (kind, where, nan)


QGM_RECORDS = {"mx_qgm_mix_call": ("QgmMixCall", 96), "mx_qgm_mix_bf16_call": ("QgmBf16Call", 104)}


@pytest.mark.parametrize("struct", sorted(QGM_RECORDS))
def test_qgm_call_struct_layout_matches_header(pkg, tmp_path, struct):
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, QGM_RECORDS[struct][0])
    fields = [f for f, _ in cls._fields_]
    assert fields == _header_fields(struct)
    for f in ("wd", "beta", "omu", "nesterov", "zero_grads", "m_ptrs_dev"):
        assert f in fields
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "matcha_gossip.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({struct}));\n'
                   + "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want and got[0] == QGM_RECORDS[struct][1]


@pytest.mark.parametrize("family", ["QgmLayout", "QgmBf16Layout"])
def test_qgm_call_records_are_packed_as_specified(pkg, family):
    """layout.call(engine, ...) of the two layouts over distinct fake addresses: every pointer table in its own
    field, the engine's geometry, fp32 roundings with omu rounded from the fp64 1 - mu, flags 0 or 1 for any
    truthy input"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, family)
    fam = cls.family
    assert fam is E.FAMILIES["qgm", "Bf16" in family] and not fam.adam and fam.optional is None
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
                wd=f32(0.1), beta=f32(0.9), omu=f32(1.0 - 0.99), nesterov=1, zero_grads=1)
    call = lay.call(_Engine, 0.9, 0.99, 0.1, "n", 2)
    assert type(call) is fam.rec
    assert {f: getattr(call, f) for f, _ in fam.rec._fields_} == want
    assert f32(1.0 - 0.99) != f32(1 - f32(0.99))                     # the roundings differ
    assert lay.call(_Engine, 0.9, 0.99, 0.1, 0, 0).nesterov == 0 and lay.call(_Engine, 0.9, 0.99, 0.1, 0, 0).zero_grads == 0
    assert E.qgm_hyper(0.9, 0.99, 0.1, True, False) == (f32(0.1), f32(0.9), f32(1.0 - 0.99), 1, 0)
    assert qgmref.omu_of(0.99) == F32(f32(1.0 - 0.99))


def test_qgm_symbols_and_knobs(pkg):
    """the twenty entry points are in the ctypes table with the SGD families' signatures, and the knobs --
    stage_plain among them -- are the family's own"""
    S = pkg._lib.SIGNATURES
    for base, twin in (("mx_qgm_mix", "mx_sgd_mix"), ("mx_qgm_mix_bf16", "mx_sgd_mix_bf16")):
        for suffix in pkg.engine._FUSED_ENTRIES:
            assert S[base + suffix] == S[twin + suffix], base + suffix
        assert getattr(pkg.lib, base + "_tile")(8) == 1024 and getattr(pkg.lib, base + "_tile")(65) == 0
    E = pkg.engine
    default = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0, "stage_plain": 1}
    assert E.qgm_mix_tuning() == E.qgm_mix_bf16_tuning() == default
    try:
        E.set_qgm_mix_tuning(grid=3, stage_plain=0)
        assert E.qgm_mix_tuning()["grid"] == 3 and E.qgm_mix_tuning()["stage_plain"] == 0
        assert E.qgm_mix_bf16_tuning() == default and E.sgd_mix_tuning()["grid"] == 0
        with pytest.raises(pkg.MXError, match="stage_plain"):
            E.set_qgm_mix_tuning(stage_plain=2)
        with pytest.raises(pkg.MXError, match="unknown key"):
            E.set_sgd_mix_tuning(stage_plain=1)                      # the other families do not have it
    finally:
        E.set_qgm_mix_tuning(grid=0, stage_plain=1)
    assert E.qgm_mix_tuning() == default
    assert pkg.lib.mx_qgm_mix(None, 0, 0.1, None, None) == pkg._lib.MX_ERR_INVALID
    assert b"mx_qgm_mix:" in pkg.lib.mx_last_error()
    assert pkg.lib.mx_qgm_mix_bf16_grouped_at(None, None, None, None, 1, 0.1, None, None) == pkg._lib.MX_ERR_INVALID


def test_attach_qgm_argument_errors(pkg):
    """attach_qgm's own checks are a host function (engine.qgm_arguments)"""
    E = pkg.engine
    assert E.qgm_arguments(0.9, None, 0.0) == (0.9, 0.9, 0.0)                # mu defaults to the momentum
    assert E.qgm_arguments(0, 0.5, 1) == (0.0, 0.5, 1.0)
    for mom in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            E.qgm_arguments(mom, 0.5, 0.0)
    for mu in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="mu"):
            E.qgm_arguments(0.9, mu, 0.0)
    for wd in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="weight_decay"):
            E.qgm_arguments(0.9, None, wd)
    words = E._FUSED_WORDS
    assert set(words) == {"sgd", "adamw", "lion", "qgm"} and words["qgm"][0] == "QGM"
    assert {k: words[k] for k in E._OPTIMIZER_WORDS} == E._OPTIMIZER_WORDS   # the three others' words are as they were
