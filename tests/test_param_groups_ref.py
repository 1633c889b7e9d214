"""Per-parameter-group weight decay and lr scale, the parts that need no GPU: the specification in
tests/groupref.py against torch's optimizers built with real param_groups, the host-side resolution of
groups to runs (param_runs), and the new C ABI (mx_param_runs_check, the _grouped entry points' refusals;
the runs record's layout is checked in tests/test_native_abi.py)."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import groupref
from adamref import bias_table

torch = pytest.importorskip("torch")

F32 = np.float32
ENDS = [3, 4, 517, 1030, 4097]
PAIRS = [(1e-2, 1.0), (0.0, 0.1), (5e-2, 0.25), (0.0, 1.0), (1e-2, 0.0)]      # (wd, lr_scale) per run
RUNS = [(a, b, wd, s) for a, b, (wd, s) in zip([0] + ENDS[:-1], ENDS, PAIRS)]


def _torch_groups(x, lr):
    """one torch Parameter per run (column slices of x) and torch's param_groups over them"""
    params = [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(x[:, a:b]))) for a, b, _, _ in RUNS]
    # torch multiplies in Python floats; the kernel takes fmul(f32(lr), f32(s)): both round to fp32 within
    # 2^-24 relative of each other, far below the bounds below
    groups = [{"params": [p], "lr": lr * s, "weight_decay": wd} for p, (_, _, wd, s) in zip(params, RUNS)]
    return params, groups


def _cat(ts):
    return np.concatenate([t.detach().numpy() for t in ts], axis=1)


@pytest.mark.parametrize("name,decoupled", [("adamw", True), ("adam_l2", False)])
def test_groupref_against_torch_adam(name, decoupled):
    """5 steps on 8 x 4097 with five runs of mixed (wd, lr_scale): |x - torch| <= 2^-22 on x, exp_avg and
    exp_avg_sq (tests/test_adam_ref.py's bound and data)"""
    b1, b2, eps = 0.9, 0.999, 1e-8
    rng = np.random.default_rng(11)
    n, P, lr = 8, 4097, 1e-3
    x = rng.uniform(-1, 1, (n, P)).astype(F32)
    m, v = np.zeros((n, P), F32), np.zeros((n, P), F32)
    params, groups = _torch_groups(x, lr)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=lr, betas=(b1, b2), eps=eps)
    table = bias_table(b1, b2)
    for step in range(1, 6):
        g = (0.01 * rng.standard_normal((n, P))).astype(F32)
        for p, (a, b, _, _) in zip(params, RUNS):
            p.grad = torch.from_numpy(np.ascontiguousarray(g[:, a:b]))
        opt.step()
        x, m, v = groupref.adam_update(x, g, m, v, step, RUNS, lr, (b1, b2, eps, 123.0, decoupled), table)
        for what, ours, theirs in (("x", x, _cat(params)), ("m", m, _cat([opt.state[p]["exp_avg"] for p in params])),
                                   ("v", v, _cat([opt.state[p]["exp_avg_sq"] for p in params]))):
            d = float(np.abs(theirs.astype(np.float64) - ours).max())
            print(f"{name} step {step}: max |{what} - torch| = {d:.3e} ({d * 2 ** 23:.2f} x 2^-23)")
            assert d <= 2.0 ** -22, (what, step)
    assert np.abs(x).max() < 1.01


@pytest.mark.parametrize("name,mom,nesterov", [("plain", 0.0, False), ("momentum", 0.9, False),
                                               ("nesterov", 0.9, True)])
def test_groupref_against_torch_sgd(name, mom, nesterov):
    """5 steps of torch.optim.SGD with the same five groups on 8 x 4097, lr 0.1: |x - torch| and
    |m - torch| <= 2^-20, tests/test_sgd_ref.py's bound.  x starts uniform in [-0.8, 0.8) and g is
    0.01 N(0, 1), and the test asserts |x| < 1 after every step.  There one rounding of x is at most
    eps = 2^-25; torch may round a + alpha * b twice where the specification fuses (<= 2 eps per step on
    x), and the differences carried through d (|m|, |g| << 1: ulps of 2^-27 and below, times lr_r <= 0.1,
    plus wd_r <= 0.05 times the difference in x) add less than eps per step: <= 5 * 3 eps < 2^-21."""
    rng = np.random.default_rng(3)
    n, P, lr = 8, 4097, 0.1
    x = rng.uniform(-0.8, 0.8, (n, P)).astype(F32)
    m = np.zeros((n, P), F32) if mom else None
    params, groups = _torch_groups(x, lr)
    opt = torch.optim.SGD(groups, lr=lr, momentum=mom, nesterov=nesterov, dampening=0)
    for step in range(5):
        g = (0.01 * rng.standard_normal((n, P))).astype(F32)
        for p, (a, b, _, _) in zip(params, RUNS):
            p.grad = torch.from_numpy(np.ascontiguousarray(g[:, a:b]))
        opt.step()
        x, m = groupref.sgd_update(x, g, m, RUNS, lr, mom, nesterov)
        dx = float(np.abs(_cat(params).astype(np.float64) - x).max())
        print(f"{name} step {step}: max |x - torch| = {dx:.3e}")
        assert dx <= 2.0 ** -20
        if mom:
            dm = float(np.abs(_cat([opt.state[p]["momentum_buffer"] for p in params]).astype(np.float64) - m).max())
            print(f"{name} step {step}: max |m - torch| = {dm:.3e}")
            assert dm <= 2.0 ** -20
        assert np.abs(x).max() < 1


def test_groupref_one_run_is_the_plain_specification():
    """one run (wd, 1.0) is adamref / sgdref on the whole row, bit for bit; a frozen run (scale 0) keeps x and
    still advances m and v"""
    import adamref
    import sgdref
    rng = np.random.default_rng(5)
    x, g, m, v = (rng.standard_normal((3, 33)).astype(F32) for _ in range(4))
    v = np.abs(v)
    table = bias_table(0.9, 0.999)
    hyper = (0.9, 0.999, 1e-8, 1e-2, True)
    a = groupref.adam_update(x, g, m, v, 3, [(0, 33, 1e-2, 1.0)], 1e-3, hyper, table)
    b = adamref.adam_ref(x, g, m, v, 3, 1e-3, hyper, table)
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))
    a = groupref.sgd_update(x, g, m, [(0, 33, 5e-4, 1.0)], 0.1, 0.9, True)
    b = sgdref.sgd_ref(x, g, m, 0.1, 5e-4, 0.9, True)
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))
    xf, mf, vf = groupref.adam_update(x, g, m, v, 3, [(0, 20, 1e-2, 1.0), (20, 33, 1e-2, 0.0)], 1e-3, hyper, table)
    assert np.array_equal(xf[:, 20:].view(np.uint32), x[:, 20:].view(np.uint32))
    assert not np.array_equal(xf[:, :20], x[:, :20]) and not np.array_equal(mf[:, 20:], m[:, 20:])


# ---------------------------------------------------------------- param_runs
SHAPES = [("fc1.weight", (16, 10)), ("fc1.bias", (16,)), ("norm.weight", (16,)), ("norm.bias", (16,)),
          ("fc2.weight", (4, 16)), ("fc2.bias", (4,))]
NUMEL = 160 + 16 + 16 + 16 + 64 + 4
WD = float(F32(1e-2))


def test_param_runs_names_predicates_and_columns(pkg):
    pr = pkg.param_runs
    by_name = pr(NUMEL, SHAPES, [{"params": ["fc1.bias", "norm.weight", "norm.bias", "fc2.bias"], "weight_decay": 0.0}],
                 1e-2)
    by_pred = pr(NUMEL, SHAPES, [{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}], 1e-2)
    # three adjacent 1-d parameters merge into one run; unselected columns take the defaults
    assert by_name == by_pred == [(0, 160, WD, 1.0), (160, 208, 0.0, 1.0), (208, 272, WD, 1.0), (272, 276, 0.0, 1.0)]
    cols = pr(NUMEL, None, [{"columns": [(160, 208), (272, 276)], "weight_decay": 0.0}], 1e-2)
    assert cols == by_name
    # values are the fp32 roundings; lr_scale and weight_decay default independently; names see name too
    got = pr(NUMEL, SHAPES, [{"params": lambda name, p: name.startswith("fc2"), "lr_scale": 0.1}], 0.0)
    assert got == [(0, 208, 0.0, 1.0), (208, 276, 0.0, float(F32(0.1)))]
    # two groups with equal pairs on adjacent columns merge; a group equal to the defaults vanishes
    assert pr(10, None, [{"columns": [(2, 4)], "lr_scale": 0.5}, {"columns": [(4, 6)], "lr_scale": 0.5}], 0.0) == \
        [(0, 2, 0.0, 1.0), (2, 6, 0.0, 0.5), (6, 10, 0.0, 1.0)]
    assert pr(10, None, [{"columns": [(2, 4)], "weight_decay": 0.25}], 0.25) == [(0, 10, 0.25, 1.0)]
    assert pr(10, None, [], 0.5) == [(0, 10, 0.5, 1.0)]
    # a predicate on a real module sees the parameter itself
    mlp = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.LayerNorm(7), torch.nn.Linear(7, 3))
    named = list(mlp.named_parameters())
    numel = sum(p.numel() for _, p in named)
    runs = pr(numel, named, [{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}], 1e-2)
    off, want = 0, []
    for _, p in named:
        pair = (0.0 if p.ndim <= 1 else WD, 1.0)
        if want and want[-1][2:] == pair:
            want[-1] = (want[-1][0], off + p.numel()) + pair
        else:
            want.append((off, off + p.numel()) + pair)
        off += p.numel()
    assert runs == want and runs[0] == (0, 35, WD, 1.0) and len(runs) == 4


@pytest.mark.parametrize("groups,named,match", [
    ([{"columns": [(0, 5)]}, {"columns": [(4, 8)]}], None, "twice"),
    ([{"params": ["fc1.bias"]}, {"params": lambda n, p: p.ndim == 1}], SHAPES, "twice"),
    ([{"params": ["nope"]}], SHAPES, "unknown parameter name"),
    ([{"columns": [(3, 3)]}], None, "empty or outside"),
    ([{"columns": [(5, 3)]}], None, "empty or outside"),
    ([{"columns": [(-1, 3)]}], None, "empty or outside"),
    ([{"columns": [(0, NUMEL + 1)]}], None, "empty or outside"),
    ([{"columns": [(0, 3)], "weight_decay": -1e-3}], None, "weight_decay"),
    ([{"columns": [(0, 3)], "weight_decay": float("nan")}], None, "weight_decay"),
    ([{"columns": [(0, 3)], "lr_scale": float("inf")}], None, "lr_scale"),
    ([{"columns": [(0, 3)], "lr_scale": -0.5}], None, "lr_scale"),
    ([{"columns": [(0, 3)], "lr_scale": 1e39}], None, "lr_scale"),
    ([{"columns": [(0, 3)], "betas": (0.9, 0.99)}], None, "unknown key"),
    ([{"params": ["fc1.bias"]}], None, "needs a group built from models"),
    ([{"weight_decay": 0.0}], SHAPES, "exactly one"),
    ([{"params": ["fc1.bias"], "columns": [(0, 3)]}], SHAPES, "exactly one"),
])
def test_param_runs_refusals(pkg, groups, named, match):
    with pytest.raises(ValueError, match=match):
        pkg.param_runs(NUMEL, named, groups, 1e-2)


def test_param_runs_other_refusals(pkg):
    with pytest.raises(ValueError, match="default weight_decay"):
        pkg.param_runs(NUMEL, None, [], -1.0)
    with pytest.raises(ValueError, match="elements"):
        pkg.param_runs(NUMEL + 1, SHAPES, [], 0.0)


# ---------------------------------------------------------------- the C ABI
def _check(pkg, seg, off, end, wd, sc):
    a = [np.asarray(seg, np.int64), np.asarray(off, np.int32), np.asarray(end, np.int64), np.asarray(wd, F32),
         np.asarray(sc, F32)]
    rc = pkg.lib.mx_param_runs_check(a[0].ctypes.data, len(seg), a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                     a[4].ctypes.data)
    return rc, pkg.lib.mx_last_error().decode()


def test_param_runs_check(pkg):
    ok = ([10], [0, 3], [2, 5, 10], [0, 0.1, 0], [1, 0, 0.5])
    assert _check(pkg, *ok)[0] == 0
    assert _check(pkg, [10, 0, 4], [0, 2, 2, 3], [4, 10, 4], [0, 0, 0], [1, 1, 1])[0] == 0      # two segments + an empty one
    for bad, msg in [
        (([10], [0, 3], [2, 2, 10], ok[3], ok[4]), "empty"),
        (([10], [0, 3], [0, 5, 10], ok[3], ok[4]), "empty"),
        (([10], [0, 3], [5, 2, 10], ok[3], ok[4]), "ascending"),
        (([10], [0, 3], [2, 5, 9], ok[3], ok[4]), "length"),
        (([10], [0, 3], [2, 5, 11], ok[3], ok[4]), "length"),
        (([10], [0, 3], ok[2], [0, -0.1, 0], ok[4]), "weight decay"),
        (([10], [0, 3], ok[2], [0, float("nan"), 0], ok[4]), "weight decay"),
        (([10], [0, 3], ok[2], ok[3], [1, float("inf"), 1]), "lr scale"),
        (([10], [0, 3], ok[2], ok[3], [1, -1, 1]), "lr scale"),
        (([10, 4], [0, 3, 3], ok[2], ok[3], ok[4]), "no runs"),
        (([10], [0, 0], ok[2], ok[3], ok[4]), "no runs"),
        (([10], [1, 3], ok[2], ok[3], ok[4]), "run_off"),
    ]:
        rc, err = _check(pkg, *bad)
        assert rc == -1 and msg in err, (bad, err)
    L = pkg.lib
    e = np.asarray(ok[2], np.int64)
    assert L.mx_param_runs_check(None, 1, e.ctypes.data, e.ctypes.data, e.ctypes.data, e.ctypes.data) == -1
    assert L.mx_param_runs_check(e.ctypes.data, 0, e.ctypes.data, e.ctypes.data, e.ctypes.data, e.ctypes.data) == -1


def test_grouped_refusals_need_no_gpu(pkg):
    """a non-NULL runs record with a null table or nruns < 1 is MX_ERR_INVALID at every _grouped entry point,
    before anything touches a device (fake addresses in an otherwise valid call record)"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    L = pkg.lib
    fake = 1 << 40
    calls = {
        "mx_sgd_mix": E.SgdMixCall, "mx_sgd_mix_bf16": E.SgdBf16Call, "mx_adamw_mix": E.AdamwMixCall,
        "mx_adamw_mix_bf16": E.AdamwBf16Call,
    }
    for base, cls in calls.items():
        call = cls()
        for f, t in cls._fields_:
            if t is ctypes.c_void_p:
                setattr(call, f, fake)
        call.nseg, call.n_local, call.n_slots, call.M, call.total_tiles = 1, 8, 8, 4, 1
        if hasattr(call, "n_bias"):
            call.n_bias = 1
        call.mom = 0.9
        adam = "adamw" in base
        for null_field, nruns in (("run_off_dev", 1), ("run_end_dev", 1), ("wd_dev", 1), ("lr_scale_dev", 1),
                                  (None, 0), (None, -3)):
            rec = E.ParamRunsRec(fake, fake, fake, fake, nruns)
            if null_field:
                setattr(rec, null_field, None)
            ra, ca = ctypes.addressof(rec), ctypes.addressof(call)
            if adam:
                rcs = (getattr(L, base + "_grouped")(ca, ra, None, 0, 1, 0.1, None, None),
                       getattr(L, base + "_grouped_at")(ca, ra, None, fake, 4, fake, 0.1, None, None))
            else:
                rcs = (getattr(L, base + "_grouped")(ca, ra, None, 0, 0.1, None, None),
                       getattr(L, base + "_grouped_at")(ca, ra, None, fake, 4, 0.1, None, None))
            assert rcs == (-1, -1), (base, null_field, nruns)
            assert b"parameter runs" in L.mx_last_error(), (base, L.mx_last_error())


def test_attach_keywords_exist(pkg):
    """the public surface: attach_sgd / attach_adamw and VirtualTrainer take param_groups, and the package
    exports param_runs"""
    import inspect
    E = importlib.import_module(pkg.__name__ + ".engine")
    assert "param_groups" in inspect.signature(E.VirtualWorkerGroup.attach_sgd).parameters
    assert "param_groups" in inspect.signature(E.VirtualWorkerGroup.attach_adamw).parameters
    assert "param_groups" in inspect.signature(pkg.harness.VirtualTrainer.__init__).parameters
    assert pkg.param_runs is E.param_runs and math.isclose(WD, 1e-2, rel_tol=1e-6)
