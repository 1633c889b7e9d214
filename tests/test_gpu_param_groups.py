"""Per-parameter-group weight decay and lr scale in the four fused optimizer rounds (csrc/sgd_mix.hip,
sgd_mix_bf16.hip, adamw_mix.hip, adamw_mix_bf16.hip: the mx_*_mix_grouped entry points;
VirtualWorkerGroup.attach_sgd / attach_adamw(param_groups=...)).

Every comparison is against the specification in tests/groupref.py (the existing specifications applied
per run on column slices with lr_r = F32(lr) * F32(s_r)), never the code under test: x / w, m and v uint32
for uint32, p uint16 for uint16.

The boundary table on P = 4097: runs ending at 1, 3, 4, 6, 7, 8 (several runs inside one 4-element chunk),
255 / 257 (the seam of a 64-row class's 256-column work item), 511 / 513 (a 512-column work item's),
1023 / 1025 (a layout tile's), 3072 (a run that spans whole work items: the uniform path) and 4097 (the
tail on the element path); and P = 5 with three runs.  Row classes as tests/test_gpu_clip_fused.py: graph 0
(8 rows), a 16-worker graph, the hand-written 32-ring and ER(64)."""
import importlib

import numpy as np
import pytest

import clipref
import groupref
from conftest import Topo
from test_gpu_clip_fused import ADAM_HYPER, ADAMW_HYPER, KINDS, LR, SGD_HYPER, Kind, _flags3, _table, _topology, _u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
ENDS = [1, 3, 4, 6, 7, 8, 255, 257, 511, 513, 1023, 1025, 3072, 4097]
WDS = [0.0, 1e-2, 5e-2]
SCALES = [1.0, 0.1, 0.25, 0.0]


def _f(v):
    return float(F32(v))


def _runs(ends, pairs):
    return [(a, b, _f(wd), _f(s)) for a, b, (wd, s) in zip([0] + list(ends[:-1]), ends, pairs)]


def _table_runs():
    """the boundary table: pairs drawn from WDS x SCALES, every value used, no two neighbours equal (so
    the public path's merge keeps every boundary)"""
    pairs = [(WDS[(i + i // 3) % 3], SCALES[i % 4]) for i in range(len(ENDS))]
    assert all(p != q for p, q in zip(pairs, pairs[1:]))
    assert {p[0] for p in pairs} == set(WDS) and {p[1] for p in pairs} == set(SCALES)
    return _runs(ENDS, pairs)


RUNS = _table_runs()
RUNS5 = _runs([1, 4, 5], [(1e-2, 1.0), (0.0, 0.25), (5e-2, 0.0)])


def _groups(runs):
    """a run list as attach_*'s param_groups ("columns" selectors, one group per run)"""
    return [{"columns": [(a, b)], "weight_decay": wd, "lr_scale": s} for a, b, wd, s in runs]


class GKind(Kind):
    """tests/test_gpu_clip_fused.py's Kind plus parameter groups"""

    def group(self, pkg, topo, P, zero=True, idle="skip", clip=None, hyper=None, groups=None):
        grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle, dtype=torch.bfloat16 if self.mixed else torch.float32)
        kw = {"zero_grads": zero, "master_weights": self.mixed}
        if clip is not None:
            kw["clip_grad_norm"] = clip
        if groups is not None:
            kw["param_groups"] = groups
        if self.adam:
            b1, b2, eps, wd, dec = self.hyper = hyper or ADAM_HYPER
            grp.attach_adamw(betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=dec, **kw)
        else:
            wd, mom, nest = self.hyper = hyper or SGD_HYPER
            grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nest, **kw)
        return grp

    def inject(self, pkg, grp, runs):
        """unmerged run tables straight into the group (the public path merges equal neighbours)"""
        E = importlib.import_module(pkg.__name__ + ".engine")
        grp._runs = E.ParamRuns(grp.numel, runs)
        grp.param_runs = list(runs)

    def gfns(self, pkg):
        L, base = pkg.lib, "mx_" + ("adamw_mix" if self.adam else "sgd_mix") + ("_bf16" if self.mixed else "")
        return getattr(L, base + "_grouped"), getattr(L, base + "_grouped_at")

    def glaunch(self, pkg, grp, runs_addr, scale_ptr, it, step, lr):
        f, _ = self.gfns(pkg)
        sp, a = pkg._lib.stream_ptr(), self.call_addr(grp)
        rc = f(a, runs_addr, scale_ptr, it, step, lr, None, sp) if self.adam else f(a, runs_addr, scale_ptr, it, lr, None, sp)
        assert rc == 0, pkg.lib.mx_last_error()

    def glaunch_at(self, pkg, grp, runs_addr, scale_ptr, iter_ptr, n_iters, step_ptr, lr):
        _, f = self.gfns(pkg)
        sp, a = pkg._lib.stream_ptr(), self.call_addr(grp)
        rc = f(a, runs_addr, scale_ptr, iter_ptr, n_iters, step_ptr, lr, None, sp) if self.adam else \
            f(a, runs_addr, scale_ptr, iter_ptr, n_iters, lr, None, sp)
        assert rc == 0, pkg.lib.mx_last_error()

    def step(self, grp, it, lr):
        return (grp.adamw_step if self.adam else grp.sgd_step)(it, lr)

    def gspec(self, O, s, G, scale, runs, t, partner, flags, alpha, lr, idle="skip"):
        """the state after one round by the specification (g excluded)"""
        if self.adam:
            args = (s["m"], s["v"], t, scale, runs, partner, flags, alpha, lr, self.hyper, _table(self.hyper), idle)
            if self.mixed:
                x, m, v, p = groupref.adam_bf16_round(O, s["x"], G, *args)
                return {"x": x, "m": m, "v": v, "p": p}
            x, m, v = groupref.adam_round(O, s["x"], G, *args)
            return {"x": x, "m": m, "v": v}
        _, mom, nest = self.hyper
        args = (s["m"], scale, runs, partner, flags, alpha, (lr, mom, nest), idle)
        if self.mixed:
            x, m, p = groupref.sgd_bf16_round(O, s["x"], G, *args)
            return {"x": x, "m": m, "p": p}
        x, m = groupref.sgd_round(O, s["x"], G, *args)
        return {"x": x, "m": m}

    def tuning(self, pkg):
        E = importlib.import_module(pkg.__name__ + ".engine")
        base = ("adamw_mix" if self.adam else "sgd_mix") + ("_bf16" if self.mixed else "")
        return getattr(E, base + "_tuning"), getattr(E, "set_" + base + "_tuning")


def _three_rounds(pkg, O, K, grp, runs, rng, partner, flags, alpha, idle, where, zero):
    n, P = grp.n_local, grp.numel
    K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
    s = K.state(grp)
    out = []
    for it in range(3):
        G = K.grads(rng, (n, P))
        K.put_g(grp, G)
        K.step(grp, it, LR)
        got = K.state(grp)
        want = K.gspec(O, s, G, None, runs, it + 1, partner, flags[it], alpha, LR, idle)
        for k in want:
            assert Kind.same(got, want, [k]), f"{where} round {it}: {k}"
        if zero:
            assert not got["g"].view(np.uint16 if K.mixed else np.uint32).any(), f"{where}: g not zeroed"
        else:
            assert Kind.same(got, {"g": G}, ["g"]), f"{where}: g was rewritten"
        s = got
        out.append(got)
    return out


@pytest.mark.parametrize("name,idle", [("g0", "skip"), ("g0", "canonical"), ("g16", "skip"), ("ring32", "skip"),
                                       ("er64", "skip")])
@pytest.mark.parametrize("kind", KINDS)
def test_boundaries(pkg, O, kind, name, idle):
    """the boundary table and the three-run P = 5 row through attach_*(param_groups=...), three carried
    rounds (every matching, the sparsest matching, all-zero flags): bit-equal to the specification"""
    K = GKind(kind)
    partner, alpha = _topology(pkg, name)
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([KINDS.index(kind), partner.shape[1], len(idle), 7])
    for P, runs, zero in ((4097, RUNS, True), (5, RUNS5, False)):
        grp = K.group(pkg, topo, P, zero, idle, groups=_groups(runs))
        assert grp.param_runs == runs                       # nothing merged: every boundary is in the tables
        hyper = grp.adamw_hyper if K.adam else grp.sgd_hyper
        assert hyper["param_groups"] == runs
        last = _three_rounds(pkg, O, K, grp, runs, rng, partner, flags, alpha, idle, f"{kind} {name} {idle} P={P}", zero)
        # a frozen run (scale 0, wd 0 or not) kept its weights through the all-zero round's optimizer step
        a, b = next((a, b) for a, b, _, s in runs if s == 0.0)
        assert np.array_equal(_u32(last[2]["x"][:, a:b]), _u32(last[1]["x"][:, a:b]))
        assert not np.array_equal(_u32(last[2]["m"][:, a:b]), _u32(last[1]["m"][:, a:b]))


@pytest.mark.parametrize("name", ["g0", "g16", "ring32", "er64"])
@pytest.mark.parametrize("kind,momentum", [(k, m) for k in KINDS for m in ((True, False) if k.startswith("sgd") else (True,))])
def test_every_instantiation(pkg, O, kind, momentum, name):
    """every (family x row class x streaming x grouped x momentum) instantiation of the row kernel, in a
    persistent grid of 2 workgroups: plain and grouped launches, streaming hints on and off, SGD with and
    without a momentum buffer, three carried rounds each, bit-equal to the specification"""
    K = GKind(kind)
    partner, alpha = _topology(pkg, name)
    n, P = partner.shape[1], 4097
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    hyper = None if momentum else (SGD_HYPER[0], 0.0, False)
    get, put = K.tuning(pkg)
    saved = get()
    for runs in (None, RUNS):
        rng = np.random.default_rng([KINDS.index(kind), n, int(momentum), 13])
        X = rng.standard_normal((n, P)).astype(F32)
        Gs = [K.grads(rng, (n, P)) for _ in range(3)]
        want = None
        for nt in (1, 0):
            put(grid=2, nontemporal=nt)
            try:
                grp = K.group(pkg, topo, P, True, hyper=hyper, groups=None if runs is None else _groups(runs))
                assert (grp.param_runs == runs) if runs else not grp.param_runs
                K.put_x(grp, X)
                s = {"m": None, **K.state(grp)}          # no momentum buffer: m stays None
                got = []
                for it in range(3):
                    K.put_g(grp, Gs[it])
                    K.step(grp, it, LR)
                    got.append(K.state(grp))
            finally:
                put(**saved)
            if want is None:                            # the specification once per (plain / grouped)
                want = []
                one_run = [(0, P, K.hyper[3] if K.adam else K.hyper[0], 1.0)]      # the ungrouped launch
                for it in range(3):
                    want.append(K.gspec(O, s, Gs[it], None, runs or one_run, it + 1, partner, flags[it], alpha, LR))
                    s = {**s, **want[-1]}
            for it in range(3):
                for k, w in want[it].items():
                    if w is not None:
                        assert Kind.same(got[it], want[it], [k]), \
                            f"{kind} momentum={momentum} {name} grouped={runs is not None} nontemporal={nt} round {it}: {k}"
    assert get() == saved


@pytest.mark.parametrize("name", ["g0", "ring32"])
@pytest.mark.parametrize("kind", KINDS)
def test_persistent_loop(pkg, kind, name):
    """grid = 3: one workgroup walks uniform and mixed work items in turn (the constants of the parked work
    item must be its own, not the prefetched one's), with streaming hints off and on: the bits of the
    default launch"""
    K = GKind(kind)
    partner, alpha = _topology(pkg, name)
    n, P = partner.shape[1], 4097
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([KINDS.index(kind), n, 11])
    X = rng.standard_normal((n, P)).astype(F32)
    Gs = [K.grads(rng, (n, P)) for _ in range(3)]
    get, put = K.tuning(pkg)
    saved = get()

    def run(**knobs):
        put(**knobs)
        try:
            grp = K.group(pkg, topo, P, True, groups=_groups(RUNS))
            K.put_x(grp, X)
            for it in range(3):
                K.put_g(grp, Gs[it])
                K.step(grp, it, LR)
            return K.state(grp)
        finally:
            put(**saved)

    want = run()
    for nt in (0, 1):
        assert Kind.same(run(grid=3, nontemporal=nt), want), f"{kind} {name} grid=3 nontemporal={nt}"
    assert get() == saved


@pytest.mark.parametrize("kind", KINDS)
def test_identities(pkg, kind):
    """runs == NULL through _grouped is _scaled (eager and _at, with factors); one run (wd, 1.0) is the
    ungrouped launch; (wd, 1.0) on every run of the boundary table is the ungrouped launch too -- the
    per-element path against the parent's kernel.  Three steps, bit for bit."""
    K = GKind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 4097
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng(KINDS.index(kind) + 600)
    X = rng.standard_normal((n, P)).astype(F32)
    Gs = [K.grads(rng, (n, P)) for _ in range(3)]
    scale = torch.from_numpy(F32([1.0, 0.5, 0.3, 2.0 ** -10, 0.0, 0.9, 0.7, 1.0])).cuda()
    names = ("scaled", "null", "null_at", "plain", "one", "table")
    g = {k: K.group(pkg, topo, P, True) for k in names}
    wd = K.hyper[3] if K.adam else K.hyper[0]
    assert wd != 0.0
    K.inject(pkg, g["one"], [(0, P, _f(wd), 1.0)])
    K.inject(pkg, g["table"], _runs(ENDS, [(wd, 1.0)] * len(ENDS)))
    for grp in g.values():
        K.put_x(grp, X)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    stp = torch.ones(1, dtype=torch.int64, device="cuda")
    for it in range(3):
        for grp in g.values():
            K.put_g(grp, Gs[it])
        ctr.fill_(it)
        stp.fill_(it + 1)
        K.launch(pkg, g["scaled"], scale.data_ptr(), it, it + 1, LR)
        K.glaunch(pkg, g["null"], None, scale.data_ptr(), it, it + 1, LR)
        K.glaunch_at(pkg, g["null_at"], None, scale.data_ptr(), ctr.data_ptr(), 3, stp.data_ptr(), LR)
        for k in ("plain", "one", "table"):
            K.step(g[k], it, LR)
        want = K.state(g["scaled"])
        for k in ("null", "null_at"):
            assert Kind.same(K.state(g[k]), want), f"{kind} step {it}: {k}"
        want = K.state(g["plain"])
        for k in ("one", "table"):
            assert Kind.same(K.state(g[k]), want), f"{kind} step {it}: {k}"
    assert np.isfinite(want["x"]).all() and not np.array_equal(_u32(want["x"]), _u32(X))
    assert not Kind.same(K.state(g["scaled"]), want, ["x"])


@pytest.mark.parametrize("kind", KINDS)
def test_with_clipping(pkg, O, kind):
    """param_groups with clip_grad_norm: the norm is over the whole row (all its runs), the factor enters
    before anything else; one step equals the specification fed the grad_scales read back"""
    K = GKind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 4097
    flags = np.ones((2, partner.shape[0]), np.uint8)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng(KINDS.index(kind) + 700)
    grp = K.group(pkg, topo, P, False, clip=1.0, groups=_groups(RUNS))
    K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
    mag = np.float32([0.01, 0.1, 1.0, 10.0, 100.0, 1e3, 1e4, 0.0]) / np.sqrt(P)
    G = K.grads(rng, (n, P), mag)
    K.put_g(grp, G)
    s = K.state(grp)
    assert K.step(grp, 0, LR)
    got = K.state(grp)
    norms, scales = grp.grad_norms.cpu().numpy(), grp.grad_scales.cpu().numpy()
    assert int(clipref.ulp_diff(norms, clipref.grad_norm_ref(K.g32(G))).max()) <= 1     # one norm over all runs
    assert np.array_equal(_u32(scales), _u32(clipref.clip_scale_ref(norms, 1.0)))
    assert 0 < int((scales < 1.0).sum()) < n
    want = K.gspec(O, s, G, scales, RUNS, 1, partner, flags[0], alpha, LR)
    for k in want:
        assert Kind.same(got, want, [k]), f"{kind}: {k}"
    assert Kind.same(got, {"g": G}, ["g"])


@pytest.mark.parametrize("kind", KINDS)
def test_device_rounds(pkg, O, kind):
    """sgd_device_round / adamw_device_round on a grouped group: three rounds with lr_dev rewritten between
    them equal the specification; a counter outside the schedule writes nothing"""
    K = GKind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 4097
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng(KINDS.index(kind) + 800)
    grp = K.group(pkg, topo, P, True, groups=_groups(RUNS))
    K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
    s = K.state(grp)
    rnd = grp.adamw_device_round if K.adam else grp.sgd_device_round
    grp.iter_dev.fill_(0)
    for it, lr in enumerate((1e-2, 3e-3, 0.5)):
        G = K.grads(rng, (n, P))
        K.put_g(grp, G)
        grp.lr_dev.fill_(lr)
        rnd()
        got = K.state(grp)
        want = K.gspec(O, s, G, None, RUNS, it + 1, partner, flags[it], alpha, float(F32(lr)), "skip")
        for k in want:
            assert Kind.same(got, want, [k]), f"{kind} round {it}: {k}"
        s = got
    assert int(grp.iter_dev.item()) == 3
    K.put_g(grp, K.grads(rng, (n, P)))
    before = K.state(grp)
    for bad in (grp.engine.T + 5, -1):
        grp.iter_dev.fill_(bad)
        rnd()
        assert Kind.same(K.state(grp), before), bad


class _Mlp(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(24, 40)
        self.norm = torch.nn.LayerNorm(40)
        self.fc2 = torch.nn.Linear(40, 7, bias=False)
        self.head = torch.nn.Linear(7, 3)

    def forward(self, x):
        return self.head(self.fc2(self.norm(torch.relu(self.fc1(x)))))


@pytest.mark.parametrize("mixed", [False, True])
def test_public_path(pkg, O, mixed):
    """8 adopted MLPs, attach_adamw(param_groups=[no decay for ndim <= 1]): param_runs are the offsets of
    named_parameters(); three adamw_communicate steps on backward()'s gradients equal the specification;
    the decayed columns differ from an undecayed run of the same data"""
    K = GKind("adamw_bf16" if mixed else "adamw")
    K.hyper = ADAMW_HYPER
    partner, alpha = _topology(pkg, "g0")
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    dtype = torch.bfloat16 if mixed else torch.float32

    def build(groups):
        torch.manual_seed(5)
        models = [_Mlp().cuda().to(dtype) for _ in range(8)]
        grp = pkg.VirtualWorkerGroup(topo, models, dtype=dtype)
        b1, b2, eps, wd, dec = ADAMW_HYPER
        grp.attach_adamw(betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=dec, master_weights=mixed,
                         param_groups=groups)
        return models, grp

    models, grp = build([{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}])
    wd = _f(ADAMW_HYPER[3])
    off, want_runs = 0, []
    for _, p in models[0].named_parameters():
        pair = (0.0 if p.ndim <= 1 else wd, 1.0)
        if want_runs and want_runs[-1][2:] == pair:
            want_runs[-1] = (want_runs[-1][0], off + p.numel()) + pair
        else:
            want_runs.append((off, off + p.numel()) + pair)
        off += p.numel()
    assert grp.param_runs == want_runs and len(want_runs) == 4 and off == grp.numel
    assert grp.adamw_hyper["param_groups"] == want_runs
    _, plain = build(None)                                    # decays everything
    assert plain.param_runs is None and "param_groups" not in plain.adamw_hyper
    s = K.state(grp)
    for it in range(3):
        for r, m in enumerate(models):                        # real gradients, through the adopted views
            torch.manual_seed(100 * it + r)
            out = m(torch.randn(16, 24, device="cuda", dtype=dtype))
            out.float().square().mean().backward()
        torch.cuda.synchronize()
        G = K.state(grp)["g"]
        assert G.view(np.uint16 if mixed else np.uint32).any()
        K.put_g(plain, G)
        grp.adamw_communicate(LR)
        plain.adamw_communicate(LR)
        got = K.state(grp)
        want = K.gspec(O, s, G, None, want_runs, it + 1, partner, flags[it], alpha, LR)
        for k in want:
            assert Kind.same(got, want, [k]), f"mixed={mixed} step {it}: {k}"
        assert not got["g"].view(np.uint16 if mixed else np.uint32).any()
        s = got
    a = K.state(plain)["x"]
    for lo, hi, w, _ in want_runs:                            # the test can fail: decay 0 is another run
        same = np.array_equal(_u32(a[:, lo:hi]), _u32(s["x"][:, lo:hi]))
        assert same == (w != 0.0), (lo, hi, w)
