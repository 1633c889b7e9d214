"""Global-norm gradient clipping in the four fused optimizer rounds (csrc/sgd_mix.hip, sgd_mix_bf16.hip,
adamw_mix.hip, adamw_mix_bf16.hip: the mx_*_mix_scaled entry points; VirtualWorkerGroup.attach_sgd /
attach_adamw(clip_grad_norm=...)).

Every comparison is against the specification in tests/clipref.py (the existing fp32 specifications fed
the gradient pre-scaled by ONE fp32 multiply), never the code under test: x / w, m and v uint32 for
uint32, p uint16 for uint16.

Shapes: widths 1 and 5 (the element path), 511 / 513 (a 512-column work item's seam), 1025 (a layout
tile's seam for 8 / 16 rows) and 4097 (several work items); graph 0 (8 rows), a 16-worker graph of
topologies.py, a 32-worker ring by hand and ER(64): the four row classes."""
import random

import numpy as np
import pytest

import bf16ref
import clipref
from adamref import bias_table
from conftest import Topo

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
LR = 1e-2
KINDS = ["sgd", "sgd_bf16", "adamw", "adamw_bf16"]
SGD_HYPER = (5e-4, 0.9, True)                      # wd (on: the L2 term sees g'), momentum, nesterov
ADAM_HYPER = (0.8, 0.95, 1e-6, 5e-4, False)        # Adam with an L2 term (it sees g'), m and v carried
ADAMW_HYPER = (0.9, 0.999, 1e-8, 1e-2, True)       # AdamW (the public-API tests)
WIDTHS = [1, 5, 511, 513, 1025, 4097]
_TOPOS, _TABLES = {}, {}


def _table(h):
    if h[:2] not in _TABLES:
        _TABLES[h[:2]] = bias_table(*h[:2])
    return _TABLES[h[:2]]


def _topology(pkg, name):
    if name not in _TOPOS:
        if name == "g0":
            gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 2 / 7)
        elif name == "g16":
            gp = pkg.GraphProcessor(pkg.select_graph(2), 1.0, 0, 16, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 0.2)
        elif name == "ring32":                     # the hand-written ring of tests/test_gpu_adamw_mix_bf16.py
            even = np.arange(32) ^ 1
            odd = (((np.arange(32) - 1) ^ 1) + 1) % 32
            _TOPOS[name] = (np.stack([even, odd]).astype(np.int32), 0.3125)
        else:                                      # ER(64, 0.1, seed 1234): 64 rows
            random.seed(0)
            base = pkg.erdos_renyi(64, 0.1, 1234)
            np.random.seed(1234)
            gp = pkg.MatchaProcessor(base, 0.5, 0, 64, 4, False)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), float(gp.neighbor_weight))
    return _TOPOS[name]


def _flags3(partner):
    """three rounds: every matching, the matching with the fewest pairs (idle workers), all zero"""
    M = partner.shape[0]
    one = np.zeros(M, np.uint8)
    one[min(range(M), key=lambda g: int((partner[g] >= 0).sum()))] = 1
    return np.stack([np.ones(M, np.uint8), one, np.zeros(M, np.uint8)])


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


class Kind:
    """one of the four fused kernels behind one interface: group construction, state in / out as
    numpy, the raw entry points and the specification"""

    def __init__(self, name):
        self.name, self.adam, self.mixed = name, name.startswith("adamw"), name.endswith("bf16")

    def group(self, pkg, topo, P, zero=True, idle="skip", clip=None, hyper=None):
        grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle, dtype=torch.bfloat16 if self.mixed else torch.float32)
        kw = {"zero_grads": zero, "master_weights": self.mixed}
        if clip is not None:
            kw["clip_grad_norm"] = clip
        if self.adam:
            b1, b2, eps, wd, dec = self.hyper = hyper or ADAM_HYPER
            grp.attach_adamw(betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=dec, **kw)
        else:
            wd, mom, nest = self.hyper = hyper or SGD_HYPER
            grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nest, **kw)
        return grp

    def grads(self, rng, shape, mag=None):
        """gradients of the existing fused tests (0.01 N(0, 1), a tenth of them 100 x larger), times a per-row
        magnitude; fp32, or bfloat16 bit patterns for the mixed kernels"""
        g = 0.01 * rng.standard_normal(shape)
        g[rng.random(shape) < 0.1] *= 100
        if mag is not None:
            g = g * np.asarray(mag)[:, None]
        g = g.astype(F32)
        return bf16ref.rne_bf16(g) if self.mixed else g

    def g32(self, G):
        return bf16ref.upcast(G) if self.mixed else G

    def put_x(self, grp, X):
        (grp.master_rows if self.mixed else grp.rows).copy_(torch.from_numpy(np.ascontiguousarray(X, F32)))

    def put_g(self, grp, G):
        if self.mixed:
            grp.grads.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(G, np.uint16).view(np.int16)))
        else:
            grp.grads.copy_(torch.from_numpy(G))

    def state(self, grp):
        """host copies: x (the fp32 rows or masters), g, m, v, p (bfloat16 rows' bits)"""
        torch.cuda.synchronize()
        s = {"x": (grp.master_rows if self.mixed else grp.rows).cpu().numpy(),
             "g": _bits(grp.grads) if self.mixed else grp.grads.cpu().numpy()}
        if self.adam:
            s["m"], s["v"] = grp.exp_avg_rows.cpu().numpy(), grp.exp_avg_sq_rows.cpu().numpy()
        elif grp.momentum_rows is not None:             # no "m" without momentum
            s["m"] = grp.momentum_rows.cpu().numpy()
        if self.mixed:
            s["p"] = _bits(grp.rows)
        return s

    @staticmethod
    def same(a, b, keys=None):
        for k in keys or a:
            ua = a[k] if a[k].dtype == np.uint16 else _u32(a[k])
            ub = b[k] if b[k].dtype == np.uint16 else _u32(b[k])
            if not np.array_equal(ua, ub):
                return False
        return True

    def call_addr(self, grp):
        return grp._adamw_state() if self.adam else grp._sgd_state()

    def fns(self, pkg):
        """(unscaled, unscaled _at, scaled, scaled _at)"""
        L, base = pkg.lib, "mx_" + ("adamw_mix" if self.adam else "sgd_mix") + ("_bf16" if self.mixed else "")
        return getattr(L, base), getattr(L, base + "_at"), getattr(L, base + "_scaled"), getattr(L, base + "_scaled_at")

    def launch(self, pkg, grp, scale_ptr, it, step, lr, scaled=True):
        """the eager entry point: the scaled one with scale_ptr (None = NULL), or the existing one"""
        f, _, fs, _ = self.fns(pkg)
        sp = pkg._lib.stream_ptr()
        a = self.call_addr(grp)
        if self.adam:
            rc = fs(a, scale_ptr, it, step, lr, None, sp) if scaled else f(a, it, step, lr, None, sp)
        else:
            rc = fs(a, scale_ptr, it, lr, None, sp) if scaled else f(a, it, lr, None, sp)
        assert rc == 0, pkg.lib.mx_last_error()

    def launch_at(self, pkg, grp, scale_ptr, iter_ptr, n_iters, step_ptr, lr, scaled=True):
        _, f, _, fs = self.fns(pkg)
        sp = pkg._lib.stream_ptr()
        a = self.call_addr(grp)
        if self.adam:
            rc = fs(a, scale_ptr, iter_ptr, n_iters, step_ptr, lr, None, sp) if scaled else \
                f(a, iter_ptr, n_iters, step_ptr, lr, None, sp)
        else:
            rc = fs(a, scale_ptr, iter_ptr, n_iters, lr, None, sp) if scaled else f(a, iter_ptr, n_iters, lr, None, sp)
        assert rc == 0, pkg.lib.mx_last_error()

    def spec(self, O, s, G, scale, t, partner, flags, alpha, lr, idle="skip"):
        """the state after one round by the specification (g excluded)"""
        if self.adam:
            args = (s["m"], s["v"], t, scale, partner, flags, alpha, lr, self.hyper, _table(self.hyper), idle)
            if self.mixed:
                x, m, v, p, _ = clipref.adam_bf16_round(O, s["x"], G, *args)
                return {"x": x, "m": m, "v": v, "p": p}
            x, m, v, _ = clipref.adam_round(O, s["x"], G, *args)
            return {"x": x, "m": m, "v": v}
        wd, mom, nest = self.hyper
        args = (s["m"], scale, partner, flags, alpha, (lr, wd, mom, nest), idle)
        if self.mixed:
            x, m, p, _ = clipref.sgd_bf16_round(O, s["x"], G, *args)
            return {"x": x, "m": m, "p": p}
        x, m, _ = clipref.sgd_round(O, s["x"], G, *args)
        return {"x": x, "m": m}


def _scales(n):
    """distinct per row: 1.0, 0.5, 0.3, 2^-10, 0, then the same shrunk a little more with every row"""
    base = F32([1.0, 0.5, 0.3, 2.0 ** -10, 0.0])
    s = np.array([base[r % 5] * F32(1.0 - (r // 5) / 64.0) for r in range(n)], F32)
    assert len(set(s[s != 0].tolist())) == int((s != 0).sum())
    return s


@pytest.mark.parametrize("name,idle", [("g0", "skip"), ("g0", "canonical"), ("g16", "skip"), ("ring32", "skip"),
                                       ("er64", "skip")])
@pytest.mark.parametrize("kind", KINDS)
def test_injected_scales(pkg, O, kind, name, idle):
    """factors set by hand, distinct per row, three carried steps (so m and v see g'): bit-equal to the
    specification; g is zeroed under zero_grads and otherwise bit-identical to what was put in"""
    K = Kind(kind)
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    scale = _scales(n)
    sc = torch.from_numpy(scale).cuda()
    rng = np.random.default_rng([KINDS.index(kind), n, len(idle)])
    for wi, P in enumerate(WIDTHS):
        zero = bool(wi & 1)
        grp = K.group(pkg, topo, P, zero, idle)
        K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
        s = K.state(grp)
        for it in range(3):
            G = K.grads(rng, (n, P))
            K.put_g(grp, G)
            K.launch(pkg, grp, sc.data_ptr(), it, it + 1, LR)
            got = K.state(grp)
            want = K.spec(O, s, G, scale, it + 1, partner, flags[it], alpha, LR, idle)
            where = f"{kind} {name} {idle} P={P} round {it}"
            for k in want:
                assert Kind.same(got, want, [k]), where + ": " + k
            if zero:
                assert not got["g"].view(np.uint16 if K.mixed else np.uint32).any(), where + ": g not zeroed"
            else:
                assert Kind.same(got, {"g": G}, ["g"]), where + ": g was rewritten"
            s = got
        if P == 4097 and name == "g0":                # the factors matter: the unscaled step differs
            plain = K.spec(O, s, G, np.ones(n, F32), 4, partner, flags[0], alpha, LR, idle)
            assert not np.array_equal(_u32(plain["x"]), _u32(K.spec(O, s, G, scale, 4, partner, flags[0], alpha,
                                                                  LR, idle)["x"]))


@pytest.mark.parametrize("kind", KINDS)
def test_public_api_clips_some_rows(pkg, O, kind):
    """attach_*(clip_grad_norm=1.0) with gradients of very different size per row: some rows clip, some do
    not; one step equals the specification fed the grad_scales read back; grad_norms / grad_scales meet
    the norm kernel's conditions; grad_norm() alone gives the same norms"""
    K = Kind(kind)
    partner, alpha = _topology(pkg, "g0")
    n = 8
    flags = np.ones((2, partner.shape[0]), np.uint8)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng(KINDS.index(kind) + 100)
    for P in (5, 4099):
        grp = K.group(pkg, topo, P, False, clip=1.0, hyper=ADAMW_HYPER if K.adam else None)
        assert grp.clip_grad_norm == 1.0 and grp.grad_norms.dtype == grp.grad_scales.dtype == torch.float32
        assert tuple(grp.grad_norms.shape) == tuple(grp.grad_scales.shape) == (n,) and grp.grad_norms.is_cuda
        K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
        mag = np.float32([0.01, 0.1, 1.0, 10.0, 100.0, 1e3, 1e4, 0.0]) / np.sqrt(P)
        G = K.grads(rng, (n, P), mag)
        K.put_g(grp, G)
        alone = grp.grad_norm()
        assert alone is grp.grad_norms
        torch.cuda.synchronize()
        norms0 = alone.cpu().numpy().copy()
        s = K.state(grp)
        step = grp.adamw_step if K.adam else grp.sgd_step
        assert step(0, LR)
        got = K.state(grp)
        norms, scales = grp.grad_norms.cpu().numpy(), grp.grad_scales.cpu().numpy()
        ref = clipref.grad_norm_ref(K.g32(G))
        assert int(clipref.ulp_diff(norms, ref).max()) <= 1 and np.array_equal(_u32(norms), _u32(norms0)), P
        assert np.array_equal(_u32(scales), _u32(clipref.clip_scale_ref(norms, 1.0))), P
        assert 0 < int((scales < 1.0).sum()) < n and scales[7] == 1.0 and norms[7] == 0.0, (P, scales)
        want = K.spec(O, s, G, scales, 1, partner, flags[0], alpha, LR)
        for k in want:
            assert Kind.same(got, want, [k]), f"{kind} P={P}: {k}"
        assert Kind.same(got, {"g": G}, ["g"])            # never rewritten scaled (zero_grads off)


@pytest.mark.parametrize("kind", KINDS)
def test_identity_and_null(pkg, kind):
    """clip_grad_norm=1e30: every factor exactly 1.0, three steps bit-identical to the same group without
    clipping; and the scaled entry points with gscale_dev = NULL are the existing ones, bit for bit, eager
    and _at"""
    K = Kind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 2 * 1024 + 77
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng(KINDS.index(kind) + 200)
    X = rng.standard_normal((n, P)).astype(F32)
    Gs = [K.grads(rng, (n, P)) for _ in range(3)]
    plain, huge, null, null_at, plain_at = (K.group(pkg, topo, P, True, clip=c) for c in (None, 1e30, None, None, None))
    for g in (plain, huge, null, null_at, plain_at):
        K.put_x(g, X)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    stp = torch.ones(1, dtype=torch.int64, device="cuda")
    for it in range(3):
        for g in (plain, huge, null, null_at, plain_at):
            K.put_g(g, Gs[it])
        (plain.adamw_step if K.adam else plain.sgd_step)(it, LR)
        (huge.adamw_step if K.adam else huge.sgd_step)(it, LR)
        K.launch(pkg, null, None, it, it + 1, LR)
        ctr.fill_(it)
        stp.fill_(it + 1)
        K.launch_at(pkg, null_at, None, ctr.data_ptr(), 3, stp.data_ptr(), LR)
        K.launch_at(pkg, plain_at, None, ctr.data_ptr(), 3, stp.data_ptr(), LR, scaled=False)
        want = K.state(plain)
        assert (huge.grad_scales.cpu().numpy() == 1.0).all() and np.isfinite(huge.grad_norms.cpu().numpy()).all()
        for g, what in ((huge, "clip 1e30"), (null, "NULL"), (null_at, "NULL _at"), (plain_at, "_at")):
            assert Kind.same(K.state(g), want), f"{kind} step {it}: {what}"
    assert np.isfinite(want["x"]).all() and not np.array_equal(_u32(want["x"]), _u32(X))


@pytest.mark.parametrize("kind", KINDS)
def test_noops_and_refusals(pkg, kind):
    """an _at counter outside the schedule and a peer-reads record write none of the optimizer arrays
    (norms and scales may be written); clip_grad_norm of 0, negative, NaN or Inf is a ValueError"""
    K = Kind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 1029
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    rng = np.random.default_rng(KINDS.index(kind) + 300)
    grp = K.group(pkg, topo, P, True, clip=0.5)
    K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
    K.put_g(grp, K.grads(rng, (n, P)))
    before = K.state(grp)
    for bad in (2, -1, 10 ** 12):
        grp.iter_dev.fill_(bad)
        (grp.adamw_device_round if K.adam else grp.sgd_device_round)()
        assert Kind.same(K.state(grp), before), bad
    assert (grp.grad_scales.cpu().numpy() < 1.0).any()                   # the norm launches did run
    eng = grp.engine
    sp = pkg._lib.stream_ptr
    pkg._lib.check(pkg.lib.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, eng.n_local, eng.M, 1, sp()))
    K.launch(pkg, grp, grp.grad_scales.data_ptr(), 0, 1, LR)
    grp.iter_dev.fill_(0)
    (grp.adamw_device_round if K.adam else grp.sgd_device_round)()
    assert Kind.same(K.state(grp), before)
    pkg._lib.check(pkg.lib.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, eng.n_local, eng.M, 0, sp()))
    assert (grp.adamw_step if K.adam else grp.sgd_step)(0, LR)            # the bit cleared: the same launch writes
    after = K.state(grp)
    assert not np.array_equal(_u32(after["x"]), _u32(before["x"])) and not after["g"].view(np.uint16).any()
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            K.group(pkg, topo, 64, True, clip=bad)
    with pytest.raises(pkg._lib.MXError, match="clip"):
        K.group(pkg, topo, 64, True).grad_norm()


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_equals_eager_steps(pkg, kind):
    """the norm launches, the scaled _at launch and the counter advances captured once and replayed for
    three iterations with fresh gradients before each replay: bit-equal to three eager steps, norms
    included"""
    K = Kind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 2 * 1024 + 77
    flags = _flags3(partner)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng(KINDS.index(kind) + 400)
    X = rng.standard_normal((n, P)).astype(F32)
    mags = [np.exp(rng.uniform(-2, 4, n)) / np.sqrt(P) for _ in range(3)]
    Gs = [K.grads(rng, (n, P), mags[i]) for i in range(3)]
    eager = K.group(pkg, topo, P, True, clip=1.0)
    K.put_x(eager, X)
    norms = []
    for it in range(3):
        K.put_g(eager, Gs[it])
        (eager.adamw_step if K.adam else eager.sgd_step)(it, LR)
        torch.cuda.synchronize()
        norms.append((eager.grad_norms.cpu().numpy().copy(), eager.grad_scales.cpu().numpy().copy()))
    want = K.state(eager)
    assert any((s < 1.0).any() for _, s in norms) and any((s == 1.0).any() for _, s in norms)

    grp = K.group(pkg, topo, P, True, clip=1.0)
    K.put_x(grp, X)
    grp.iter_dev.fill_(0)
    grp.lr_dev.fill_(LR)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            (grp.adamw_device_round if K.adam else grp.sgd_device_round)()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0                                  # capture ran nothing
    for it in range(3):
        K.put_g(grp, Gs[it])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_u32(grp.grad_norms.cpu().numpy()), _u32(norms[it][0])), it
        assert np.array_equal(_u32(grp.grad_scales.cpu().numpy()), _u32(norms[it][1])), it
    assert Kind.same(K.state(grp), want) and int(grp.iter_dev.item()) == 3


@pytest.mark.parametrize("kind", ["sgd", "adamw_bf16"])
def test_checkpoint_round_trips_between_clipping_and_plain_groups(pkg, kind):
    """clipping has no state: state_dict has the same keys with and without it, and a checkpoint of either
    group loads into the other"""
    K = Kind(kind)
    partner, alpha = _topology(pkg, "g0")
    n, P = 8, 517
    topo = Topo(partner, alpha, np.ones((4, partner.shape[0]), np.uint8))
    rng = np.random.default_rng(KINDS.index(kind) + 500)
    X = rng.standard_normal((n, P)).astype(F32)
    Gs = [K.grads(rng, (n, P), np.full(n, 30.0)) for _ in range(2)]
    clip, plain = K.group(pkg, topo, P, True, clip=1.0), K.group(pkg, topo, P, True)
    for g in (clip, plain):
        K.put_x(g, X)
        K.put_g(g, Gs[0])
        (g.adamw_step if K.adam else g.sgd_step)(0, LR)
        g.iter = 1
    ca, pa = clip.state_dict(), plain.state_dict()
    assert sorted(ca) == sorted(pa)
    assert not Kind.same(K.state(clip), K.state(plain), ["x"])             # the clipped run is another run
    clip2, plain2 = K.group(pkg, topo, P, True, clip=1.0), K.group(pkg, topo, P, True)
    clip2.load_state_dict(pa)                    # a plain checkpoint into a clipping group, and the reverse
    plain2.load_state_dict(ca)
    for a, b in ((clip2, plain), (plain2, clip)):
        assert a.iter == b.iter == 1 and Kind.same(K.state(a), K.state(b), [k for k in K.state(b) if k != "g"])
    for g in (clip, plain2):                     # ... and they go on as their own kind
        K.put_g(g, Gs[1])
        (g.adamw_step if K.adam else g.sgd_step)(1, LR)
    K.put_g(clip2, Gs[1])
    (clip2.adamw_step if K.adam else clip2.sgd_step)(1, LR)
    cont = K.group(pkg, topo, P, True, clip=1.0)
    cont.load_state_dict(ca)
    K.put_g(cont, Gs[1])
    (cont.adamw_step if K.adam else cont.sgd_step)(1, LR)
    assert Kind.same(K.state(cont), K.state(clip))
    assert not Kind.same(K.state(plain2), K.state(clip), ["x"])


@pytest.mark.parametrize("fused", ["fused_sgd", "fused_adamw"])
def test_virtual_trainer_clips(pkg, fused):
    """VirtualTrainer(fused_*=True, clip_grad_norm=X) trains the small model with finite loss; its logged
    norms are the norms of the gradient arena as backward left it; asking for clipping with torch's
    optimizers is the documented error"""
    H = pkg.harness

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=0.5, graphid=0, lr=1e-3 if fused == "fused_adamw" else 0.05,
                             matcha=True, warmup=False, momentum=0.9)
        return H.VirtualTrainer(args, H.model_factory(args), n_batches=3, **kw)

    tr = make(**{fused: True}, clip_grad_norm=0.05)
    assert tr.group.clip_grad_norm == 0.05
    seen = []

    def hook(when, t):
        if when == "before":
            torch.cuda.synchronize()
            seen.append(clipref.grad_norm_ref(t.group.grads.cpu().numpy()))

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats)
    assert len(tr.grad_norm_log) == len(seen) == 3
    clipped = 0
    for logged, ref in zip(tr.grad_norm_log, seen):
        logged = logged.numpy()
        assert logged.dtype == F32 and (ref > 0).all() and int(clipref.ulp_diff(logged, ref).max()) <= 1
        clipped += int((clipref.clip_scale_ref(logged, 0.05) < 1.0).sum())
    assert clipped > 0                                                     # the bound was in play
    assert all(s["grad_norm"] == float(tr.grad_norm_log[-1][s["worker"]]) for s in stats)
    with pytest.raises(ValueError, match="fused"):
        make(clip_grad_norm=1.0)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        make(**{fused: True}, clip_grad_norm=-1.0)
