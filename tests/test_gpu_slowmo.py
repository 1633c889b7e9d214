"""The SlowMo outer step on the GPU (csrc/slowmo.hip, VirtualWorkerGroup.attach_slowmo / slowmo_step): the raw
ABI against the specification restated in tests/slowmoref.py (never the code under test), the mean against
mx_mean_rows' own output, graph replay, the group level composed with sgdref / sgdbf16ref, refusals,
checkpoints and the harness.

rows, a and u compare uint32 for uint32 and p uint16 for uint16 (a NaN of any payload where the specification
is a NaN, in the special-values test only).  Shapes are the smallest at which each path can go wrong: both
sides of every row-class boundary (8 | 9, 16 | 17, 32 | 33), 1-5 columns (below one vector, the vector tail),
a 512-column tile's edge, and several tiles with a tail."""
import ctypes
import importlib

import numpy as np
import pytest

import bf16ref
import rowtopos
import sgdbf16ref
import sgdref
import slowmoref as S
from conftest import Topo, special_values

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
NS = [1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 64]
COUNTS = [1, 3, 4, 5, 511, 512, 513, 1027, 4097]
GUARD32 = np.uint32(0xDEADBEEF)          # -6.26e18: a finite pattern no arithmetic here produces
GUARD16 = np.uint16(0xBEEF)


def _u(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _eq(got, want):
    return np.array_equal(_u(got), _u(want))


def _ld(count):
    return (count + 63) // 64 * 64 + 64


class Tables:
    """rows [n][ld], a, u [ld] (and p [n][ld] bfloat16 bits) on the device, each inside a larger buffer of guard
    words: the data start `off` elements in (off = 1: nothing is 16-byte aligned), and everything outside the
    first `count` columns of a row is guard.  `expect(...)` builds the same buffers on the host."""

    def __init__(self, pkg, rows, a, u, mixed, off=0):
        self.pkg, self.n, self.count = pkg, rows.shape[0], rows.shape[1]
        self.ld, self.off, self.mixed = _ld(self.count), off, mixed
        self.h_rows = self._host32(rows)
        self.h_a, self.h_u = self._host32(a[None]), self._host32(u[None])
        self.h_p = np.full(self.n * self.ld + 8, GUARD16, np.uint16) if mixed else None
        self.d_rows, self.d_a, self.d_u = (torch.from_numpy(h.view(np.int32)).cuda() for h in (self.h_rows, self.h_a, self.h_u))
        self.d_p = torch.from_numpy(self.h_p.view(np.int16)).cuda() if mixed else None

    def _host32(self, data):
        buf = np.full(data.shape[0] * self.ld + 8, GUARD32, np.uint32)
        for r in range(data.shape[0]):
            buf[self.off + r * self.ld: self.off + r * self.ld + self.count] = _u(data[r])
        return buf

    def record(self, order, alpha, beta):
        E = importlib.import_module(self.pkg.__name__ + ".engine")
        return E.SlowmoCall(self.d_rows.data_ptr() + 4 * self.off, self.d_a.data_ptr() + 4 * self.off,
                            self.d_u.data_ptr() + 4 * self.off,
                            (self.d_p.data_ptr() + 2 * self.off) if self.mixed else None, self.ld, self.ld, self.count,
                            self.n, order, alpha, beta)

    def step(self, order, alpha, beta, lr, lr_dev=None):
        rec = self.record(order, alpha, beta)
        rc = self.pkg.lib.mx_slowmo_step(ctypes.addressof(rec), lr, lr_dev, self.pkg._lib.stream_ptr())
        assert rc == 0, self.pkg.lib.mx_last_error()
        torch.cuda.synchronize()

    def got(self):
        """(rows, a, u, p) whole buffers as uint32 / uint16"""
        out = [t.cpu().numpy().view(np.uint32) for t in (self.d_rows, self.d_a, self.d_u)]
        return out + [self.d_p.cpu().numpy().view(np.uint16) if self.mixed else None]

    def expect(self, rows, a, u, p):
        """the whole buffers a correct launch leaves: the given data, guard everywhere else"""
        want = [self._host32(rows), self._host32(a[None]), self._host32(u[None]), None]
        if self.mixed:
            want[3] = self.h_p.copy()
            if p is not None:
                for r in range(self.n):
                    want[3][self.off + r * self.ld: self.off + r * self.ld + self.count] = p[r]
        return want


def _same(got, want, nan_ok=False):
    """whole buffers equal; nan_ok: a NaN of any payload where the specification has one (outside the guard)"""
    for g, w in zip(got, want):
        if w is None:
            continue
        if np.array_equal(g, w):
            continue
        if not nan_ok:
            return False
        if g.dtype == np.uint32:
            guard = w == GUARD32
            ok = np.array_equal(g[guard], w[guard]) and sgdref.same_f32(g[~guard].view(F32), w[~guard].view(F32))
        else:
            guard = w == GUARD16
            ok = np.array_equal(g[guard], w[guard]) and bf16ref.same_bf16(g[~guard], w[~guard])
        if not ok:
            return False
    return True


def _inputs(rng, n, count):
    return (rng.standard_normal((n, count)).astype(F32), rng.standard_normal(count).astype(F32),
            rng.standard_normal(count).astype(F32))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n", NS)
def test_abi_matches_spec(pkg, n, mixed):
    """every count and both orders: the arrays bit for bit, the guard words past `count` intact"""
    rng = np.random.default_rng([n, int(mixed)])
    lr, alpha, beta = 0.05, 0.7, 0.5
    for count in COUNTS:
        rows, a, u = _inputs(rng, n, count)
        for order in (0, 1):
            t = Tables(pkg, rows, a, u, mixed)
            t.step(order, alpha, beta, lr)
            want = t.expect(*S.spec_step(rows, a, u, lr, alpha, beta, order, mixed))
            assert _same(t.got(), want), f"n={n} count={count} order={order} mixed={mixed}"


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n", [3, 8, 12, 24, 40])
def test_abi_unaligned_tables(pkg, n, mixed):
    """every table offset by one element: the per-element path of every row class, the same bits"""
    rng = np.random.default_rng([n, int(mixed), 1])
    for count in (5, 513, 1027):
        rows, a, u = _inputs(rng, n, count)
        t = Tables(pkg, rows, a, u, mixed, off=1)
        t.step(0, 1.3, 0.25, 0.1)
        want = t.expect(*S.spec_step(rows, a, u, 0.1, 1.3, 0.25, 0, mixed))
        assert _same(t.got(), want), f"n={n} count={count}"


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", [3, 8, 9, 16, 33, 64])
def test_mean_is_mx_mean_rows_bits(pkg, n, order):
    """u = 0, beta = 0, alpha = 1, lr = 1: the stored u' is fsub(a, mean) with mean taken from mx_mean_rows' own
    output for the same rows (aligned: its vector kernels; 1027 columns: two tiles, the rest, a tail)"""
    rng = np.random.default_rng([n, order, 2])
    count = 1027
    rows, a, _ = _inputs(rng, n, count)
    t = Tables(pkg, rows, a, np.zeros(count, F32), False)
    out = torch.empty(count, dtype=torch.float32, device="cuda")
    pkg._lib.check(pkg.lib.mx_mean_rows(t.d_rows.data_ptr(), n, t.ld, count, order, out.data_ptr(),
                                        pkg._lib.stream_ptr()))
    torch.cuda.synchronize()
    mean = out.cpu().numpy()
    assert _eq(mean, S.mean_rows(rows, order))
    t.step(order, 1.0, 0.0, 1.0)
    got_u = t.got()[2][:count].view(F32)
    assert _eq(got_u, (a - mean).astype(F32))


@pytest.mark.parametrize("n,mixed", [(5, False), (8, True), (12, True), (20, False), (64, True)])
def test_special_values(pkg, n, mixed):
    """NaNs of several payloads, +-Inf, +-0, denormals and +-FLT_MAX planted in some rows, in a and in u: the
    specification's bits (a NaN of any payload where it has one), and a non-finite column stays one column"""
    count = 700
    rng = np.random.default_rng([n, 3])
    rows, a, u = _inputs(rng, n, count)
    rows[0] = special_values(count, 11)
    rows[n - 1] = special_values(count, 12)
    a = special_values(count, 13)
    u = special_values(count, 14, n_nan=2, n_inf=2)
    for order in (0, 1):
        t = Tables(pkg, rows, a, u, mixed)
        t.step(order, 0.9, 0.5, 0.25)
        w_rows, w_a, w_u, w_p = S.spec_step(rows, a, u, 0.25, 0.9, 0.5, order, mixed)
        assert _same(t.got(), t.expect(w_rows, w_a, w_u, w_p), nan_ok=True)
        bad_in = ~(np.isfinite(rows).all(axis=0) & np.isfinite(a) & np.isfinite(u))
        got_rows = t.got()[0]
        data = np.stack([got_rows[r * t.ld: r * t.ld + count] for r in range(n)]).view(F32)
        assert not np.isfinite(data[:, bad_in]).any()
        # overflow of a finite column (FLT_MAX among the rows) is the specification's too
        assert np.array_equal(np.isfinite(data), np.isfinite(w_rows))


def test_lr_dev_is_read_when_the_kernel_runs(pkg):
    """raw ABI: lr_dev overrides the argument, and exactly 0 there is a complete no-op in every row class"""
    rng = np.random.default_rng(4)
    lr_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    for n in (8, 16, 32, 64):
        rows, a, u = _inputs(rng, n, 1027)
        t = Tables(pkg, rows, a, u, True)
        before = t.got()
        t.step(0, 1.0, 0.5, 123.0, lr_dev.data_ptr())                # lr_dev == 0: nothing is written, p neither
        assert _same(t.got(), before)
        lr_dev.fill_(0.125)
        t.step(0, 1.0, 0.5, float("nan"), lr_dev.data_ptr())          # the argument is not looked at
        assert _same(t.got(), t.expect(*S.spec_step(rows, a, u, 0.125, 1.0, 0.5, 0, True)))
        lr_dev.zero_()


def test_knobs_change_no_bits(pkg):
    E = importlib.import_module(pkg.__name__ + ".engine")
    rng = np.random.default_rng(5)
    rows, a, u = _inputs(rng, 8, 4097)
    want = None
    try:
        for knobs in ({"store_policy": 1, "wgpc": 3}, {"store_policy": 3, "wgpc": 0}, {"store_policy": 3, "wgpc": 8}):
            E.set_slowmo_tuning(**knobs)
            t = Tables(pkg, rows, a, u, True)
            t.step(0, 1.0, 0.5, 0.1)
            want = want or t.expect(*S.spec_step(rows, a, u, 0.1, 1.0, 0.5, 0, True))
            assert _same(t.got(), want), knobs
    finally:
        E.set_slowmo_tuning(store_policy=1, wgpc=3)


# ---------------------------------------------------------------------------------------------- group level
_TOPOS = {}


def _topology(pkg, name):
    if name not in _TOPOS:
        if name == "g0":                           # graph 0, 8 workers
            gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 2 / 7)
        else:                                      # 16 rows by hand: the round robin of tests/rowtopos.py
            _TOPOS[name] = (rowtopos.round_robin(16), rowtopos.ALPHA)
    return _TOPOS[name]


def _flags(partner, rounds, seed):
    rng = np.random.default_rng(seed)
    f = (rng.random((rounds, partner.shape[0])) < 0.5).astype(np.uint8)
    f[:, 0] = 1
    f[2] = 0                                       # an all-zero round just before the first outer step
    return f


def _put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, F32)))


def _put_bits(t, bits):
    t.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)))


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


LR, WD, MOM, TAU = 0.1, 5e-4, 0.9, 3


def _sgd_group(pkg, topo, P, mixed, **slowmo):
    grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16 if mixed else torch.float32)
    grp.attach_sgd(momentum=MOM, weight_decay=WD, master_weights=mixed)
    if slowmo:
        grp.attach_slowmo(**slowmo)
    return grp


@pytest.mark.parametrize("buffers", ["maintain", "reset", "average"])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", ["g0", "rr16"])
def test_group_two_outer_iterations(pkg, O, name, mixed, buffers):
    """two outer iterations of tau = 3 fused SGD-momentum steps == sgdref / sgdbf16ref composed with slowmoref:
    rows (masters and their bf16 image), momentum rows, anchor and slow momentum after every launch"""
    partner, alpha = _topology(pkg, name)
    n, P = partner.shape[1], 1027
    flags = _flags(partner, 2 * TAU, 7)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([n, int(mixed), len(buffers)])
    order = 1 if name == "rr16" else 0
    grp = _sgd_group(pkg, topo, P, mixed, beta=0.5, alpha=0.8, buffers=buffers, order=order)
    x0 = rng.standard_normal(P).astype(F32)
    if mixed:
        x0 = bf16ref.upcast(bf16ref.rne_bf16(x0))                      # synced bf16 rows and their exact masters
    X = np.tile(x0, (n, 1))
    _put(grp.master_rows if mixed else grp.rows, X)
    if mixed:
        _put_bits(grp.rows, bf16ref.rne_bf16(X))
    grp.slowmo_anchor_from_rows()
    A, U, Mo = x0.copy(), np.zeros(P, F32), np.zeros((n, P), F32)
    assert _eq(grp.slowmo_anchor.cpu().numpy(), A) and not grp.slowmo_momentum.any().item()
    for it in range(2 * TAU):
        if mixed:
            G = bf16ref.random_bits(rng, (n, P), specials=False)
            _put_bits(grp.grads, G)
            X, Mo, Pb, _ = sgdbf16ref.spec_round(O, X, G, Mo, partner, flags[it], alpha, (LR, WD, MOM, False))
        else:
            G = rng.standard_normal((n, P)).astype(F32)
            _put(grp.grads, G)
            X, Mo, _ = sgdref.spec_round(O, X, G, Mo, partner, flags[it], alpha, (LR, WD, MOM, False))
        grp.sgd_communicate(LR)
        where = f"{name} mixed={mixed} {buffers} iteration {it}"
        if (it + 1) % TAU == 0:
            assert float(grp.consensus_distance()[0].item()) > 0 and grp.consensus_stats[0].item() > 0, where
            grp.slowmo_step(LR)
            assert grp.iter == it + 1, where                           # the outer step is not an iteration
            X, A, U, Pb = S.spec_step(X, A, U, LR, 0.8, 0.5, order, mixed)
            if buffers == "reset":
                Mo = np.zeros_like(Mo)
            elif buffers == "average":
                Mo = np.tile(O.central_mean(Mo, "sequential" if order else "tree"), (n, 1))
            torch.cuda.synchronize()
            got = (grp.master_rows if mixed else grp.rows).cpu().numpy()
            assert all(_eq(got[r], got[0]) for r in range(n)), where
            grp.consensus_distance()
            torch.cuda.synchronize()
            assert grp.consensus_stats[0].item() == 0.0 and not grp.consensus_dists.any().item(), where
        torch.cuda.synchronize()
        assert _eq((grp.master_rows if mixed else grp.rows).cpu().numpy(), X), where + ": rows"
        assert _eq(grp.momentum_rows.cpu().numpy(), Mo), where + ": momentum"
        assert _eq(grp.slowmo_anchor.cpu().numpy(), A) and _eq(grp.slowmo_momentum.cpu().numpy(), U), where
        if mixed:
            assert np.array_equal(_bits(grp.rows), Pb), where + ": p"
    assert grp.iter == 2 * TAU and U.any()
    for arena in (grp.arena, grp.mom_arena, grp._slowmo_bufs) + ((grp.master_arena,) if mixed else ()):
        assert not arena[:, P:].view(torch.int16 if arena.dtype == torch.bfloat16 else torch.int32).any().item()


def test_adamw_reset_restarts_the_step_count(pkg):
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, _flags(partner, 6, 8))
    grp = pkg.VirtualWorkerGroup(topo, numel=300)
    grp.attach_adamw()
    grp.attach_slowmo(beta=0.5, alpha=1.0, buffers="reset")
    rng = np.random.default_rng(9)
    for it in range(3):
        _put(grp.grads, rng.standard_normal((8, 300)).astype(F32))
        grp.adamw_communicate(1e-3)
    for _ in range(2):
        grp.adamw_device_round()
    torch.cuda.synchronize()
    assert grp.opt_step == 3 and int(grp.opt_step_dev.item()) == 3 and grp.exp_avg_rows.any().item()
    grp.slowmo_step(1e-3)
    torch.cuda.synchronize()
    assert grp.opt_step == 0 and int(grp.opt_step_dev.item()) == 1
    assert not grp.exp_avg_arena.any().item() and not grp.exp_avg_sq_arena.any().item()
    _put(grp.grads, rng.standard_normal((8, 300)).astype(F32))
    grp.adamw_communicate(1e-3)                                        # the first step of a fresh optimizer again
    grp.lr_dev.fill_(1e-3)
    grp.slowmo_device_step()                                           # the device form leaves the host count alone
    torch.cuda.synchronize()
    assert grp.opt_step == 1 and int(grp.opt_step_dev.item()) == 1 and not grp.exp_avg_arena.any().item()


def test_graph_replay_equals_eager_steps(pkg):
    """slowmo_device_step captured once (one stream: the outer step and the buffer strategy's launches are a
    single chain, nothing forks), replayed three times with three learning rates == three slowmo_step calls on
    a twin; lr_dev == 0 leaves rows, anchor and slow momentum untouched"""
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, _flags(partner, 4, 10))
    n, P = 8, 2 * 512 + 77
    rng = np.random.default_rng(11)
    X0 = np.tile(rng.standard_normal(P).astype(F32), (n, 1))
    Xs = [rng.standard_normal((n, P)).astype(F32) for _ in range(4)]
    Ms = [rng.standard_normal((n, P)).astype(F32) for _ in range(4)]
    lrs = [0.1, 0.025, 0.4]

    def fresh():
        grp = _sgd_group(pkg, topo, P, False)
        _put(grp.rows, X0)
        grp.attach_slowmo(beta=0.5, alpha=1.0, buffers="average")
        return grp

    def state(grp):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (grp.rows, grp.momentum_rows, grp.slowmo_anchor, grp.slowmo_momentum)]

    eager = fresh()
    A, U = X0[0].copy(), np.zeros(P, F32)
    for k, lr in enumerate(lrs):
        _put(eager.rows, Xs[k])
        _put(eager.momentum_rows, Ms[k])
        eager.slowmo_step(lr)
        _, A, U, _ = S.spec_step(Xs[k], A, U, lr, 1.0, 0.5)
    want = state(eager)
    assert _eq(want[2], A) and _eq(want[3], U) and _eq(want[0], np.tile(A, (n, 1)))
    assert _eq(want[1], np.tile(S.mean_rows(Ms[2], 0), (n, 1)))

    grp = fresh()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            grp.slowmo_device_step()
    torch.cuda.synchronize()
    assert _eq(state(grp)[0], X0) and not grp.slowmo_momentum.any().item()      # capture ran nothing
    for k, lr in enumerate(lrs):
        _put(grp.rows, Xs[k])
        _put(grp.momentum_rows, Ms[k])
        grp.lr_dev.fill_(lr)
        g.replay()
    assert all(_eq(a, b) for a, b in zip(state(grp), want))
    _put(grp.rows, Xs[3])
    grp.lr_dev.zero_()
    g.replay()
    past = state(grp)
    assert _eq(past[0], Xs[3]) and _eq(past[2], want[2]) and _eq(past[3], want[3])


def test_python_refusals(pkg):
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, _flags(partner, 4, 12))
    V = pkg.VirtualWorkerGroup
    with pytest.raises(pkg.MXError, match="attach_slowmo"):
        V(topo, numel=100).slowmo_step(0.1)
    with pytest.raises(pkg.MXError, match="attach_slowmo"):
        V(topo, numel=100).slowmo_device_step()
    with pytest.raises(pkg.MXError, match="attach_slowmo"):
        V(topo, numel=100).slowmo_anchor_from_rows()
    for kw, word in (({"beta": 1.0}, "beta"), ({"beta": -0.1}, "beta"), ({"beta": float("nan")}, "beta"),
                     ({"alpha": 0.0}, "alpha"), ({"alpha": -1.0}, "alpha"), ({"alpha": float("inf")}, "alpha"),
                     ({"order": 2}, "order"), ({"buffers": "keep"}, "buffers"),
                     ({"buffers": "reset"}, "none attached"), ({"buffers": "average"}, "none attached")):
        with pytest.raises(ValueError, match=word):
            V(topo, numel=100).attach_slowmo(**kw)
    with pytest.raises(ValueError, match="master weights"):
        V(topo, numel=100, dtype=torch.bfloat16).attach_slowmo()
    lion = V(topo, numel=100, dtype=torch.bfloat16)
    lion.attach_lion(master_weights=True, momentum_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16 Lion"):
        lion.attach_slowmo(buffers="average")
    lion.attach_slowmo(buffers="reset")                                # zeroing a bf16 arena is fine
    grp = V(topo, numel=100)
    grp.attach_slowmo()                                                # no family: "maintain" only
    with pytest.raises(RuntimeError, match="already attached"):
        grp.attach_slowmo()
    with pytest.raises(RuntimeError, match="attach_slowmo"):
        grp.attach_sgd()                                               # the base optimizer comes first
    for lr in (0.0, -0.1, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError, match="lr"):
            grp.slowmo_step(lr)
    before = grp.rows.clone()
    torch.cuda.synchronize()
    assert torch.equal(grp.rows, before)                               # the refusals launched nothing
    hub_topo = Topo(partner, alpha, _flags(partner, 4, 12))
    from conftest import LoopbackHub
    hub = LoopbackHub(2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        V(hub_topo, numel=100, rank=0, nranks=2, comm=hub.comm(0)).attach_slowmo()


def test_abi_refusals_on_real_tables(pkg):
    """the refusals of tests/test_slowmo_ref.py on live device arrays: MX_ERR_INVALID, and nothing written"""
    rng = np.random.default_rng(13)
    rows, a, u = _inputs(rng, 8, 100)
    t = Tables(pkg, rows, a, u, True)
    before = t.got()
    E = importlib.import_module(pkg.__name__ + ".engine")
    base = t.record(0, 1.0, 0.5)
    fields = [k for k, _ in E.SlowmoCall._fields_]
    for over in (dict(rows=None), dict(a=None), dict(u=None), dict(n_local=0), dict(n_local=65), dict(ld=99), dict(order=2),
                 dict(a=base.rows), dict(u=base.rows + 4 * (7 * t.ld + 99)), dict(a=base.u), dict(a=base.p),
                 dict(u=base.p + 2 * t.ld), dict(alpha=0.0), dict(alpha=float("nan")), dict(beta=1.0), dict(beta=-0.5)):
        rec = E.SlowmoCall(*[over.get(k, getattr(base, k)) for k in fields])
        assert pkg.lib.mx_slowmo_step(ctypes.addressof(rec), 0.1, None, pkg._lib.stream_ptr()) == pkg._lib.MX_ERR_INVALID, over
    for lr in (0.0, -1.0, float("inf"), float("nan")):
        assert pkg.lib.mx_slowmo_step(ctypes.addressof(base), lr, None, pkg._lib.stream_ptr()) == pkg._lib.MX_ERR_INVALID
    torch.cuda.synchronize()
    assert _same(t.got(), before)


@pytest.mark.parametrize("mixed", [False, True])
def test_checkpoint_round_trip(pkg, O, mixed):
    """a run resumed from a checkpoint taken after an outer step continues bit for bit; half a state and a
    state without attach_slowmo are refused; a checkpoint without the pair gives the anchor of row 0"""
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, _flags(partner, 8, 14))
    n, P = 8, 777
    rng = np.random.default_rng(15)
    x0 = bf16ref.upcast(bf16ref.rne_bf16(rng.standard_normal(P).astype(F32)))
    Gs = [bf16ref.random_bits(rng, (n, P), specials=False) for _ in range(8)]

    def grads(grp, it):
        _put_bits(grp.grads, Gs[it]) if mixed else _put(grp.grads, bf16ref.upcast(Gs[it]))

    def run(grp, its):
        for it in its:
            grads(grp, it)
            grp.sgd_communicate(LR)
            if (it + 1) % 2 == 0:
                grp.slowmo_step(LR)

    def fresh():
        grp = _sgd_group(pkg, topo, P, mixed)
        _put(grp.master_rows if mixed else grp.rows, np.tile(x0, (n, 1)))
        if mixed:
            _put_bits(grp.rows, np.tile(bf16ref.rne_bf16(x0), (n, 1)))
        grp.attach_slowmo(beta=0.5, alpha=0.9, buffers="maintain")
        return grp

    full = fresh()
    run(full, range(5))
    ckpt = full.state_dict()
    assert tuple(ckpt["slowmo_anchor"].shape) == tuple(ckpt["slowmo_momentum"].shape) == (P,)
    assert ckpt["slowmo_momentum"].any().item()
    run(full, range(5, 8))
    resumed = fresh()
    resumed.load_state_dict(ckpt)
    assert resumed.iter == 5
    run(resumed, range(5, 8))
    torch.cuda.synchronize()
    for name in ("rows", "momentum_rows", "slowmo_anchor", "slowmo_momentum") + (("master_rows",) if mixed else ()):
        a, b = getattr(full, name), getattr(resumed, name)
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), name

    for k in ("slowmo_anchor", "slowmo_momentum"):
        half = {kk: v for kk, v in ckpt.items() if kk != k}
        with pytest.raises(ValueError, match="half of the SlowMo state"):
            fresh().load_state_dict(half)
    with pytest.raises(ValueError, match="attach_slowmo"):
        _sgd_group(pkg, topo, P, mixed).load_state_dict(ckpt)
    plain = {k: v for k, v in ckpt.items() if not k.startswith("slowmo_")}
    grp = fresh()
    grp.slowmo_momentum.fill_(3.0)
    grp.load_state_dict(plain)
    torch.cuda.synchronize()
    src = grp.master_rows if mixed else grp.rows
    assert torch.equal(grp.slowmo_anchor, src[0]) and not grp.slowmo_momentum.any().item()
    assert torch.equal(src, ckpt["master_rows" if mixed else "rows"])


def test_virtual_trainer_slowmo(pkg):
    """VirtualTrainer(fused_sgd=True, slowmo_every=2) on the tiny MLP for 4 iterations: the rows are equal across
    the workers after iterations 2 and 4 (and not after 1 and 3), and the consensus log shows 0.0 there"""
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=0.5, graphid=0, lr=0.1, matcha=True, momentum=0.9)
    tr = H.VirtualTrainer(args, H.model_factory(args), n_batches=4, fused_sgd=True, slowmo_every=2,
                          consensus_every=1, slowmo_hyper={"beta": 0.5})
    assert tr.group.slowmo_hyper == {"beta": 0.5, "alpha": 1.0, "buffers": "reset", "order": 0}
    equal = []

    def hook(when, t):
        if when == "after":
            rows = t.group.rows
            equal.append(bool((rows == rows[0]).all().item()))
            if equal[-1]:
                assert torch.equal(rows[0], t.group.slowmo_anchor) and not t.group.mom_arena.any().item()

    tr.train_epoch(on_round=hook)
    assert equal == [False, True, False, True] and tr.group.iter == 4
    cons = [float(row[-2]) for row in tr.consensus_log]
    assert len(cons) == 4 and cons[1] == 0.0 and cons[3] == 0.0 and cons[0] > 0 and cons[2] > 0
    with pytest.raises(ValueError, match="slowmo_every"):
        H.VirtualTrainer(args, H.model_factory(args), n_batches=2, slowmo_every=2)
    with pytest.raises(ValueError, match="slowmo_every"):
        H.VirtualTrainer(args, H.model_factory(args), n_batches=2, fused_sgd=True, slowmo_every=0)
