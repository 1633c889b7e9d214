"""The SGD update fused into the single-GPU gossip round (csrc/sgd_mix.hip, VirtualWorkerGroup.attach_sgd).

Every comparison is against the specification restated in tests/sgdref.py, never the code under test:
x' by torch.optim.SGD's lines in float32 with exact fmas, then the oracle's mixing round on x' --
uint32 for uint32 (a NaN of any payload where the specification is a NaN, in the special-values
test only).

Shapes are the smallest at which each path can go wrong: 1-65 columns (the element path, one 16-byte
chunk, a wave's 256-column pass seam) and per row class one layout tile - 1, one tile, one tile + 9
and three tiles + 5 (the vector path, the tail, the tile seam, several work items)."""
import ctypes
import random

import numpy as np
import pytest

from conftest import LoopbackHub, Topo, special_values
from sgdref import is_nan32, same_f32, sgd_ref, spec_round

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LR = 0.1
HYPERS = {"H0": (0.0, 0.0, False), "H1": (5e-4, 0.9, False), "H2": (5e-4, 0.9, True)}   # wd, mom, nesterov
_TOPOS = {}


def _topology(pkg, name):
    """(partner int32 [M][n], alpha) of the four topologies, built once"""
    if name not in _TOPOS:
        if name == "g0":                           # graph 0, 8 workers: the 8-row class
            gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 2 / 7)
        elif name == "g16":                        # a 16-worker graph of topologies.py: the 16-row class
            gp = pkg.GraphProcessor(pkg.select_graph(2), 1.0, 0, 16, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 0.2)
        elif name == "er64":                       # ER(64, 0.1, seed 1234): the 64-row class
            random.seed(0)
            base = pkg.erdos_renyi(64, 0.1, 1234)
            np.random.seed(1234)
            gp = pkg.MatchaProcessor(base, 0.5, 0, 64, 4, False)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), float(gp.neighbor_weight))
        else:                                      # 3 workers by hand: the 8-row class with unused rows
            _TOPOS[name] = (np.array([[1, 0, -1], [-1, 2, 1]], np.int32), -2.0 ** -8)
    partner, alpha = _TOPOS[name]
    assert partner.shape[0] <= 32
    return partner, alpha


def _flag_kinds(partner, seed):
    """four kinds of rounds, three consecutive rounds each: all zero, the matching with the fewest
    pairs (leaves idle workers), every matching, random 0.5"""
    M = partner.shape[0]
    rng = np.random.default_rng(seed)
    one = np.zeros(M, np.uint8)
    one[min(range(M), key=lambda g: int((partner[g] >= 0).sum()))] = 1
    rand = (rng.random((3, M)) < 0.5).astype(np.uint8)
    rand[0, rng.integers(M)] = 1                   # at least one active round among them
    return np.concatenate([np.zeros((3, M), np.uint8), np.tile(one, (3, 1)), np.ones((3, M), np.uint8), rand])


def _shapes(pkg, n):
    T = int(pkg.lib.mx_sgd_mix_tile(n))
    assert T > 0
    return [1, 3, 4, 5, 63, 64, 65, T - 1, T, T + 9, 3 * T + 5]


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want):
    return np.array_equal(_u(got), _u(want))


def _put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


def _get(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _state(grp):
    """host copies of (x, g, m) -- m None without momentum"""
    torch.cuda.synchronize()
    return (grp.rows.cpu().numpy(), grp.grads.cpu().numpy(),
            grp.momentum_rows.cpu().numpy() if grp.momentum_rows is not None else None)


def _tails_zero(grp, P):
    arenas = [grp.arena, grp.grad_arena] + ([grp.mom_arena] if grp.mom_arena is not None else [])
    return all(not a[:, P:].view(torch.int32).any().item() for a in arenas)


@pytest.mark.parametrize("hyper", ["H0", "H1", "H2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows, hyper):
    wd, mom, nesterov = HYPERS[hyper]
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flag_kinds(partner, 5)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([len(name), len(idle_rows), n, int(hyper[1])])
    for pi, P in enumerate(_shapes(pkg, n)):
        zero = bool(pi & 1)                          # both settings of zero_grads, alternating by P
        grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows)
        grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=zero)
        assert tuple(grp.grads.shape) == (n, P) and tuple(grp.grad_arena.shape) == (n, grp.ld)
        assert (grp.momentum_rows is None) == (mom == 0)
        X = rng.standard_normal((n, P)).astype(np.float32)
        Mo = np.zeros((n, P), np.float32) if mom else None
        _put(grp.rows, X)
        for it in range(len(flags)):                 # three rounds of each kind, x and m carried throughout
            G = rng.standard_normal((n, P)).astype(np.float32)
            _put(grp.grads, G)
            ran = grp.sgd_step(it, LR)
            gx, gg, gm = _state(grp)
            wx, wm, xp = spec_round(O, X, G, Mo, partner, flags[it], alpha, (LR, wd, mom, nesterov), idle_rows)
            where = f"{name} {idle_rows} {hyper} P={P} round {it}"
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the SGD step alone: not a no-op
                assert _eq(gx, xp) and not _eq(gx, X), where
            assert _eq(gx, wx), where + ": x"
            if mom:
                assert _eq(gm, wm), where + ": m"
            assert (not gg.view(np.uint32).any()) if zero else _eq(gg, G), where + ": g"
            assert _tails_zero(grp, P), where + ": wrote past the row"
            X, Mo = gx, gm


def _run_rounds(pkg, topo, P, hyper, X, Gs, its):
    wd, mom, nesterov = HYPERS[hyper]
    grp = pkg.VirtualWorkerGroup(topo, numel=P)
    grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=False)
    _put(grp.rows, X)
    for it, G in zip(its, Gs):
        _put(grp.grads, G)
        grp.sgd_step(it, LR)
    assert _tails_zero(grp, P)
    return _state(grp)


def _spec_rounds(O, partner, flags, alpha, hyper, X, Gs, its):
    wd, mom, nesterov = HYPERS[hyper]
    Mo = np.zeros_like(X) if mom else None
    for it, G in zip(its, Gs):
        X, Mo, _ = spec_round(O, X, G, Mo, partner, flags[it], alpha, (LR, wd, mom, nesterov))
    return X, Mo


def test_persistent_loop(pkg, O):
    """grid = 3: three workgroups loop over 82 work items each holding the next item's first loads
    while it mixes -- the same bits as the default grid, and as the specification."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 2)[[6, 3, 0, 9]]
    topo = Topo(partner, alpha, flags)
    T = int(pkg.lib.mx_sgd_mix_tile(8))
    P = 40 * T + 5
    rng = np.random.default_rng(21)
    X = rng.standard_normal((8, P)).astype(np.float32)
    Gs = [rng.standard_normal((8, P)).astype(np.float32) for _ in range(4)]
    base = _run_rounds(pkg, topo, P, "H1", X, Gs, range(4))
    wx, wm = _spec_rounds(O, partner, flags, alpha, "H1", X, Gs, range(4))
    assert _eq(base[0], wx) and _eq(base[2], wm)
    assert pkg.lib.mx_sgd_mix_get(b"grid") == 0
    try:
        assert pkg.lib.mx_sgd_mix_set(b"grid", 3) == 0
        looped = _run_rounds(pkg, topo, P, "H1", X, Gs, range(4))
    finally:
        pkg.lib.mx_sgd_mix_set(b"grid", 0)
    assert _eq(looped[0], base[0]) and _eq(looped[2], base[2]) and _eq(looped[1], base[1])


@pytest.mark.parametrize("knobs", [{"nontemporal": 0}, {"nontemporal": 1, "wgpc": 5},
                                   {"flat_small": 0, "blocks_per_cu": 1}, {"grid": 2}])
def test_knobs_change_no_bits(pkg, O, knobs):
    """mx_sgd_mix_set's knobs tune speed only: every row class stays exact under each."""
    E = pkg.engine
    saved = {k: v for k, v in E.sgd_mix_tuning().items() if k in knobs}
    try:
        E.set_sgd_mix_tuning(**knobs)
        assert all(E.sgd_mix_tuning()[k] == v for k, v in knobs.items())
        for name in ("g0", "g16", "er64"):
            partner, alpha = _topology(pkg, name)
            n = partner.shape[1]
            flags = _flag_kinds(partner, 6)[[6, 3, 9]]
            topo = Topo(partner, alpha, flags)
            T = int(pkg.lib.mx_sgd_mix_tile(n))
            for P in (65, 3 * T + 5):
                rng = np.random.default_rng([P, n])
                X = rng.standard_normal((n, P)).astype(np.float32)
                Gs = [rng.standard_normal((n, P)).astype(np.float32) for _ in range(3)]
                got = _run_rounds(pkg, topo, P, "H2", X, Gs, range(3))
                wx, wm = _spec_rounds(O, partner, flags, alpha, "H2", X, Gs, range(3))
                assert _eq(got[0], wx) and _eq(got[2], wm), f"{knobs} {name} P={P}"
    finally:
        E.set_sgd_mix_tuning(**saved)
    assert pkg.lib.mx_sgd_mix_set(b"no_such_knob", 1) == pkg._lib.MX_ERR_INVALID


@pytest.mark.parametrize("where", ["x", "g"])
def test_special_values(pkg, O, where):
    """NaNs, +-Inf, +-0, denormals and +-FLT_MAX planted in x (normal g), then in g (normal x)."""
    partner, alpha = _topology(pkg, "g0")
    flags = np.ones((1, partner.shape[0]), np.uint8)
    n, P = 8, 4099
    wd, mom, nesterov = HYPERS["H1"]
    rng = np.random.default_rng(31)
    special = np.stack([special_values(P, 100 + r) for r in range(n)])
    normal = rng.standard_normal((n, P)).astype(np.float32)
    X, G = (special, normal) if where == "x" else (normal, special)
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P)
    grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=False)
    _put(grp.rows, X)
    _put(grp.grads, G)
    assert grp.sgd_step(0, LR)
    gx, gg, gm = _state(grp)
    wx, wm, _ = spec_round(O, X, G, np.zeros((n, P), np.float32), partner, flags[0], alpha, (LR, wd, mom, nesterov))
    nan = int(is_nan32(wx).sum())
    print(f"special {where}: {nan} NaN outputs of {n * P} in the specification")
    assert 0 < nan <= 0.02 * n * P                   # on the spec itself: the comparison below compares something
    assert same_f32(gx, wx), "x"
    assert same_f32(gm, wm), "m"
    assert _eq(gg, G) and _tails_zero(grp, P)


@pytest.mark.parametrize("misaligned", ["xgm", "g"])
def test_abi_unaligned_multi_segment(pkg, O, misaligned):
    """mx_sgd_mix on two-segment tables (5 and T + 3 floats) whose second segment starts one float
    past a 16-byte boundary in x, g and m -- or in g alone, which must take x and m off the 16-byte
    path too: exact, and the floats around every segment untouched."""
    E = pkg.engine
    partner, alpha = _topology(pkg, "hand3")
    flags = np.array([[1, 1], [0, 1], [0, 0]], np.uint8)
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    wd, mom, nesterov = HYPERS["H2"]
    n = 3
    T = int(pkg.lib.mx_sgd_mix_tile(n))
    lens = [5, T + 3]
    stride = T + 32
    SENT = np.float32(777.25)
    rng = np.random.default_rng(41)
    off = {k: (8, 16 + (1 if k in misaligned else 0)) for k in "xgm"}
    host, dev = {}, {}
    for k in "xgm":
        host[k] = np.full((n, stride), SENT, np.float32)
        for s in range(2):
            vals = np.zeros((n, lens[s]), np.float32) if k == "m" else rng.standard_normal((n, lens[s]))
            host[k][:, off[k][s]:off[k][s] + lens[s]] = vals
        dev[k] = torch.from_numpy(host[k]).cuda()
        assert dev[k].data_ptr() % 16 == 0 and (4 * stride) % 16 == 0

    def ptrs(k):
        return [[dev[k][r].data_ptr() + 4 * off[k][s] for s in range(2)] for r in range(n)]

    assert all((p[1] % 16 == 4) == (k in misaligned) and p[0] % 16 == 0 for k in "xgm" for p in ptrs(k))
    lay = E.SgdLayout(lens, ptrs("x"), ptrs("g"), ptrs("m"), n)
    assert lay.total_tiles == 3
    call = lay.call(eng, wd, mom, nesterov, False)

    def cat(k, a=None):
        a = host[k] if a is None else a
        return np.concatenate([a[:, off[k][s]:off[k][s] + lens[s]] for s in range(2)], axis=1)

    X, G, Mo = cat("x"), cat("g"), cat("m")
    for it in range(3):
        assert pkg.lib.mx_sgd_mix(ctypes.addressof(call), it, LR, None, pkg._lib.stream_ptr()) == 0
        X, Mo, _ = spec_round(O, X, G, Mo, partner, flags[it], alpha, (LR, wd, mom, nesterov))
    torch.cuda.synchronize()
    got = {k: dev[k].cpu().numpy() for k in "xgm"}
    assert _eq(cat("x", got["x"]), X) and _eq(cat("m", got["m"]), Mo) and _eq(got["g"], host["g"])
    for k in "xm":
        outside = np.ones(stride, bool)
        for s in range(2):
            outside[off[k][s]:off[k][s] + lens[s]] = False
        assert (got[k][:, outside] == SENT).all(), f"{k}: wrote outside its segments"


def test_refusals_launch_nothing(pkg):
    L, E = pkg.lib, pkg.engine
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=300)
    grp.attach_sgd(momentum=0.9, weight_decay=5e-4)
    X = np.random.default_rng(51).standard_normal((8, 300)).astype(np.float32)
    _put(grp.rows, X)
    _put(grp.grads, X[::-1])
    _put(grp.momentum_rows, X * 0.5)
    before = _state(grp)
    lay = grp._sgd[0]
    for field, value in (("n_slots", 9), ("n_local", 65), ("M", 33)):
        call = lay.call(grp.engine, 5e-4, 0.9, False, True)
        setattr(call, field, value)
        if field == "n_local":
            call.n_slots = 65
        assert L.mx_sgd_mix(ctypes.addressof(call), 0, LR, None, pkg._lib.stream_ptr()) == pkg._lib.MX_ERR_INVALID
        assert L.mx_sgd_mix_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, LR, None,
                               pkg._lib.stream_ptr()) == pkg._lib.MX_ERR_INVALID
    assert L.mx_sgd_mix_tile(65) == 0 and L.mx_sgd_mix_tile(64) > 0
    after = _state(grp)
    assert all(_eq(a, b) for a, b in zip(after, before))
    with pytest.raises(RuntimeError, match="already attached"):
        grp.attach_sgd()
    with pytest.raises(ValueError, match="[Nn]esterov"):
        pkg.VirtualWorkerGroup(topo, numel=100).attach_sgd(nesterov=True)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).attach_sgd()
    with pytest.raises(NotImplementedError, match="one GPU"):
        pkg.VirtualWorkerGroup(topo, numel=100, nranks=2, rank=0, comm=LoopbackHub(2).comm(0)).attach_sgd()
    with pytest.raises(NotImplementedError, match="chunk_cols"):
        pkg.VirtualWorkerGroup(topo, numel=100_000, chunk_cols=4096).attach_sgd()
    with pytest.raises(pkg.MXError, match="attach_sgd"):
        pkg.VirtualWorkerGroup(topo, numel=100).sgd_step(0, LR)


def test_graph_replay_equals_eager_steps(pkg, O):
    """sgd_device_round captured once, replayed over a 6-round schedule with fresh gradients and a
    learning rate changed after round 3 through lr_dev == six sgd_step calls on a twin; replays past
    the schedule write nothing."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    wd, mom, nesterov = HYPERS["H1"]
    n, P = 8, 2 * int(pkg.lib.mx_sgd_mix_tile(8)) + 77
    rng = np.random.default_rng(61)
    X0 = rng.standard_normal((n, P)).astype(np.float32)
    Gs = [rng.standard_normal((n, P)).astype(np.float32) for _ in range(8)]
    lrs = [0.1, 0.1, 0.1, 0.1, 0.025, 0.025]
    eager = pkg.VirtualWorkerGroup(topo, numel=P)
    eager.attach_sgd(momentum=mom, weight_decay=wd)
    _put(eager.rows, X0)
    X, Mo = X0, np.zeros_like(X0)
    for it in range(6):
        _put(eager.grads, Gs[it])
        eager.sgd_step(it, lrs[it])
        X, Mo, _ = spec_round(O, X, Gs[it], Mo, partner, flags[it], alpha, (lrs[it], wd, mom, nesterov))
    want = _state(eager)
    assert _eq(want[0], X) and _eq(want[2], Mo) and not want[1].any()

    grp = pkg.VirtualWorkerGroup(topo, numel=P)
    grp.attach_sgd(momentum=mom, weight_decay=wd)
    _put(grp.rows, X0)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            grp.sgd_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and _eq(_get(grp.rows), X0)      # capture ran nothing
    for it in range(6):
        _put(grp.grads, Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = _state(grp)
    assert all(_eq(a, b) for a, b in zip(got, want))
    _put(grp.grads, Gs[6])                           # past the schedule: no mix, no SGD step, g not zeroed
    for _ in range(2):
        g.replay()
    past = _state(grp)
    assert int(grp.iter_dev.item()) == 8
    assert _eq(past[0], want[0]) and _eq(past[2], want[2]) and _eq(past[1], Gs[6])


def _mlp():
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5)).cuda()


def test_gradient_views(pkg, O):
    """Adopted models: every p.grad is the parameter's slice of the gradient arena, backward()
    accumulates there in place, and a zero_grads step leaves zeros a second backward starts from."""
    n = 8
    torch.manual_seed(0)
    models = [_mlp() for _ in range(n)]
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, models)
    grp.attach_sgd(momentum=0.9, weight_decay=5e-4)

    def where():
        return [[p.grad.data_ptr() for p in m.parameters()] for m in models]

    want_ptrs = []
    for r, m in enumerate(models):
        off, row = 0, []
        for p in m.parameters():
            assert p.grad is not None and p.grad.shape == p.shape
            row.append(grp.grad_arena[r].data_ptr() + 4 * off)
            assert p.data_ptr() == grp.arena[r].data_ptr() + 4 * off
            off += p.numel()
        want_ptrs.append(row)
    assert where() == want_ptrs
    data = torch.randn(n, 6, 33, device="cuda")

    def backward():
        """every worker's backward(); the gradients recomputed out of place, as rows"""
        ref = []
        for r, m in enumerate(models):
            m(data[r]).square().mean().backward()
            gr = torch.autograd.grad(m(data[r]).square().mean(), list(m.parameters()))
            ref.append(torch.cat([t.reshape(-1) for t in gr]))
        return torch.stack(ref)

    ref = backward()
    assert where() == want_ptrs
    assert ref.abs().max().item() > 0 and torch.allclose(grp.grads, ref, rtol=1e-5, atol=1e-7)
    X, G, Mo = _state(grp)
    assert grp.sgd_step(0, LR)
    gx, gg, gm = _state(grp)
    wx, wm, _ = spec_round(O, X, G, Mo, partner, np.ones(partner.shape[0], np.uint8), alpha, (LR, 5e-4, 0.9, False))
    assert _eq(gx, wx) and _eq(gm, wm) and not gg.view(np.uint32).any()
    ref2 = backward()                                # on the updated parameters, accumulated from zero
    assert where() == want_ptrs
    assert torch.allclose(grp.grads, ref2, rtol=1e-5, atol=1e-7) and not torch.equal(ref2, ref)


def test_against_torch_sgd_then_step(pkg):
    """The fused launch against torch.optim.SGD.step() on 8 plain CUDA tensors followed by the
    unfused round: |diff| <= 2^-20.  Every intermediate is below 2, so a rounding is at most 2^-24;
    the two op sequences differ by at most one extra rounding in each of three ops, <= 3 * 2^-24 in
    x', which the mix (a convex combination) carries through, adding at most 2 * (deg + 1) <= 8
    roundings of its own: <= 11 * 2^-24.  A wrong coefficient or sign shows at 1e-4 or more."""
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((1, partner.shape[0]), np.uint8))
    wd, mom, nesterov = HYPERS["H2"]
    n, P = 8, 4097
    rng = np.random.default_rng(81)
    X = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    G = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    fused = pkg.VirtualWorkerGroup(topo, numel=P)
    fused.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov)
    _put(fused.rows, X)
    _put(fused.grads, G)
    assert fused.sgd_step(0, LR)
    params = [torch.nn.Parameter(torch.from_numpy(X[r].copy()).cuda()) for r in range(n)]
    for r, p in enumerate(params):
        p.grad = torch.from_numpy(G[r].copy()).cuda()
        torch.optim.SGD([p], lr=LR, momentum=mom, weight_decay=wd, nesterov=nesterov, dampening=0).step()
    twin = pkg.VirtualWorkerGroup(topo, numel=P)
    with torch.no_grad():
        twin.rows.copy_(torch.stack([p.detach() for p in params]))
    assert twin.step(0)
    a, b = _get(fused.rows).astype(np.float64), _get(twin.rows).astype(np.float64)
    diff = float(np.abs(a - b).max())
    print(f"fused vs torch.optim.SGD + step: max |diff| = {diff:.3e} ({diff * 2 ** 24:.2f} x 2^-24)")
    assert np.abs(b).max() < 2 and diff <= 2.0 ** -20


def test_virtual_trainer_fused_sgd(pkg, O):
    """harness.VirtualTrainer(fused_sgd=True): every iteration's fused launch by the specification
    from the rows, gradients and momentum rows the backward passes left; a checkpoint resumed in a
    new trainer continues bit for bit."""
    H = pkg.harness

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=0.1, matcha=True, momentum=0.9)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        return H.VirtualTrainer(args, H.model_factory(args), n_batches=3, fused_sgd=True, **kw)

    tr = make()
    grp = tr.group
    assert grp.momentum_rows is not None and grp.sgd_hyper == {"momentum": 0.9, "weight_decay": 5e-4,
                                                               "nesterov": False, "zero_grads": True}
    partner = np.asarray(tr.GP.neighbors_info, np.int32)
    state, seen = {}, {"rounds": 0}

    def hook(when, t):
        if when == "before":
            state["s"], state["it"] = _state(t.group), t.group.iter
            assert np.abs(state["s"][1]).max() > 0                    # backward() filled the gradient arena
            return
        flags = np.asarray(tr.GP.active_flags[state["it"]], np.uint8)
        lr = t.optimizers[0].param_groups[0]["lr"]
        X, G, Mo = state["s"]
        wx, wm, _ = spec_round(O, X, G, Mo, partner[:len(flags)], flags, tr.GP.neighbor_weight, (lr, 5e-4, 0.9, False))
        gx, gg, gm = _state(t.group)
        assert _eq(gx, wx) and _eq(gm, wm) and not gg.view(np.uint32).any(), f"round {state['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats)
    assert seen["rounds"] == 3 and grp.iter == 3
    assert all(not o.state for o in tr.optimizers)                    # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert _eq(ckpt["group"]["momentum_rows"].cpu().numpy(), _get(grp.momentum_rows))
    tr2 = make()
    tr2.load_state_dict(ckpt)
    assert tr2.epoch == 1 and tr2.group.iter == 3
    tr.train_epoch()
    tr2.train_epoch()
    a, b = _state(tr.group), _state(tr2.group)
    assert _eq(a[0], b[0]) and _eq(a[2], b[2]) and tr.group.iter == tr2.group.iter == 6

    # checkpoints: momentum rows missing -> zeros; present but no SGD state to take them -> refused
    bare = {k: v for k, v in ckpt["group"].items() if k != "momentum_rows"}
    tr2.group.load_state_dict(bare)
    assert not tr2.group.momentum_rows.any().item()
    plain = pkg.VirtualWorkerGroup(tr.GP, numel=grp.numel)
    with pytest.raises(ValueError, match="momentum"):
        plain.load_state_dict(ckpt["group"])
    with pytest.raises(ValueError, match="fused_sgd"):
        make(batched=True)
    with pytest.raises(ValueError, match="fused_sgd"):
        make(args={"compress": True})
