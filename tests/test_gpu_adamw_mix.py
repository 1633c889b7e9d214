"""The AdamW / Adam update fused into the single-GPU gossip round (csrc/adamw_mix.hip,
VirtualWorkerGroup.attach_adamw).

Every comparison is against the specification restated in tests/adamref.py, never the code under test:
x', m', v' by torch.optim.AdamW's / Adam's lines in float32, one rounding per operation (exact fmas,
numpy's correctly rounded sqrt and division), then the oracle's mixing round on x' -- uint32 for uint32
(a NaN of any payload where the specification is a NaN, in the special-values test only).

Shapes are those of tests/test_gpu_sgd_mix.py: 1-65 columns (the element path, one 16-byte chunk, a
wave's 256-column pass seam) and per row class one layout tile - 1, one tile, one tile + 9 and three
tiles + 5 (the vector path, the tail, the tile seam, several work items)."""
import ctypes
import random

import numpy as np
import pytest

from adamref import bias_at, bias_table, spec_round
from conftest import LoopbackHub, Topo, special_values
from sgdref import fmaf32, is_nan32, same_f32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LR = 1e-3
# beta1, beta2, eps, wd, decoupled
HYPERS = {"A0": (0.9, 0.999, 1e-8, 0.0, False),      # plain Adam
          "A1": (0.9, 0.999, 1e-8, 1e-2, True),      # AdamW
          "A2": (0.8, 0.95, 1e-6, 5e-4, False)}      # Adam with L2
_TOPOS = {}
_TABLES = {}


def _table(hyper):
    key = tuple(hyper[:2])
    if key not in _TABLES:
        _TABLES[key] = bias_table(*key)
    return _TABLES[key]


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
    T = int(pkg.lib.mx_adamw_mix_tile(n))
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
    """host copies of (x, g, m, v)"""
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (grp.rows, grp.grads, grp.exp_avg_rows, grp.exp_avg_sq_rows))


def _tails_zero(grp, P):
    arenas = [grp.arena, grp.grad_arena, grp.exp_avg_arena, grp.exp_avg_sq_arena]
    return all(not a[:, P:].view(torch.int32).any().item() for a in arenas)


def _attach(grp, hyper, zero_grads):
    b1, b2, eps, wd, decoupled = HYPERS[hyper]
    grp.attach_adamw(betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=decoupled, zero_grads=zero_grads)


def _grads(rng, shape):
    """gradients of the scale Adam sees (0.01 N(0, 1)), a tenth of them 100 x larger"""
    g = 0.01 * rng.standard_normal(shape)
    g[rng.random(shape) < 0.1] *= 100
    return g.astype(np.float32)


@pytest.mark.parametrize("hyper", ["A0", "A1", "A2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows, hyper):
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flag_kinds(partner, 5)
    topo = Topo(partner, alpha, flags)
    table = _table(HYPERS[hyper])
    rng = np.random.default_rng([len(name), len(idle_rows), n, int(hyper[1])])
    for pi, P in enumerate(_shapes(pkg, n)):
        zero = bool(pi & 1)                          # both settings of zero_grads, alternating by P
        grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows)
        _attach(grp, hyper, zero)
        assert tuple(grp.grads.shape) == (n, P) and tuple(grp.grad_arena.shape) == (n, grp.ld)
        assert tuple(grp.exp_avg_rows.shape) == tuple(grp.exp_avg_sq_rows.shape) == (n, P)
        assert grp.opt_step == 0 and int(grp.opt_step_dev.item()) == 1
        X = rng.uniform(-1, 1, (n, P)).astype(np.float32)
        Mo, V = np.zeros((n, P), np.float32), np.zeros((n, P), np.float32)
        _put(grp.rows, X)
        for it in range(len(flags)):                 # three rounds of each kind; x, m, v and the step carried
            G = _grads(rng, (n, P))
            _put(grp.grads, G)
            ran = grp.adamw_step(it, LR)
            gx, gg, gm, gv = _state(grp)
            wx, wm, wv, xp = spec_round(O, X, G, Mo, V, it + 1, partner, flags[it], alpha, LR, HYPERS[hyper], table,
                                        idle_rows)
            where = f"{name} {idle_rows} {hyper} P={P} round {it}"
            assert grp.opt_step == it + 1, where
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the optimizer step alone: not a no-op
                assert _eq(gx, xp) and not _eq(gx, X), where
            assert _eq(gx, wx), where + ": x"
            assert _eq(gm, wm), where + ": m"
            assert _eq(gv, wv), where + ": v"
            assert (not gg.view(np.uint32).any()) if zero else _eq(gg, G), where + ": g"
            assert _tails_zero(grp, P), where + ": wrote past the row"
            X, Mo, V = gx, gm, gv


def test_bias_table_seam(pkg, O):
    """betas (0.5, 0.5): a table of a few dozen rows.  The steps n_bias - 1, n_bias, n_bias + 1 and
    10^9 (the last three read the table's last row) each match the specification."""
    hyper = (0.5, 0.5, 1e-8, 1e-2, True)
    table = bias_table(0.5, 0.5)
    nb = len(table)
    assert 12 <= nb <= 64 and tuple(table[-1]) == (1.0, 1.0) and tuple(table[-2]) != (1.0, 1.0)
    partner, alpha = _topology(pkg, "g0")
    flags = np.ones((1, partner.shape[0]), np.uint8)
    n, P = 8, 1029
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P)
    grp.attach_adamw(betas=(0.5, 0.5), eps=1e-8, weight_decay=1e-2, zero_grads=False)
    assert grp._adamw[0].n_bias == nb
    rng = np.random.default_rng(71)
    X = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    Mo = _grads(rng, (n, P))
    V = (Mo * Mo).astype(np.float32)
    _put(grp.rows, X)
    _put(grp.exp_avg_rows, Mo)
    _put(grp.exp_avg_sq_rows, V)
    for t in (nb - 1, nb, nb + 1, 10 ** 9):
        assert bias_at(table, t) == ((np.float32(1), np.float32(1)) if t >= nb else tuple(table[nb - 2]))
        G = _grads(rng, (n, P))
        _put(grp.grads, G)
        grp.opt_step = t - 1
        assert grp.adamw_step(0, LR) and grp.opt_step == t
        X, Mo, V, _ = spec_round(O, X, G, Mo, V, t, partner, flags[0], alpha, LR, hyper, table)
        gx, _, gm, gv = _state(grp)
        assert _eq(gx, X) and _eq(gm, Mo) and _eq(gv, V), f"step {t}"


@pytest.mark.parametrize("where", ["x", "g", "g_edge"])
def test_special_values(pkg, O, where):
    """NaNs, +-Inf, +-0, denormals and +-FLT_MAX planted in x (normal g), then in g (normal x); then
    the gradients at which Adam's own arithmetic leaves the normal range: g = 0 on zero state
    (den = eps, x only decays), |g| = 1e-20 (g^2 denormal: the square root of a denormal), 1e-30 (g^2
    underflows to zero) and 1e20 (v overflows to Inf) -- two steps, so the second starts from that
    state."""
    partner, alpha = _topology(pkg, "g0")
    flags = np.ones((2, partner.shape[0]), np.uint8)
    n, P = 8, 4099
    hyper = HYPERS["A1"]
    table = _table(hyper)
    rng = np.random.default_rng(31)
    special = np.stack([special_values(P, 100 + r) for r in range(n)])
    normal = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    if where == "x":
        X, G = special, _grads(rng, (n, P))
    elif where == "g":
        X, G = normal, special
    else:
        X, G = normal, _grads(rng, (n, P))
        edge = np.array([0.0, -0.0, 1e-20, -1e-20, 1e-30, -1e-30, 1e20, -1e20, 1e-42, 3e38], np.float32)
        for r in range(n):
            pos = rng.permutation(P)[:4 * len(edge)]
            G[r, pos] = np.tile(edge, 4)
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P)
    _attach(grp, "A1", False)
    _put(grp.rows, X)
    Mo, V = np.zeros((n, P), np.float32), np.zeros((n, P), np.float32)
    for step in (1, 2):
        _put(grp.grads, G)
        assert grp.adamw_step(step - 1, LR)
        gx, gg, gm, gv = _state(grp)
        wx, wm, wv, xp = spec_round(O, X, G, Mo, V, step, partner, flags[0], alpha, LR, hyper, table)
        nan = int(is_nan32(wx).sum())
        print(f"special {where} step {step}: {nan} NaN outputs of {n * P} in the specification")
        if where == "g_edge":                        # on the spec itself: the cases are what the docstring says
            with np.errstate(all="ignore"):
                sq = G * G
            assert nan == 0 and np.isinf(wv).any() and (wv == 0).any()
            assert ((sq > 0) & (sq < 1.1754944e-38)).any() and ((G != 0) & (sq == 0)).any()
            if step == 1:                            # g = 0 on zero state: x only decays
                z = G == 0
                decay = fmaf32(-np.float32(LR), np.float32(hyper[3]), np.float32(1))
                assert z.any() and not wm[z].any() and _eq(xp[z], X[z] * decay)
        else:
            assert 0 < nan <= 0.04 * n * P           # the comparison below compares something
        assert same_f32(gx, wx), f"x, step {step}"
        assert same_f32(gm, wm), f"m, step {step}"
        assert same_f32(gv, wv), f"v, step {step}"
        assert _eq(gg, G) and _tails_zero(grp, P)
        X, Mo, V = gx, gm, gv
        if where != "g_edge":
            break                                    # one step: NaNs spread along the matchings


@pytest.mark.parametrize("misaligned", ["xgmv", "g", "v"])
def test_abi_unaligned_multi_segment(pkg, O, misaligned):
    """mx_adamw_mix on two-segment tables (5 and T + 3 floats) whose second segment starts one float
    past a 16-byte boundary in all four arrays -- or in g alone, or in v alone, which must take the
    other three off the 16-byte path too: exact, and the guard floats around every segment untouched
    (g's too, under zero_grads)."""
    E = pkg.engine
    partner, alpha = _topology(pkg, "hand3")
    flags = np.array([[1, 1], [0, 1], [0, 0]], np.uint8)
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    hyper = HYPERS["A2"]
    table = _table(hyper)
    n = 3
    T = int(pkg.lib.mx_adamw_mix_tile(n))
    lens = [5, T + 3]
    stride = T + 32
    SENT = np.float32(777.25)
    rng = np.random.default_rng(41)
    off = {k: (8, 16 + (1 if k in misaligned else 0)) for k in "xgmv"}
    host, dev = {}, {}
    for k in "xgmv":
        host[k] = np.full((n, stride), SENT, np.float32)
        for s in range(2):
            vals = np.zeros((n, lens[s]), np.float32) if k in "mv" else rng.uniform(-1, 1, (n, lens[s]))
            host[k][:, off[k][s]:off[k][s] + lens[s]] = vals
        dev[k] = torch.from_numpy(host[k]).cuda()
        assert dev[k].data_ptr() % 16 == 0 and (4 * stride) % 16 == 0

    def ptrs(k):
        return [[dev[k][r].data_ptr() + 4 * off[k][s] for s in range(2)] for r in range(n)]

    assert all((p[1] % 16 == 4) == (k in misaligned) and p[0] % 16 == 0 for k in "xgmv" for p in ptrs(k))
    lay = E.AdamwLayout(lens, ptrs("x"), ptrs("g"), ptrs("m"), ptrs("v"), n, table)
    assert lay.total_tiles == 3 and lay.n_bias == len(table)
    call = lay.call(eng, hyper[:2], hyper[2], hyper[3], hyper[4], True)

    def cat(k, a=None):
        a = host[k] if a is None else a
        return np.concatenate([a[:, off[k][s]:off[k][s] + lens[s]] for s in range(2)], axis=1)

    X, G, Mo, V = cat("x"), cat("g"), cat("m"), cat("v")
    for it in range(3):
        assert pkg.lib.mx_adamw_mix(ctypes.addressof(call), it, it + 1, LR, None, pkg._lib.stream_ptr()) == 0
        X, Mo, V, _ = spec_round(O, X, G, Mo, V, it + 1, partner, flags[it], alpha, LR, hyper, table)
        G = np.zeros_like(G)                         # zero_grads: the later steps see zeros
    torch.cuda.synchronize()
    got = {k: dev[k].cpu().numpy() for k in "xgmv"}
    assert _eq(cat("x", got["x"]), X) and _eq(cat("m", got["m"]), Mo) and _eq(cat("v", got["v"]), V)
    assert not cat("g", got["g"]).view(np.uint32).any()
    for k in "xgmv":
        outside = np.ones(stride, bool)
        for s in range(2):
            outside[off[k][s]:off[k][s] + lens[s]] = False
        assert (got[k][:, outside] == SENT).all(), f"{k}: wrote outside its segments"


def _run_rounds(pkg, topo, P, hyper, X, Gs, its):
    grp = pkg.VirtualWorkerGroup(topo, numel=P)
    _attach(grp, hyper, False)
    _put(grp.rows, X)
    for it, G in zip(its, Gs):
        _put(grp.grads, G)
        grp.adamw_step(it, LR)
    assert _tails_zero(grp, P)
    return _state(grp)


def _spec_rounds(O, partner, flags, alpha, hyper, X, Gs, its):
    Mo, V = np.zeros_like(X), np.zeros_like(X)
    for t, (it, G) in enumerate(zip(its, Gs)):
        X, Mo, V, _ = spec_round(O, X, G, Mo, V, t + 1, partner, flags[it], alpha, LR, HYPERS[hyper], _table(HYPERS[hyper]))
    return X, Mo, V


@pytest.mark.parametrize("knobs", [{"nontemporal": 0}, {"nontemporal": 1, "wgpc": 5},
                                   {"flat_small": 0, "blocks_per_cu": 1}, {"grid": 2}])
def test_knobs_change_no_bits(pkg, O, knobs):
    """mx_adamw_mix_set's knobs tune speed only: every row class stays exact under each (grid = 2:
    two workgroups loop over the work items, each holding the next item's first loads while it mixes)."""
    E = pkg.engine
    saved = {k: v for k, v in E.adamw_mix_tuning().items() if k in knobs}
    try:
        E.set_adamw_mix_tuning(**knobs)
        assert all(E.adamw_mix_tuning()[k] == v for k, v in knobs.items())
        for name in ("g0", "g16", "er64"):
            partner, alpha = _topology(pkg, name)
            n = partner.shape[1]
            flags = _flag_kinds(partner, 6)[[6, 3, 9]]
            topo = Topo(partner, alpha, flags)
            T = int(pkg.lib.mx_adamw_mix_tile(n))
            for P in (65, 3 * T + 5):
                rng = np.random.default_rng([P, n])
                X = rng.uniform(-1, 1, (n, P)).astype(np.float32)
                Gs = [_grads(rng, (n, P)) for _ in range(3)]
                got = _run_rounds(pkg, topo, P, "A2", X, Gs, range(3))
                wx, wm, wv = _spec_rounds(O, partner, flags, alpha, "A2", X, Gs, range(3))
                assert _eq(got[0], wx) and _eq(got[2], wm) and _eq(got[3], wv), f"{knobs} {name} P={P}"
    finally:
        E.set_adamw_mix_tuning(**saved)
    assert pkg.lib.mx_adamw_mix_set(b"no_such_knob", 1) == pkg._lib.MX_ERR_INVALID


def test_refusals_launch_nothing(pkg):
    L, E, INVALID = pkg.lib, pkg.engine, pkg._lib.MX_ERR_INVALID
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=300)
    grp.attach_adamw()
    X = np.random.default_rng(51).uniform(-1, 1, (8, 300)).astype(np.float32)
    _put(grp.rows, X)
    _put(grp.grads, X[::-1])
    _put(grp.exp_avg_rows, X * 0.5)
    _put(grp.exp_avg_sq_rows, X * X)
    before = _state(grp)
    lay = grp._adamw[0]
    sp = pkg._lib.stream_ptr

    def fresh():
        return lay.call(grp.engine, (0.9, 0.999), 1e-8, 1e-2, True, True)

    one = torch.ones(1, dtype=torch.int64, device="cuda")
    for field, value in (("n_slots", 9), ("n_local", 65), ("M", 33)):
        call = fresh()
        setattr(call, field, value)
        if field == "n_local":
            call.n_slots = 65
        assert L.mx_adamw_mix(ctypes.addressof(call), 0, 1, LR, None, sp()) == INVALID
        assert L.mx_adamw_mix_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, one.data_ptr(), LR, None,
                                 sp()) == INVALID
    assert L.mx_adamw_mix_tile(65) == 0 and L.mx_adamw_mix_tile(64) > 0
    call = fresh()
    for step in (0, -3):                             # no such optimizer step
        assert L.mx_adamw_mix(ctypes.addressof(call), 0, step, LR, None, sp()) == INVALID
    assert all(_eq(a, b) for a, b in zip(_state(grp), before))

    # refusals made by the launch itself, on the device: nothing is written
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    for it_value, step_value in ((2, 1), (-1, 1), (0, 0), (1, -5)):     # round outside [0, 2); step below 1
        ctr.fill_(it_value)
        one.fill_(step_value)
        assert L.mx_adamw_mix_at(ctypes.addressof(call), ctr.data_ptr(), 2, one.data_ptr(), LR, None, sp()) == 0
        assert all(_eq(a, b) for a, b in zip(_state(grp), before)), (it_value, step_value)
    eng = grp.engine                                 # a peer-reads record is not this kernel's
    assert L.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, eng.n_local, eng.M, 1, sp()) == 0
    assert L.mx_adamw_mix(ctypes.addressof(call), 0, 1, LR, None, sp()) == 0
    assert all(_eq(a, b) for a, b in zip(_state(grp), before))
    assert L.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, eng.n_local, eng.M, 0, sp()) == 0
    assert grp.adamw_step(0, LR) and not _eq(_get(grp.rows), before[0])   # and with the bit cleared it runs

    with pytest.raises(RuntimeError, match="already attached"):
        grp.attach_adamw()
    with pytest.raises(RuntimeError, match="AdamW"):
        grp.attach_sgd()
    sgd = pkg.VirtualWorkerGroup(topo, numel=100)
    sgd.attach_sgd(momentum=0.9)
    with pytest.raises(RuntimeError, match="SGD"):
        sgd.attach_adamw()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).attach_adamw()
    with pytest.raises(NotImplementedError, match="one GPU"):
        pkg.VirtualWorkerGroup(topo, numel=100, nranks=2, rank=0, comm=LoopbackHub(2).comm(0)).attach_adamw()
    with pytest.raises(NotImplementedError, match="chunk_cols"):
        pkg.VirtualWorkerGroup(topo, numel=100_000, chunk_cols=4096).attach_adamw()
    with pytest.raises(ValueError):
        pkg.VirtualWorkerGroup(topo, numel=100).attach_adamw(betas=(0.9, 1.0 - 2.0 ** -24))
    with pytest.raises(pkg.MXError, match="attach_adamw"):
        pkg.VirtualWorkerGroup(topo, numel=100).adamw_step(0, LR)


def test_graph_replay_equals_eager_steps(pkg, O):
    """adamw_device_round captured once, replayed over a 6-round schedule with fresh gradients and a
    learning rate changed after round 3 through lr_dev == six adamw_step calls on a twin == the
    specification; both device counters advance by one per replay, and a replay past the schedule
    writes nothing."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    hyper = HYPERS["A1"]
    table = _table(hyper)
    n, P = 8, 2 * int(pkg.lib.mx_adamw_mix_tile(8)) + 77
    rng = np.random.default_rng(61)
    X0 = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    Gs = [_grads(rng, (n, P)) for _ in range(7)]
    lrs = [1e-3, 1e-3, 1e-3, 1e-3, 2.5e-4, 2.5e-4]
    eager = pkg.VirtualWorkerGroup(topo, numel=P)
    _attach(eager, "A1", True)
    _put(eager.rows, X0)
    X, Mo, V = X0, np.zeros_like(X0), np.zeros_like(X0)
    for it in range(6):
        _put(eager.grads, Gs[it])
        eager.adamw_step(it, lrs[it])
        X, Mo, V, _ = spec_round(O, X, Gs[it], Mo, V, it + 1, partner, flags[it], alpha, lrs[it], hyper, table)
    want = _state(eager)
    assert _eq(want[0], X) and _eq(want[2], Mo) and _eq(want[3], V) and not want[1].any()

    grp = pkg.VirtualWorkerGroup(topo, numel=P)
    _attach(grp, "A1", True)
    _put(grp.rows, X0)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            grp.adamw_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and int(grp.opt_step_dev.item()) == 1      # capture ran nothing
    assert _eq(_get(grp.rows), X0)
    for it in range(6):
        _put(grp.grads, Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = _state(grp)
    assert all(_eq(a, b) for a, b in zip(got, want))
    assert int(grp.iter_dev.item()) == 6 and int(grp.opt_step_dev.item()) == 7
    _put(grp.grads, Gs[6])                           # past the schedule: no mix, no step, g not zeroed
    g.replay()
    past = _state(grp)
    assert int(grp.iter_dev.item()) == 7 and int(grp.opt_step_dev.item()) == 8
    assert _eq(past[0], want[0]) and _eq(past[2], want[2]) and _eq(past[3], want[3]) and _eq(past[1], Gs[6])


def _mlp():
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5)).cuda()


def test_gradient_views_and_checkpoint(pkg, O):
    """Adopted models: every p.grad is the parameter's slice of the gradient arena and backward()
    accumulates there.  state_dict -> a new group -> attach_adamw -> load_state_dict -> a step equals
    the uninterrupted run, bit for bit; a checkpoint with Adam state is refused by a plain group."""
    n = 8
    torch.manual_seed(0)
    models = [_mlp() for _ in range(n)]
    partner, alpha = _topology(pkg, "g0")
    flags = np.ones((4, partner.shape[0]), np.uint8)
    topo = Topo(partner, alpha, flags)
    hyper = HYPERS["A1"]
    table = _table(hyper)
    grp = pkg.VirtualWorkerGroup(topo, models)
    _attach(grp, "A1", True)
    for r, m in enumerate(models):
        off = 0
        for p in m.parameters():
            assert p.grad is not None and p.grad.shape == p.shape
            assert p.grad.data_ptr() == grp.grad_arena[r].data_ptr() + 4 * off
            assert p.data_ptr() == grp.arena[r].data_ptr() + 4 * off
            off += p.numel()
    data = torch.randn(n, 6, 33, device="cuda")
    ref = []
    for r, m in enumerate(models):
        m(data[r]).square().mean().backward()
        gr = torch.autograd.grad(m(data[r]).square().mean(), list(m.parameters()))
        ref.append(torch.cat([t.reshape(-1) for t in gr]))
    ref = torch.stack(ref)
    assert ref.abs().max().item() > 0 and torch.allclose(grp.grads, ref, rtol=1e-5, atol=1e-7)
    X, G, Mo, V = _state(grp)
    assert grp.adamw_step(0, LR)
    wx, wm, wv, _ = spec_round(O, X, G, Mo, V, 1, partner, flags[0], alpha, LR, hyper, table)
    gx, gg, gm, gv = _state(grp)
    assert _eq(gx, wx) and _eq(gm, wm) and _eq(gv, wv) and not gg.view(np.uint32).any()

    rng = np.random.default_rng(91)
    G2, G3 = _grads(rng, G.shape), _grads(rng, G.shape)
    _put(grp.grads, G2)
    grp.adamw_step(1, LR)
    grp.iter = 2
    ckpt = grp.state_dict()
    assert ckpt["opt_step"] == 2 and _eq(ckpt["exp_avg_rows"].cpu().numpy(), _get(grp.exp_avg_rows))
    assert _eq(ckpt["exp_avg_sq_rows"].cpu().numpy(), _get(grp.exp_avg_sq_rows))
    _put(grp.grads, G3)
    grp.adamw_step(2, LR)
    want = _state(grp)

    twin = pkg.VirtualWorkerGroup(topo, numel=grp.numel)
    _attach(twin, "A1", True)
    twin.load_state_dict(ckpt)
    assert twin.opt_step == 2 and int(twin.opt_step_dev.item()) == 3 and twin.iter == 2
    _put(twin.grads, G3)
    twin.adamw_step(2, LR)
    got = _state(twin)
    assert all(_eq(a, b) for a, b in zip(got, want))

    plain = pkg.VirtualWorkerGroup(topo, numel=grp.numel)
    assert sorted(plain.state_dict()) == ["iter", "kind", "row_base", "rows", "workers"]    # today's checkpoint
    with pytest.raises(ValueError, match="attach_adamw"):
        plain.load_state_dict(ckpt)
    bare = {k: v for k, v in ckpt.items() if k not in ("exp_avg_rows", "exp_avg_sq_rows", "opt_step")}
    plain.load_state_dict(bare)
    twin.load_state_dict(bare)                       # no Adam state in it: zero buffers, step 0
    assert not twin.exp_avg_rows.any().item() and not twin.exp_avg_sq_rows.any().item()
    assert twin.opt_step == 0 and int(twin.opt_step_dev.item()) == 1
    with pytest.raises(RuntimeError):
        twin.attach_sgd()
    with pytest.raises(NotImplementedError):
        pkg.VirtualWorkerGroup(topo, numel=64, dtype=torch.bfloat16).attach_adamw()


# max |fused - (torch.optim.AdamW.step() + group.step)| measured on an MI355X for the run below
# (DESIGN 6c); the test asserts twice that
TORCH_GPU_MEASURED = 2.0 ** -24      # 5.96e-08 at every one of the 5 steps


def test_against_torch_adamw_then_step(pkg):
    """The fused launches against torch.optim.AdamW.step() on 8 plain CUDA tensors followed by the
    unfused round, 5 steps, x in [-1, 1).  The uint32 comparisons above are the gate; this one says
    that the contract is torch's algorithm on the GPU as well, up to the rounding order of torch's
    kernels."""
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((5, partner.shape[0]), np.uint8))
    b1, b2, eps, wd, _ = HYPERS["A1"]
    n, P = 8, 4097
    rng = np.random.default_rng(81)
    X = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    fused = pkg.VirtualWorkerGroup(topo, numel=P)
    _attach(fused, "A1", True)
    _put(fused.rows, X)
    params = [torch.nn.Parameter(torch.from_numpy(X[r].copy()).cuda()) for r in range(n)]
    opts = [torch.optim.AdamW([p], lr=LR, betas=(b1, b2), eps=eps, weight_decay=wd) for p in params]
    twin = pkg.VirtualWorkerGroup(topo, numel=P)
    worst = 0.0
    for it in range(5):
        G = _grads(rng, (n, P))
        _put(fused.grads, G)
        assert fused.adamw_step(it, LR)
        for r, p in enumerate(params):
            p.grad = torch.from_numpy(G[r].copy()).cuda()
            opts[r].step()
        with torch.no_grad():
            twin.rows.copy_(torch.stack([p.detach() for p in params]))
            assert twin.step(it)
            for r, p in enumerate(params):
                p.copy_(twin.rows[r])
        a, b = _get(fused.rows).astype(np.float64), _get(twin.rows).astype(np.float64)
        diff = float(np.abs(a - b).max())
        worst = max(worst, diff)
        print(f"step {it + 1}: fused vs torch.optim.AdamW + step: max |diff| = {diff:.3e} ({diff * 2 ** 24:.2f} x 2^-24)")
    assert np.abs(b).max() < 1.01 and worst <= 2 * TORCH_GPU_MEASURED


def test_virtual_trainer_fused_adamw(pkg, O):
    """harness.VirtualTrainer(fused_adamw=True): every iteration's fused launch by the specification
    from the rows, gradients and Adam state the backward passes left; a checkpoint resumed in a new
    trainer continues bit for bit."""
    H = pkg.harness

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=1e-3, matcha=True, warmup=False)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        kw.setdefault("fused_adamw", True)
        return H.VirtualTrainer(args, H.model_factory(args), n_batches=3, **kw)

    tr = make()
    grp = tr.group
    assert grp.adamw_hyper == {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 5e-4, "decoupled": True,
                               "zero_grads": True}
    hyper = (0.9, 0.999, 1e-8, 5e-4, True)
    table = _table(hyper)
    partner = np.asarray(tr.GP.neighbors_info, np.int32)
    state, seen = {}, {"rounds": 0}

    def hook(when, t):
        if when == "before":
            state["s"], state["it"], state["step"] = _state(t.group), t.group.iter, t.group.opt_step
            assert np.abs(state["s"][1]).max() > 0                    # backward() filled the gradient arena
            return
        flags = np.asarray(tr.GP.active_flags[state["it"]], np.uint8)
        lr = t.optimizers[0].param_groups[0]["lr"]
        X, G, Mo, V = state["s"]
        wx, wm, wv, _ = spec_round(O, X, G, Mo, V, state["step"] + 1, partner[:len(flags)], flags,
                                   tr.GP.neighbor_weight, lr, hyper, table)
        gx, gg, gm, gv = _state(t.group)
        assert _eq(gx, wx) and _eq(gm, wm) and _eq(gv, wv) and not gg.view(np.uint32).any(), f"round {state['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats)
    assert seen["rounds"] == 3 and grp.iter == 3 and grp.opt_step == 3
    assert all(not o.state for o in tr.optimizers)                    # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert ckpt["group"]["opt_step"] == 3
    tr2 = make()
    tr2.load_state_dict(ckpt)
    assert tr2.epoch == 1 and tr2.group.iter == 3 and tr2.group.opt_step == 3
    tr.train_epoch()
    tr2.train_epoch()
    a, b = _state(tr.group), _state(tr2.group)
    assert _eq(a[0], b[0]) and _eq(a[2], b[2]) and _eq(a[3], b[3]) and tr.group.opt_step == tr2.group.opt_step == 6
    with pytest.raises(ValueError, match="fused_adamw"):
        make(batched=True)
    with pytest.raises(ValueError, match="fused_adamw"):
        make(args={"compress": True})
    with pytest.raises(ValueError, match="mutually exclusive"):
        make(fused_sgd=True)
