"""Mixed-precision SGD fused into the bf16 gossip round (csrc/sgd_mix_bf16.hip,
VirtualWorkerGroup.attach_sgd(master_weights=True)): fp32 master rows w and momentum m, bfloat16
gradients g, bfloat16 model rows p = bf16(w).

Every comparison is against the specification restated in tests/sgdbf16ref.py, never the code under
test: w and m uint32 for uint32, p uint16 for uint16 (a NaN of any payload where the specification is
a NaN, in the special-values test only).

Shapes are the smallest at which each path can go wrong: 1-9 columns (the element path, one and two
4-element chunks), 63-65 (a wave's seam), 255-257 (a 256-column pass seam) and per row class one layout
tile - 1, one tile, one tile + 9 and three tiles + 5 (the vector path, the tail, the tile seam, several
work items)."""
import ctypes
import random

import numpy as np
import pytest

import bf16ref
from conftest import LoopbackHub, Topo, special_values
from sgdbf16ref import eq32, sgd_only, spec_round, u32
from sgdref import is_nan32, same_f32

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
    T = int(pkg.lib.mx_sgd_mix_bf16_tile(n))
    assert T > 0
    return [1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, T - 1, T, T + 9, 3 * T + 5]


def _put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


def _put_bits(t, bits):
    """bfloat16 bit patterns (uint16) into a bfloat16 tensor"""
    t.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)))


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _state(grp):
    """host copies of (w, g bits, m, p bits) -- m None without momentum"""
    torch.cuda.synchronize()
    return (grp.master_rows.cpu().numpy(), _bits(grp.grads),
            grp.momentum_rows.cpu().numpy() if grp.momentum_rows is not None else None, _bits(grp.rows))


def _same_state(a, b):
    return eq32(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and \
        ((a[2] is None and b[2] is None) or eq32(a[2], b[2]))


def _tails_zero(grp, P):
    arenas = [(grp.arena, torch.int16), (grp.grad_arena, torch.int16), (grp.master_arena, torch.int32)]
    if grp.mom_arena is not None:
        arenas.append((grp.mom_arena, torch.int32))
    return all(not a[:, P:].view(dt).any().item() for a, dt in arenas)


def _group(pkg, topo, P, hyper, zero, idle_rows="skip"):
    wd, mom, nesterov = HYPERS[hyper]
    grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows, dtype=torch.bfloat16)
    grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=zero, master_weights=True)
    return grp


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
        grp = _group(pkg, topo, P, hyper, zero, idle_rows)
        assert tuple(grp.grads.shape) == (n, P) and tuple(grp.grad_arena.shape) == (n, grp.ld)
        assert grp.grad_arena.dtype == torch.bfloat16 and grp.master_arena.dtype == torch.float32
        assert tuple(grp.master_rows.shape) == (n, P) and tuple(grp.master_arena.shape) == (n, grp.ld)
        assert (grp.momentum_rows is None) == (mom == 0)
        W = rng.standard_normal((n, P)).astype(np.float32)       # low mantissa bits populated: p != widened w
        Mo = np.zeros((n, P), np.float32) if mom else None
        _put(grp.master_rows, W)
        for it in range(len(flags)):                 # three rounds of each kind, w and m carried throughout
            G = bf16ref.random_bits(rng, (n, P), specials=False)
            _put_bits(grp.grads, G)
            ran = grp.sgd_step(it, LR)
            gw, gg, gm, gp = _state(grp)
            ww, wm, wp, wprime = spec_round(O, W, G, Mo, partner, flags[it], alpha, (LR, wd, mom, nesterov), idle_rows)
            where = f"{name} {idle_rows} {hyper} P={P} round {it}"
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the SGD step alone: not a no-op, and p follows
                assert eq32(gw, wprime) and not eq32(gw, W), where
                assert np.array_equal(gp, bf16ref.rne_bf16(wprime)), where
            assert eq32(gw, ww), where + ": w"
            if mom:
                assert eq32(gm, wm), where + ": m"
            assert bf16ref.same_bf16(gp, wp), where + ": p"
            assert (not gg.any()) if zero else np.array_equal(gg, G), where + ": g"
            assert _tails_zero(grp, P), where + ": wrote past the row"
            W, Mo = gw, gm
        if P > 64:
            assert not np.array_equal(u32(bf16ref.upcast(gp)), u32(gw)), "p is the rounded image, not the master"


def test_small_updates_are_not_lost(pkg):
    """All-zero flags (the SGD step alone), wd = 0, mom = 0, lr = 2^-12, every master 1.0, every
    gradient 1.0: each step takes 2^-12 off the master exactly.  After 256 steps every master is
    exactly 0.9375 and every p is bf16(0.9375); a pure-bf16 update would still hold 1.0, since 2^-12
    is below half a bf16 ulp below 1 (2^-9).

    p = bf16_rne(w) by the contract, so p stays bf16(1.0) through step 8 (w = 1 - 2^-9 is the tie
    between 0x3F7F and 0x3F80, and goes to the even 0x3F80) while the masters move, and first moves at
    step 9 (w = 0.997802734375 -> 0x3F7F).  (The issue text puts that first move at step 129; with
    lr = 2^-12 and p = bf16_rne(w) that figure cannot hold -- 129 steps take the master to 0.9685 --
    so the steps asserted here are the ones the contract gives.  Every step is also compared with the
    specification.)"""
    partner, alpha = _topology(pkg, "g0")
    steps = 256
    topo = Topo(partner, alpha, np.zeros((steps, partner.shape[0]), np.uint8))
    n, P = 8, 1029
    grp = _group(pkg, topo, P, "H0", False)
    one = np.full((n, P), 0x3F80, np.uint16)
    _put(grp.master_rows, np.ones((n, P), np.float32))
    _put_bits(grp.grads, one)
    _put_bits(grp.rows, one)
    W = np.ones((n, P), np.float32)
    lr = 2.0 ** -12
    for it in range(steps):
        assert grp.sgd_step(it, lr) is False
        if it + 1 in (1, 8, 9, 100, 256):
            gw, gg, _, gp = _state(grp)
            want_w = np.full((n, P), 1.0 - (it + 1) * lr, np.float32)
            assert eq32(gw, want_w) and np.array_equal(gp, bf16ref.rne_bf16(want_w)) and np.array_equal(gg, one)
            if it + 1 <= 8:                          # the masters have moved, p has not
                assert (gp == 0x3F80).all() and (gw < 1.0).all()
            if it + 1 == 9:
                assert (gp == 0x3F7F).all()
    for it in range(3):                              # the specification agrees with the closed form
        W, _, p = sgd_only(W, one, None, (lr, 0.0, 0.0, False))
        assert float(W[0, 0]) == 1.0 - (it + 1) * lr and int(p[0, 0]) == 0x3F80
    gw, _, _, gp = _state(grp)
    assert (gw == np.float32(0.9375)).all() and (gp == 0x3F70).all()
    assert bf16ref.rne_bf16(np.float32([0.9375]))[0] == 0x3F70
    # the pure-bf16 update: bf16(1.0 - 2^-12) is 1.0 again
    assert bf16ref.rne_bf16(np.float32([1.0 - lr]))[0] == 0x3F80
    assert _tails_zero(grp, P)


@pytest.mark.parametrize("where", ["w", "g"])
def test_special_values(pkg, O, where):
    """NaNs, +-Inf, +-0, subnormals and the largest finite values planted in the masters (normal g),
    then in the gradients (normal w); the masters include the largest finite fp32, which rounds up to
    bf16 Inf at the store."""
    partner, alpha = _topology(pkg, "g0")
    flags = np.ones((1, partner.shape[0]), np.uint8)
    n, P = 8, 4099
    wd, mom, nesterov = HYPERS["H1"]
    rng = np.random.default_rng(31)
    if where == "w":
        W = np.stack([special_values(P, 100 + r) for r in range(n)])
        G = bf16ref.random_bits(rng, (n, P), specials=False)
    else:
        W = rng.standard_normal((n, P)).astype(np.float32)
        G = bf16ref.random_bits(rng, (n, P), specials=True)
        assert all((G == s).any() for s in bf16ref.SPECIALS)
    topo0 = Topo(partner, alpha, np.zeros((1, partner.shape[0]), np.uint8))
    for topo, fl in ((Topo(partner, alpha, flags), flags[0]), (topo0, np.zeros_like(flags[0]))):
        grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16)
        # lr = 0 in the all-zero round: w' = fmaf(-0, d, w) keeps every finite master, FLT_MAX included
        lr = LR if fl.any() else 0.0
        grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=False, master_weights=True)
        _put(grp.master_rows, W)
        _put_bits(grp.grads, G)
        assert grp.sgd_step(0, lr) == bool(fl.any())
        gw, gg, gm, gp = _state(grp)
        ww, wm, wp, _ = spec_round(O, W, G, np.zeros((n, P), np.float32), partner, fl, alpha, (lr, wd, mom, nesterov))
        nan = int(is_nan32(ww).sum())
        print(f"special {where} flags {int(fl.any())}: {nan} NaN outputs of {n * P} in the specification")
        assert 0 < nan <= 0.05 * n * P               # on the spec itself: the comparison below compares something
        assert same_f32(gw, ww), "w"
        assert same_f32(gm, wm), "m"
        assert bf16ref.same_bf16(gp, wp), "p"
        assert np.array_equal(gg, G) and _tails_zero(grp, P)
        if where == "w" and not fl.any():            # the largest finite masters survive lr = 0 and round up to Inf
            big = u32(ww) == 0x7F7FFFFF
            assert big.any() and (gp[big] == 0x7F80).all()
            assert (gp[u32(ww) == 0xFF7FFFFF] == 0xFF80).all()


@pytest.mark.parametrize("case", ["element", "g_p_8_not_16", "aligned"])
def test_abi_unaligned_multi_segment(pkg, O, case):
    """mx_sgd_mix_bf16 on two-segment tables (5 and T + 3 elements) whose pointers are offset into padded
    buffers: w / m one float past a 16-byte boundary with g / p one element past an 8-byte one (the
    element path); g / p 8-byte but not 16-byte aligned with w / m 16-byte aligned (the vector path);
    everything 16-byte aligned.  Bit-equal to the specification, guard words around every segment
    untouched -- with zero_grads, so g is stored to as well."""
    E = pkg.engine
    partner, alpha = _topology(pkg, "hand3")
    flags = np.array([[1, 1], [0, 1], [0, 0]], np.uint8)
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    wd, mom, nesterov = HYPERS["H2"]
    n = 3
    T = int(pkg.lib.mx_sgd_mix_bf16_tile(n))
    lens = [5, T + 3]
    stride = T + 64
    SENT32, SENT16 = np.float32(777.25), np.uint16(0x4D4D)
    rng = np.random.default_rng(41)
    d32 = 1 if case == "element" else 0
    d16 = {"element": 1, "g_p_8_not_16": 4, "aligned": 0}[case]
    off = {k: (8 + d32, 24 + d32) for k in "wm"}
    off.update({k: (8 + d16, 24 + d16) for k in "gp"})
    host, dev = {}, {}
    for k in "wm":
        host[k] = np.full((n, stride), SENT32, np.float32)
        for s in range(2):
            host[k][:, off[k][s]:off[k][s] + lens[s]] = 0.0 if k == "m" else rng.standard_normal((n, lens[s]))
        dev[k] = torch.from_numpy(host[k]).cuda()
    for k in "gp":
        host[k] = np.full((n, stride), SENT16, np.uint16)
        for s in range(2):
            host[k][:, off[k][s]:off[k][s] + lens[s]] = 0x1234       # p: never read, always overwritten
        dev[k] = torch.from_numpy(host[k].view(np.int16)).cuda()
    assert all(dev[k].data_ptr() % 16 == 0 for k in "wgmp") and (2 * stride) % 16 == 0

    def ptrs(k):
        size = 4 if k in "wm" else 2
        return [[dev[k][r].data_ptr() + size * off[k][s] for s in range(2)] for r in range(n)]

    for k in "wm":
        assert all(p % 16 == 4 * d32 for row in ptrs(k) for p in row)
    for k in "gp":
        assert all(p % 16 == 2 * d16 for row in ptrs(k) for p in row)
    lay = E.SgdBf16Layout(lens, ptrs("w"), ptrs("g"), ptrs("m"), ptrs("p"), n)
    assert lay.total_tiles == 3
    call = lay.call(eng, wd, mom, nesterov, True)

    def cat(k, a):
        return np.concatenate([a[:, off[k][s]:off[k][s] + lens[s]] for s in range(2)], axis=1)

    def outside_ok(k, a, sent):
        outside = np.ones(stride, bool)
        for s in range(2):
            outside[off[k][s]:off[k][s] + lens[s]] = False
        return bool((a[:, outside] == sent).all())

    W, Mo = cat("w", host["w"]), cat("m", host["m"])
    for it in range(3):
        G = bf16ref.random_bits(rng, (n, sum(lens)), specials=False)
        gh = host["g"].copy()
        gh[:, off["g"][0]:off["g"][0] + 5] = G[:, :5]
        gh[:, off["g"][1]:off["g"][1] + lens[1]] = G[:, 5:]
        dev["g"].copy_(torch.from_numpy(gh.view(np.int16)))
        assert pkg.lib.mx_sgd_mix_bf16(ctypes.addressof(call), it, LR, None, pkg._lib.stream_ptr()) == 0
        W, Mo, Pb, _ = spec_round(O, W, G, Mo, partner, flags[it], alpha, (LR, wd, mom, nesterov))
        torch.cuda.synchronize()
        got = {k: dev[k].cpu().numpy() for k in "wm"}
        got.update({k: dev[k].cpu().numpy().view(np.uint16) for k in "gp"})
        where = f"{case} round {it}"
        assert eq32(cat("w", got["w"]), W) and eq32(cat("m", got["m"]), Mo), where
        assert np.array_equal(cat("p", got["p"]), Pb), where
        assert not cat("g", got["g"]).any(), where
        assert outside_ok("w", got["w"], SENT32) and outside_ok("m", got["m"], SENT32), where + ": guard words"
        assert outside_ok("g", got["g"], SENT16) and outside_ok("p", got["p"], SENT16), where + ": guard words"


def test_refusals_write_nothing(pkg):
    L, INVALID = pkg.lib, pkg._lib.MX_ERR_INVALID
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    grp = _group(pkg, topo, 300, "H1", True)
    rng = np.random.default_rng(51)
    X = rng.standard_normal((8, 300)).astype(np.float32)
    _put(grp.master_rows, X)
    _put(grp.momentum_rows, X * 0.5)
    _put_bits(grp.grads, bf16ref.random_bits(rng, (8, 300), specials=False))
    _put_bits(grp.rows, bf16ref.random_bits(rng, (8, 300), specials=False))
    before = _state(grp)
    lay = grp._sgd[0]

    def refused(**fields):
        call = lay.call(grp.engine, 5e-4, 0.9, False, True)
        for k, v in fields.items():
            setattr(call, k, v)
        s = pkg._lib.stream_ptr()
        return L.mx_sgd_mix_bf16(ctypes.addressof(call), 0, LR, None, s) == INVALID and \
            L.mx_sgd_mix_bf16_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, LR, None, s) == INVALID

    assert refused(n_slots=9)
    assert refused(n_local=65, n_slots=65)                       # 65 rows
    assert refused(M=33)
    assert refused(p_ptrs_dev=None)                              # a null p table
    assert refused(m_ptrs_dev=None)                              # mom != 0 without its table
    assert refused(mom=0.0)                                      # a table without mom
    assert refused(mom=0.0, m_ptrs_dev=None, nesterov=1)         # Nesterov without momentum
    call = lay.call(grp.engine, 5e-4, 0.9, False, True)
    assert L.mx_sgd_mix_bf16_at(ctypes.addressof(call), None, 2, LR, None, pkg._lib.stream_ptr()) == INVALID
    assert L.mx_sgd_mix_bf16(None, 0, LR, None, pkg._lib.stream_ptr()) == INVALID
    assert _same_state(_state(grp), before)
    # a peer-reads plan record: the launch runs and writes nothing (the bit lives on the device)
    pkg._lib.check(L.mx_plan_set_peer_reads(grp.engine.plan.data_ptr(), grp.engine.T + 1, grp.n_local, grp.engine.M,
                                            1, pkg._lib.stream_ptr()))
    grp.sgd_step(0, LR)
    grp.iter_dev.fill_(0)
    grp.sgd_device_round()
    assert _same_state(_state(grp), before)
    pkg._lib.check(L.mx_plan_set_peer_reads(grp.engine.plan.data_ptr(), grp.engine.T + 1, grp.n_local, grp.engine.M,
                                            0, pkg._lib.stream_ptr()))
    assert grp.sgd_step(0, LR)                                   # the bit cleared: the same launch now writes
    after = _state(grp)
    assert not eq32(after[0], before[0]) and not after[1].any()


def test_graph_replay_equals_eager_steps(pkg, O):
    """sgd_device_round captured once, replayed over a 6-round schedule with fresh gradients and a
    learning rate changed after round 3 through lr_dev == six sgd_step calls on a twin, for all four
    arrays; two replays past the schedule write nothing to any of them."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    wd, mom, nesterov = HYPERS["H1"]
    n, P = 8, 2 * int(pkg.lib.mx_sgd_mix_bf16_tile(8)) + 77
    rng = np.random.default_rng(61)
    W0 = rng.standard_normal((n, P)).astype(np.float32)
    Gs = [bf16ref.random_bits(rng, (n, P), specials=False) for _ in range(7)]
    lrs = [0.1, 0.1, 0.1, 0.1, 0.025, 0.025]
    eager = _group(pkg, topo, P, "H1", True)
    _put(eager.master_rows, W0)
    W, Mo = W0, np.zeros_like(W0)
    for it in range(6):
        _put_bits(eager.grads, Gs[it])
        eager.sgd_step(it, lrs[it])
        W, Mo, Pb, _ = spec_round(O, W, Gs[it], Mo, partner, flags[it], alpha, (lrs[it], wd, mom, nesterov))
    want = _state(eager)
    assert eq32(want[0], W) and eq32(want[2], Mo) and np.array_equal(want[3], Pb) and not want[1].any()

    grp = _group(pkg, topo, P, "H1", True)
    _put(grp.master_rows, W0)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            grp.sgd_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and eq32(grp.master_rows.cpu().numpy(), W0)      # capture ran nothing
    assert not _bits(grp.rows).any()
    for it in range(6):
        _put_bits(grp.grads, Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = _state(grp)
    assert _same_state(got, want)
    _put_bits(grp.grads, Gs[6])                      # past the schedule: no mix, no SGD step, g not zeroed
    for _ in range(2):
        g.replay()
    past = _state(grp)
    assert int(grp.iter_dev.item()) == 8
    assert eq32(past[0], want[0]) and eq32(past[2], want[2]) and np.array_equal(past[3], want[3])
    assert np.array_equal(past[1], Gs[6])


_KNOB_BASE = {}


def _knob_run(pkg, name):
    """three rounds (every matching, the sparsest, random) on 3T + 5 columns with Nesterov, zeroing"""
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flag_kinds(partner, 6)[[6, 3, 9]]
    P = 3 * int(pkg.lib.mx_sgd_mix_bf16_tile(n)) + 5
    rng = np.random.default_rng([P, n])
    grp = _group(pkg, Topo(partner, alpha, flags), P, "H2", True)
    _put(grp.master_rows, rng.standard_normal((n, P)).astype(np.float32))
    for it in range(3):
        _put_bits(grp.grads, bf16ref.random_bits(rng, (n, P), specials=False))
        grp.sgd_step(it, LR)
    assert _tails_zero(grp, P)
    return _state(grp)


@pytest.mark.parametrize("knobs", [{"grid": 2}, {"nontemporal": 0}, {"nontemporal": 1}, {"wgpc": 4},
                                   {"blocks_per_cu": 1}, {"flat_small": 0}])
def test_knobs_change_no_bits(pkg, knobs):
    """mx_sgd_mix_bf16_set's knobs tune speed only: the 8-row and 64-row classes give the default's bits
    under each (grid = 2: two workgroups loop over the work items, each holding the next item's first
    loads while it mixes).  The default itself is held to the specification by test_rounds_match_spec."""
    E = pkg.engine
    for name in ("g0", "er64"):
        if name not in _KNOB_BASE:
            assert E.sgd_mix_bf16_tuning() == {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256,
                                               "grid": 0}
            _KNOB_BASE[name] = _knob_run(pkg, name)
    saved = {k: v for k, v in E.sgd_mix_bf16_tuning().items() if k in knobs}
    try:
        E.set_sgd_mix_bf16_tuning(**knobs)
        assert all(E.sgd_mix_bf16_tuning()[k] == v for k, v in knobs.items())
        got = {name: _knob_run(pkg, name) for name in ("g0", "er64")}
    finally:
        E.set_sgd_mix_bf16_tuning(**saved)
    for name in ("g0", "er64"):
        assert _same_state(got[name], _KNOB_BASE[name]), f"{knobs} {name}"
    assert E.sgd_mix_tuning()["grid"] == 0           # the fp32 kernel's knobs are its own


def _mlp():
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5)).cuda().to(torch.bfloat16)


def test_python_surface(pkg, O):
    partner, alpha = _topology(pkg, "g0")
    M = partner.shape[0]
    topo = Topo(partner, alpha, np.ones((4, M), np.uint8))
    with pytest.raises(NotImplementedError, match="bfloat16") as ei:
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).attach_sgd()
    assert "master_weights=True" in str(ei.value)
    with pytest.raises(ValueError, match="master_weights"):
        pkg.VirtualWorkerGroup(topo, numel=100).attach_sgd(master_weights=True)
    with pytest.raises(pkg.MXError, match="master"):
        pkg.VirtualWorkerGroup(topo, numel=100).master_from_rows()
    with pytest.raises(ValueError, match="[Nn]esterov"):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).attach_sgd(nesterov=True, master_weights=True)

    n = 8
    torch.manual_seed(0)
    models = [_mlp() for _ in range(n)]
    start = [torch.cat([p.detach().reshape(-1) for p in m.parameters()]) for m in models]
    grp = pkg.VirtualWorkerGroup(topo, models, dtype=torch.bfloat16)
    grp.attach_sgd(momentum=0.9, weight_decay=5e-4, master_weights=True)
    with pytest.raises(RuntimeError, match="already attached"):
        grp.attach_sgd(master_weights=True)
    assert torch.equal(grp.rows, torch.stack(start))
    assert torch.equal(grp.master_rows, grp.rows.float())            # the exact widening
    for r, m in enumerate(models):
        off = 0
        for p in m.parameters():
            assert p.dtype == torch.bfloat16 and p.data_ptr() == grp.arena[r].data_ptr() + 2 * off
            assert p.grad is not None and p.grad.dtype == torch.bfloat16 and p.grad.shape == p.shape
            assert p.grad.data_ptr() == grp.grad_arena[r].data_ptr() + 2 * off
            off += p.numel()
    data = torch.randn(n, 6, 33, device="cuda").to(torch.bfloat16)
    ref = []
    for r, m in enumerate(models):
        m(data[r]).square().mean().backward()
        gr = torch.autograd.grad(m(data[r]).square().mean(), list(m.parameters()))
        ref.append(torch.cat([t.reshape(-1) for t in gr]))
    ref = torch.stack(ref)
    # backward() filled the bf16 arena (within a bf16 ulp of the out-of-place gradients)
    assert ref.abs().max().item() > 0 and torch.allclose(grp.grads.float(), ref.float(), rtol=2.0 ** -7, atol=1e-6)

    def steps(g, its):
        for it in its:
            _put_bits(g.grads, Gs[it])
            g.sgd_step(it, LR)

    rng = np.random.default_rng(71)
    Gs = [bf16ref.random_bits(rng, (n, grp.numel), specials=False) for _ in range(4)]
    steps(grp, range(2))
    grp.iter = 2
    ckpt = grp.state_dict()
    assert set(ckpt) == {"kind", "iter", "row_base", "workers", "rows", "momentum_rows", "master_rows"}
    assert ckpt["master_rows"].dtype == torch.float32 and ckpt["rows"].dtype == torch.bfloat16

    def fresh(**kw):
        g = pkg.VirtualWorkerGroup(topo, numel=grp.numel, dtype=torch.bfloat16)
        g.attach_sgd(momentum=0.9, weight_decay=5e-4, master_weights=True, **kw)
        return g

    twin = fresh()
    twin.load_state_dict(ckpt)
    assert twin.iter == 2 and _same_state(_state(twin), _state(grp))
    steps(grp, range(2, 4))
    steps(twin, range(2, 4))
    assert _same_state(_state(twin), _state(grp))                    # continues bit for bit
    # a checkpoint without masters: the widened rows; after a direct write to rows, master_from_rows()
    bare = {k: v for k, v in ckpt.items() if k != "master_rows"}
    twin.load_state_dict(bare)
    assert torch.equal(twin.master_rows, ckpt["rows"].float()) and not torch.equal(twin.master_rows, ckpt["master_rows"])
    with torch.no_grad():
        twin.rows.copy_(grp.rows)
    twin.master_from_rows()
    assert torch.equal(twin.master_rows, grp.rows.float())
    # masters are refused by groups that have none: a bf16 group that is not attached, an fp32 group
    with pytest.raises(ValueError, match="master"):
        pkg.VirtualWorkerGroup(topo, numel=grp.numel, dtype=torch.bfloat16).load_state_dict(
            {k: v for k, v in ckpt.items() if k != "momentum_rows"})
    plain = pkg.VirtualWorkerGroup(topo, numel=grp.numel)
    plain.attach_sgd(momentum=0.9)
    with pytest.raises(ValueError, match="master"):
        plain.load_state_dict({**ckpt, "rows": ckpt["rows"].float()})
    assert set(plain.state_dict()) == {"kind", "iter", "row_base", "workers", "rows", "momentum_rows"}
    # the unchanged refusals
    with pytest.raises(NotImplementedError, match="one GPU"):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16, nranks=2, rank=0, comm=LoopbackHub(2).comm(0))
    with pytest.raises(NotImplementedError, match="chunk_cols"):
        pkg.VirtualWorkerGroup(topo, numel=100_000, dtype=torch.bfloat16, chunk_cols=4096)


def test_against_torch_sgd_then_step(pkg):
    """The fused launch against the unfused sequence on plain CUDA tensors: g.float(),
    torch.optim.SGD.step() (Nesterov) on fp32 masters, the fp32 group.step of a twin fp32 group,
    .to(torch.bfloat16).  Masters: |diff| <= 2^-20, the bound and input range of
    tests/test_gpu_sgd_mix.py's torch comparison -- the master arithmetic is the same lines (g.float()
    is exact): every intermediate is below 2, so a rounding is at most 2^-24; the two op sequences
    differ by at most one extra rounding in each of three ops, <= 3 * 2^-24 in w', which the mix (a
    convex combination) carries through, adding at most 2 * (deg + 1) <= 8 roundings of its own:
    <= 11 * 2^-24.  p equals torch's .to(torch.bfloat16) of THIS kernel's masters exactly."""
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((1, partner.shape[0]), np.uint8))
    wd, mom, nesterov = HYPERS["H2"]
    n, P = 8, 4097
    rng = np.random.default_rng(81)
    W = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    G = bf16ref.rne_bf16(rng.uniform(-1, 1, (n, P)).astype(np.float32))
    fused = _group(pkg, topo, P, "H2", True)
    _put(fused.master_rows, W)
    _put_bits(fused.grads, G)
    assert fused.sgd_step(0, LR)
    gbf = torch.from_numpy(G.view(np.int16)).cuda().view(torch.bfloat16)
    params = [torch.nn.Parameter(torch.from_numpy(W[r].copy()).cuda()) for r in range(n)]
    for r, p in enumerate(params):
        p.grad = gbf[r].float()
        torch.optim.SGD([p], lr=LR, momentum=mom, weight_decay=wd, nesterov=nesterov, dampening=0).step()
    twin = pkg.VirtualWorkerGroup(topo, numel=P)
    with torch.no_grad():
        twin.rows.copy_(torch.stack([p.detach() for p in params]))
    assert twin.step(0)
    torch.cuda.synchronize()
    a, b = fused.master_rows.cpu().numpy().astype(np.float64), twin.rows.cpu().numpy().astype(np.float64)
    diff = float(np.abs(a - b).max())
    print(f"fused mixed-precision vs g.float() + torch.optim.SGD + step: max |diff| = {diff:.3e} "
          f"({diff * 2 ** 24:.2f} x 2^-24)")
    assert np.abs(b).max() < 2 and diff <= 2.0 ** -20
    assert not np.isnan(a).any()
    assert torch.equal(fused.rows, fused.master_rows.to(torch.bfloat16))
    tp = _bits(twin.rows.to(torch.bfloat16))
    print(f"p vs torch's bf16 of the unfused masters: {int((tp != _bits(fused.rows)).sum())} of {n * P} differ")


def test_virtual_trainer_fused_sgd_bf16(pkg, O):
    """harness.VirtualTrainer(fused_sgd=True) with bfloat16 models: every iteration's fused launch by
    the specification from the masters, gradients and momentum rows the backward passes left; the torch
    optimizers never step; a checkpoint resumed in a new trainer continues bit for bit."""
    H = pkg.harness

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=0.1, matcha=True, momentum=0.9)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        fn = H.model_factory(args)
        return H.VirtualTrainer(args, lambda: fn().to(torch.bfloat16), n_batches=3, fused_sgd=True, **kw)

    tr = make()
    grp = tr.group
    assert grp.dtype == torch.bfloat16 and grp.master_rows is not None and grp.momentum_rows is not None
    assert grp.sgd_hyper == {"momentum": 0.9, "weight_decay": 5e-4, "nesterov": False, "zero_grads": True}
    assert all(p.dtype == torch.bfloat16 and p.grad.dtype == torch.bfloat16 for m in tr.models for p in m.parameters())
    assert torch.equal(grp.master_rows, grp.rows.float())            # master_from_rows() after sync_rows
    assert all(torch.equal(grp.rows[0], grp.rows[r]) for r in range(8))
    partner = np.asarray(tr.GP.neighbors_info, np.int32)
    state, seen = {}, {"rounds": 0}

    def hook(when, t):
        if when == "before":
            state["s"], state["it"] = _state(t.group), t.group.iter
            assert state["s"][1].any()                               # backward() filled the gradient arena
            return
        flags = np.asarray(tr.GP.active_flags[state["it"]], np.uint8)
        lr = t.optimizers[0].param_groups[0]["lr"]
        W, G, Mo, _ = state["s"]
        ww, wm, wp, _ = spec_round(O, W, G, Mo, partner[:len(flags)], flags, tr.GP.neighbor_weight,
                                   (lr, 5e-4, 0.9, False))
        gw, gg, gm, gp = _state(t.group)
        assert eq32(gw, ww) and eq32(gm, wm) and bf16ref.same_bf16(gp, wp) and not gg.any(), f"round {state['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats)
    assert seen["rounds"] == 3 and grp.iter == 3
    assert all(not o.state for o in tr.optimizers)                   # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert eq32(ckpt["group"]["master_rows"].cpu().numpy(), grp.master_rows.cpu().numpy())
    tr2 = make()
    tr2.load_state_dict(ckpt)
    assert tr2.epoch == 1 and tr2.group.iter == 3
    tr.train_epoch()
    tr2.train_epoch()
    assert _same_state(_state(tr.group), _state(tr2.group)) and tr.group.iter == tr2.group.iter == 6
    with pytest.raises(ValueError, match="fused_sgd"):
        make(batched=True)
    with pytest.raises(ValueError, match="fused_sgd"):
        make(args={"compress": True})
