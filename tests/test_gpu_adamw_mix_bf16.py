"""Mixed-precision AdamW / Adam fused into the bf16 gossip round (csrc/adamw_mix_bf16.hip,
VirtualWorkerGroup.attach_adamw(master_weights=True)): fp32 master rows w, exp_avg m and exp_avg_sq v,
bfloat16 gradients g, bfloat16 model rows p = bf16(w).

Every comparison is against the specification restated in tests/adambf16ref.py, never the code under
test: w, m and v uint32 for uint32, p uint16 for uint16 (a NaN of any payload where the specification
is a NaN, in the special-values test only).

Shapes are the smallest at which each path can go wrong: 1-9 columns (the element path, one and two
4-element chunks), 63-65 (a wave's seam), 255-257 (a 256-column pass seam) and per row class one layout
tile - 1, one tile, one tile + 9 and three tiles + 5 (the vector path, the tail, the tile seam, several
work items).  The 32-row class has no graph in topologies.py; a 32-worker ring written by hand covers it
in test_32_row_class and test_knobs_change_no_bits."""
import ctypes
import random

import numpy as np
import pytest

import bf16ref
from adambf16ref import adam_only, eq32, spec_round, u32
from adamref import bias_at, bias_table
from conftest import LoopbackHub, Topo, special_values
from sgdref import is_nan32, same_f32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LR = 1e-3
# beta1, beta2, eps, wd, decoupled: tests/test_gpu_adamw_mix.py's
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
    """(partner int32 [M][n], alpha) of the topologies, built once"""
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
        elif name == "ring32":                     # a 32-worker ring by hand, two matchings: the 32-row class
            even = np.arange(32) ^ 1
            odd = (((np.arange(32) - 1) ^ 1) + 1) % 32
            _TOPOS[name] = (np.stack([even, odd]).astype(np.int32), 0.3125)
        else:                                      # 3 workers by hand: the 8-row class with unused rows
            _TOPOS[name] = (np.array([[1, 0, -1], [-1, 2, 1]], np.int32), -2.0 ** -8)
    partner, alpha = _TOPOS[name]
    assert partner.shape[0] <= 32
    for row in partner:                            # every matching is an involution
        assert all(row[j] < 0 or row[row[j]] == j for j in range(len(row)))
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
    T = int(pkg.lib.mx_adamw_mix_bf16_tile(n))
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
    """host copies of (w, g bits, m, v, p bits)"""
    torch.cuda.synchronize()
    return (grp.master_rows.cpu().numpy(), _bits(grp.grads), grp.exp_avg_rows.cpu().numpy(),
            grp.exp_avg_sq_rows.cpu().numpy(), _bits(grp.rows))


def _same_state(a, b):
    return eq32(a[0], b[0]) and np.array_equal(a[1], b[1]) and eq32(a[2], b[2]) and eq32(a[3], b[3]) and \
        np.array_equal(a[4], b[4])


def _tails_zero(grp, P):
    arenas = [(grp.arena, torch.int16), (grp.grad_arena, torch.int16), (grp.master_arena, torch.int32),
              (grp.exp_avg_arena, torch.int32), (grp.exp_avg_sq_arena, torch.int32)]
    return all(not a[:, P:].view(dt).any().item() for a, dt in arenas)


def _group(pkg, topo, P, hyper, zero, idle_rows="skip"):
    b1, b2, eps, wd, decoupled = HYPERS[hyper]
    grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows, dtype=torch.bfloat16)
    grp.attach_adamw(betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=decoupled, zero_grads=zero,
                     master_weights=True)
    return grp


def _grads(rng, shape):
    """bfloat16 bit patterns of gradients of the scale Adam sees (0.01 N(0, 1)), a tenth of them 100 x
    larger: the fp32 test's, rounded to bfloat16"""
    g = 0.01 * rng.standard_normal(shape)
    g[rng.random(shape) < 0.1] *= 100
    return bf16ref.rne_bf16(g.astype(np.float32))


def _rounds_against_spec(pkg, O, name, idle_rows, hyper, rounds):
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flag_kinds(partner, 5)[rounds]
    topo = Topo(partner, alpha, flags)
    table = _table(HYPERS[hyper])
    rng = np.random.default_rng([len(name), len(idle_rows), n, int(hyper[1])])
    for pi, P in enumerate(_shapes(pkg, n)):
        zero = bool(pi & 1)                          # both settings of zero_grads, alternating by P
        grp = _group(pkg, topo, P, hyper, zero, idle_rows)
        assert tuple(grp.grads.shape) == (n, P) and tuple(grp.grad_arena.shape) == (n, grp.ld)
        assert grp.grad_arena.dtype == torch.bfloat16 and grp.master_arena.dtype == torch.float32
        assert grp.exp_avg_arena.dtype == grp.exp_avg_sq_arena.dtype == torch.float32
        assert tuple(grp.master_rows.shape) == (n, P) and tuple(grp.master_arena.shape) == (n, grp.ld)
        assert tuple(grp.exp_avg_rows.shape) == tuple(grp.exp_avg_sq_rows.shape) == (n, P)
        assert grp.opt_step == 0 and int(grp.opt_step_dev.item()) == 1
        W = rng.standard_normal((n, P)).astype(np.float32)       # low mantissa bits populated: p != widened w
        Mo, V = np.zeros((n, P), np.float32), np.zeros((n, P), np.float32)
        _put(grp.master_rows, W)
        for it in range(len(flags)):                 # w, m, v and the step carried throughout
            G = _grads(rng, (n, P))
            _put_bits(grp.grads, G)
            ran = grp.adamw_step(it, LR)
            gw, gg, gm, gv, gp = _state(grp)
            ww, wm, wv, wp, wprime = spec_round(O, W, G, Mo, V, it + 1, partner, flags[it], alpha, LR, HYPERS[hyper],
                                                table, idle_rows)
            where = f"{name} {idle_rows} {hyper} P={P} round {it}"
            assert grp.opt_step == it + 1, where
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the optimizer step alone: not a no-op, and p follows
                assert eq32(gw, wprime) and not eq32(gw, W), where
                assert np.array_equal(gp, bf16ref.rne_bf16(wprime)), where
            assert eq32(gw, ww), where + ": w"
            assert eq32(gm, wm), where + ": m"
            assert eq32(gv, wv), where + ": v"
            assert np.array_equal(gp, wp) and bf16ref.same_bf16(gp, wp), where + ": p"
            assert (not gg.any()) if zero else np.array_equal(gg, G), where + ": g"
            assert _tails_zero(grp, P), where + ": wrote past the row"
            if P > 64:                               # p is the ROUNDED image: neither the master nor its upper half
                assert not np.array_equal(u32(bf16ref.upcast(gp)), u32(gw)), where
                assert not np.array_equal(gp, (u32(gw) >> 16).astype(np.uint16)), where + ": p is truncated"
            W, Mo, V = gw, gm, gv


@pytest.mark.parametrize("hyper", ["A0", "A1", "A2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows, hyper):
    _rounds_against_spec(pkg, O, name, idle_rows, hyper, slice(None))


def test_32_row_class(pkg, O):
    """the 32-row class (persistent grid, 512-column tile) on a ring of 32 by hand: every width, one
    round of each kind"""
    assert pkg.lib.mx_adamw_mix_bf16_tile(32) == 512
    _rounds_against_spec(pkg, O, "ring32", "skip", "A1", [0, 3, 6, 9])


def test_small_updates_are_not_lost(pkg):
    """All-zero flags (the optimizer step alone), betas (0.9, 0.999), eps 1e-8, wd 0, lr = 2^-12, every
    master 1.0, every gradient bf16(1.0).  By the specification on the CPU (tests/adamref.py +
    tests/bf16ref.py, computed here): the master is exactly 1 - t * 2^-12 for t = 1..64; p stays 0x3F80
    through step 8 (the tie at 1 - 2^-9 goes to even), is 0x3F7F at step 9 and 0x3F7C at step 64; a
    pure-bf16 recurrence, which re-rounds the weight every step, holds 1.0 for ever.  The GPU gives
    those values, 64 steps, 8 x 257."""
    hyper = (0.9, 0.999, 1e-8, 0.0, True)
    table = _table(hyper)
    lr, steps = 2.0 ** -12, 64
    one = np.array([0x3F80], np.uint16)
    w, m, v = np.ones(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    want = []
    for t in range(1, steps + 1):
        w, m, v, p = adam_only(w, one, m, v, t, lr, hyper, table)
        assert float(w[0]) == 1.0 - t * lr, t
        want.append((w[0], m[0], v[0], int(p[0])))
    assert all(want[t - 1][3] == 0x3F80 for t in range(1, 9)) and want[8][3] == 0x3F7F and want[63][3] == 0x3F7C
    assert bf16ref.rne_bf16(np.float32([1.0 - lr]))[0] == 0x3F80         # the pure-bf16 recurrence never moves

    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.zeros((steps, partner.shape[0]), np.uint8))
    n, P = 8, 257
    grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16)
    grp.attach_adamw(betas=hyper[:2], eps=hyper[2], weight_decay=0.0, zero_grads=False, master_weights=True)
    ones = np.full((n, P), 0x3F80, np.uint16)
    _put(grp.master_rows, np.ones((n, P), np.float32))
    _put_bits(grp.grads, ones)
    _put_bits(grp.rows, ones)
    for t in range(1, steps + 1):
        assert grp.adamw_step(t - 1, lr) is False
        gw, gg, gm, gv, gp = _state(grp)
        ww, wm, wv, wp = want[t - 1]
        assert (u32(gw) == u32(ww)).all() and (gw == np.float32(1.0 - t * lr)).all(), t
        assert (u32(gm) == u32(wm)).all() and (u32(gv) == u32(wv)).all(), t
        assert (gp == wp).all() and np.array_equal(gg, ones), t
    assert (gp == 0x3F7C).all() and (gw == np.float32(0.984375)).all()
    assert _tails_zero(grp, P)


@pytest.mark.parametrize("where", ["w", "g", "g_edge"])
def test_special_values(pkg, O, where):
    """NaNs, +-Inf, +-0, subnormals and +-FLT_MAX planted in the masters (normal g): an active round,
    then an all-zero round at lr = 0, where every master survives and the largest finite ones round up
    to bf16 Inf in p.  Then bf16's own special patterns in the gradients (normal w).  Then the
    gradients at which Adam's arithmetic leaves the normal range -- bfloat16 has fp32's exponent range,
    so they are all representable: |g| near 2^-70 (g^2 denormal: the square root of a denormal), 2^-80
    (g^2 underflows to zero), 2^70 (v overflows to Inf) and +-0 on zero state -- two steps, so the
    second starts from that state."""
    partner, alpha = _topology(pkg, "g0")
    M = partner.shape[0]
    n, P = 8, 4099
    hyper = HYPERS["A1"]
    table = _table(hyper)
    rng = np.random.default_rng(31)
    normal = rng.standard_normal((n, P)).astype(np.float32)
    if where == "w":
        W, G = np.stack([special_values(P, 100 + r) for r in range(n)]), _grads(rng, (n, P))
    elif where == "g":
        W, G = normal, bf16ref.random_bits(rng, (n, P), specials=True)
        assert all((G == s).any() for s in bf16ref.SPECIALS)
    else:
        W, G = normal, _grads(rng, (n, P))
        edge = bf16ref.rne_bf16(np.float32([0.0, -0.0, 2.0 ** -70, -1.5 * 2.0 ** -70, 2.0 ** -80, -1.25 * 2.0 ** -80,
                                            2.0 ** 70, -1.75 * 2.0 ** 70, 2.0 ** -133, 2.0 ** 127]))
        assert np.array_equal(bf16ref.upcast(edge)[[2, 4, 6]], np.float32([2.0 ** -70, 2.0 ** -80, 2.0 ** 70]))
        for r in range(n):
            pos = rng.permutation(P)[:4 * len(edge)]
            G[r, pos] = np.tile(edge, 4)
    if where == "g_edge":
        runs = [(np.ones((2, M), np.uint8), LR, 2)]
    else:                                            # one step each: NaNs spread along the matchings
        runs = [(np.ones((1, M), np.uint8), LR, 1), (np.zeros((1, M), np.uint8), 0.0, 1)]
    for flags, lr, steps in runs:
        grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P, dtype=torch.bfloat16)
        grp.attach_adamw(betas=hyper[:2], eps=hyper[2], weight_decay=hyper[3], decoupled=hyper[4], zero_grads=False,
                         master_weights=True)
        _put(grp.master_rows, W)
        X, Mo, V = W, np.zeros((n, P), np.float32), np.zeros((n, P), np.float32)
        for step in range(1, steps + 1):
            _put_bits(grp.grads, G)
            assert grp.adamw_step(step - 1, lr) == bool(flags[0].any())
            gw, gg, gm, gv, gp = _state(grp)
            ww, wm, wv, wp, wprime = spec_round(O, X, G, Mo, V, step, partner, flags[0], alpha, lr, hyper, table)
            nan = int(is_nan32(ww).sum())
            print(f"special {where} flags {int(flags[0].any())} step {step}: {nan} NaN outputs of {n * P} in the "
                  "specification")
            if where == "g_edge":                    # on the spec itself: the cases are what the docstring says
                g32 = bf16ref.upcast(G)
                with np.errstate(all="ignore"):
                    sq = g32 * g32
                assert nan == 0 and np.isinf(wv).any() and (wv == 0).any()
                assert ((sq > 0) & (sq < 1.1754944e-38)).any() and ((g32 != 0) & (sq == 0)).any() and np.isinf(sq).any()
            else:
                assert 0 < nan <= 0.05 * n * P       # the comparison below compares something
            assert same_f32(gw, ww), f"w, step {step}"
            assert same_f32(gm, wm), f"m, step {step}"
            assert same_f32(gv, wv), f"v, step {step}"
            assert bf16ref.same_bf16(gp, wp), f"p, step {step}"
            assert np.array_equal(gg, G) and _tails_zero(grp, P)
            if where == "w" and not flags[0].any():  # lr = 0: every non-NaN master survives; FLT_MAX rounds up to Inf
                keep = ~is_nan32(W) & (W != 0)       # (a -0 master may come back as +0: fmaf(-0, q, -0))
                assert np.array_equal(u32(gw)[keep], u32(W)[keep])
                big = u32(gw) == 0x7F7FFFFF
                assert big.any() and (gp[big] == 0x7F80).all()
                neg = u32(gw) == 0xFF7FFFFF
                assert neg.any() and (gp[neg] == 0xFF80).all()
            X, Mo, V = gw, gm, gv


@pytest.mark.parametrize("case", ["element", "g_p_8_not_16", "v", "aligned"])
def test_abi_unaligned_multi_segment(pkg, O, case):
    """mx_adamw_mix_bf16 on two-segment tables (5 and T + 3 elements) whose pointers are offset into
    padded buffers: w / m / v one float past a 16-byte boundary with g / p one element past an 8-byte
    one (the element path); g / p 8-byte but not 16-byte aligned with w / m / v 16-byte aligned (the
    vector path must still be taken, and stay exact); v alone one float off (which must take the other
    four off the vector path too); everything 16-byte aligned.  Bit-equal to the specification, guard
    words around every segment untouched -- with zero_grads, so g is stored to as well."""
    E = pkg.engine
    partner, alpha = _topology(pkg, "hand3")
    flags = np.array([[1, 1], [0, 1], [0, 0]], np.uint8)
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    hyper = HYPERS["A2"]
    table = _table(hyper)
    n = 3
    T = int(pkg.lib.mx_adamw_mix_bf16_tile(n))
    lens = [5, T + 3]
    stride = T + 64
    SENT32, SENT16 = np.float32(777.25), np.uint16(0x4D4D)
    rng = np.random.default_rng(41)
    d32 = {k: 1 if case == "element" or (case == "v" and k == "v") else 0 for k in "wmv"}
    d16 = {"element": 1, "g_p_8_not_16": 4, "v": 0, "aligned": 0}[case]
    off = {k: (8 + d32[k], 24 + d32[k]) for k in "wmv"}
    off.update({k: (8 + d16, 24 + d16) for k in "gp"})
    host, dev = {}, {}
    for k in "wmv":
        host[k] = np.full((n, stride), SENT32, np.float32)
        for s in range(2):
            host[k][:, off[k][s]:off[k][s] + lens[s]] = rng.standard_normal((n, lens[s])) if k == "w" else 0.0
        dev[k] = torch.from_numpy(host[k]).cuda()
    for k in "gp":
        host[k] = np.full((n, stride), SENT16, np.uint16)
        for s in range(2):
            host[k][:, off[k][s]:off[k][s] + lens[s]] = 0x1234       # p: never read, always overwritten
        dev[k] = torch.from_numpy(host[k].view(np.int16)).cuda()
    assert all(dev[k].data_ptr() % 16 == 0 for k in "wgmvp") and (2 * stride) % 16 == 0

    def ptrs(k):
        size = 4 if k in "wmv" else 2
        return [[dev[k][r].data_ptr() + size * off[k][s] for s in range(2)] for r in range(n)]

    for k in "wmv":
        assert all(p % 16 == 4 * d32[k] for row in ptrs(k) for p in row)
    for k in "gp":
        assert all(p % 16 == 2 * d16 for row in ptrs(k) for p in row)
    lay = E.AdamwBf16Layout(lens, ptrs("w"), ptrs("g"), ptrs("m"), ptrs("v"), ptrs("p"), n, table)
    assert lay.total_tiles == 3 and lay.n_bias == len(table)
    call = lay.call(eng, hyper[:2], hyper[2], hyper[3], hyper[4], True)

    def cat(k, a):
        return np.concatenate([a[:, off[k][s]:off[k][s] + lens[s]] for s in range(2)], axis=1)

    def outside_ok(k, a, sent):
        outside = np.ones(stride, bool)
        for s in range(2):
            outside[off[k][s]:off[k][s] + lens[s]] = False
        return bool((a[:, outside] == sent).all())

    W, Mo, V = cat("w", host["w"]), cat("m", host["m"]), cat("v", host["v"])
    for it in range(3):
        G = _grads(rng, (n, sum(lens)))
        gh = host["g"].copy()
        gh[:, off["g"][0]:off["g"][0] + 5] = G[:, :5]
        gh[:, off["g"][1]:off["g"][1] + lens[1]] = G[:, 5:]
        dev["g"].copy_(torch.from_numpy(gh.view(np.int16)))
        assert pkg.lib.mx_adamw_mix_bf16(ctypes.addressof(call), it, it + 1, LR, None, pkg._lib.stream_ptr()) == 0
        W, Mo, V, Pb, _ = spec_round(O, W, G, Mo, V, it + 1, partner, flags[it], alpha, LR, hyper, table)
        torch.cuda.synchronize()
        got = {k: dev[k].cpu().numpy() for k in "wmv"}
        got.update({k: dev[k].cpu().numpy().view(np.uint16) for k in "gp"})
        where = f"{case} round {it}"
        assert eq32(cat("w", got["w"]), W) and eq32(cat("m", got["m"]), Mo) and eq32(cat("v", got["v"]), V), where
        assert np.array_equal(cat("p", got["p"]), Pb), where
        assert not cat("g", got["g"]).any(), where
        assert all(outside_ok(k, got[k], SENT32) for k in "wmv"), where + ": guard words"
        assert all(outside_ok(k, got[k], SENT16) for k in "gp"), where + ": guard words"


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
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P, dtype=torch.bfloat16)
    grp.attach_adamw(betas=(0.5, 0.5), eps=1e-8, weight_decay=1e-2, zero_grads=False, master_weights=True)
    assert grp._adamw[0].n_bias == nb
    rng = np.random.default_rng(71)
    W = rng.standard_normal((n, P)).astype(np.float32)
    Mo = bf16ref.upcast(_grads(rng, (n, P)))
    V = (Mo * Mo).astype(np.float32)
    _put(grp.master_rows, W)
    _put(grp.exp_avg_rows, Mo)
    _put(grp.exp_avg_sq_rows, V)
    for t in (nb - 1, nb, nb + 1, 10 ** 9):
        assert bias_at(table, t) == ((np.float32(1), np.float32(1)) if t >= nb else tuple(table[nb - 2]))
        G = _grads(rng, (n, P))
        _put_bits(grp.grads, G)
        grp.opt_step = t - 1
        assert grp.adamw_step(0, LR) and grp.opt_step == t
        W, Mo, V, Pb, _ = spec_round(O, W, G, Mo, V, t, partner, flags[0], alpha, LR, hyper, table)
        gw, _, gm, gv, gp = _state(grp)
        assert eq32(gw, W) and eq32(gm, Mo) and eq32(gv, V) and np.array_equal(gp, Pb), f"step {t}"


_KNOB_BASE = {}
_KNOB_DEFAULT = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0}


def _knob_run(pkg, name):
    """three rounds (every matching, the sparsest, random) on 3T + 5 columns with Adam + L2, zeroing"""
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flag_kinds(partner, 6)[[6, 3, 9]]
    P = 3 * int(pkg.lib.mx_adamw_mix_bf16_tile(n)) + 5
    rng = np.random.default_rng([P, n])
    grp = _group(pkg, Topo(partner, alpha, flags), P, "A2", True)
    _put(grp.master_rows, rng.standard_normal((n, P)).astype(np.float32))
    for it in range(3):
        _put_bits(grp.grads, _grads(rng, (n, P)))
        grp.adamw_step(it, LR)
    assert _tails_zero(grp, P)
    return _state(grp)


@pytest.mark.parametrize("knobs", [{"grid": 2}, {"nontemporal": 0}, {"nontemporal": 1}, {"wgpc": 4},
                                   {"blocks_per_cu": 1, "flat_small": 0}])
def test_knobs_change_no_bits(pkg, knobs):
    """mx_adamw_mix_bf16_set's knobs tune speed only: the 8-row, 32-row and 64-row classes give the
    default's bits under each (grid = 2: two workgroups loop over the work items, each holding the next
    item's first loads while it mixes; flat_small = 0: the 8-row class on the persistent grid).  The
    default itself is held to the specification by test_rounds_match_spec and test_32_row_class."""
    E = pkg.engine
    names = ("g0", "ring32", "er64")
    for name in names:
        if name not in _KNOB_BASE:
            assert E.adamw_mix_bf16_tuning() == _KNOB_DEFAULT
            _KNOB_BASE[name] = _knob_run(pkg, name)
    saved = {k: v for k, v in E.adamw_mix_bf16_tuning().items() if k in knobs}
    try:
        E.set_adamw_mix_bf16_tuning(**knobs)
        assert all(E.adamw_mix_bf16_tuning()[k] == v for k, v in knobs.items())
        got = {name: _knob_run(pkg, name) for name in names}
    finally:
        E.set_adamw_mix_bf16_tuning(**saved)
    for name in names:
        assert _same_state(got[name], _KNOB_BASE[name]), f"{knobs} {name}"
    assert E.adamw_mix_tuning() == _KNOB_DEFAULT and E.adamw_mix_bf16_tuning() == _KNOB_DEFAULT   # knobs of its own
    assert pkg.lib.mx_adamw_mix_bf16_set(b"no_such_knob", 1) == pkg._lib.MX_ERR_INVALID


def test_refusals_write_nothing(pkg):
    L, INVALID = pkg.lib, pkg._lib.MX_ERR_INVALID
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    grp = _group(pkg, topo, 300, "A1", True)
    rng = np.random.default_rng(51)
    X = rng.standard_normal((8, 300)).astype(np.float32)
    _put(grp.master_rows, X)
    _put(grp.exp_avg_rows, X * 0.5)
    _put(grp.exp_avg_sq_rows, X * X)
    _put_bits(grp.grads, _grads(rng, (8, 300)))
    _put_bits(grp.rows, bf16ref.random_bits(rng, (8, 300), specials=False))
    before = _state(grp)
    lay = grp._adamw[0]
    sp = pkg._lib.stream_ptr
    one = torch.ones(1, dtype=torch.int64, device="cuda")

    def fresh(**fields):
        call = lay.call(grp.engine, (0.9, 0.999), 1e-8, 1e-2, True, True)
        for k, v in fields.items():
            setattr(call, k, v)
        return call

    def refused(**fields):
        call = fresh(**fields)
        return L.mx_adamw_mix_bf16(ctypes.addressof(call), 0, 1, LR, None, sp()) == INVALID and \
            L.mx_adamw_mix_bf16_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, one.data_ptr(), LR, None,
                                   sp()) == INVALID

    # host-side refusals: MX_ERR_INVALID, nothing launched
    assert refused(n_slots=9)
    assert refused(n_local=65, n_slots=65)                       # 65 rows
    assert refused(M=33)
    assert refused(n_bias=0)
    for table in ("w_ptrs_dev", "g_ptrs_dev", "m_ptrs_dev", "v_ptrs_dev", "p_ptrs_dev", "bias_dev", "plan_dev"):
        assert refused(**{table: None}), table                   # a null table, p included
    call = fresh()
    for step in (0, -3):                                         # no such optimizer step
        assert L.mx_adamw_mix_bf16(ctypes.addressof(call), 0, step, LR, None, sp()) == INVALID
    assert L.mx_adamw_mix_bf16_at(ctypes.addressof(call), None, 2, one.data_ptr(), LR, None, sp()) == INVALID
    assert L.mx_adamw_mix_bf16_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, None, LR, None, sp()) == INVALID
    assert L.mx_adamw_mix_bf16(None, 0, 1, LR, None, sp()) == INVALID
    assert L.mx_adamw_mix_bf16_tile(65) == 0 and L.mx_adamw_mix_bf16_tile(64) > 0
    assert _same_state(_state(grp), before)

    # refusals made by the launch itself, on the device: none of the five arrays is written
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    for it_value, step_value in ((2, 1), (-1, 1), (0, 0), (1, -5)):     # round outside [0, 2); step below 1
        ctr.fill_(it_value)
        one.fill_(step_value)
        assert L.mx_adamw_mix_bf16_at(ctypes.addressof(call), ctr.data_ptr(), 2, one.data_ptr(), LR, None, sp()) == 0
        assert _same_state(_state(grp), before), (it_value, step_value)
    eng = grp.engine                                             # a peer-reads record is not this kernel's
    pkg._lib.check(L.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, eng.n_local, eng.M, 1, sp()))
    assert L.mx_adamw_mix_bf16(ctypes.addressof(call), 0, 1, LR, None, sp()) == 0
    grp.iter_dev.fill_(0)
    grp.adamw_device_round()
    assert _same_state(_state(grp), before)
    pkg._lib.check(L.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, eng.n_local, eng.M, 0, sp()))
    assert grp.adamw_step(0, LR)                                 # the bit cleared: the same launch now writes
    after = _state(grp)
    assert not eq32(after[0], before[0]) and not after[1].any() and not np.array_equal(after[4], before[4])

    # Python refusals
    with pytest.raises(RuntimeError, match="already attached"):
        grp.attach_adamw(master_weights=True)
    with pytest.raises(RuntimeError, match="AdamW"):
        grp.attach_sgd(master_weights=True)
    with pytest.raises(ValueError, match="master_weights"):
        pkg.VirtualWorkerGroup(topo, numel=100).attach_adamw(master_weights=True)
    with pytest.raises(NotImplementedError, match="bfloat16") as ei:
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).attach_adamw()
    assert "master_weights=True" in str(ei.value)
    sgd = pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16)
    sgd.attach_sgd(momentum=0.9, master_weights=True)
    with pytest.raises(RuntimeError, match="SGD"):
        sgd.attach_adamw(master_weights=True)
    with pytest.raises(NotImplementedError, match="one GPU"):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16, nranks=2, rank=0, comm=LoopbackHub(2).comm(0))
    with pytest.raises(NotImplementedError, match="chunk_cols"):
        pkg.VirtualWorkerGroup(topo, numel=100_000, dtype=torch.bfloat16, chunk_cols=4096)
    with pytest.raises(ValueError):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).attach_adamw(betas=(0.9, 1.0 - 2.0 ** -24),
                                                                                   master_weights=True)


def test_graph_replay_equals_eager_steps(pkg, O):
    """adamw_device_round captured once, replayed over a 6-round schedule with fresh gradients and a
    learning rate changed after round 3 through lr_dev == six adamw_step calls on a twin == the
    specification, for all five arrays; both device counters advance by one per replay, and a replay
    past the schedule writes nothing."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    hyper = HYPERS["A1"]
    table = _table(hyper)
    n, P = 8, 2 * int(pkg.lib.mx_adamw_mix_bf16_tile(8)) + 77
    rng = np.random.default_rng(61)
    W0 = rng.standard_normal((n, P)).astype(np.float32)
    Gs = [_grads(rng, (n, P)) for _ in range(7)]
    lrs = [1e-3, 1e-3, 1e-3, 1e-3, 2.5e-4, 2.5e-4]
    eager = _group(pkg, topo, P, "A1", True)
    _put(eager.master_rows, W0)
    W, Mo, V = W0, np.zeros_like(W0), np.zeros_like(W0)
    for it in range(6):
        _put_bits(eager.grads, Gs[it])
        eager.adamw_step(it, lrs[it])
        W, Mo, V, Pb, _ = spec_round(O, W, Gs[it], Mo, V, it + 1, partner, flags[it], alpha, lrs[it], hyper, table)
    want = _state(eager)
    assert eq32(want[0], W) and eq32(want[2], Mo) and eq32(want[3], V) and np.array_equal(want[4], Pb)
    assert not want[1].any()

    grp = _group(pkg, topo, P, "A1", True)
    _put(grp.master_rows, W0)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            grp.adamw_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and int(grp.opt_step_dev.item()) == 1      # capture ran nothing
    assert eq32(grp.master_rows.cpu().numpy(), W0) and not _bits(grp.rows).any()
    for it in range(6):
        _put_bits(grp.grads, Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = _state(grp)
    assert _same_state(got, want)
    assert int(grp.iter_dev.item()) == 6 and int(grp.opt_step_dev.item()) == 7
    _put_bits(grp.grads, Gs[6])                      # past the schedule: no mix, no step, g not zeroed
    g.replay()
    past = _state(grp)
    assert int(grp.iter_dev.item()) == 7 and int(grp.opt_step_dev.item()) == 8
    assert eq32(past[0], want[0]) and eq32(past[2], want[2]) and eq32(past[3], want[3])
    assert np.array_equal(past[4], want[4]) and np.array_equal(past[1], Gs[6])


def _mlp():
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5)).cuda().to(torch.bfloat16)


def test_python_surface(pkg, O):
    partner, alpha = _topology(pkg, "g0")
    M = partner.shape[0]
    topo = Topo(partner, alpha, np.ones((4, M), np.uint8))
    with pytest.raises(pkg.MXError, match="master"):
        pkg.VirtualWorkerGroup(topo, numel=100).master_from_rows()
    with pytest.raises(pkg.MXError, match="attach_adamw"):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.bfloat16).adamw_step(0, LR)

    n = 8
    torch.manual_seed(0)
    models = [_mlp() for _ in range(n)]
    start = [torch.cat([p.detach().reshape(-1) for p in m.parameters()]) for m in models]
    grp = pkg.VirtualWorkerGroup(topo, models, dtype=torch.bfloat16)
    grp.attach_adamw(weight_decay=1e-2, master_weights=True)
    assert grp.adamw_hyper == {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2, "decoupled": True,
                               "zero_grads": True}
    assert torch.equal(grp.rows, torch.stack(start))
    assert torch.equal(grp.master_rows, grp.rows.float())            # the exact widening
    assert grp.exp_avg_arena.dtype == grp.exp_avg_sq_arena.dtype == torch.float32
    assert not grp.exp_avg_arena.any().item() and not grp.exp_avg_sq_arena.any().item()
    assert grp.opt_step == 0 and int(grp.opt_step_dev.item()) == 1 and grp.lr_dev.dtype == torch.float32
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
    # one step from what backward() left, by the specification
    W, G, Mo, V, _ = _state(grp)
    hyper = (0.9, 0.999, 1e-8, 1e-2, True)
    assert grp.adamw_step(0, LR)
    ww, wm, wv, wp, _ = spec_round(O, W, G, Mo, V, 1, partner, np.ones(M, np.uint8), alpha, LR, hyper, _table(hyper))
    gw, gg, gm, gv, gp = _state(grp)
    assert eq32(gw, ww) and eq32(gm, wm) and eq32(gv, wv) and np.array_equal(gp, wp) and not gg.any()

    def steps(g, its):
        for it in its:
            _put_bits(g.grads, Gs[it])
            g.adamw_step(it, LR)

    rng = np.random.default_rng(71)
    Gs = [_grads(rng, (n, grp.numel)) for _ in range(4)]
    steps(grp, range(1, 2))
    grp.iter = 2
    ckpt = grp.state_dict()
    assert set(ckpt) == {"kind", "iter", "row_base", "workers", "rows", "master_rows", "exp_avg_rows",
                         "exp_avg_sq_rows", "opt_step"}
    assert ckpt["master_rows"].dtype == torch.float32 and ckpt["rows"].dtype == torch.bfloat16
    assert ckpt["exp_avg_rows"].dtype == ckpt["exp_avg_sq_rows"].dtype == torch.float32 and ckpt["opt_step"] == 2

    def fresh():
        g = pkg.VirtualWorkerGroup(topo, numel=grp.numel, dtype=torch.bfloat16)
        g.attach_adamw(weight_decay=1e-2, master_weights=True)
        return g

    twin = fresh()
    twin.load_state_dict(ckpt)
    assert twin.iter == 2 and twin.opt_step == 2 and int(twin.opt_step_dev.item()) == 3
    assert _same_state(_state(twin), _state(grp))
    steps(grp, range(2, 4))
    steps(twin, range(2, 4))
    assert _same_state(_state(twin), _state(grp)) and twin.opt_step == grp.opt_step == 4   # continues bit for bit
    # a bare checkpoint: the widened rows, zero buffers, step 0; after a direct write to rows, master_from_rows()
    bare = {k: v for k, v in ckpt.items() if k not in ("master_rows", "exp_avg_rows", "exp_avg_sq_rows", "opt_step")}
    twin.load_state_dict(bare)
    assert torch.equal(twin.master_rows, ckpt["rows"].float()) and not torch.equal(twin.master_rows, ckpt["master_rows"])
    assert not twin.exp_avg_rows.any().item() and not twin.exp_avg_sq_rows.any().item()
    assert twin.opt_step == 0 and int(twin.opt_step_dev.item()) == 1
    with torch.no_grad():
        twin.rows.copy_(grp.rows)
    assert not torch.equal(twin.master_rows, grp.rows.float())
    twin.master_from_rows()
    assert torch.equal(twin.master_rows, grp.rows.float())
    # masters and Adam state are refused by groups that have none
    with pytest.raises(ValueError, match="master"):
        pkg.VirtualWorkerGroup(topo, numel=grp.numel, dtype=torch.bfloat16).load_state_dict(
            {k: v for k, v in ckpt.items() if k not in ("exp_avg_rows", "exp_avg_sq_rows", "opt_step")})
    with pytest.raises(ValueError, match="attach_adamw"):
        pkg.VirtualWorkerGroup(topo, numel=grp.numel, dtype=torch.bfloat16).load_state_dict(
            {k: v for k, v in ckpt.items() if k != "master_rows"})


def test_against_torch_adamw_then_step(pkg):
    """The fused launches against the unfused sequence on plain CUDA tensors, 5 steps, masters in
    [-1, 1): g.float(), torch.optim.AdamW.step() on fp32 masters, the fp32 group.step of a twin fp32
    group, .to(torch.bfloat16).  Masters: |diff| <= 2^-23, the bound of tests/test_gpu_adamw_mix.py's
    torch comparison -- g.float() is exact, so the arithmetic on the masters is the same.  p equals
    torch's .to(torch.bfloat16) of THIS kernel's masters exactly."""
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((5, partner.shape[0]), np.uint8))
    b1, b2, eps, wd, _ = HYPERS["A1"]
    n, P = 8, 4097
    rng = np.random.default_rng(81)
    W = rng.uniform(-1, 1, (n, P)).astype(np.float32)
    fused = _group(pkg, topo, P, "A1", True)
    _put(fused.master_rows, W)
    params = [torch.nn.Parameter(torch.from_numpy(W[r].copy()).cuda()) for r in range(n)]
    opts = [torch.optim.AdamW([p], lr=LR, betas=(b1, b2), eps=eps, weight_decay=wd) for p in params]
    twin = pkg.VirtualWorkerGroup(topo, numel=P)
    worst = 0.0
    for it in range(5):
        G = _grads(rng, (n, P))
        _put_bits(fused.grads, G)
        assert fused.adamw_step(it, LR)
        gbf = torch.from_numpy(G.view(np.int16)).cuda().view(torch.bfloat16)
        for r, p in enumerate(params):
            p.grad = gbf[r].float()
            opts[r].step()
        with torch.no_grad():
            twin.rows.copy_(torch.stack([p.detach() for p in params]))
            assert twin.step(it)
            for r, p in enumerate(params):
                p.copy_(twin.rows[r])
        torch.cuda.synchronize()
        a, b = fused.master_rows.cpu().numpy().astype(np.float64), twin.rows.cpu().numpy().astype(np.float64)
        diff = float(np.abs(a - b).max())
        worst = max(worst, diff)
        tp = _bits(twin.rows.to(torch.bfloat16))
        print(f"step {it + 1}: fused mixed-precision vs g.float() + torch.optim.AdamW + step: max |diff| = {diff:.3e} "
              f"({diff * 2 ** 24:.2f} x 2^-24); p vs torch's bf16 of the unfused masters: "
              f"{int((tp != _bits(fused.rows)).sum())} of {n * P} differ")
        assert torch.equal(fused.rows, fused.master_rows.to(torch.bfloat16)), it
    assert not np.isnan(a).any() and np.abs(b).max() < 1.01 and worst <= 2.0 ** -23


def test_virtual_trainer_fused_adamw_bf16(pkg, O):
    """harness.VirtualTrainer(fused_adamw=True) with bfloat16 models: every iteration's fused launch by
    the specification from the masters, gradients and Adam state the backward passes left; the torch
    optimizers never step; a checkpoint resumed in a new trainer continues bit for bit."""
    H = pkg.harness

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=1e-3, matcha=True, warmup=False)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        fn = H.model_factory(args)
        kw.setdefault("fused_adamw", True)
        return H.VirtualTrainer(args, lambda: fn().to(torch.bfloat16), n_batches=3, **kw)

    tr = make()
    grp = tr.group
    assert grp.dtype == torch.bfloat16 and grp.master_rows is not None and grp.exp_avg_rows is not None
    assert grp.adamw_hyper == {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 5e-4, "decoupled": True,
                               "zero_grads": True}
    assert all(p.dtype == torch.bfloat16 and p.grad.dtype == torch.bfloat16 for m in tr.models for p in m.parameters())
    assert torch.equal(grp.master_rows, grp.rows.float())            # master_from_rows() after sync_rows
    assert all(torch.equal(grp.rows[0], grp.rows[r]) for r in range(8))
    hyper = (0.9, 0.999, 1e-8, 5e-4, True)
    table = _table(hyper)
    partner = np.asarray(tr.GP.neighbors_info, np.int32)
    state, seen = {}, {"rounds": 0}

    def hook(when, t):
        if when == "before":
            state["s"], state["it"], state["step"] = _state(t.group), t.group.iter, t.group.opt_step
            assert state["s"][1].any()                               # backward() filled the gradient arena
            return
        flags = np.asarray(tr.GP.active_flags[state["it"]], np.uint8)
        lr = t.optimizers[0].param_groups[0]["lr"]
        W, G, Mo, V, _ = state["s"]
        ww, wm, wv, wp, _ = spec_round(O, W, G, Mo, V, state["step"] + 1, partner[:len(flags)], flags,
                                       tr.GP.neighbor_weight, lr, hyper, table)
        gw, gg, gm, gv, gp = _state(t.group)
        assert eq32(gw, ww) and eq32(gm, wm) and eq32(gv, wv) and bf16ref.same_bf16(gp, wp) and not gg.any(), \
            f"round {state['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats)
    assert seen["rounds"] == 3 and grp.iter == 3 and grp.opt_step == 3
    assert all(not o.state for o in tr.optimizers)                   # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert ckpt["group"]["opt_step"] == 3
    assert eq32(ckpt["group"]["master_rows"].cpu().numpy(), grp.master_rows.cpu().numpy())
    tr2 = make()
    tr2.load_state_dict(ckpt)
    assert tr2.epoch == 1 and tr2.group.iter == 3 and tr2.group.opt_step == 3
    tr.train_epoch()
    tr2.train_epoch()
    assert _same_state(_state(tr.group), _state(tr2.group)) and tr.group.opt_step == tr2.group.opt_step == 6
    with pytest.raises(ValueError, match="fused_adamw"):
        make(batched=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        make(fused_sgd=True)
