"""The five LDS row kernels -- mix_bf16_rows (csrc/mix_bf16.hip) and the four fused_round_rows families
(csrc/fused_round.h) -- where the graphs of topologies.py do not take them: partly filled row classes (9-15,
17-31 and 33-63 rows: staging steps skipped by k < n_local, uneven -1 suffixes in the dealing), the 32-slot
bf16 class, M = 32 matchings (the largest plan record, src[r * M + e] at stride 32), chains of 32 partners
and chains of 32 beside chains of 1 and 0 inside one wave's interleaved pair (tail loops of dozens of
steps), and alignment that differs from row to row inside one segment.

Every comparison is against the existing specifications (bf16ref, sgdref / sgdbf16ref / adamref /
adambf16ref through clipref and groupref), never the code under test: uint32 for uint32, uint16 for uint16.
The tables of tests/rowtopos.py with ALPHA = 1/64 make every round a convex combination, so no NaN or Inf
arises (tests/test_row_topos_cpu.py; asserted on every reference output here) and every element is compared
bit for bit; special values stay with the existing tests.

Widths per case: 1, 9, one work item - 1, one layout tile + 9, three tiles + 5.

The dealing ranks the items by weight, descending, and a wave's list keeps that order, so of a wave's
interleaved pair the first item never has the shorter chain: the long tail loop is the first one (`ea`), and
the second (`eb`) runs only under another dealing.  These tests pin results, not scheduling: they pass
unchanged when every used row is dealt with weight 1, which makes the second tail loop the live one."""
import ctypes

import numpy as np
import pytest

import bf16ref
import clipref
from abitables import PaddedTables
from conftest import Topo
from rowtopos import ALPHA, N_ALL, cases, flag_rounds, round_robin, table
from test_gpu_bf16 import _raw_call
from test_gpu_clip_fused import ADAM_HYPER, KINDS, LR, SGD_HYPER, _scales, _table, _u32
from test_gpu_grad_norm import _launch as _norm_launch
from test_gpu_param_groups import SCALES, WDS, GKind, _f, _runs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
BF16 = torch.bfloat16
# per row class (8, 16, 32, 64): layout tile and work-item width
BF16_TILE, BF16_TW = (2048, 2048, 1024, 512), (1024, 1024, 1024, 512)
FUSED_TILE, FUSED_TW = (1024, 1024, 512, 256), (512, 512, 512, 256)
N_FUSED = [1, 5, 12, 24, 32, 33, 63, 64]
ENDS6 = [3, 6, 255, 257, 513, 1029]


def _cls(n):
    return 0 if n <= 8 else 1 if n <= 16 else 2 if n <= 32 else 3


def _widths(tile, tw):
    return [1, 9, tw - 1, tile + 9, 3 * tile + 5]


def _put16(t, bits):
    t.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)))


def _get16(t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _finite16(bits):
    return bool(np.isfinite(bf16ref.upcast(bits)).all())


def _tails_zero(grp, P):
    """nothing of any arena of the group past column P was written"""
    for name in ("arena", "grad_arena", "master_arena", "mom_arena", "exp_avg_arena", "exp_avg_sq_arena"):
        a = getattr(grp, name, None)
        if a is not None and a[:, P:].view(torch.int16 if a.dtype == BF16 else torch.int32).any().item():
            return False
    return True


def _bf16_rounds(pkg, O, partner, flags, idle_rows, P, rng, where):
    """the rounds of `flags` on a fresh bf16 group of width P, the state carried: each equal to the
    specification, uint16 for uint16"""
    n = partner.shape[1]
    grp = pkg.VirtualWorkerGroup(Topo(partner, ALPHA, flags), numel=P, idle_rows=idle_rows, dtype=BF16)
    X = bf16ref.random_bits(rng, (n, P), specials=False)
    _put16(grp.rows, X)
    for it, f in enumerate(flags):
        ran = grp.step(it)
        got = _get16(grp.rows)
        want = bf16ref.spec_round(O, X, partner, f, ALPHA, idle_rows)
        assert _finite16(want), f"{where} P={P} round {it}: the specification is not finite"
        assert ran == bool(f.any())
        bad = int((got != want).sum())
        assert bad == 0, f"{where} P={P} round {it}: {bad} elements differ"
        X = got
    assert not grp.arena[:, P:].view(torch.int16).any().item(), f"{where} P={P}: wrote past the row"


@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("n,name", cases(N_ALL))
def test_bf16_mix_every_class(pkg, O, n, name, idle_rows):
    """mix_bf16_rows at every row count of N_ALL -- n = 17, 24 and 32 reach the 32-slot kernel
    mix_bf16_rows<32, 1024, NT>, which no other test launches -- on round_robin (32 matchings, chains of 25-32)
    and star (a chain of min(32, n - 1) beside chains of 1 and 0): four carried rounds (every matching, a
    random half, the sparsest matching, all zero)"""
    partner = table(name, n)
    tile = int(pkg.lib.mx_mix_bf16_tile(n))
    assert tile == BF16_TILE[_cls(n)]
    flags = flag_rounds(partner, n)
    rng = np.random.default_rng([n, len(name), len(idle_rows)])
    for P in _widths(tile, BF16_TW[_cls(n)]):
        _bf16_rounds(pkg, O, partner, flags, idle_rows, P, rng, f"{name} n={n} {idle_rows}")


@pytest.mark.parametrize("knobs", [{"nontemporal": 0}, {"nontemporal": 1}, {"grid": 2}, {"blocks_per_cu": 1}])
@pytest.mark.parametrize("n,name", [(32, "rr"), (24, "star")])
def test_bf16_mix_32_class_knobs(pkg, O, n, name, knobs):
    """both streaming modes of mix_bf16_rows<32, 1024, NT>, and its persistent loop (the next work item's
    loads in flight while this one is mixed): "grid": 2 workgroups over 4 work items, and "blocks_per_cu": 1
    on the one width with more work items than the device has compute units.  Speed only: the bits of the
    specification under each."""
    L = pkg.lib
    partner = table(name, n)
    tile = int(L.mx_mix_bf16_tile(n))
    assert tile == 1024 == BF16_TW[2]
    flags = flag_rounds(partner, n)
    widths = [9, tile - 1, 3 * tile + 5]
    if "blocks_per_cu" in knobs:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        widths = [3 * tile + 5, (cus + 1) * tile + 5]          # cus + 2 work items on a grid of cus
        flags = flags[:2]                                      # (the wide reference: two rounds)
    rng = np.random.default_rng([n, len(name), 17])
    saved = {k: int(L.mx_mix_bf16_get(k.encode())) for k in knobs}
    try:
        for k, v in knobs.items():
            assert L.mx_mix_bf16_set(k.encode(), v) == 0
        for P in widths:
            _bf16_rounds(pkg, O, partner, flags, "skip", P, rng, f"{knobs} {name} n={n}")
    finally:
        for k, v in saved.items():
            L.mx_mix_bf16_set(k.encode(), v)


@pytest.mark.parametrize("n,name", [(33, "star"), (64, "rr")])
def test_bf16_mix_hints_beyond_eight_rows(pkg, O, n, name):
    """need_host masks over more than 8 rows through mx_gossip_mix_bf16_packed -- none, 0, the exact row set,
    every row of [0, n_local) and a wrong subset: identical bits (the plan record decides what is parked,
    mixed and stored; a hint only starts loads early).  Only bits below n_local are set."""
    partner = table(name, n)
    flags = flag_rounds(partner, n)
    topo = Topo(partner, ALPHA, flags)
    P = 3 * int(pkg.lib.mx_mix_bf16_tile(n)) + 5
    X0 = bf16ref.random_bits(np.random.default_rng([n, 23]), (n, P), specials=False)
    ones = (1 << n) - 1
    outs = []
    for mask in (None, 0, "exact", ones, 0x5555555555555555 & ones, 0xAAAAAAAAAAAAAAAA & ones):
        grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=BF16)
        exact = grp.engine.need_host
        assert exact is not None and len(exact) == len(flags) + 1 and all(int(v) <= ones for v in exact)
        need = None if mask is None else exact.copy() if mask == "exact" else np.full(len(flags) + 1, mask, np.uint64)
        call = _raw_call(pkg, grp.layout, grp.engine, need)
        _put16(grp.rows, X0)
        for it in range(len(flags)):
            assert pkg.lib.mx_gossip_mix_bf16_packed(ctypes.addressof(call), it, pkg._lib.stream_ptr()) == 0
        outs.append(_get16(grp.rows))
        assert not grp.arena[:, P:].view(torch.int16).any().item()
    X = X0
    for f in flags:
        X = bf16ref.spec_round(O, X, partner, f, ALPHA)
        assert _finite16(X)
    assert np.array_equal(outs[0], X)
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def _one_run(K, P):
    """the ungrouped launch as a run list for groupref: the family's own weight decay, lr scale 1"""
    return [(0, P, _f(K.hyper[3] if K.adam else K.hyper[0]), 1.0)]


def _finite_state(s):
    return all(np.isfinite(bf16ref.upcast(a) if a.dtype == np.uint16 else a).all() for a in s.values())


def _zeroed(K, g):
    return not g.view(np.uint16 if K.mixed else np.uint32).any()


_FUSED_CASES = [(n, name, "skip") for n, name in cases(N_FUSED)] + [(5, "star", "canonical"), (33, "star", "canonical")]


@pytest.mark.parametrize("n,name,idle", _FUSED_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_every_class(pkg, O, kind, n, name, idle):
    """the four fused families at partly filled and full row classes with M = 32 (one worker included: no
    fused test had n_local = 1): three carried rounds (every matching, a random half, all zero), zero_grads
    alternating by width; SGD with momentum and Nesterov, Adam with a live L2 term.  "canonical" where rows
    of degree 0 sit beside the hub."""
    K = GKind(kind)
    partner = table(name, n)
    flags = flag_rounds(partner, n)[[0, 1, 3]]
    topo = Topo(partner, ALPHA, flags)
    fam = pkg.engine.FAMILIES["adamw" if K.adam else "sgd", K.mixed]
    tile = int(fam.tile(n))
    assert tile == FUSED_TILE[_cls(n)]
    rng = np.random.default_rng([KINDS.index(kind), n, len(name), len(idle)])
    for wi, P in enumerate(_widths(tile, FUSED_TW[_cls(n)])):
        zero = bool(wi & 1)
        grp = K.group(pkg, topo, P, zero, idle, hyper=ADAM_HYPER if K.adam else SGD_HYPER)
        K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
        s = K.state(grp)
        for it in range(3):
            G = K.grads(rng, (n, P))
            K.put_g(grp, G)
            K.step(grp, it, LR)
            got = K.state(grp)
            want = K.gspec(O, s, G, None, _one_run(K, P), it + 1, partner, flags[it], ALPHA, LR, idle)
            where = f"{kind} {name} n={n} {idle} P={P} round {it}"
            assert _finite_state(want), where + ": the specification is not finite"
            for k in want:
                assert GKind.same(got, want, [k]), where + ": " + k
            if zero:
                assert _zeroed(K, got["g"]), where + ": g not zeroed"
            else:
                assert GKind.same(got, {"g": G}, ["g"]), where + ": g was rewritten"
            s = got
        assert _tails_zero(grp, P), f"{kind} {name} n={n} P={P}: wrote past the row"


@pytest.mark.parametrize("n,name", [(33, "star"), (12, "rr")])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_grouped_scaled_partial_class(pkg, O, kind, n, name):
    """the grouped launch with per-row clip factors on a partly filled class at M = 32 (33 rows of the
    64-row class, 12 of the 16-row class): runs ending at 3, 6, 255, 257, 513 and 1029 with pairs from
    WDS x SCALES, factors distinct per row; eagerly, and on a persistent grid of 2 workgroups"""
    K = GKind(kind)
    partner = table(name, n)
    flags = flag_rounds(partner, n)[[0, 1, 3]]
    topo = Topo(partner, ALPHA, flags)
    P = ENDS6[-1]
    runs = _runs(ENDS6, [(WDS[(i + i // 3) % 3], SCALES[i % 4]) for i in range(len(ENDS6))])
    assert {r[3] for r in runs} == {_f(v) for v in SCALES} and {r[2] for r in runs} == {_f(v) for v in WDS}
    scale = _scales(n)
    sc = torch.from_numpy(scale).cuda()
    get, put = K.tuning(pkg)
    saved = get()
    for zero, knobs in ((True, {}), (False, {"grid": 2})):
        rng = np.random.default_rng([KINDS.index(kind), n, 29])
        put(**knobs)
        try:
            grp = K.group(pkg, topo, P, zero, hyper=ADAM_HYPER if K.adam else SGD_HYPER)
            K.inject(pkg, grp, runs)
            K.put_x(grp, rng.standard_normal((n, P)).astype(F32))
            s = K.state(grp)
            for it in range(3):
                G = K.grads(rng, (n, P))
                K.put_g(grp, G)
                K.glaunch(pkg, grp, grp._runs.addr, sc.data_ptr(), it, it + 1, LR)
                got = K.state(grp)
                want = K.gspec(O, s, G, scale, runs, it + 1, partner, flags[it], ALPHA, LR)
                where = f"{kind} {name} n={n} {knobs} round {it}"
                assert _finite_state(want), where + ": the specification is not finite"
                for k in want:
                    assert GKind.same(got, want, [k]), where + ": " + k
                assert _zeroed(K, got["g"]) if zero else GKind.same(got, {"g": G}, ["g"]), where + ": g"
                s = got
            assert _tails_zero(grp, P), f"{kind} {name} n={n} {knobs}: wrote past the row"
        finally:
            put(**saved)
    assert get() == saved


# ---------------------------------------------------------------- alignment that differs from row to row

def _fused_offsets(K):
    """the element offset of (array, segment, row), the same in every segment, by r % 4:
    0: everything 16-byte aligned; 1: the fp32 arrays one float off; 2: bf16 families g and p 8-byte but not
    16-byte aligned (4 elements: the vector path still), fp32 families g alone one float off; 3: one state
    array alone one float off, v for AdamW and m for SGD"""
    state = "v" if K.adam else "m"

    def off(k, s, r):
        q = r % 4
        if q == 1:
            return 0 if k in "gp" and K.mixed else 1
        if q == 2:
            return (4 if k in "gp" else 0) if K.mixed else (1 if k == "g" else 0)
        if q == 3:
            return 1 if k == state else 0
        return 0
    return off


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_abi_rows_of_mixed_alignment(pkg, O, kind, grouped):
    """the raw C ABI on three-segment tables (5, 0 and T + 3 elements: a zero-length segment between two
    others) over padded buffers, 5 rows, every row of a segment aligned differently (see _fused_offsets) --
    vector rows and element rows in one work item.  Three rounds with zero_grads: bit-equal to the
    specification, g zeroed exactly within the lengths, every guard word intact; grouped: a run boundary
    inside a 4-element chunk (column 6) and inside another (257).  mx_grad_norm on the same g table: within
    1 ulp of clipref's norm."""
    E = pkg.engine
    K = GKind(kind)
    K.hyper = ADAM_HYPER if K.adam else SGD_HYPER
    fam = E.FAMILIES["adamw" if K.adam else "sgd", K.mixed]
    n = 5
    partner = round_robin(n)
    flags = flag_rounds(partner, n)[[0, 1, 3]]
    eng = pkg.GossipEngine(Topo(partner, ALPHA, flags))
    T = int(fam.tile(n))
    lens = [5, 0, T + 3]
    dtypes = {k: np.uint16 if (K.mixed and k in "gp") else np.float32 for k in fam.tables}
    pt = PaddedTables(n, lens, dtypes, _fused_offsets(K))
    # the alignments the docstring promises
    xk = fam.tables[0]
    for k in fam.tables:
        p = np.array(pt.ptrs(k))
        assert (p[0] % 16 == 0).all() and (p[4] % 16 == 0).all()
    assert (np.array(pt.ptrs(xk))[1] % 16 == 4).all() and (np.array(pt.ptrs(xk))[2] % 16 == 0).all()
    assert (np.array(pt.ptrs("g"))[2] % 16 == (8 if K.mixed else 4)).all()
    assert (np.array(pt.ptrs("v" if K.adam else "m"))[3] % 16 == 4).all() and (np.array(pt.ptrs(xk))[3] % 16 == 0).all()

    tabs = [pt.ptrs(k) for k in fam.tables]
    if K.adam:
        lay = E.FUSED_LAYOUTS["adamw", K.mixed](lens, *tabs, n, _table(K.hyper))
        b1, b2, eps, wd, dec = K.hyper
        call = lay.call(eng, (b1, b2), eps, wd, dec, True)
    else:
        lay = E.FUSED_LAYOUTS["sgd", K.mixed](lens, *tabs, n)
        wd, mom, nest = K.hyper
        call = lay.call(eng, wd, mom, nest, True)
    assert lay.total_tiles == 3
    addr = ctypes.addressof(call)

    P = pt.P
    if grouped:                                   # per segment: (3, 5) | none | (6, 257, T + 3)
        seg_runs = [[3, 5], [], [6, 257, T + 3]]
        pairs = [(WDS[(i + i // 3) % 3], SCALES[i % 4]) for i in range(5)]
        off = np.cumsum([0] + [len(r) for r in seg_runs]).astype(np.int32)
        end = np.array([e for r in seg_runs for e in r], np.int64)
        wds = np.array([_f(p[0]) for p in pairs], F32)
        lrs = np.array([_f(p[1]) for p in pairs], F32)
        sl = np.array(lens, np.int64)
        assert pkg.lib.mx_param_runs_check(sl.ctypes.data, 3, off.ctypes.data, end.ctypes.data, wds.ctypes.data,
                                           lrs.ctypes.data) == 0, pkg.lib.mx_last_error()
        dev_runs = [torch.from_numpy(a).cuda() for a in (off, end, wds, lrs)]
        rec = E.ParamRunsRec(*(t.data_ptr() for t in dev_runs), len(end))
        runs_addr = ctypes.addressof(rec)
        runs = _runs([3, 5, 5 + 6, 5 + 257, P], pairs)        # the same runs on the segments side by side
    else:
        runs_addr, runs = None, _one_run(K, P)

    rng = np.random.default_rng([KINDS.index(kind), int(grouped), 31])
    pt.put(xk, rng.standard_normal((n, P)).astype(F32))
    for k in fam.tables[2:]:
        pt.put(k, np.zeros((n, P), dtypes[k]))     # m, v: zeros; p: never read, always overwritten
    s = {"x": pt.get(xk), "m": pt.get("m")}
    if K.adam:
        s["v"] = pt.get("v")
    grouped_fn, _ = K.gfns(pkg)
    sp = pkg._lib.stream_ptr()
    for it in range(3):
        G = K.grads(rng, (n, P))
        pt.put("g", G)
        if it == 0:                                # the norm kernel on the same table: vector and element rows
            g_tab = np.ascontiguousarray(np.array(pt.ptrs("g"), np.int64).T)
            norm, scale = _norm_launch(pkg, g_tab, lens, 2 if K.mixed else 4)
            assert np.isfinite(norm).all() and int(clipref.ulp_diff(norm, clipref.grad_norm_ref(K.g32(G))).max()) <= 1
            assert np.array_equal(_u32(scale), _u32(clipref.clip_scale_ref(norm, 1.0)))
            assert np.array_equal(pt.get("g"), G) and pt.guards_intact("g")
        rc = grouped_fn(addr, runs_addr, None, it, it + 1, LR, None, sp) if K.adam else \
            grouped_fn(addr, runs_addr, None, it, LR, None, sp)
        assert rc == 0, pkg.lib.mx_last_error()
        want = K.gspec(O, s, G, None, runs, it + 1, partner, flags[it], ALPHA, LR)
        got = {"x": pt.get(xk), "m": pt.get("m")}
        if K.adam:
            got["v"] = pt.get("v")
        if K.mixed:
            got["p"] = pt.get("p")
        where = f"{kind} grouped={grouped} round {it}"
        assert _finite_state(want), where + ": the specification is not finite"
        for k in want:
            assert GKind.same(got, want, [k]), where + ": " + k
        assert _zeroed(K, pt.get("g")), where + ": g not zeroed within the lengths"
        for k in fam.tables:
            assert pt.guards_intact(k), where + f": guard words of {k}"
        s = got


def test_abi_rows_of_mixed_alignment_bf16_mix(pkg, O):
    """mx_gossip_mix_bf16_packed on the three-segment tables (5, 0, T + 3) with rows alternating between
    16-byte aligned and 2 bytes off: load_chunk / store_chunk take the row's own pointer, so one work item
    holds 16-byte rows and element rows.  Exact, every guard word intact."""
    n = 5
    partner = round_robin(n)
    flags = flag_rounds(partner, n)
    eng = pkg.GossipEngine(Topo(partner, ALPHA, flags))
    T = int(pkg.lib.mx_mix_bf16_tile(n))
    lens = [5, 0, T + 3]
    pt = PaddedTables(n, lens, {"x": np.uint16}, lambda k, s, r: r & 1)
    ptrs = pt.ptrs("x")
    assert all(p % 16 == 2 * (r & 1) for r, row in enumerate(ptrs) for p in row)
    lay = pkg.Layout(lens, ptrs, eng.n_slots, dtype=BF16)
    assert lay.total_tiles == 3
    call = _raw_call(pkg, lay, eng)
    X = bf16ref.random_bits(np.random.default_rng(37), (n, pt.P), specials=False)
    pt.put("x", X)
    for it, f in enumerate(flags):
        assert pkg.lib.mx_gossip_mix_bf16_packed(ctypes.addressof(call), it, pkg._lib.stream_ptr()) == 0
        X = bf16ref.spec_round(O, X, partner, f, ALPHA)
        assert _finite16(X)
        assert np.array_equal(pt.get("x"), X), f"round {it}"
        assert pt.guards_intact("x"), f"round {it}: guard words"

