"""GPU: the store policy of the streaming kernels' 16-byte row stores (mx_mix_set "store_policy":
0 auto, 1 nt, 2 sc1, 3 sc1 nt, 4 sc0 sc1) in mix_kernel_rows' 8- and 16-slot classes (plain flat-grid
form and the SPEC form, registers and LDS-DMA) and in mean_tile_kernel, and the fused optimizer rounds'
own knob (mx_<family>_set "store_policy": 0 auto, 1 nt, 2 sc1, 3 sc1 nt) on x, m, v and the masters.

A policy decides when a written line leaves the L2, never what is written: every case runs under every
forced policy and compares uint32 for uint32 against the oracle (decenCommunicator.averaging,
communicator.py:92-122; centralizedCommunicator, communicator.py:46-76) and against the forced nt run."""
import ctypes

import numpy as np
import pytest

from abitables import PaddedTables
from conftest import Topo
from rowtopos import ALPHA, flag_rounds, round_robin
from test_gpu_clip_fused import ADAM_HYPER, KINDS, LR, SGD_HYPER, Kind, _table, _topology

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POLICIES = (1, 2, 3, 4)          # nt first: the run every other policy is compared with
P_SMALL = 1541                   # three full 512-column sub-tiles and a ragged tail of 5
P_SPEC = 2_100_003               # 8 rows > 64 MB: the SPEC form applies with nontemporal = 1
P_MEAN = (4099, 2_500_003)       # flat launch; > 64 MB: the capped launch


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _spec_launches(pkg):
    return int(pkg.lib.mx_mix_get(b"spec_launches"))


def _under_policies(pkg, run, want, knobs=None):
    """run() under every forced policy: each result equals `want` and the nt result, bit for bit"""
    E = pkg.engine
    saved = E.mix_tuning()
    try:
        first = None
        for pol in POLICIES:
            E.set_mix_tuning(store_policy=pol, **(knobs or {}))
            got = _u32(run())
            assert np.array_equal(got, _u32(want)), f"policy {pol}: differs from the oracle"
            if first is None:
                first = got
            assert np.array_equal(got, first), f"policy {pol}: differs from nt"
    finally:
        E.set_mix_tuning(**saved)


def _group_rounds(pkg, topo, X0, rounds):
    """`rounds` rounds of a fresh arena group holding X0"""
    n, P = X0.shape
    g = pkg.VirtualWorkerGroup(topo, numel=P)
    g.rows[:, :P] = torch.from_numpy(X0).cuda()
    for it in range(rounds):
        g.step(it)
    torch.cuda.synchronize()
    got = g.rows[:, :P].cpu().numpy()
    tail = bool(g.arena[:, P:].view(torch.int32).any().item())
    g.close()
    assert not tail, "wrote past the row"
    return got


def _oracle_rounds(O, X, partner, flags, alpha, rounds):
    partner = np.asarray(partner, np.int32)
    flags = np.asarray(flags, np.uint8)
    for it in range(rounds):
        if flags[it].any():
            X = O.decen_round(X, partner, flags[it], alpha)
    return X


@pytest.mark.parametrize("budget", [1.0, 0.5])
def test_rows_plain_form(pkg, O, budget):
    """8 workers, graph 0, 3 rounds of 8 x 1541: the flat-grid plain form, 16-byte stores in the full
    sub-tiles and element stores in the tail."""
    np.random.seed(1234)
    GP = pkg.MatchaProcessor(pkg.select_graph(0), budget, 0, 8, 3, True)
    X0 = np.stack([O.synth(4100 + i, P_SMALL) for i in range(8)])
    want = _oracle_rounds(O, X0, GP.neighbors_info, GP.active_flags, GP.neighbor_weight, 3)
    _under_policies(pkg, lambda: _group_rounds(pkg, GP, X0, 3), want)


@pytest.mark.parametrize("base", [0, 1])
def test_rows_pointer_table(pkg, O, base):
    """A pointer-table layout with segments of 5, 1024 and 3000 columns; base 1 starts every row 4 bytes
    off a 16-byte boundary, so every store takes the element path whatever the policy."""
    n = 8
    lens = [5, 1024, 3000]
    P = sum(lens)
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, n, 4, True)
    flags = np.ones((3, len(gp.neighbors_info)), np.uint8)
    flags[1, 1::2] = 0
    flags[2, ::3] = 0
    topo = Topo(gp.neighbors_info, 0.21, flags)
    X0 = np.stack([O.synth(800 + i, P) for i in range(n)])
    want = _oracle_rounds(O, X0, topo.neighbors_info, flags, 0.21, 3)
    # segments at multiples of 4 floats inside a row, so at base 0 every segment start is 16-byte aligned
    starts = np.cumsum([0] + [(v + 3) // 4 * 4 for v in lens])
    width = int(starts[-1]) + 8

    def run():
        eng = pkg.GossipEngine(topo)
        big = torch.zeros((n, width), dtype=torch.float32, device="cuda")
        for s, ln in enumerate(lens):
            a, b = int(np.cumsum([0] + lens)[s]), base + int(starts[s])
            big[:, b:b + ln] = torch.from_numpy(X0[:, a:a + ln]).cuda()
        ptrs = [[big[i].data_ptr() + 4 * (base + int(starts[s])) for s in range(len(lens))] for i in range(n)]
        assert all((p % 16 == 4 * base) for row in ptrs for p in row)
        lay = pkg.Layout(lens, ptrs, eng.n_slots)
        for it in range(3):
            eng.mix(it, lay)
        torch.cuda.synchronize()
        out = big.cpu().numpy()
        got = np.concatenate([out[:, base + int(starts[s]):base + int(starts[s]) + ln] for s, ln in enumerate(lens)], axis=1)
        mask = np.ones(width, bool)
        for s, ln in enumerate(lens):
            mask[base + int(starts[s]):base + int(starts[s]) + ln] = False
        assert not _u32(out[:, mask]).any(), "wrote outside the segments"
        return got

    _under_policies(pkg, run, want)


def test_rows_16_slot_class(pkg, O):
    """16 workers on the round-robin table (32 matchings): the 16-slot class, 8 x ... x 1541."""
    partner = round_robin(16)
    flags = flag_rounds(partner, 16)
    topo = Topo(partner, ALPHA, flags)
    assert pkg.engine.mix_kernel_name(16) == "mix_kernel_rows"
    X0 = np.stack([O.synth(300 + i, P_SMALL) for i in range(16)])
    want = _oracle_rounds(O, X0, partner, flags, ALPHA, len(flags))
    _under_policies(pkg, lambda: _group_rounds(pkg, topo, X0, len(flags)), want)


_SPEC_REF = {}


def _spec_case(pkg, O):
    """the SPEC cases' schedule, rows and oracle result, computed once"""
    if not _SPEC_REF:
        np.random.seed(1234)
        GP = pkg.MatchaProcessor(pkg.select_graph(0), 0.5, 0, 8, 3, True)
        X0 = np.stack([O.synth(4100 + i, P_SPEC) for i in range(8)])
        want = _oracle_rounds(O, X0, GP.neighbors_info, GP.active_flags, GP.neighbor_weight, 3)
        active = int(np.asarray(GP.active_flags, np.uint8)[:3].any(axis=1).sum())
        _SPEC_REF.update(GP=GP, X0=X0, want=want, active=active)
    return _SPEC_REF


@pytest.mark.parametrize("glds", [0, 1])
def test_rows_spec_form(pkg, O, glds):
    """8 x 2,100,003 (> 64 MB) with nontemporal = 1 and spec = 1, through registers and by LDS-DMA, budget
    0.5, 3 rounds: every policy launches the SPEC form (counted) and gives the oracle's bits."""
    ref = _spec_case(pkg, O)
    assert ref["active"] >= 1
    counts = []

    def run():
        n0 = _spec_launches(pkg)
        got = _group_rounds(pkg, ref["GP"], ref["X0"], 3)
        counts.append(_spec_launches(pkg) - n0)
        return got

    _under_policies(pkg, run, ref["want"], {"nontemporal": 1, "spec": 1, "spec_wgpc": 5, "spec_glds": glds})
    assert counts == [ref["active"]] * len(POLICIES)


_MEAN_REF = {}


@pytest.mark.parametrize("order", ["tree", "sequential"])
@pytest.mark.parametrize("P", P_MEAN)
def test_mean_tile(pkg, O, P, order):
    """mx_mean_rows_to on 8 rows in place, both summation orders: every destination row is the oracle's
    reference-order mean under every policy."""
    L = pkg.lib
    n = 8
    ld = (P + 63) // 64 * 64
    if P not in _MEAN_REF:
        _MEAN_REF[P] = np.stack([O.synth(500 + i, P) * np.float32(1 + i % 3) for i in range(n)])
    X = _MEAN_REF[P]
    want = np.broadcast_to(O.central_mean(X, order), (n, P))
    code = {"tree": 0, "sequential": 1}[order]
    assert L.mx_mean_kernel_name(0, n, ld, P, code, 0, n, ld).decode().startswith("mean_tile_kernel")

    def run():
        rows = torch.zeros((n, ld), dtype=torch.float32, device="cuda")
        rows[:, :P] = torch.from_numpy(X).cuda()
        pkg._lib.check(L.mx_mean_rows_to(rows.data_ptr(), n, ld, P, code, rows.data_ptr(), n, ld,
                                         pkg._lib.stream_ptr()), "mx_mean_rows_to")
        torch.cuda.synchronize()
        assert not rows[:, P:].view(torch.int32).any().item(), "wrote past the row"
        return rows[:, :P].cpu().numpy()

    _under_policies(pkg, run, want)


def test_store_policy_knob(pkg, O):
    """store_policy is readable, settable and range-checked, listed among the engine's tuning keys, and
    auto at a small size gives the bits of forced nt (the parent's path there)."""
    L = pkg.lib
    E = pkg.engine
    saved = E.mix_tuning()
    assert "store_policy" in saved and saved["store_policy"] == 0
    try:
        for v in (0, 1, 2, 3, 4):
            assert L.mx_mix_set(b"store_policy", v) == 0 and L.mx_mix_get(b"store_policy") == v
        assert L.mx_mix_set(b"store_policy", 5) != 0 and L.mx_mix_set(b"store_policy", -1) != 0
        assert L.mx_mix_get(b"store_policy") == 4
        np.random.seed(1234)
        GP = pkg.MatchaProcessor(pkg.select_graph(0), 0.5, 0, 8, 3, True)
        X0 = np.stack([O.synth(4100 + i, P_SMALL) for i in range(8)])
        want = _oracle_rounds(O, X0, GP.neighbors_info, GP.active_flags, GP.neighbor_weight, 3)
        outs = []
        for v in (0, 1):
            E.set_mix_tuning(store_policy=v)
            outs.append(_u32(_group_rounds(pkg, GP, X0, 3)))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], _u32(want))
    finally:
        E.set_mix_tuning(**saved)
    assert E.mix_tuning() == saved


# ---------------------------------------------------------------- the fused optimizer rounds

FUSED_POLICIES = (1, 2, 3)
ONES = np.ones(8, np.float32)    # clipref's per-row factor: 1.0 * g is g, bit for bit


def _family_policy(pkg, K):
    """(get, put) of the family's store_policy, through its mx_<family>_get / _set"""
    fam = pkg.engine.FAMILIES["adamw" if K.adam else "sgd", K.mixed]

    def put(v):
        assert fam.set(b"store_policy", v) == 0, pkg.lib.mx_last_error()

    return (lambda: int(fam.get(b"store_policy"))), put


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_family(pkg, O, kind, zero):
    """8 rows of graph 0 x 1541, 2 steps (every matching, then the sparsest one), with and without zero_grads:
    x / w, m, v uint32 for uint32 and p uint16 for uint16 against the specification (tests/sgdref.py,
    sgdbf16ref.py, adamref.py, adambf16ref.py through clipref with the exact factor 1.0) under every policy, and
    every policy against nt."""
    K = Kind(kind)
    partner, alpha = _topology(pkg, "g0")
    flags = np.stack([np.ones(partner.shape[0], np.uint8), np.eye(partner.shape[0], dtype=np.uint8)[0]])
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([KINDS.index(kind), int(zero), 41])
    X0 = rng.standard_normal((8, P_SMALL)).astype(np.float32)
    Gs = [K.grads(rng, (8, P_SMALL)) for _ in range(2)]
    get, put = _family_policy(pkg, K)
    assert get() == 0
    want, first = None, None
    try:
        for pol in FUSED_POLICIES:
            put(pol)
            assert get() == pol
            grp = K.group(pkg, topo, P_SMALL, zero, hyper=ADAM_HYPER if K.adam else SGD_HYPER)
            K.put_x(grp, X0)
            s = K.state(grp)
            ref = [] if want is None else want
            outs = []
            for it in range(2):
                K.put_g(grp, Gs[it])
                (grp.adamw_step if K.adam else grp.sgd_step)(it, LR)
                got = K.state(grp)
                if want is None:
                    ref.append(K.spec(O, s, Gs[it], ONES, it + 1, partner, flags[it], alpha, LR))
                for k in ref[it]:
                    assert Kind.same(got, ref[it], [k]), f"{kind} policy {pol} round {it}: {k} differs from the specification"
                if zero:
                    assert not got["g"].view(np.uint16 if K.mixed else np.uint32).any(), f"policy {pol}: g not zeroed"
                else:
                    assert Kind.same(got, {"g": Gs[it]}, ["g"]), f"policy {pol}: g was rewritten"
                s = got
                outs.append(got)
            want = ref
            if first is None:
                first = outs
            for it in range(2):
                assert Kind.same(outs[it], first[it]), f"{kind} policy {pol} round {it}: differs from nt"
            for name in ("arena", "grad_arena", "master_arena", "mom_arena", "exp_avg_arena", "exp_avg_sq_arena"):
                a = getattr(grp, name, None)
                if a is not None:
                    assert not a[:, P_SMALL:].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32).any().item()
            grp.close()
    finally:
        put(0)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_state_pointer_misaligned(pkg, O, kind):
    """The raw C ABI on padded tables, 8 rows x (5 + 1541 columns in two segments): the momentum / exp_avg
    pointer of every odd row is one float off a 16-byte boundary, so those rows take the element path in
    every array beside even rows on the 16-byte path.  Two steps with zero_grads under every policy: the
    specification's bits, nt's bits, every guard word intact."""
    E = pkg.engine
    K = Kind(kind)
    K.hyper = ADAM_HYPER if K.adam else SGD_HYPER
    fam = E.FAMILIES["adamw" if K.adam else "sgd", K.mixed]
    n = 8
    partner, alpha = _topology(pkg, "g0")
    flags = np.stack([np.ones(partner.shape[0], np.uint8), np.eye(partner.shape[0], dtype=np.uint8)[0]])
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    lens = [5, P_SMALL]
    dtypes = {k: np.uint16 if (K.mixed and k in "gp") else np.float32 for k in fam.tables}
    rng = np.random.default_rng([KINDS.index(kind), 43])
    get, put = _family_policy(pkg, K)
    want, first = None, None
    try:
        for pol in FUSED_POLICIES:
            put(pol)
            pt = PaddedTables(n, lens, dtypes, lambda k, s, r: 1 if (k == "m" and r & 1) else 0)
            mp = np.array(pt.ptrs("m"))
            assert (mp[1::2] % 16 == 4).all() and (mp[0::2] % 16 == 0).all()
            tabs = [pt.ptrs(k) for k in fam.tables]
            if K.adam:
                lay = E.FUSED_LAYOUTS["adamw", K.mixed](lens, *tabs, n, _table(K.hyper))
                b1, b2, eps, wd, dec = K.hyper
                call = lay.call(eng, (b1, b2), eps, wd, dec, True)
            else:
                lay = E.FUSED_LAYOUTS["sgd", K.mixed](lens, *tabs, n)
                wd, mom, nest = K.hyper
                call = lay.call(eng, wd, mom, nest, True)
            addr = ctypes.addressof(call)
            P = pt.P
            xk = fam.tables[0]
            if want is None:
                X0 = rng.standard_normal((n, P)).astype(np.float32)
                Gs = [K.grads(rng, (n, P)) for _ in range(2)]
            pt.put(xk, X0)
            for k in fam.tables[2:]:
                pt.put(k, np.zeros((n, P), dtypes[k]))
            s = {"x": pt.get(xk), "m": pt.get("m")}
            if K.adam:
                s["v"] = pt.get("v")
            run = getattr(pkg.lib, fam.base)
            sp = pkg._lib.stream_ptr()
            ref = [] if want is None else want
            outs = []
            for it in range(2):
                pt.put("g", Gs[it])
                rc = run(addr, it, it + 1, LR, None, sp) if K.adam else run(addr, it, LR, None, sp)
                assert rc == 0, pkg.lib.mx_last_error()
                got = {"x": pt.get(xk), "m": pt.get("m")}
                if K.adam:
                    got["v"] = pt.get("v")
                if K.mixed:
                    got["p"] = pt.get("p")
                if want is None:
                    ref.append(K.spec(O, s, Gs[it], ONES, it + 1, partner, flags[it], alpha, LR))
                for k in ref[it]:
                    assert Kind.same(got, ref[it], [k]), f"{kind} policy {pol} round {it}: {k} differs from the specification"
                assert not pt.get("g").view(np.uint16 if K.mixed else np.uint32).any(), f"policy {pol}: g not zeroed"
                for k in fam.tables:
                    assert pt.guards_intact(k), f"policy {pol} round {it}: guard words of {k}"
                s = got
                outs.append(got)
            want = ref
            if first is None:
                first = outs
            for it in range(2):
                assert Kind.same(outs[it], first[it]), f"{kind} policy {pol} round {it}: differs from nt"
    finally:
        put(0)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_knob(pkg, kind):
    """a family's store_policy is readable, settable, independent of mx_mix_set's and refuses values outside
    0..3"""
    K = Kind(kind)
    fam = pkg.engine.FAMILIES["adamw" if K.adam else "sgd", K.mixed]
    get, put = _family_policy(pkg, K)
    assert get() == 0
    try:
        for v in (0, 1, 2, 3):
            assert fam.set(b"store_policy", v) == 0 and fam.get(b"store_policy") == v
            assert int(pkg.lib.mx_mix_get(b"store_policy")) == 0
        assert fam.set(b"store_policy", 4) != 0 and fam.set(b"store_policy", -1) != 0
        assert fam.get(b"store_policy") == 3
    finally:
        put(0)
    assert get() == 0
