"""bfloat16 worker rows through the single-GPU mixing path (csrc/mix_bf16.hip).

Every comparison is against the specification restated in tests/bf16ref.py, never the code under
test: out_bits == rne_bf16(O.decen_round(upcast(X), partner, flags, alpha)) -- uint16 for uint16
for finite values, +-0, subnormals and +-Inf (an fp32 result that overflows when rounded included),
a NaN of any payload where the oracle's fp32 result is a NaN.

Shapes are the smallest at which each path can go wrong: 1-65 columns (the element path, one 16-byte
chunk, a wave's 512-column pass seam), and per slot class one layout tile - 1, one tile, one tile
+ 9 and three tiles + 5 (the vector path, the tail, the tile seam, several work items)."""
import ctypes
import random

import numpy as np
import pytest

from bf16ref import is_nan16, random_bits, rne_bf16, same_bf16, spec_round, upcast
from conftest import Topo, golden_json, golden_npz

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
_TOPOS = {}


def _topology(pkg, name):
    """(partner int32 [M][n], alpha) of the topologies, built once"""
    if name not in _TOPOS:
        if name == "g0":                           # graph 0, 8 workers: the 8-slot class
            gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 2 / 7)
        elif name == "g16":                        # a 16-worker graph of topologies.py: the 16-slot class
            gp = pkg.GraphProcessor(pkg.select_graph(2), 1.0, 0, 16, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 0.2)
        elif name == "er64":                       # ER(64, 0.1, seed 1234): the 64-slot class
            random.seed(0)
            base = pkg.erdos_renyi(64, 0.1, 1234)
            np.random.seed(1234)
            gp = pkg.MatchaProcessor(base, 0.5, 0, 64, 4, False)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), float(gp.neighbor_weight))
        elif name == "ring32":                     # the hand-written ring of tests/test_gpu_adamw_mix_bf16.py:
            even = np.arange(32) ^ 1               # the 32-slot class
            odd = (((np.arange(32) - 1) ^ 1) + 1) % 32
            _TOPOS[name] = (np.stack([even, odd]).astype(np.int32), 0.3125)
        else:                                      # 3 workers by hand: the 8-slot class with unused slots
            # alpha = -2^-8: a worker at the largest finite bf16 with one active partner gets
            # (1 + 2^-8) * max - 2^-8 * x_j, finite in fp32 and past the halfway point to Inf
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
    tile = int(pkg.lib.mx_mix_bf16_tile(n))
    assert tile > 0
    return [1, 7, 8, 9, 63, 64, 65, tile - 1, tile, tile + 9, 3 * tile + 5]


def _put(grp, bits):
    grp.rows.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))


def _get(grp):
    torch.cuda.synchronize()
    return grp.rows.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows):
    partner, alpha = _topology(pkg, name)
    n = partner.shape[1]
    flags = _flag_kinds(partner, 5)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([len(name), len(idle_rows), n])
    for P in _shapes(pkg, n):
        grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows, dtype=BF16)
        assert grp.rows.dtype == BF16 and tuple(grp.rows.shape) == (n, P)
        assert grp.arena.data_ptr() % 128 == 0 and (grp.ld * 2) % 128 == 0
        for kind in range(4):
            X = random_bits(rng, (n, P))
            _put(grp, X)
            for j in range(3):
                it = 3 * kind + j
                ran = grp.step(it)
                got = _get(grp)
                want = spec_round(O, X, partner, flags[it], alpha, idle_rows)
                assert ran == bool(flags[it].any())
                if not flags[it].any():
                    assert np.array_equal(got, X), f"{name} P={P}: an all-zero round wrote"
                assert same_bf16(got, want), f"{name} P={P} round {it}"
                X = got
        assert not grp.arena[:, P:].view(torch.int16).any().item(), f"{name} P={P}: wrote past the row"


def test_rounded_sum_overflows_to_inf(pkg, O):
    """The one rounding can itself overflow: fp32 chain finite, bf16 result Inf."""
    partner, alpha = _topology(pkg, "hand3")
    flags = np.array([[1, 0]], np.uint8)
    P = 9
    X = np.full((3, P), 0x3F80, np.uint16)         # 1.0 everywhere ...
    X[0, :5] = 0x7F7F                              # ... worker 0 (partner: worker 1) at +-max
    X[0, 5:] = 0xFF7F
    chain = O.decen_round(upcast(X), partner, flags[0], alpha)
    assert np.isfinite(chain).all()                # (1 + 2^-8) * max - 2^-8: finite in fp32
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P, dtype=BF16)
    _put(grp, X)
    assert grp.step(0)
    got = _get(grp)
    assert (got[0, :5] == 0x7F80).all() and (got[0, 5:] == 0xFF80).all() and (got[2] == 0x3F80).all()
    assert np.array_equal(got, spec_round(O, X, partner, flags[0], alpha))


@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
def test_idle_rows_negative_zero(pkg, O, idle_rows):
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 1)[3:4]           # the one-matching round
    idle = [i for i in range(8) if partner[flags[0].astype(bool)][0, i] < 0]
    assert idle, "the one-matching round must leave some worker idle"
    P = 2057
    X = random_bits(np.random.default_rng(3), (8, P))
    X[:, ::3] = 0x8000
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=P, idle_rows=idle_rows, dtype=BF16)
    _put(grp, X)
    assert grp.step(0)
    got = _get(grp)
    assert same_bf16(got, spec_round(O, X, partner, flags[0], alpha, idle_rows))
    for i in idle:
        if idle_rows == "skip":
            assert np.array_equal(got[i], X[i])                      # the 16-bit patterns untouched
        else:
            assert (got[i, ::3] == 0).all()                          # -0.0 -> +0.0
            keep = ~is_nan16(X[i]) & (X[i] != 0x8000)
            assert np.array_equal(got[i][keep], X[i][keep])


def _model_bits(models):
    return np.stack([torch.cat([p.detach().reshape(-1) for p in m.parameters()]).view(torch.int16).cpu().numpy()
                     for m in models]).view(np.uint16)


def test_adopted_bf16_models(pkg, O):
    """nn.Modules with bf16 parameters of ragged shapes: identity and shapes kept, storage inside
    the arena row, two rounds equal to the spec."""
    n = 8
    torch.manual_seed(0)
    models = [torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5)).cuda().to(BF16)
              for _ in range(n)]
    ids = [[id(p) for p in m.parameters()] for m in models]
    shapes = [[tuple(p.shape) for p in m.parameters()] for m in models]
    X = _model_bits(models)
    partner, alpha = _topology(pkg, "g0")
    flags = np.array([[1, 1, 1, 1, 1], [1, 0, 0, 1, 0]], np.uint8)[:, :partner.shape[0]]
    grp = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), models, dtype=BF16)
    assert ids == [[id(p) for p in m.parameters()] for m in models]
    assert shapes == [[tuple(p.shape) for p in m.parameters()] for m in models]
    for r, m in enumerate(models):
        lo = grp.arena[r].data_ptr()
        for p in m.parameters():
            assert p.dtype == BF16 and lo <= p.data_ptr() and p.data_ptr() + 2 * p.numel() <= lo + 2 * grp.ld
    assert np.array_equal(_model_bits(models), X)
    for f in flags:
        grp.communicate()
        X = spec_round(O, X, partner, f, alpha)
    torch.cuda.synchronize()
    assert same_bf16(_model_bits(models), X)
    assert models[3](torch.ones(2, 33, device="cuda", dtype=BF16)).shape == (2, 5)   # still a working module


def test_decen_communicator_bf16_model(pkg, O):
    """decenCommunicator(size=1) passes a bf16 CUDA model's dtype through: the parameters are adopted
    into a bf16 row and communicate() mixes them (one worker: every round rewrites 0 + 1.0 * x in
    "canonical" mode, so -0.0 comes out as +0.0 and everything else as it went in)."""
    partner, flags = np.array([[-1]], np.int32), np.array([[1], [1]], np.uint8)
    topo = Topo(partner, 0.25, flags)
    model = torch.nn.Linear(37, 5).cuda().to(BF16)
    with torch.no_grad():
        model.weight.view(-1)[::4] = -0.0
    X = _model_bits([model])
    assert (X == 0x8000).any()
    comm = pkg.decenCommunicator(0, 1, topo, idle_rows="canonical")
    for t in range(2):
        comm.communicate(model)
        X = spec_round(O, X, partner, flags[t], 0.25, "canonical")
    assert comm._group.dtype == BF16 and comm._group.rows.dtype == BF16
    assert model.weight.data_ptr() == comm._group.arena.data_ptr()
    got = _model_bits([model])
    assert same_bf16(got, X) and not (got == 0x8000).any()
    comm.close()


@pytest.mark.parametrize("batched", [False, True])
def test_virtual_trainer_bf16_models(pkg, O, batched):
    """harness.VirtualTrainer with bf16 models: bf16 rows, sync_allreduce leaves every row equal, and
    every communicate() is one bf16 round (by the spec) of the post-step rows."""
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=0.5, graphid=0, lr=0.1, matcha=True)
    factory = H.model_factory(args)
    tr = H.VirtualTrainer(args, lambda: factory().to(BF16), n_batches=3, batched=batched)
    assert tr.group.dtype == BF16 and tr.group.rows.dtype == BF16
    rows0 = _get(tr.group)
    assert all(np.array_equal(rows0[0], rows0[r]) for r in range(8))
    partner = np.asarray(tr.GP.neighbors_info, np.int32)
    state, seen = {}, {"rounds": 0}

    def hook(when, t):
        if when == "before":
            state["X"], state["it"] = _get(t.group).copy(), t.group.iter
            return
        flags = np.asarray(tr.GP.active_flags[state["it"]], np.uint8)
        want = spec_round(O, state["X"], partner[:len(flags)], flags, tr.GP.neighbor_weight)
        assert same_bf16(_get(t.group), want), f"round {state['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats)
    assert seen["rounds"] == 3 and tr.group.iter == 3
    p0 = next(tr.models[3].parameters())
    assert p0.dtype == BF16 and p0.data.data_ptr() >= tr.group.arena.data_ptr()


def _raw_call(pkg, lay, eng, need=None):
    E = pkg.engine
    return E.MixCall(lay._args[0], lay._args[1], lay._args[2], lay._args[3], eng._plan_ptr, lay.total_tiles,
                     lay.nseg, lay.n_slots, eng.n_local, eng.M, eng.alpha32, 0,
                     need.ctypes.data if need is not None else None, len(need) if need is not None else 0)


def test_abi_unaligned_rows(pkg, O):
    """mx_gossip_mix_bf16_packed on row pointers 2 bytes into a larger buffer (never 16-byte
    aligned): exact, and the elements around every row untouched."""
    partner, alpha = _topology(pkg, "g0")
    flags = np.array([[1, 1, 1, 1, 1], [0, 1, 0, 1, 0]], np.uint8)[:, :partner.shape[0]]
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    n, P, stride, off = 8, 1029, 1048, 1
    X = random_bits(np.random.default_rng(11), (n, P))
    host = np.full((n, stride), 0x5A5A, np.uint16)
    host[:, off:off + P] = X
    big = torch.from_numpy(host.view(np.int16)).cuda()
    assert big.data_ptr() % 16 == 0 and (2 * stride) % 16 == 0
    ptrs = [[big[i].data_ptr() + 2 * off] for i in range(n)]
    assert all(p[0] % 16 == 2 for p in ptrs)
    lay = pkg.Layout([P], ptrs, eng.n_slots, dtype=BF16)
    call = _raw_call(pkg, lay, eng)
    for it, f in enumerate(flags):
        assert pkg.lib.mx_gossip_mix_bf16_packed(ctypes.addressof(call), it, pkg._lib.stream_ptr()) == 0
        X = spec_round(O, X, partner, f, alpha)
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint16)
    assert same_bf16(got[:, off:off + P], X)
    assert (got[:, :off] == 0x5A5A).all() and (got[:, off + P:] == 0x5A5A).all()


def test_hint_masks_change_no_bits(pkg, O):
    """need_host masks of 0, all ones and a wrong subset: identical bits (the plan record decides)."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 2)[[3, 6, 9]]       # one matching, every matching, random
    topo = Topo(partner, alpha, flags)
    n, P = 8, 3 * 2048 + 5
    X0 = random_bits(np.random.default_rng(12), (n, P))
    outs = []
    for mask in (None, 0, 0xFF, 0x05, 0xFFFFFFFFFFFFFFFF):
        grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=BF16)
        need = None if mask is None else np.full(len(flags) + 1, mask, np.uint64)
        call = _raw_call(pkg, grp.layout, grp.engine, need)
        _put(grp, X0)
        for it in range(len(flags)):
            assert pkg.lib.mx_gossip_mix_bf16_packed(ctypes.addressof(call), it, pkg._lib.stream_ptr()) == 0
        outs.append(_get(grp))
    X = X0
    for f in flags:
        X = spec_round(O, X, partner, f, alpha)
    assert same_bf16(outs[0], X)
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


@pytest.mark.parametrize("knobs", [{"split": 1}, {"split": 4}, {"nontemporal": 0}, {"nontemporal": 1, "wgpc": 5},
                                   {"grid": 3}, {"grid": 2, "split": 4}])
def test_knobs_change_no_bits(pkg, O, knobs):
    """mx_mix_bf16_set's knobs (work-item width, streaming hints, workgroups-per-CU cap, persistent
    grid -- "grid": 2-3 workgroups looping over the work items, next item's loads in flight) tune
    speed only: every slot class stays exact under each."""
    L = pkg.lib
    saved = {k: int(L.mx_mix_bf16_get(k.encode())) for k in knobs}
    try:
        for k, v in knobs.items():
            assert L.mx_mix_bf16_set(k.encode(), v) == 0
        for name in ("g0", "g16", "ring32", "er64"):
            partner, alpha = _topology(pkg, name)
            n = partner.shape[1]
            flags = _flag_kinds(partner, 6)[[6, 3, 9]]
            topo = Topo(partner, alpha, flags)
            for P in (65, 2047, 3 * 2048 + 5):
                grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=BF16)
                X = random_bits(np.random.default_rng([P, n]), (n, P))
                _put(grp, X)
                for it, f in enumerate(flags):
                    grp.step(it)
                    X = spec_round(O, X, partner, f, alpha)
                assert same_bf16(_get(grp), X), f"{knobs} {name} P={P}"
    finally:
        for k, v in saved.items():
            L.mx_mix_bf16_set(k.encode(), v)


def test_graph_replay_equals_eager_steps(pkg, O):
    """device_round / device_rounds captured once and replayed over 5 iterations == 5 eager steps."""
    partner, alpha = _topology(pkg, "g0")
    flags = _flag_kinds(partner, 4)[[6, 3, 0, 9, 10]]
    topo = Topo(partner, alpha, flags)
    n, P = 8, 2 * 2048 + 77
    X0 = random_bits(np.random.default_rng(13), (n, P))
    eager = pkg.VirtualWorkerGroup(topo, numel=P, dtype=BF16)
    _put(eager, X0)
    X = X0
    for it in range(5):
        eager.step(it)
        X = spec_round(O, X, partner, flags[it], alpha)
    want = _get(eager)
    assert same_bf16(want, X)
    for K in (0, 2):                                 # one device_round per replay; device_rounds(2) + one
        grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=BF16)
        _put(grp, X0)
        grp.iter_dev.fill_(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g):
                if K:
                    grp.device_rounds(K)
                grp.device_round()
        torch.cuda.synchronize()
        assert int(grp.iter_dev.item()) == 0 and np.array_equal(_get(grp), X0)      # capture ran nothing
        for _ in range(5 if K == 0 else 3):          # K = 2: 9 rounds asked, the last 4 past the schedule
            g.replay()
        assert np.array_equal(_get(grp), want)


def test_refusals_launch_nothing(pkg):
    partner, alpha = _topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))
    with pytest.raises(NotImplementedError, match="one GPU"):
        pkg.VirtualWorkerGroup(topo, numel=100, nranks=2, rank=0, dtype=BF16)
    with pytest.raises(NotImplementedError, match="chunk_cols"):
        pkg.VirtualWorkerGroup(topo, numel=100_000, chunk_cols=4096, dtype=BF16)
    with pytest.raises(NotImplementedError, match="fp32-only"):
        pkg.ChocoWorkerGroup(topo, numel=1000, ratio=0.9, consensus_lr=0.2, dtype=BF16)
    mixed = [torch.nn.Linear(4, 3).cuda().to(BF16) for _ in range(8)]
    mixed[5].bias.data = mixed[5].bias.data.float()
    with pytest.raises(TypeError, match="bfloat16"):
        pkg.VirtualWorkerGroup(topo, mixed, dtype=BF16)
    with pytest.raises(TypeError, match="float32"):
        pkg.VirtualWorkerGroup(topo, mixed)          # the fp32 default refuses bf16 parameters as before
    with pytest.raises(TypeError):
        pkg.VirtualWorkerGroup(topo, numel=100, dtype=torch.float16)


def test_fp32_golden_unchanged_after_bf16(pkg, O):
    """A bf16 group first, then the fp32 golden case g0 in the same process: still uint32-exact."""
    partner, alpha = _topology(pkg, "g0")
    flags = np.ones((1, partner.shape[0]), np.uint8)
    grp16 = pkg.VirtualWorkerGroup(Topo(partner, alpha, flags), numel=4099, dtype=BF16)
    X = random_bits(np.random.default_rng(14), (8, 4099), specials=False)
    _put(grp16, X)
    grp16.communicate()
    assert same_bf16(_get(grp16), spec_round(O, X, partner, flags[0], alpha))
    d = golden_npz("decen")
    meta = {m["name"]: m for m in golden_json("decen")}["g0"]
    topo = Topo(d["g0_partner"], meta["alpha"], d["g0_flags"])
    grp = pkg.VirtualWorkerGroup(topo, numel=meta["P"])
    assert grp.rows.dtype == torch.float32
    grp.rows.copy_(torch.from_numpy(d["g0_X0"]))
    for r in range(meta["rounds"]):
        grp.communicate()
        got = grp.rows.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), d["g0_Y"][r].view(np.uint32)), f"round {r}"
