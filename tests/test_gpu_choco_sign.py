"""ChocoSGD with the scaled-sign (1-bit) compressor on the GPU against tests/signref.py: the packed bits
and the padding, the scale within 1 fp32 ulp and identical whatever computes the row, and x / x_hat / s after
every round bit for bit given the scales the device produced -- at the smallest shapes where the kernels can
still go wrong (one element, around one 64-column word, around one 256-column pass, around one 4096-column
tile, several tiles with a partial one, more work items than a small grid has workgroups), from aligned and
unaligned starts."""
import numpy as np
import pytest

import signref
from clipref import ulp_diff
from conftest import LoopbackHub, Topo, special_values

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5, 40_001)
# three workers, each pair matched once
PARTNER3 = [[1, 0, -1], [-1, 2, 1], [2, -1, 0]]

_cache = {}


def _row(seed, P):
    """standard normal, with an exact +0 and -0 planted when there is room (read-only, shared)"""
    if (seed, P) not in _cache:
        x = np.random.default_rng(seed).standard_normal(P).astype(F32)
        if P > 10:
            x[3], x[P - 2] = F32(0.0), F32(-0.0)
        x.setflags(write=False)
        _cache[seed, P] = x
    return _cache[seed, P]


def _spec(key, d):
    """signref.sign_message of d, computed once per key"""
    if ("spec",) + key not in _cache:
        _cache[("spec",) + key] = signref.sign_message(d)
    return _cache[("spec",) + key]


def _padded(bits, P):
    """the whole bits region of a slot: 8 ceil(P / 64) bytes, zeros after the message's"""
    out = np.zeros(8 * ((P + 63) // 64), np.uint8)
    out[:bits.size] = bits
    return out


class _knobs:
    def __init__(self, pkg, **knobs):
        self.pkg, self.knobs = pkg, knobs

    def __enter__(self):
        L = self.pkg.lib
        self.saved = {k: int(L.mx_choco_sign_get(k.encode())) for k in self.knobs}
        for k, v in self.knobs.items():
            self.pkg._lib.check(L.mx_choco_sign_set(k.encode(), v))

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.pkg.lib.mx_choco_sign_set(k.encode(), v)


def _slot(grp, slot):
    """(scale float32, L float64, P int64, the rest of the header, the whole bits region) of a message slot"""
    torch.cuda.synchronize()
    raw = grp.msgs[slot * grp.msg_ld:slot * grp.msg_ld + grp.msg_bytes].cpu().numpy()
    return (raw[:4].view(F32)[0], raw[8:16].view(np.float64)[0], raw[16:24].view(np.int64)[0],
            np.concatenate([raw[4:8], raw[24:64]]), raw[64:])


def _scales(grp):
    return np.array([_slot(grp, r)[0] for r in range(grp.n_local)], F32)


def _state(grp):
    P = grp.numel
    return grp.rows.cpu().numpy(), grp.x_hat[:, :P].cpu().numpy(), grp.s[:, :P].cpu().numpy()


def _assert_state(grp, X, XH, S, what, same=None):
    same = same or (lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    gx, gh, gs = _state(grp)
    assert same(gh, XH), f"x_hat {what}"
    assert same(gs, S), f"s {what}"
    assert same(gx, X), f"x {what}"


def _check_message(grp, r, d, key, P):
    """slot r of grp holds the message of d: header, bits with their padding, scale within 1 ulp; its scale"""
    want_scale, want_bits = _spec(key, d)
    scale, L, Ph, rest, bits = _slot(grp, r)
    assert np.array_equal(bits, _padded(want_bits, P)), (key, r)
    assert int(ulp_diff(scale, want_scale)) <= 1, (key, r, scale, want_scale)
    assert Ph == P and not rest.any() and F32(L / np.float64(P)) == scale, (key, r)
    ms, mb = grp.message(r)
    assert ms.dim() == 0 and ms.dtype == torch.float32 and mb.dtype == torch.uint8 and mb.numel() == (P + 7) // 8
    assert ms.cpu().numpy().view(np.uint32) == scale.view(np.uint32)
    assert np.array_equal(mb.cpu().numpy(), want_bits)
    return scale


@pytest.mark.parametrize("P", SIZES)
def test_compress_small_shapes(pkg, P):
    """get_scaled_sign from an aligned and an unaligned start, a 1-row group and a 3-row group (x_hat zero
    and nonzero) under every compress-knob value: bits, padding, header, scale within 1 ulp of the spec --
    and the SAME scale bits for the same row wherever and however it is computed."""
    x = _row(100, P)
    want_scale, want_bits = _spec((100, P), x)
    big = torch.zeros(P + 8, dtype=torch.float32, device="cuda")
    seen = set()
    for off in (4, 5):                               # the allocation is 256-byte aligned
        xv = big[off:off + P]
        xv.copy_(torch.tensor(x))
        assert (xv.data_ptr() % 16 == 0) == (off == 4)
        scale, bits = pkg.get_scaled_sign(xv)
        assert scale.dim() == 0 and scale.dtype == torch.float32 and bits.dtype == torch.uint8
        assert np.array_equal(bits.cpu().numpy(), want_bits), off
        sc = scale.cpu().numpy()
        assert int(ulp_diff(sc, want_scale)) <= 1, (off, sc, want_scale)
        seen.add(int(sc.view(np.uint32)))
        dense = pkg.unpack_scaled_sign(scale, bits, P).cpu().numpy()
        assert np.array_equal(dense.view(np.uint32), signref.dense(sc, signref.unpack(want_bits, P)).view(np.uint32))
    hs, hb = pkg.get_scaled_sign(torch.tensor(x))             # CPU input: staged, returned on the CPU
    assert hs.device.type == "cpu" and hb.device.type == "cpu" and np.array_equal(hb.numpy(), want_bits)
    seen.add(int(hs.numpy().view(np.uint32)))

    topo = Topo(PARTNER3, 1 / 3, np.ones((1, 3), np.uint8))
    one = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1, rank=0, nranks=3,
                               comm=LoopbackHub(3).comm(0))
    assert one.n_local == 1 and one.k == 0 and one.msg_bytes == signref.msg_bytes(P) and one.msg_ld % 256 == 0
    one.rows[0].copy_(torch.tensor(x))
    one.compress(0)
    one.check_topk()                                              # a no-op
    seen.add(int(_check_message(one, 0, x, (100, P), P).view(np.uint32)))

    grp = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    assert grp.n_local == 3
    X = np.stack([_row(101, P), _row(102, P), x])                 # row 2 is the row above
    grp.rows.copy_(torch.from_numpy(X))
    for knobs in ({}, {"grid": 1}, {"grid": 3}, {"blocks_per_cu": 1}, {"blocks_per_cu": 64}, {"apply_nt": 0},
                  {"apply_nt": 1}):
        with _knobs(pkg, **knobs):
            grp.msgs.fill_(0xAB)                                   # every byte of a slot is written again
            grp.compress(0)
            for r, seed in enumerate((101, 102, 100)):
                sc = _check_message(grp, r, X[r], (seed, P), P)
                if r == 2:
                    seen.add(int(sc.view(np.uint32)))
    assert len(seen) == 1, seen                                   # one row, one scale, bit for bit
    XH = np.stack([F32(0.5) * _row(200 + r, P) for r in range(3)])
    grp.x_hat[:, :P].copy_(torch.from_numpy(XH))
    grp.compress(0)
    for r in range(3):
        _check_message(grp, r, (X[r] - XH[r]).astype(F32), ("hat", r, P), P)


FLAGS3 = np.array([[1, 1, 1], [1, 0, 1], [1, 0, 0], [0, 0, 0]], np.uint8)


def _run_rounds(pkg, topo, flags, P, n, alpha, gamma, seed, same=None, X0=None):
    """communicate() over the schedule with the rows perturbed between rounds; after every round the state
    equals signref.sign_round given the device's scales (themselves within 1 ulp of the spec's)"""
    grp = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=gamma)
    X = np.stack([_row(seed + i, P) for i in range(n)]).copy() if X0 is None else X0.copy()
    XH, S = np.zeros_like(X), np.zeros_like(X)
    grp.rows.copy_(torch.from_numpy(X))
    for t, f in enumerate(flags):
        if t:
            D = np.stack([F32(0.01) * _row(seed + 50 + i, P) for i in range(n)])
            X = (X + D).astype(F32)
            grp.rows.add_(torch.from_numpy(D).cuda())
        assert grp.iter == t
        grp.communicate()
        if f.any():
            dev = _scales(grp)
            with np.errstate(all="ignore"):
                spec = np.array([signref.sign_message((X[i] - XH[i]).astype(F32))[0] for i in range(n)], F32)
            fin = np.isfinite(spec)
            assert np.array_equal(np.isnan(dev), np.isnan(spec)) and np.array_equal(np.isinf(dev), np.isinf(spec))
            assert (ulp_diff(dev[fin], spec[fin]) <= 1).all(), (t, dev, spec)
            signref.sign_round(X, XH, S, topo.neighbors_info, f, alpha, gamma, scale=dev)
        _assert_state(grp, X, XH, S, f"round {t}", same)          # an all-zero round: untouched
    return grp


@pytest.mark.parametrize("apply_nt", [0, 1])
@pytest.mark.parametrize("P", [1, 65, 3 * 4096 + 5])
def test_apply_small_shapes(pkg, P, apply_nt):
    """Four rounds of a 3-row group -- all matchings, two, one (a row of degree 0 inside an active round),
    none (communicate() leaves the state untouched) -- over whole tiles and a 5-element one, one element,
    and one word plus a column, under both access-hint values."""
    topo = Topo(PARTNER3, 1 / 3, FLAGS3)
    with _knobs(pkg, apply_nt=apply_nt):
        _run_rounds(pkg, topo, FLAGS3, P, 3, 1 / 3, 0.1, 300)


def test_apply_eight_workers(pkg):
    """graph 0's matchings on 8 workers: several partners per row, more than 3 slots, tiles of rows whose
    stride is not the row length"""
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
    flags = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 1, 1, 1, 0]], np.uint8)
    topo = Topo(gp.neighbors_info, 2 / 7, flags)
    grp = _run_rounds(pkg, topo, flags, 4096 + 77, 8, 2 / 7, 0.3, 400)
    assert grp.engine.n_slots >= 8


def test_average_without_active_matching_applies_the_own_message(pkg):
    """average() called directly on a round with no active matching: every row's own message, self weight 1"""
    P = 4097
    topo = Topo(PARTNER3, 1 / 3, np.zeros((1, 3), np.uint8))
    grp = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    X = np.stack([_row(500 + i, P) for i in range(3)]).copy()
    XH, S = np.zeros_like(X), np.zeros_like(X)
    grp.rows.copy_(torch.from_numpy(X))
    assert grp.step(0) is False
    _assert_state(grp, X, XH, S, "skipped")
    grp.compress(0)
    grp.average(0)
    signref.sign_round(X, XH, S, PARTNER3, [0, 0, 0], 1 / 3, 0.1, scale=_scales(grp))
    _assert_state(grp, X, XH, S, "own message only")
    assert np.abs(XH).min() > 0


def test_special_values(pkg):
    """Rows with NaN, +-Inf, +-0, denormals and +-FLT_MAX: the bits are d < 0 (false for NaN and both zeros),
    the scale is NaN (a NaN in the row), Inf (an Inf, no NaN) or finite exactly as the spec's, and the state
    after a round holds NaN / Inf exactly where the spec puts them, everything else equal as uint32."""
    P = 4096 + 9
    X = np.stack([special_values(P, 7), special_values(P, 8, n_nan=0), _row(600, P)])
    with np.errstate(all="ignore"):
        spec = [signref.sign_message(X[i]) for i in range(3)]
    assert np.isnan(spec[0][0]) and np.isinf(spec[1][0]) and np.isfinite(spec[2][0])
    topo = Topo(PARTNER3, 1 / 3, np.ones((1, 3), np.uint8))
    grp = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    grp.rows.copy_(torch.from_numpy(X))
    grp.compress(0)
    for i in range(3):
        scale, _, _, _, bits = _slot(grp, i)
        assert np.array_equal(bits, _padded(spec[i][1], P)), i
        assert np.isnan(scale) == np.isnan(spec[i][0]) and np.isinf(scale) == np.isinf(spec[i][0]), i
    s0, b0 = pkg.get_scaled_sign(torch.from_numpy(X[1]).cuda())
    assert np.isinf(s0.cpu().numpy()) and np.array_equal(b0.cpu().numpy(), spec[1][1])
    _run_rounds(pkg, topo, np.ones((1, 3), np.uint8), P, 3, 1 / 3, 0.1, 0, same=signref.same_bits, X0=X)

    zero = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    zero.communicate()
    assert (_scales(zero).view(np.uint32) == 0).all()
    for a in _state(zero):
        assert not a.view(np.uint32).any()                        # all +0


def test_device_round_graph_replay(pkg):
    """device_round captured once and replayed over a 4-round schedule with an all-zero round: the state of
    the same rounds through step(), bit for bit; past the schedule a replay changes nothing."""
    P = 3 * 4096 + 5
    flags = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 0]], np.uint8)
    topo = Topo(PARTNER3, 1 / 3, flags)
    a = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    b = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    X = np.stack([_row(700 + i, P) for i in range(3)])
    for g in (a, b):
        g.rows.copy_(torch.from_numpy(X))
    a.iter_dev.fill_(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            a.device_round()
    torch.cuda.synchronize()
    assert int(a.iter_dev.item()) == 0 and np.array_equal(a.rows.cpu().numpy(), X)     # capture ran nothing
    for t in range(len(flags) + 2):
        graph.replay()
        if t < len(flags):
            assert b.step(t) == bool(flags[t].any())
        torch.cuda.synchronize()
        _assert_state(a, *_state(b), f"replay {t}")
    assert int(a.iter_dev.item()) == len(flags) + 2
    assert not np.array_equal(a.rows.cpu().numpy(), X)


@pytest.mark.parametrize("nranks", [2, 4])
def test_multirank_loopback(pkg, nranks):
    """8 workers over N simulated ranks: every rank compresses, the byte-generic exchange moves the
    partners' slots (loopback transport, native exchange order), every rank averages; 3 rounds bit-exact
    given the scales in the groups' slot headers."""
    n, P = 8, 9_001
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, n, 4, True)
    flags = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 1, 1, 1, 0]], np.uint8)
    topo = Topo(gp.neighbors_info, 2 / 7, flags)
    hub = LoopbackHub(nranks)
    groups = [pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.3, rank=r, nranks=nranks,
                                   comm=hub.comm(r)) for r in range(nranks)]
    X = np.stack([_row(800 + i, P) for i in range(n)]).copy()
    XH, S = np.zeros_like(X), np.zeros_like(X)
    for g in groups:
        g.rows.copy_(torch.from_numpy(X[g.row_base:g.row_base + g.n_local]))
    for t, f in enumerate(flags):
        if t:
            D = np.stack([F32(0.02) * _row(850 + 10 * t + i, P) for i in range(n)])
            X = (X + D).astype(F32)
            for g in groups:
                g.rows.add_(torch.from_numpy(D[g.row_base:g.row_base + g.n_local]).cuda())
        for g in groups:
            g.compress(t)
            hub.register(g.row_base, [g.msgs.data_ptr() + r * g.msg_ld for r in range(g.n_local)])
        dev = np.concatenate([_scales(g) for g in groups])
        for g in groups:
            g.average(t)
        torch.cuda.synchronize()
        spec = np.array([signref.sign_message((X[i] - XH[i]).astype(F32))[0] for i in range(n)], F32)
        assert (ulp_diff(dev, spec) <= 1).all(), t
        signref.sign_round(X, XH, S, topo.neighbors_info, f, 2 / 7, 0.3, scale=dev)
        for name, want in (("rows", X), ("x_hat", XH), ("s", S)):
            got = np.concatenate([(g.rows if name == "rows" else getattr(g, name)[:, :P]).cpu().numpy() for g in groups])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name} round {t}"


def test_communicator_substeps_on_a_loopback_pair(pkg):
    """ChocoCommunicator(compressor="sign") on two ranks over the loopback transport: prepare_comm_buffer
    exposes `compressed` = {"scale", "bits"}, averaging runs the round, x_hat and s persist."""
    P = 1000
    topo = Topo([[1, 0]], 0.5, np.ones((2, 1), np.uint8))
    hub = LoopbackHub(2)
    comms = [pkg.ChocoCommunicator(r, 2, topo, None, 0.2, transport=hub.comm(r), compressor="sign") for r in range(2)]
    X = np.stack([_row(900 + r, P) for r in range(2)]).copy()
    XH, S = np.zeros_like(X), np.zeros_like(X)
    tensors = [torch.from_numpy(X[r]).cuda() for r in range(2)]
    for t in range(2):
        dev = np.zeros(2, F32)
        for r in range(2):
            comms[r].tensor_list = [tensors[r]]
            assert comms[r].prepare_comm_buffer() >= 0
            c = comms[r].compressed
            assert set(c) == {"scale", "bits"}
            want_scale, want_bits = signref.sign_message((X[r] - XH[r]).astype(F32))
            assert np.array_equal(c["bits"].cpu().numpy(), want_bits)
            dev[r] = c["scale"].cpu().numpy()
            assert int(ulp_diff(dev[r], want_scale)) <= 1
            hub.register(r, [comms[r]._group.msgs.data_ptr()])
        hub.snap.clear()
        for r in range(2):
            assert comms[r].averaging([1]) >= 0
            comms[r].reset_model()
        signref.sign_round(X, XH, S, [[1, 0]], [1], 0.5, 0.2, scale=dev)
        for r in range(2):
            assert np.array_equal(tensors[r].cpu().numpy().view(np.uint32), X[r].view(np.uint32)), (t, r)
            assert np.array_equal(comms[r].x_hat.cpu().numpy().view(np.uint32), XH[r].view(np.uint32)), (t, r)
            assert np.array_equal(comms[r].s.cpu().numpy().view(np.uint32), S[r].view(np.uint32)), (t, r)


def test_constructor_refusals_and_checkpoints(pkg):
    topo = Topo(PARTNER3, 1 / 3, np.ones((2, 3), np.uint8))
    with pytest.raises(ValueError, match="ratio"):
        pkg.ChocoWorkerGroup(topo, numel=100, compressor="sign", ratio=0.9, consensus_lr=0.1)
    with pytest.raises(ValueError, match="ratio"):
        pkg.ChocoWorkerGroup(topo, numel=100, consensus_lr=0.1)
    with pytest.raises(ValueError, match="compressor"):
        pkg.ChocoWorkerGroup(topo, numel=100, compressor="qsgd", consensus_lr=0.1)
    pull = object.__new__(pkg.PullTransport)                     # only its type is looked at
    with pytest.raises(NotImplementedError, match="PullTransport"):
        pkg.ChocoWorkerGroup(topo, numel=100, compressor="sign", consensus_lr=0.1, nranks=3, comm=pull)
    P = 777
    a = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    a.rows.copy_(torch.from_numpy(np.stack([_row(950 + i, P) for i in range(3)])))
    a.communicate()
    sd = a.state_dict()
    assert sd["compressor"] == "sign" and sd["k"] == 0 and sd["iter"] == 1
    b = pkg.ChocoWorkerGroup(topo, numel=P, compressor="sign", consensus_lr=0.1)
    b.load_state_dict(sd)
    a.communicate()
    b.communicate()
    _assert_state(b, *_state(a), "resumed")
    top = pkg.ChocoWorkerGroup(topo, numel=P, ratio=0.9, consensus_lr=0.1)
    assert "compressor" not in top.state_dict()
    with pytest.raises(ValueError, match="does not match"):
        top.load_state_dict(sd)
    with pytest.raises(ValueError, match="does not match"):
        b.load_state_dict(top.state_dict())


def test_virtual_trainer_runs_with_the_sign_compressor(pkg):
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=1.0, graphid=0, lr=0.1, compress=True, compressor="sign")
    tr = H.VirtualTrainer(args, H.model_factory(args), n_batches=2)
    assert tr.group.compressor == "sign" and tr.group.k == 0
    stats = tr.train_epoch()
    assert len(stats) == 8 and tr.group.iter == 2
    assert float(tr.group.x_hat.abs().max()) > 0 and bool(torch.isfinite(tr.group.rows).all())
    assert "compressor" not in str(H.HarnessArgs(compress=True))          # the logged argument line of top-k runs
