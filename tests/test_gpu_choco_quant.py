"""compressor="quant" on the GPU against tests/quantref.py: slots and state exact given the norms, those within 1 ulp"""
import contextlib

import numpy as np
import pytest

import quantref
import signref
from clipref import ulp_diff
from conftest import Topo
from sgdref import sgd_ref
from test_gpu_choco_sign import PARTNER3, _assert_state, _row, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, U32, SEED = np.float32, np.uint32, 77
BITS = pytest.mark.parametrize("bits", [4, 8])
FLAGS3 = np.array([[1, 1, 1], [1, 0, 1], [1, 0, 0]], np.uint8)
FLAGS4 = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 0]], np.uint8)


@contextlib.contextmanager
def _knob(pkg, key, value):
    old = pkg.lib.mx_choco_quant_get(key.encode())
    pkg._lib.check(pkg.lib.mx_choco_quant_set(key.encode(), value))
    try:
        yield
    finally:
        pkg.lib.mx_choco_quant_set(key.encode(), old)


def _group(pkg, flags, P, bits, partner=PARTNER3, alpha=1 / 3, gamma=0.1, seed=SEED, rows=None):
    grp = pkg.ChocoWorkerGroup(Topo(partner, alpha, flags), numel=P, compressor="quant", bits=bits, seed=seed,
                               consensus_lr=gamma)
    if rows is not None:
        grp.rows.copy_(torch.from_numpy(rows))
    return grp


def _rows(seed, n, P):
    return np.stack([_row(seed + i, P) for i in range(n)]).copy()


def _slots(grp):
    torch.cuda.synchronize()
    return grp.msgs.view(-1, grp.msg_ld)[:grp.n_local, :grp.msg_bytes].cpu().numpy()


def _check_slots(raw, D, bits, rnd):
    # norms within 1 ulp of the spec's (NaN and Inf alike), every slot byte exact given them; returns the norms
    n, P = D.shape
    dev = raw[:, 64:64 + 4 * ((P + 255) // 256)].copy().view(F32)
    for i in range(n):
        spec = quantref.quantize(D[i], bits, SEED, rnd, i)[0]
        fin = np.isfinite(spec)
        assert np.array_equal(np.isnan(dev[i]), np.isnan(spec)) and np.array_equal(np.isinf(dev[i]), np.isinf(spec))
        assert (ulp_diff(dev[i][fin], spec[fin]) <= 1).all(), (i, dev[i], spec)
        norm, code, _ = quantref.quantize(D[i], bits, SEED, rnd, i, norm=dev[i])
        assert np.array_equal(raw[i], quantref.slot(P, bits, norm, code)), (rnd, i)
    return dev


@BITS
@pytest.mark.parametrize("P", [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5])
def test_compress_any_grid_and_alignment(pkg, bits, P):
    X, XH = _rows(101, 3, P), F32(0.5) * _rows(200, 3, P)
    grp = _group(pkg, np.ones((1, 3), np.uint8), P, bits, rows=X)
    assert grp.k == 0 and grp.msg_bytes == quantref.msg_bytes(P, bits) and grp.work.numel() == 0
    grp.x_hat[:, :P].copy_(torch.from_numpy(XH))
    D = (X - XH).astype(F32)
    images = []
    for grid in (0, 1, 3):
        with _knob(pkg, "grid", grid):
            grp.msgs.fill_(0xAB)                                   # every byte of a slot is written again
            grp.compress(5)
            images.append(_slots(grp))
    assert np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2])
    dev = _check_slots(images[0], D, bits, 5)
    norms, codes = grp.message(2)
    big = torch.zeros(P + 8, dtype=torch.float32, device="cuda")
    for off in (4, 5):                                             # the allocation is 256-byte aligned
        xv = big[off:off + P]
        xv.copy_(torch.from_numpy(D[2]))
        assert (xv.data_ptr() % 16 == 0) == (off == 4)
        n, c = pkg.get_quantized(xv, bits=bits, seed=SEED, round=5, row=2)
        assert torch.equal(n.view(torch.int32), norms.view(torch.int32)) and torch.equal(c, codes), off
        dense = pkg.unpack_quantized(n, c, P, bits).cpu().numpy()
        assert np.array_equal(dense.view(U32), quantref.quantize(D[2], bits, SEED, 5, 2, norm=dev[2])[2].view(U32))


def _run_rounds(grp, X, flags, bits, same=None):
    topo, (n, P) = grp.topology, X.shape
    XH, S = np.zeros_like(X), np.zeros_like(X)
    for t, f in enumerate(flags):
        if t:
            D = F32(0.01) * _rows(350, n, P)
            X = (X + D).astype(F32)
            grp.rows.add_(torch.from_numpy(D).cuda())
        grp.communicate()
        with np.errstate(all="ignore"):
            dev = _check_slots(_slots(grp), (X - XH).astype(F32), bits, t)
        quantref.quant_round(X, XH, S, topo.neighbors_info, f, topo.neighbor_weight, grp.consensus_lr, bits, SEED, t,
                             norm=dev)
        _assert_state(grp, X, XH, S, f"round {t}", same)


@BITS
@pytest.mark.parametrize("apply_nt", [0, 1])
@pytest.mark.parametrize("P", [65, 3 * 4096 + 5])
def test_rounds(pkg, bits, P, apply_nt):
    # three rounds of 3 rows (all matchings, two, one: a row of degree 0), then one of graph 0 on 8 workers
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
    all8 = np.ones((1, len(gp.neighbors_info)), np.uint8)
    with _knob(pkg, "apply_nt", apply_nt):
        X = _rows(300, 3, P)
        _run_rounds(_group(pkg, FLAGS3, P, bits, rows=X), X, FLAGS3, bits)
        X = _rows(300, 8, P)
        grp = _group(pkg, all8, P, bits, gp.neighbors_info, 2 / 7, 0.3, rows=X)
        _run_rounds(grp, X, all8, bits)


@BITS
def test_special_values(pkg, bits):
    """a zero bucket; a NaN in bucket 2 of row 1 (NaN there and in its partner row 0, nowhere else); the clamp bucket"""
    P = 4096 + 300
    X = _rows(600, 3, P)
    X[0, :256], X[1, 700], X[2, 256:300], X[2, 300], X[2, 301:512] = 0, np.nan, 0, -3.0, 0
    flags = np.array([[1, 0, 0]], np.uint8)                         # workers 0 and 1 matched, 2 alone
    grp = _group(pkg, flags, P, bits, rows=X)
    _run_rounds(grp, X.copy(), flags, bits, same=signref.same_bits)
    want = (np.arange(3)[:, None] < 2) & (np.arange(P) // 256 == 2)
    (x, xh, s), raw = _state(grp), _slots(grp)
    assert np.array_equal(np.isnan(x), want) and np.array_equal(np.isnan(s), want)
    assert not raw[0, 64:68].any() and not xh[0, :256].view(U32).any()
    assert quantref.unpack(raw[2, grp.codes_off:], bits)[300] == (1 << bits) - 1


@BITS
def test_device_round_graph_replay_equals_communicate(pkg, bits):
    P = 3 * 4096 + 5
    X = _rows(700, 3, P)
    a, b = _group(pkg, FLAGS4, P, bits, rows=X), _group(pkg, FLAGS4, P, bits, rows=X)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(torch.cuda.Stream()):
        with torch.cuda.graph(graph):
            a.device_round()
    for t in range(len(FLAGS4) + 2):
        graph.replay()
        if t < len(FLAGS4):
            b.communicate()
        torch.cuda.synchronize()
        _assert_state(a, *_state(b), f"replay {t}")
    assert int(a.iter_dev.item()) == len(FLAGS4) + 2 and not np.array_equal(a.rows.cpu().numpy(), X)


def test_constructor_refusals_and_checkpoints(pkg):
    flags, P = np.ones((2, 3), np.uint8), 777
    pull = object.__new__(pkg.PullTransport)                     # only its type is looked at
    quant = dict(compressor="quant")
    for kw, match in ((dict(quant, ratio=0.9), "ratio"), (dict(quant, bits=5), "bits"), (dict(ratio=0.9, bits=4), "bits"),
                      (dict(compressor="sign", bits=8), "bits"), (dict(quant, nranks=3, comm=pull), "PullTransport")):
        with pytest.raises(NotImplementedError if "comm" in kw else ValueError, match=match):
            pkg.ChocoWorkerGroup(Topo(PARTNER3, 1 / 3, flags), numel=100, consensus_lr=0.1, **kw)
    a = _group(pkg, flags, P, 4, rows=_rows(950, 3, P))
    a.communicate()
    sd = a.state_dict()
    assert (sd["compressor"], sd["bits"], sd["seed"], sd["k"], sd["iter"]) == ("quant", 4, SEED, 0, 1)
    b = _group(pkg, flags, P, 4, seed=0)
    b.load_state_dict(sd)                                          # the checkpoint's seed comes with it
    a.communicate()
    b.communicate()
    _assert_state(b, *_state(a), "resumed")
    sign = pkg.ChocoWorkerGroup(a.topology, numel=P, compressor="sign", consensus_lr=0.1)
    for other in (_group(pkg, flags, P, 8), sign, pkg.ChocoWorkerGroup(a.topology, numel=P, ratio=0.9, consensus_lr=0.1)):
        with pytest.raises(ValueError, match="does not match"):
            other.load_state_dict(sd)


@BITS
def test_sgd_step_is_the_step_then_the_round(pkg, bits):
    P, lr, flags = 4096 + 77, 0.05, np.ones((2, 3), np.uint8)
    X = _rows(800, 3, P)
    grp = _group(pkg, flags, P, bits, rows=X)
    grp.attach_sgd(momentum=0.9)
    M, XH, S = np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)
    for t in range(2):
        G = _rows(850 + 3 * t, 3, P)
        grp.grads.copy_(torch.from_numpy(G))
        assert grp.sgd_step(t, lr) is True
        X, M = (np.array(v) for v in sgd_ref(X, G, M, lr, 0.0, 0.9, False))
        dev = _check_slots(_slots(grp), (X - XH).astype(F32), bits, t)
        quantref.quant_round(X, XH, S, PARTNER3, flags[t], 1 / 3, 0.1, bits, SEED, t, norm=dev)
        _assert_state(grp, X, XH, S, f"round {t}")
        assert np.array_equal(grp.momentum_rows.cpu().numpy().view(U32), M.view(U32)) and not grp.grads.any()
