"""compressor="randk" on the GPU against the selection rule of DESIGN.md (numpy, below): messages, rounds and graph
replays bit for bit, the coverage of fixed seeds, refusals and checkpoints"""
import numpy as np
import pytest

from conftest import Topo
from quantref import mix32
from sgdref import fmaf32
from test_gpu_choco_sign import PARTNER3, _assert_state, _row, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, U32, SEED = np.float32, np.uint32, 77
FLAGS4 = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 0]], np.uint8)


def select(P, k, seed, rnd, worker):
    """(idx int64[k] ascending, bnd int32[T + 1]) of one worker's message"""
    T = (P + 4095) // 4096
    rk = int(mix32(mix32(mix32(seed & 0xffffffff) ^ U32(rnd & 0xffffffff)) ^ U32(worker)))
    o = (int(mix32(rk ^ 0xA5A5A5A5)) * P) >> 32
    bnd = [(k * min(4096 * t, P) + o) // P for t in range(T + 1)]
    idx = []
    for t in range(T):
        j = np.arange(min(4096, P - 4096 * t), dtype=U32)
        with np.errstate(over="ignore"):
            v = (mix32(mix32(rk ^ (t + 1)) + j) & U32(0xFFFFF000)) | j          # unique within the tile
        idx.append(4096 * t + np.sort(np.argsort(v)[:bnd[t + 1] - bnd[t]]))
    return np.concatenate(idx).astype(np.int64), np.array(bnd, np.int32)


def randk_round(X, XH, S, partner, flags, alpha, gamma, k, seed, rnd):
    """One round on float32 [n, P] arrays IN PLACE (quantref.quant_round's contract): the oracle's Choco round with
    the rand-k columns in top-k's place"""
    n, P = X.shape
    partner, a32, g32 = np.asarray(partner, np.int64), F32(alpha), F32(gamma)
    D = (X - XH).astype(F32)
    sel = [select(P, k, seed, rnd, i)[0] for i in range(n)]
    for i in range(n):
        act = [int(partner[m, i]) for m in range(partner.shape[0]) if flags[m] and partner[m, i] >= 0]
        for j in act:
            S[i, sel[j]] = (S[i, sel[j]] + (a32 * D[j, sel[j]]).astype(F32)).astype(F32)
        sw = F32(1.0 - float(len(act)) * float(alpha))
        S[i, sel[i]] = (S[i, sel[i]] + (sw * D[i, sel[i]]).astype(F32)).astype(F32)
        XH[i, sel[i]] = (XH[i, sel[i]] + D[i, sel[i]]).astype(F32)
        X[i] = fmaf32(-g32, XH[i], fmaf32(g32, S[i], X[i]))


def _rows(seed, n, P):
    return np.stack([_row(seed + i, P) for i in range(n)]).copy()


def _group(pkg, flags, P, ratio, seed=SEED, rows=None, **kw):
    grp = pkg.ChocoWorkerGroup(Topo(PARTNER3, 1 / 3, flags), numel=P, compressor="randk", ratio=ratio, seed=seed,
                               consensus_lr=0.1, **kw)
    if rows is not None:
        grp.rows.copy_(torch.from_numpy(rows))
    return grp


@pytest.mark.parametrize("ratio", [1.0, 0.99, 0.5, 0.0])
@pytest.mark.parametrize("P", [1, 4095, 4096, 4097, 3 * 4096 + 5, 40_001])
def test_messages(pkg, P, ratio):
    X, XH = _rows(101, 3, P), F32(0.5) * _rows(200, 3, P)
    grp = _group(pkg, np.ones((1, 3), np.uint8), P, ratio, rows=X)
    grp.x_hat[:, :P].copy_(torch.from_numpy(XH))
    k = grp.k
    assert k == pkg.topk_count(P, ratio) and grp.work.numel() == 0
    assert grp.msg_bytes == pkg.lib.mx_choco_msg_bytes(P, k)
    for rnd in (0, 5):
        grp.msgs.fill_(0xAB)                                       # every byte of a slot is written again
        grp.compress(rnd)
        grp.check_topk()
        raw = grp.msgs.view(-1, grp.msg_ld)[:3, :grp.msg_bytes].cpu().numpy()
        for r in range(3):
            idx, bnd = select(P, k, SEED, rnd, r)
            assert bnd[0] == 0 and bnd[-1] == k == idx.size
            vals, got = (v.cpu().numpy() for v in grp.message(r))
            assert np.array_equal(got, idx), (rnd, r)
            assert np.array_equal(vals.view(U32), (X[r, idx] - XH[r, idx]).astype(F32).view(U32)), (rnd, r)
            assert np.array_equal(raw[r, grp.bnd_off:].view(np.int32), bnd), (rnd, r)
            assert not raw[r, 4 * k:4 * grp.kpad].any()            # the pad element of an odd k is +0


@pytest.mark.parametrize("ratio", [0.99, 0.5])
@pytest.mark.parametrize("P", [4097, 3 * 4096 + 5])
def test_rounds_and_graph_replay(pkg, P, ratio):
    """communicate() against the numpy round, and device_round() replayed from a graph against communicate()"""
    X = _rows(700, 3, P)
    a, b = _group(pkg, FLAGS4, P, ratio, rows=X), _group(pkg, FLAGS4, P, ratio, rows=X)
    XH, S = np.zeros_like(X), np.zeros_like(X)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(torch.cuda.Stream()):
        with torch.cuda.graph(graph):
            a.device_round()
    for t in range(len(FLAGS4) + 2):
        graph.replay()
        if t < len(FLAGS4):
            b.communicate()
            if FLAGS4[t].any():
                randk_round(X, XH, S, PARTNER3, FLAGS4[t], 1 / 3, 0.1, b.k, SEED, t)
            _assert_state(b, X, XH, S, f"round {t}")
        torch.cuda.synchronize()
        _assert_state(a, *_state(b), f"replay {t}")
    assert int(a.iter_dev.item()) == len(FLAGS4) + 2 and XH.any()


@pytest.mark.parametrize("P, ratio, worker, rounds", [(2 * 4096 + 5, 0.5, 1, 400), (40_001, 1.0, 0, 200)])
def test_coverage(pkg, P, ratio, worker, rounds):
    """fixed seeds: every column within 6 binomial standard deviations of rounds k / P; k = 1 reaches every tile"""
    grp = _group(pkg, np.ones((1, 3), np.uint8), P, ratio, seed=11)
    count = torch.zeros(P, dtype=torch.int64, device="cuda")
    for rnd in range(rounds):
        grp.compress(rnd)
        count[grp.message(worker)[1]] += 1                         # a message's indices are distinct
    count, p = count.cpu().numpy(), grp.k / P
    assert count.sum() == rounds * grp.k
    if grp.k == 1:
        assert set(np.flatnonzero(count) // 4096) == set(range(10))
    else:
        assert np.abs(count - rounds * p).max() <= 6 * np.sqrt(rounds * p * (1 - p)), (count.min(), count.max())


def test_constructor_refusals_and_checkpoints(pkg):
    flags, P = np.ones((2, 3), np.uint8), 4096 + 777
    topo = Topo(PARTNER3, 1 / 3, flags)
    pull = object.__new__(pkg.PullTransport)                       # only its type is looked at
    for kw, err, match in ((dict(), ValueError, "ratio"), (dict(ratio=0.9, bits=4), ValueError, "bits"),
                           (dict(ratio=0.9, one_launch=True), ValueError, "one_launch"),
                           (dict(ratio=0.9, dtype=torch.bfloat16), NotImplementedError, "bfloat16"),
                           (dict(ratio=0.9, nranks=3, comm=pull), NotImplementedError, "PullTransport")):
        with pytest.raises(err, match=match):
            pkg.ChocoWorkerGroup(topo, numel=100, consensus_lr=0.1, compressor="randk", **kw)
    a = _group(pkg, flags, P, 0.9, rows=_rows(950, 3, P))
    a.communicate()
    sd = a.state_dict()
    assert (sd["compressor"], sd["seed"], sd["k"], sd["iter"]) == ("randk", SEED, a.k, 1)
    b = _group(pkg, flags, P, 0.9, seed=0)
    b.load_state_dict(sd)                                          # the checkpoint's seed comes with it
    a.communicate()
    b.communicate()
    _assert_state(b, *_state(a), "resumed")
    topk = pkg.ChocoWorkerGroup(topo, numel=P, ratio=0.9, consensus_lr=0.1)
    for grp, state in ((topk, sd), (b, topk.state_dict())):
        with pytest.raises(ValueError, match="does not match"):
            grp.load_state_dict(state)
