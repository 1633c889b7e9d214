"""compressor="quant", one_launch=True (csrc/choco_quant_round.hip) against tests/quantref.py and tests/sgdref.py:
x, x_hat and s bit for bit given the norms the launch reports, those within 1 fp32 ulp of the specification, and
everything equal to the two-launch form's bits."""
import numpy as np
import pytest

import quantref
import rowtopos
import signref
from clipref import ulp_diff
from conftest import Topo
from sgdref import sgd_ref
from test_gpu_choco_quant import BITS, FLAGS3, FLAGS4, SEED, _knob, _rows, _slots
from test_gpu_choco_sign import PARTNER3, _assert_state, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
SGD = pytest.mark.parametrize("hyper", [(0.9, 0.0, False), (0.0, 5e-4, False), (0.9, 5e-4, True)])   # mom, wd, nesterov


def _group(pkg, flags, P, bits, partner=PARTNER3, alpha=1 / 3, gamma=0.1, rows=None, one_launch=True, seed=SEED):
    grp = pkg.ChocoWorkerGroup(Topo(partner, alpha, flags), numel=P, compressor="quant", bits=bits, seed=seed,
                               consensus_lr=gamma, one_launch=one_launch)
    if rows is not None:
        grp.rows.copy_(torch.from_numpy(rows))
    return grp


def _norms(grp, D):
    """round_norms, each within 1 ulp of the specification's (NaN and Inf alike: _check_slots' rule)"""
    torch.cuda.synchronize()
    dev = grp.round_norms.cpu().numpy()
    with np.errstate(all="ignore"):
        spec = np.stack([quantref.norms(np.pad(d, (0, -d.size % 256))) for d in D])
    fin = np.isfinite(spec)
    assert np.array_equal(np.isnan(dev), np.isnan(spec)) and np.array_equal(np.isinf(dev), np.isinf(spec))
    assert (ulp_diff(dev[fin], spec[fin]) <= 1).all(), (dev, spec)
    return dev


def _check_round(grp, X, XH, S, flags, bits, t, what, same=None):
    """the reference round in place on X, XH, S from the device's norms, then the group's state against it"""
    topo = grp.topology
    with np.errstate(all="ignore"):
        dev = _norms(grp, (X - XH).astype(F32))
    quantref.quant_round(X, XH, S, topo.neighbors_info, flags, topo.neighbor_weight, grp.consensus_lr, bits, SEED, t,
                         norm=dev)
    _assert_state(grp, X, XH, S, what, same)


def _topo(pkg, n):
    if n == 3:                                                       # the last round leaves row 1 at degree 0
        return PARTNER3, FLAGS3, 1 / 3, 0.1
    if n == 8:
        info = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True).neighbors_info
        return info, np.ones((2, len(info)), np.uint8), 2 / 7, 0.3
    partner = rowtopos.round_robin(16)                               # 32 matchings: chains of 32, of 16, of 1 partner
    return partner, rowtopos.flag_rounds(partner, 5)[:3], rowtopos.ALPHA, 0.3


@BITS
@pytest.mark.parametrize("n", [3, 8, 16])
@pytest.mark.parametrize("P", [1, 255, 257, 4096 + 77, 3 * 4096 + 5])
def test_rounds_any_grid_and_the_two_launch_twin(pkg, bits, P, n):
    partner, flags, alpha, gamma = _topo(pkg, n)
    X = _rows(300, n, P)
    grps = [_group(pkg, flags, P, bits, partner, alpha, gamma, X, one_launch=k < 3) for k in range(4)]
    XH, S = np.zeros_like(X), np.zeros_like(X)
    for t, f in enumerate(flags):
        if t:
            D = F32(0.01) * _rows(350, n, P)
            X = (X + D).astype(F32)
            for g in grps:
                g.rows.add_(torch.from_numpy(D).cuda())
        for g, grid in zip(grps, (0, 1, 3, 0)):                      # round_grid; the last group takes two launches
            with _knob(pkg, "round_grid", grid):
                g.communicate()
        _check_round(grps[0], X, XH, S, f, bits, t, f"round {t}")
        norms = grps[0].round_norms.view(torch.int32)
        for g in grps[1:3]:
            _assert_state(g, X, XH, S, f"round {t}, another grid")
            assert torch.equal(g.round_norms.view(torch.int32), norms)
        _assert_state(grps[3], X, XH, S, f"round {t}, two launches")   # the same summation order: the same norms
        twin = _slots(grps[3])[:, 64:64 + 4 * norms.shape[1]].copy().view(np.int32)
        assert np.array_equal(twin, norms.cpu().numpy())


@BITS
def test_rows_off_a_16_byte_boundary_through_the_c_entry(pkg, bits):
    """rows at 4, 0 and 12 bytes past a 16-byte boundary inside guarded buffers: the aligned group's bits, and
    not a word outside the rows' P columns is written"""
    P, n, ld, base, guard = 4096 + 77, 3, 4096 + 79, 65, F32(7.25)
    X, XH, S = _rows(400, n, P), F32(0.5) * _rows(410, n, P), F32(0.25) * _rows(420, n, P)
    grp = _group(pkg, FLAGS3, P, bits, rows=X)
    bufs, views = [], []
    for src, dst in ((X, grp.rows), (XH, grp.x_hat[:, :P]), (S, grp.s[:, :P])):
        dst.copy_(torch.from_numpy(src))
        buf = torch.full((base + n * ld + 64,), float(guard), dtype=torch.float32, device="cuda")
        view = buf[base:base + n * ld].view(n, ld)
        view[:, :P].copy_(torch.from_numpy(src))
        bufs.append(buf)
        views.append(view)
    assert [views[0][r].data_ptr() % 16 for r in range(n)] == [4, 0, 12]
    nb = (P + 255) // 256
    nrm = torch.full((n * nb + 2,), float(guard), dtype=torch.float32, device="cuda")
    eng = grp.engine
    pkg._lib.check(pkg.lib.mx_choco_quant_round(*(v.data_ptr() for v in views), ld, n, P, bits, eng.plan.data_ptr(), 0,
                                                eng.M, eng.alpha32, grp.gamma32, SEED, 0, nrm.data_ptr() + 4, nb, None))
    grp.communicate()
    want = _state(grp)
    for buf, view, w in zip(bufs, views, want):
        assert np.array_equal(view[:, :P].cpu().numpy().view(U32), w.view(U32))
        view[:, :P].fill_(float(guard))
        assert bool((buf == float(guard)).all())                    # the guards, the padding between rows too
    assert torch.equal(nrm[1:-1].view(n, nb).view(torch.int32), grp.round_norms.view(torch.int32))
    assert float(nrm[0]) == guard and float(nrm[-1]) == guard


@BITS
@SGD
def test_sgd_step_is_the_step_then_the_round(pkg, bits, hyper):
    (mom, wd, nesterov), P, lr = hyper, 4096 + 77, 0.05
    flags = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 1]], np.uint8)
    X = _rows(800, 3, P)
    grp = _group(pkg, flags, P, bits, rows=X)
    grp.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov)
    M, XH, S = np.zeros_like(X) if mom else None, np.zeros_like(X), np.zeros_like(X)
    for t, f in enumerate(flags):
        grp.grads.copy_(torch.from_numpy(_rows(850 + 3 * t, 3, P)))
        assert grp.sgd_step(t, lr) is bool(f.any())                  # no active matching: the step alone
        X, M = sgd_ref(X, _rows(850 + 3 * t, 3, P), M, lr, wd, mom, nesterov)
        X = np.array(X)
        if f.any():
            _check_round(grp, X, XH, S, f, bits, t, f"round {t}")
        _assert_state(grp, X, XH, S, f"iteration {t}")
        assert not grp.grads.any()
        assert M is None or np.array_equal(grp.momentum_rows.cpu().numpy().view(U32), np.asarray(M).view(U32))


@BITS
def test_special_values(pkg, bits):
    """test_gpu_choco_quant's inputs: a zero bucket; a NaN in bucket 2 of row 1 (NaN there and in its partner row 0,
    nowhere else); the clamp bucket (one nonzero value: v = s + xi floors to s + 1 without the clamp)"""
    P = 4096 + 300
    X = _rows(600, 3, P)
    X[0, :256], X[1, 700], X[2, 256:300], X[2, 300], X[2, 301:512] = 0, np.nan, 0, -3.0, 0
    flags = np.array([[1, 0, 0]], np.uint8)                         # workers 0 and 1 matched, 2 alone
    grp = _group(pkg, flags, P, bits, rows=X)
    grp.communicate()
    _check_round(grp, X.copy(), np.zeros_like(X), np.zeros_like(X), flags[0], bits, 0, "round 0", signref.same_bits)
    want = (np.arange(3)[:, None] < 2) & (np.arange(P) // 256 == 2)
    x, xh, s = _state(grp)
    assert np.array_equal(np.isnan(x), want) and np.array_equal(np.isnan(s), want)
    assert float(grp.round_norms[0, 0]) == 0 and not xh[0, :256].view(U32).any()
    s_lv, c = quantref.consts(bits)
    assert xh[2, 300] == -(F32(s_lv) * (F32(3.0) * c).astype(F32))   # level s, not s + 1


@BITS
@pytest.mark.parametrize("sgd", [False, True])
def test_graph_replay_equals_the_host_rounds(pkg, bits, sgd):
    """device_round / sgd_device_round (lr_dev) captured once, replayed over a schedule with an all-zero round and
    twice past its end, against communicate / sgd_communicate on a twin"""
    P, T = 3 * 4096 + 5, len(FLAGS4)
    a, b = (_group(pkg, FLAGS4, P, bits, rows=_rows(700, 3, P)) for _ in range(2))
    for grp in (a, b) if sgd else ():
        grp.attach_sgd(0.9, 5e-4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(torch.cuda.Stream()):
        with torch.cuda.graph(graph):
            a.sgd_device_round() if sgd else a.device_round()
    for t in range(T + 2):
        if sgd:
            G = torch.from_numpy(F32(0.3) * _rows(3100 + 10 * t, 3, P)).cuda()
            a.grads.copy_(G)
            b.grads.copy_(G)                                         # past the schedule: g stays as it was written
            a.lr_dev.fill_(0.05 / (t + 1))
        graph.replay()
        if t < T:
            b.sgd_communicate(0.05 / (t + 1)) if sgd else b.communicate()
        torch.cuda.synchronize()
        _assert_state(a, *_state(b), f"replay {t}")
        for name in ("momentum_rows", "grads") if sgd else ():
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), (name, t)
    assert int(a.iter_dev.item()) == T + 2 and (not sgd or bool(a.grads.any()))


def test_refusals_and_checkpoints_across_the_two_forms(pkg):
    flags, P = np.ones((3, 3), np.uint8), 777
    mk = lambda topo=Topo(PARTNER3, 1 / 3, flags), **kw: pkg.ChocoWorkerGroup(topo, numel=100, consensus_lr=0.1,
                                                                            one_launch=True, **kw)
    for kw in (dict(compressor="sign"), dict(ratio=0.9)):
        with pytest.raises(ValueError, match="one_launch"):
            mk(**kw)
    with pytest.raises(NotImplementedError, match="two-launch"):
        mk(compressor="quant", nranks=3)
    with pytest.raises(NotImplementedError, match="two-launch"):
        mk(Topo(rowtopos.round_robin(17, 4), 0.1, np.ones((1, 4), np.uint8)), compressor="quant")
    X = _rows(950, 3, P)
    one, two = _group(pkg, flags, P, 4, rows=X), _group(pkg, flags, P, 4, rows=X, one_launch=False)
    for call in (lambda: one.message(0), lambda: one.compress(0), lambda: one.average(0)):
        with pytest.raises(pkg.MXError, match="no message slots"):
            call()
    one.communicate()
    two.communicate()
    assert set(one.state_dict()) == set(two.state_dict())
    b_two, b_one = _group(pkg, flags, P, 4, one_launch=False, seed=0), _group(pkg, flags, P, 4, seed=0)
    b_two.load_state_dict(one.state_dict())                          # saved by one form, resumed by the other
    b_one.load_state_dict(two.state_dict())
    for grp in (one, b_two, b_one):
        grp.communicate()
    _assert_state(b_two, *_state(one), "one launch -> two")
    _assert_state(b_one, *_state(one), "two launches -> one")
    # a plan record with the peer-reads bit is not this kernel's: the launch writes nothing
    eng = one.engine
    pkg._lib.check(pkg.lib.mx_plan_set_peer_reads(eng.plan.data_ptr(), eng.T + 1, 3, eng.M, 1, None))
    before = _state(one)
    one.step(2)
    _assert_state(one, *before, "peer-reads record")


def test_virtual_trainer_fused_sgd_with_quant(pkg):
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=1.0, graphid=0, lr=0.1, momentum=0.9, compress=True,
                         compressor="quant")
    tr = H.VirtualTrainer(args, H.model_factory(args), n_batches=2, fused_sgd=True)
    grp, snap = tr.group, {}
    assert grp.one_launch and grp.bits == 8

    def hook(when, trainer):
        if when == "before":
            snap["st"] = [np.array(v) for v in _state(grp)] + [grp.grads.cpu().numpy(), grp.momentum_rows.cpu().numpy()]
            return
        X, XH, S, G, M = snap["st"]
        t, lr, hy = grp.iter - 1, trainer.optimizers[0].param_groups[0]["lr"], grp.sgd_hyper
        X, M = sgd_ref(X, G, M, lr, hy["weight_decay"], hy["momentum"], hy["nesterov"])
        X = np.array(X)
        if np.any(grp.topology.active_flags[t]):
            quantref.quant_round(X, XH, S, grp.topology.neighbors_info, grp.topology.active_flags[t],
                                 grp.topology.neighbor_weight, grp.consensus_lr, 8, grp.seed, t,
                                 norm=grp.round_norms.cpu().numpy())
        _assert_state(grp, X, XH, S, f"iteration {t}")
        assert np.array_equal(grp.momentum_rows.cpu().numpy().view(U32), M.view(U32)) and not grp.grads.any()

    tr.train_epoch(hook)
    assert grp.iter == 2 and bool(torch.isfinite(grp.rows).all()) and float(grp.x_hat.abs().max()) > 0
