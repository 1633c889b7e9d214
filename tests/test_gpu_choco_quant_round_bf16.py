"""dtype=torch.bfloat16 on the one-launch quantized round (csrc/choco_quant_round_bf16.hip) against tests/quantref.py,
tests/sgdref.py and tests/bf16ref.py: the fp32 state bit for bit given the norms the launch reports (the fp32
test's rule), the models the one rounding of the masters, and everything equal to an fp32 twin's bits."""
from types import SimpleNamespace

import numpy as np
import pytest

import quantref
import signref
from bf16ref import rne_bf16, same_bf16, upcast
from conftest import Topo
from sgdref import sgd_ref
from test_gpu_choco_quant import BITS, FLAGS3, FLAGS4, SEED, _knob, _rows
from test_gpu_choco_quant_round import SGD, _check_round, _topo
from test_gpu_choco_sign import PARTNER3, _assert_state, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, U32, BF16 = np.float32, np.uint32, torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _put_bits(t, bits):
    t.copy_(torch.from_numpy(bits.view(np.int16)).cuda().view(BF16))


def _group(pkg, flags, P, bits, partner=PARTNER3, alpha=1 / 3, gamma=0.1, rows=None, dtype=BF16):
    grp = pkg.ChocoWorkerGroup(Topo(partner, alpha, flags), numel=P, compressor="quant", bits=bits, seed=SEED,
                               consensus_lr=gamma, one_launch=True, dtype=dtype)
    if rows is not None:
        (grp.rows if grp.master_rows is None else grp.master_rows).copy_(torch.from_numpy(rows))
    return grp


def _masters(grp):
    """what _state / _assert_state / _check_round read of a group, with the fp32 masters as its rows"""
    rows = grp.rows if grp.master_rows is None else grp.master_rows
    return SimpleNamespace(numel=grp.numel, rows=rows, x_hat=grp.x_hat, s=grp.s, topology=grp.topology,
                           consensus_lr=grp.consensus_lr, round_norms=grp.round_norms)


def _full_state(grp):
    torch.cuda.synchronize()
    m = grp.momentum_rows
    return [*_state(_masters(grp)), None if m is None else m.cpu().numpy(), grp.round_norms.cpu().numpy()]


@BITS
@SGD
@pytest.mark.parametrize("n", [3, 8, 16])
@pytest.mark.parametrize("P", [1, 257, 3 * 4096 + 5])
def test_sgd_step_then_round_bit_for_bit(pkg, bits, hyper, n, P):
    (mom, wd, nesterov), lr = hyper, 0.05
    partner, flags, alpha, gamma = _topo(pkg, n)
    flags = np.insert(np.asarray(flags, np.uint8)[:2], 1, 0, axis=0)         # one all-zero round
    special = n == 3 and P == 257                   # a NaN and an Inf gradient, and an fp32 twin on the widened g
    same = signref.same_bits if special else None
    X = _rows(800, n, P)
    grps = [_group(pkg, flags, P, bits, partner, alpha, gamma, X) for _ in range(2)]      # round_grid 0 and 1
    grps += [_group(pkg, flags, P, bits, partner, alpha, gamma, X, dtype=torch.float32)] if special else []
    for g in grps:
        g.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov)
    M, XH, S = np.zeros_like(X) if mom else None, np.zeros_like(X), np.zeros_like(X)
    for t, f in enumerate(flags):
        G = rne_bf16(_rows(850 + 3 * t, n, P))
        if special and t == 0:
            G[0, 3], G[2, P - 1] = 0x7FC0, 0xFF80
        for g, grid in zip(grps, (0, 1, 0)):
            g.grads.copy_(torch.from_numpy(upcast(G))) if g.master_rows is None else _put_bits(g.grads, G)
            with _knob(pkg, "round_grid", grid):
                assert g.sgd_step(t, lr) is bool(f.any())            # no active matching: the step and the image
        X, M = sgd_ref(X, upcast(G), M, lr, wd, mom, nesterov)
        X = np.array(X)
        if f.any():
            _check_round(_masters(grps[0]), X, XH, S, f, bits, t, f"round {t}", same)
        want = _full_state(grps[0])
        for g in grps[:2]:
            _assert_state(_masters(g), X, XH, S, f"iteration {t}", same)
            assert M is None or (same or signref.same_bits)(g.momentum_rows.cpu().numpy(), M)
            assert same_bf16(_bits(g.rows), rne_bf16(X)) and not _bits(g.grads).any()
        for g in grps[1:]:                                           # the other grid, the fp32 twin: the same bits
            assert all(a is None or np.array_equal(a.view(U32), b.view(U32)) for a, b in zip(_full_state(g), want)), t


@BITS
def test_rows_off_the_vector_boundaries_through_the_c_entry(pkg, bits):
    """fp32 rows at 4, 0 and 12 bytes past a 16-byte boundary, g and p rows at 2, 0 and 6 past an 8-byte one, inside
    guarded buffers: the aligned group's bits, and nothing outside the rows' P columns is written"""
    P, n, ld, base, guard, lr, (mom, wd) = 4096 + 77, 3, 4096 + 79, 65, 7.25, 0.05, (0.9, 5e-4)
    grp = _group(pkg, FLAGS3, P, bits, rows=_rows(400, n, P))
    grp.attach_sgd(momentum=mom, weight_decay=wd)
    for dst, seed, scale in ((grp.x_hat, 410, 0.5), (grp.s, 420, 0.25), (grp.mom_arena, 430, 0.125)):
        dst[:, :P].copy_(torch.from_numpy(F32(scale) * _rows(seed, n, P)))
    _put_bits(grp.grads, rne_bf16(_rows(440, n, P)))
    bufs, views = [], []
    for src in (grp.x, grp.grad_arena, grp.mom_arena, grp.x_hat, grp.s, grp.arena):       # the entry point's order
        buf = torch.full((base + n * ld + 64,), guard, dtype=src.dtype, device="cuda")
        view = buf[base:base + n * ld].view(n, ld)
        view[:, :P].copy_(src[:, :P])
        bufs.append(buf)
        views.append(view)
    assert [views[0][r].data_ptr() % 16 for r in range(n)] == [4, 0, 12]
    assert [views[1][r].data_ptr() % 8 for r in range(n)] == [views[5][r].data_ptr() % 8 for r in range(n)] == [2, 0, 6]
    nb, eng = (P + 255) // 256, grp.engine
    nrm = torch.full((n * nb + 2,), guard, dtype=torch.float32, device="cuda")
    pkg._lib.check(pkg.lib.mx_choco_quant_sgd_round_bf16(
        *(v.data_ptr() for v in views), ld, n, P, bits, eng.plan.data_ptr(), 0, eng.M, eng.alpha32, grp.gamma32, SEED,
        0, nrm.data_ptr() + 4, nb, lr, None, wd, mom, 0, 1, None))
    grp.sgd_step(0, lr)
    torch.cuda.synchronize()
    for buf, view, want in zip(bufs, views, (grp.x, grp.grad_arena, grp.mom_arena, grp.x_hat, grp.s, grp.arena)):
        ints = torch.int32 if buf.dtype == torch.float32 else torch.int16
        assert torch.equal(view[:, :P].contiguous().view(ints), want[:, :P].contiguous().view(ints))
        view[:, :P].fill_(guard)
        assert bool((buf == guard).all())                            # the guards, the padding between rows too
    assert not grp.grads.any() and torch.equal(nrm[1:-1].view(n, nb).view(torch.int32),
                                               grp.round_norms.view(torch.int32))
    assert float(nrm[0]) == guard and float(nrm[-1]) == guard


@BITS
@pytest.mark.parametrize("sgd", [True, False])
def test_graph_replay_equals_the_host_rounds(pkg, bits, sgd):
    """sgd_device_round (lr_dev) / device_round captured once, replayed over a schedule with an all-zero round and
    twice past its end, against sgd_communicate / communicate on a twin: every array, the image included"""
    P, T = 3 * 4096 + 5, len(FLAGS4)
    a, b = (_group(pkg, FLAGS4, P, bits, rows=_rows(700, 3, P)) for _ in range(2))
    for grp in (a, b):
        grp.attach_sgd(0.9, 5e-4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(torch.cuda.Stream()):
        with torch.cuda.graph(graph):
            a.sgd_device_round() if sgd else a.device_round()
    for t in range(T + 2):
        G = rne_bf16(F32(0.3) * _rows(3100 + 10 * t, 3, P))
        _put_bits(a.grads, G)
        _put_bits(b.grads, G)                                        # past the schedule: g stays as it was written
        a.lr_dev.fill_(0.05 / (t + 1))
        graph.replay()
        if t < T:
            b.sgd_communicate(0.05 / (t + 1)) if sgd else b.communicate()
        torch.cuda.synchronize()
        for name, ints in (("master_rows", torch.int32), ("x_hat", torch.int32), ("s", torch.int32),
                           ("momentum_rows", torch.int32), ("rows", torch.int16), ("grads", torch.int16)):
            assert torch.equal(getattr(a, name).contiguous().view(ints), getattr(b, name).contiguous().view(ints)), \
                (name, t)
    assert int(a.iter_dev.item()) == T + 2 and bool(a.grads.any())


def test_python_surface_refusals_and_checkpoints(pkg):
    flags, P = np.ones((3, 3), np.uint8), 777
    topo = Topo(PARTNER3, 1 / 3, flags)
    models = [torch.nn.Linear(5, 3).to(device="cuda", dtype=BF16) for _ in range(3)]
    kw = dict(compressor="quant", one_launch=True, consensus_lr=0.1, dtype=BF16)
    grp = pkg.ChocoWorkerGroup(topo, models, **kw)
    grp.attach_sgd(0.9)
    for r, m in enumerate(models):
        w, b = m.weight, m.bias
        assert w.dtype == w.grad.dtype == BF16 and w.data_ptr() == grp.rows[r].data_ptr()
        assert b.data_ptr() == grp.rows[r, 15:].data_ptr() and b.grad.data_ptr() == grp.grads[r, 15:].data_ptr()
    assert grp.master_rows.dtype == torch.float32 and torch.equal(grp.master_rows, grp.rows.float())
    grp.rows.fill_(0.5)
    grp.master_from_rows()
    assert bool((grp.master_rows == 0.5).all())
    for bad in (dict(compressor="topk", ratio=0.9, one_launch=False), dict(compressor="sign", one_launch=False),
                dict(one_launch=False), dict(nranks=3), dict(comm=object())):
        with pytest.raises(NotImplementedError, match="fp32-only"):
            pkg.ChocoWorkerGroup(topo, numel=100, **{**kw, **bad})
    with pytest.raises(TypeError):
        pkg.ChocoWorkerGroup(topo, [torch.nn.Linear(5, 3).cuda() for _ in range(3)], **kw)
    # checkpoints: `rows` are the fp32 masters, so the two dtypes load each other's
    one, f32 = _group(pkg, flags, P, 4, rows=_rows(950, 3, P)), _group(pkg, flags, P, 4, dtype=torch.float32)
    one.communicate()
    assert f32.master_rows is None and set(one.state_dict()) - set(f32.state_dict()) == {"dtype"}
    b16, b32 = _group(pkg, flags, P, 4), _group(pkg, flags, P, 4, dtype=torch.float32)
    for dst in (b16, b32):
        dst.load_state_dict(one.state_dict())
    assert same_bf16(_bits(b16.rows), rne_bf16(b16.master_rows.cpu().numpy()))
    for g in (one, b16, b32):
        g.communicate()
    back = _group(pkg, flags, P, 4)
    back.load_state_dict(b32.state_dict())                           # fp32 -> bf16
    for g in (one, b16, b32, back):
        g.communicate()
    want = _state(_masters(one))
    for g in (_masters(b16), b32, _masters(back)):
        _assert_state(g, *want, "a loaded checkpoint")
    assert np.array_equal(_bits(back.rows), _bits(one.rows))


def test_virtual_trainer_fused_sgd_with_quant_and_bf16_models(pkg):
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=1.0, graphid=0, lr=0.1, momentum=0.9, compress=True,
                         compressor="quant")
    model_fn = H.model_factory(args)
    tr = H.VirtualTrainer(args, lambda: model_fn().to(BF16), n_batches=2, fused_sgd=True)
    grp, snap = tr.group, {}
    assert grp.one_launch and grp.dtype == BF16 and grp.rows.dtype == BF16

    def hook(when, trainer):
        if when == "before":
            snap["st"] = [np.array(v) for v in _state(_masters(grp))] + [_bits(grp.grads),
                                                                         grp.momentum_rows.cpu().numpy()]
            return
        X, XH, S, G, M = snap["st"]
        t, lr, hy = grp.iter - 1, trainer.optimizers[0].param_groups[0]["lr"], grp.sgd_hyper
        X, M = sgd_ref(X, upcast(G), M, lr, hy["weight_decay"], hy["momentum"], hy["nesterov"])
        X = np.array(X)
        if np.any(grp.topology.active_flags[t]):
            quantref.quant_round(X, XH, S, grp.topology.neighbors_info, grp.topology.active_flags[t],
                                 grp.topology.neighbor_weight, grp.consensus_lr, 8, grp.seed, t,
                                 norm=grp.round_norms.cpu().numpy())
        _assert_state(_masters(grp), X, XH, S, f"iteration {t}")
        assert np.array_equal(grp.momentum_rows.cpu().numpy().view(U32), M.view(U32)) and not _bits(grp.grads).any()
        assert same_bf16(_bits(grp.rows), rne_bf16(X))

    tr.train_epoch(hook)
    assert grp.iter == 2 and bool(torch.isfinite(grp.master_rows).all()) and float(grp.x_hat.abs().max()) > 0
