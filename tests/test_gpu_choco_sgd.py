"""The SGD step fused into the ChocoSGD round (csrc/choco_sgd.hip) against tests/sgdref.py and tests/signref.py:
x', m' and g exact, the bits those of x' - x_hat, the scale within 1 fp32 ulp of the spec and the same bits
whatever computes the row, and the state after every round bit for bit given the device's scales."""
import numpy as np
import pytest

import signref
from clipref import ulp_diff
from conftest import Topo
from sgdref import sgd_ref
from test_gpu_choco_sign import PARTNER3, _assert_state, _knobs, _padded, _row, _scales, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
LR = 0.05
# momentum, weight decay, nesterov, zero_grads
HYPERS = [(0.0, 0.0, False, True), (0.9, 5e-4, False, True), (0.9, 5e-4, True, True), (0.9, 5e-4, False, False)]
FLAGS = np.array([[1, 1, 1], [1, 0, 1], [0, 0, 0], [1, 0, 0]], np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _case(seed, n, P, hyper):
    """x, g, m (None without momentum), x_hat [n, P] and the spec's x', m', d = x' - x_hat; with room, column
    3's difference is an exact +0 (x_hat = x') and column P - 2's an exact -0 (x = -0, g = m = x_hat = +0)"""
    mom, wd, nesterov, _ = hyper
    X, G, M, XH = (np.stack([F32(sc) * _row(seed + 10 * a + i, P) for i in range(n)]).copy()
                   for a, sc in enumerate((1.0, 0.3, 0.2, 0.5)))
    if P > 10:
        X[:, P - 2], G[:, P - 2], M[:, P - 2], XH[:, P - 2] = F32(-0.0), 0, 0, 0
    M = M if mom else None
    XP, MP = sgd_ref(X, G, M, LR, wd, mom, nesterov)
    if P > 10:
        XH[:, 3] = XP[:, 3]
    return X, G, M, XH, XP, MP, (XP - XH).astype(F32)


def _check_step(x, g, m, raw, XP, MP, D, G_after, what):
    """device arrays after a fused launch against the spec; `raw` [n, msg_bytes] uint8.  Returns the scales."""
    torch.cuda.synchronize()
    P = XP.shape[1]
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(XP)), f"x' {what}"
    assert MP is None or np.array_equal(_bits(m.cpu().numpy()), _bits(MP)), f"m' {what}"
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(G_after)), f"g {what}"
    raw = raw.cpu().numpy()
    scales = raw[:, :4].copy().view(F32)[:, 0]
    for r in range(XP.shape[0]):
        want_scale, want_bits = signref.sign_message(D[r])
        assert np.array_equal(raw[r, 64:], _padded(want_bits, P)), (what, r)
        assert int(ulp_diff(scales[r], want_scale)) <= 1, (what, r, scales[r], want_scale)
        L = raw[r, 8:16].copy().view(np.float64)[0]
        assert raw[r, 16:24].copy().view(np.int64)[0] == P and F32(L / np.float64(P)) == scales[r], (what, r)
        assert not raw[r, 4:8].any() and not raw[r, 24:64].any(), (what, r)
    return scales


@pytest.mark.parametrize("P,hyper", [(P, h) for P in (1, 65, 257, 4095, 4096, 4097, 3 * 4096 + 5) for h in HYPERS[:3]] +
                         [(4097, HYPERS[3])])                      # zero_grads=False: one case
def test_step_compress_small_shapes(pkg, P, hyper):
    """a 3-row sign group under every compress-knob value, then the unfused pass on the updated rows"""
    X, G, M, XH, XP, MP, D = _case(1000, 3, P, hyper)
    grp = pkg.ChocoWorkerGroup(Topo(PARTNER3, 1 / 3, FLAGS), numel=P, compressor="sign", consensus_lr=0.1)
    grp.attach_sgd(*hyper)
    assert (grp.momentum_rows is None) == (MP is None) and not grp.grads.any()
    slots = grp.msgs[:3 * grp.msg_ld].view(3, grp.msg_ld)[:, :grp.msg_bytes]
    seen = []
    for knobs in ({}, {"grid": 1}, {"grid": 3}, {"blocks_per_cu": 64}):
        with _knobs(pkg, **knobs):
            for dst, src in ((grp.rows, X), (grp.grads, G), (grp.momentum_rows, M), (grp.x_hat[:, :P], XH)):
                if src is not None:
                    dst.copy_(torch.from_numpy(src))
            grp.msgs.fill_(0xAB)                                   # every byte of a slot is written again
            grp.sgd_compress(LR)
            seen.append(_check_step(grp.rows, grp.grads, grp.momentum_rows, slots, XP, MP, D,
                                    np.zeros_like(G) if hyper[3] else G, knobs))
    grp.compress(0)                                                # the unfused pass on the updated rows
    torch.cuda.synchronize()
    seen.append(_scales(grp))
    assert all(np.array_equal(_bits(s), _bits(seen[0])) for s in seen), seen


@pytest.mark.parametrize("P", [257, 4097])
def test_unaligned_rows_through_the_c_entry_point(pkg, P):
    """one row whose x, g, m and x_hat all start 4 bytes off a 16-byte boundary: the element-wise path"""
    L, lib = pkg.lib, pkg._lib
    mom, wd, nesterov, _ = hyper = HYPERS[2]
    *host, XP, MP, D = _case(1200, 1, P, hyper)
    x, g, m, xh = (torch.zeros(P + 8, dtype=torch.float32, device="cuda")[1:P + 1] for _ in range(4))
    for v, a in zip((x, g, m, xh), host):                          # allocations are 256-byte aligned
        v.copy_(torch.from_numpy(a[0]))
        assert v.data_ptr() % 16 == 4
    nbytes = signref.msg_bytes(P)
    msgs = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    work = torch.zeros(int(L.mx_choco_sign_work_bytes(P, 1)), dtype=torch.uint8, device="cuda")
    lib.check(L.mx_choco_sign_sgd_compress(x.data_ptr(), g.data_ptr(), m.data_ptr(), xh.data_ptr(), P, 1, P,
                                           msgs.data_ptr(), nbytes, work.data_ptr(), LR, None, wd, mom, nesterov, 1,
                                           None, 0, lib.stream_ptr()))
    scale = _check_step(x[None], g[None], m[None], msgs[None], XP, MP, D, np.zeros_like(XP), "unaligned")
    lib.check(L.mx_choco_sign_compress(x.data_ptr(), xh.data_ptr(), P, 1, P, msgs.data_ptr(), nbytes, work.data_ptr(),
                                       lib.stream_ptr()))
    torch.cuda.synchronize()
    assert msgs[:4].cpu().numpy().view(np.uint32) == _bits(scale)


def _group(pkg, topo, P, compressor, gamma=0.1):
    kw = dict(compressor="sign") if compressor == "sign" else dict(ratio=0.9)
    return pkg.ChocoWorkerGroup(topo, numel=P, consensus_lr=gamma, **kw)


def _run_rounds(pkg, topo, flags, P, n, compressor, alpha, gamma, seed):
    """sgd_communicate over the schedule with fresh gradients each iteration.  sign: the state after every
    iteration is sgd_ref followed by signref.sign_round given the device scales; topk: that of a twin group whose
    rows receive sgd_ref's x' and then run communicate().  An all-zero round is the step alone."""
    mom, wd, nesterov, _ = HYPERS[2]
    grp = _group(pkg, topo, P, compressor, gamma)
    grp.attach_sgd(mom, wd, nesterov)
    twin = None if compressor == "sign" else _group(pkg, topo, P, compressor, gamma)
    X = np.stack([_row(seed + i, P) for i in range(n)]).copy()
    XH, S, M = np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)
    grp.rows.copy_(torch.from_numpy(X))
    for t, f in enumerate(flags):
        G = np.stack([F32(0.3) * _row(seed + 100 * (t + 1) + i, P) for i in range(n)])
        grp.grads.copy_(torch.from_numpy(G))
        X, M = sgd_ref(X, G, M, LR, wd, mom, nesterov)
        assert grp.iter == t
        grp.sgd_communicate(LR)
        if twin is not None:
            twin.rows.copy_(torch.from_numpy(X))
            twin.communicate()
            X, XH, S = _state(twin)
        elif f.any():
            dev = _scales(grp)
            spec = np.array([signref.sign_message((X[i] - XH[i]).astype(F32))[0] for i in range(n)], F32)
            assert (ulp_diff(dev, spec) <= 1).all(), (t, dev, spec)
            signref.sign_round(X, XH, S, topo.neighbors_info, f, alpha, gamma, scale=dev)
        _assert_state(grp, X, XH, S, f"iteration {t}")
        assert np.array_equal(_bits(grp.momentum_rows.cpu().numpy()), _bits(M)), t
        assert not _bits(grp.grads.cpu().numpy()).any(), t


@pytest.mark.parametrize("compressor", ["sign", "topk"])
@pytest.mark.parametrize("P", [65, 3 * 4096 + 5])
def test_rounds(pkg, P, compressor):
    _run_rounds(pkg, Topo(PARTNER3, 1 / 3, FLAGS), FLAGS, P, 3, compressor, 1 / 3, 0.1, 2000)


def test_rounds_eight_workers(pkg):
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
    flags = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 1, 1, 1, 0]], np.uint8)
    _run_rounds(pkg, Topo(gp.neighbors_info, 2 / 7, flags), flags, 4096 + 77, 8, "sign", 2 / 7, 0.3, 2100)


@pytest.mark.parametrize("compressor", ["sign", "topk"])
def test_device_round_graph_replay(pkg, compressor):
    """sgd_device_round captured once and replayed over a 4-round schedule with an all-zero round, lr_dev changed
    between replays: sgd_step on a twin group, bit for bit; past the schedule a replay changes nothing."""
    P = 3 * 4096 + 5
    flags = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 0]], np.uint8)
    a, b = (_group(pkg, Topo(PARTNER3, 1 / 3, flags), P, compressor) for _ in range(2))
    X = np.stack([_row(3000 + i, P) for i in range(3)])
    for grp in (a, b):
        grp.attach_sgd(0.9, 5e-4, False)
        grp.rows.copy_(torch.from_numpy(X))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(torch.cuda.Stream()):
        with torch.cuda.graph(graph):
            a.sgd_device_round()
    torch.cuda.synchronize()
    assert int(a.iter_dev.item()) == 0 and np.array_equal(a.rows.cpu().numpy(), X)     # capture ran nothing
    for t in range(len(flags) + 2):
        G = torch.from_numpy(np.stack([F32(0.3) * _row(3100 + 10 * t + i, P) for i in range(3)])).cuda()
        lr = 0.05 / (t + 1)
        a.grads.copy_(G)
        b.grads.copy_(G)                                           # past the schedule: g stays as it was written
        a.lr_dev.fill_(lr)
        graph.replay()
        if t < len(flags):
            assert b.sgd_step(t, lr) == bool(flags[t].any())
        torch.cuda.synchronize()
        _assert_state(a, *_state(b), f"replay {t}")
        for name in ("momentum_rows", "grads"):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), (name, t)
    a.check_topk()
    assert int(a.iter_dev.item()) == len(flags) + 2 and bool(a.grads.any()) and bool(a.momentum_rows.any())


def test_refusals_and_checkpoints(pkg):
    topo, P = Topo(PARTNER3, 1 / 3, np.ones((4, 3), np.uint8)), 777
    a, b = (_group(pkg, topo, P, "sign") for _ in range(2))
    with pytest.raises(ValueError, match="Nesterov"):
        a.attach_sgd(0.0, nesterov=True)
    plain = a.state_dict()
    assert set(plain) == {"kind", "iter", "row_base", "k", "workers", "rows", "x_hat", "s", "compressor"}
    models = [torch.nn.Linear(4, 3).cuda() for _ in range(3)]
    with pytest.raises(ValueError, match="adopt=False"):
        pkg.ChocoWorkerGroup(topo, models, compressor="sign", consensus_lr=0.1, adopt=False).attach_sgd(0.9)
    ad = pkg.ChocoWorkerGroup(topo, models, compressor="sign", consensus_lr=0.1)
    ad.attach_sgd(0.9)
    models[1](torch.ones(2, 4, device="cuda")).sum().backward()
    assert models[1].weight.grad.data_ptr() == ad.grad_arena[1].data_ptr() and bool(ad.grads[1].any())
    a.attach_sgd(0.9, 5e-4)
    a.rows.copy_(torch.from_numpy(np.stack([_row(4000 + i, P) for i in range(3)])))
    G = torch.from_numpy(np.stack([_row(4010 + i, P) for i in range(3)])).cuda()
    a.grads.copy_(G)
    a.sgd_communicate(LR)
    sd = a.state_dict()
    assert sd["iter"] == 1 and torch.equal(sd["momentum_rows"], a.momentum_rows)
    with pytest.raises(ValueError, match="does not match"):
        b.load_state_dict(sd)                                      # saved with momentum, group without
    b.attach_sgd(0.9, 5e-4)
    with pytest.raises(ValueError, match="does not match"):
        b.load_state_dict(plain)                                   # saved without, group with
    b.load_state_dict(sd)
    for grp in (a, b):
        grp.grads.copy_(G)
        grp.sgd_communicate(LR)
    _assert_state(b, *_state(a), "resumed")
    assert torch.equal(a.momentum_rows, b.momentum_rows)


def test_virtual_trainer_fused_sgd_with_compress(pkg):
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=1.0, graphid=0, lr=0.1, momentum=0.9, compress=True,
                         compressor="sign")
    tr = H.VirtualTrainer(args, H.model_factory(args), n_batches=2, fused_sgd=True)
    tr.train_epoch()
    assert tr.group.iter == 2 and bool(torch.isfinite(tr.group.rows).all()) and bool(tr.group.momentum_rows.any())
    assert float(tr.group.x_hat.abs().max()) > 0 and not bool(tr.group.grads.any())
    with pytest.raises(ValueError, match="fused_adamw"):
        H.VirtualTrainer(args, H.model_factory(args), n_batches=2, fused_adamw=True)
