"""attach_adamw on the one-launch quantized ChocoSGD round (csrc/choco_quant_adamw_round.hip, _bf16.hip) against
tests/adamref.py followed by tests/quantref.py: exp_avg, exp_avg_sq and, given the norms the launch reports, x, x_hat
and s bit for bit; the norms within 1 fp32 ulp of the specification (test_gpu_choco_quant_round's rule)."""
import numpy as np
import pytest

from adamref import adam_ref, bias_table
from bf16ref import rne_bf16, same_bf16, upcast
from conftest import Topo
from sgdref import sgd_ref
from test_gpu_choco_quant import BITS, FLAGS3, SEED, _knob, _rows
from test_gpu_choco_quant_round import _check_round, _topo
from test_gpu_choco_quant_round_bf16 import _bits, _group, _masters, _put_bits
from test_gpu_choco_sign import PARTNER3, _assert_state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, U32, BF16 = np.float32, np.uint32, torch.bfloat16
BETAS, EPS, LR = (0.9, 0.99), 1e-8, 1e-3            # beta2 0.99: the bias corrections move visibly within 3 steps
TABLE = bias_table(*BETAS)
HYPERS = [(1e-2, True), (5e-4, False), (0.0, True)]                  # (weight decay, decoupled): AdamW, Adam + L2, none
FLAGS = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 1]], np.uint8)        # a full round, the step alone, a degree-0 row
STATE = ("master_rows", "x_hat", "s", "exp_avg_rows", "exp_avg_sq_rows", "round_norms")


def _adamw_group(pkg, flags, P, bits, X, hyper=HYPERS[0], dtype=torch.float32, **topo):
    grp = _group(pkg, flags, P, bits, rows=X, dtype=dtype, **topo)
    grp.attach_adamw(betas=BETAS, eps=EPS, weight_decay=hyper[0], decoupled=hyper[1])
    return grp


def _int_bits(grp, name):
    t = getattr(_masters(grp), "rows") if name == "master_rows" else getattr(grp, name)
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b, names, what):
    torch.cuda.synchronize()
    for name in names:
        assert torch.equal(_int_bits(a, name), _int_bits(b, name)), (name, what)


def _ref_iteration(st, G, t, f, hyper, grp, bits):
    """adam_ref at optimizer step t + 1 on st = [X, M, V, XH, S], then round t from the device's norms; the group's
    whole state against it"""
    st[:3] = (np.array(a) for a in adam_ref(st[0], G, st[1], st[2], t + 1, LR, (*BETAS, EPS, *hyper), TABLE))
    if f.any():
        _check_round(_masters(grp), st[0], st[3], st[4], f, bits, t, f"round {t}")
    _assert_state(_masters(grp), st[0], st[3], st[4], f"iteration {t}")
    for name, want in (("exp_avg_rows", st[1]), ("exp_avg_sq_rows", st[2])):
        assert np.array_equal(getattr(grp, name).cpu().numpy().view(U32), want.view(U32)), (name, t)
    assert not grp.grads.any()


@BITS
@pytest.mark.parametrize("hyper", HYPERS)
def test_adamw_step_is_the_step_then_the_round(pkg, bits, hyper):
    P, X = 4096 + 77, _rows(800, 3, 4096 + 77)
    grp = _adamw_group(pkg, FLAGS, P, bits, X, hyper)
    st = [X, np.zeros_like(X), np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)]
    for t, f in enumerate(FLAGS):
        G = _rows(850 + 3 * t, 3, P)
        grp.grads.copy_(torch.from_numpy(G))
        assert grp.adamw_step(t, LR) is bool(f.any())                # no active matching: the step alone
        _ref_iteration(st, G, t, f, hyper, grp, bits)
    assert grp.opt_step == 3


@BITS
@pytest.mark.parametrize("n,P", [(16, 257), (8, 1), (3, 3 * 4096 + 5)])
def test_shapes_and_grids(pkg, bits, n, P):
    """bshift 0 and 4, a lone partial bucket, several tiles per workgroup through both LDS buffers"""
    partner, flags, alpha, gamma = _topo(pkg, n)
    X = _rows(300, n, P)
    grps = [_adamw_group(pkg, flags, P, bits, X, partner=partner, alpha=alpha, gamma=gamma) for _ in range(2)]
    st = [X, np.zeros_like(X), np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)]
    for t, f in enumerate(np.asarray(flags, np.uint8)[:2]):
        G = _rows(350 + n * t, n, P)
        for g, grid in zip(grps, (0, 1)):                            # round_grid
            g.grads.copy_(torch.from_numpy(G))
            with _knob(pkg, "round_grid", grid):
                g.adamw_step(t, LR)
        _ref_iteration(st, G, t, f, HYPERS[0], grps[0], bits)
        _same(grps[1], grps[0], STATE + ("grads",), f"round {t}, one workgroup")


@BITS
def test_rows_off_a_16_byte_boundary_through_the_c_entry(pkg, bits):
    """all six fp32 arrays at 4, 0 and 12 bytes past a 16-byte boundary inside guarded buffers: the aligned group's
    bits, and not a word outside the rows' P columns is written"""
    P, n, ld, base, guard, (wd, dec) = 4096 + 77, 3, 4096 + 79, 65, 7.25, HYPERS[0]
    grp = _adamw_group(pkg, FLAGS3, P, bits, _rows(400, n, P))
    for dst, seed, scale in ((grp.x_hat, 410, 0.5), (grp.s, 420, 0.25), (grp.exp_avg_arena, 430, 0.125),
                             (grp.grad_arena, 440, 1.0)):
        dst[:, :P].copy_(torch.from_numpy(F32(scale) * _rows(seed, n, P)))
    grp.exp_avg_sq_rows.copy_(torch.from_numpy(F32(0.01) * _rows(450, n, P) ** 2))
    arenas = (grp.x, grp.grad_arena, grp.exp_avg_arena, grp.exp_avg_sq_arena, grp.x_hat, grp.s)   # the entry's order
    bufs, views = [], []
    for src in arenas:
        buf = torch.full((base + n * ld + 64,), guard, dtype=torch.float32, device="cuda")
        view = buf[base:base + n * ld].view(n, ld)
        view[:, :P].copy_(src[:, :P])
        bufs.append(buf)
        views.append(view)
    assert all([v[r].data_ptr() % 16 for r in range(n)] == [4, 0, 12] for v in views)
    nb, eng = (P + 255) // 256, grp.engine
    nrm = torch.full((n * nb + 2,), guard, dtype=torch.float32, device="cuda")
    f32 = lambda v: float(F32(v))
    pkg._lib.check(pkg.lib.mx_choco_quant_adamw_round(
        *(v.data_ptr() for v in views), ld, n, P, bits, eng.plan.data_ptr(), 0, eng.M, eng.alpha32, grp.gamma32, SEED,
        0, nrm.data_ptr() + 4, nb, LR, None, f32(1 - BETAS[0]), f32(BETAS[1]), f32(1 - BETAS[1]), f32(EPS), f32(wd),
        int(dec), 1, grp._bias_dev.data_ptr(), len(TABLE), 1, None, None))
    grp.adamw_step(0, LR)
    torch.cuda.synchronize()
    for buf, view, want in zip(bufs, views, arenas):
        assert torch.equal(view[:, :P].contiguous().view(torch.int32), want[:, :P].contiguous().view(torch.int32))
        view[:, :P].fill_(guard)
        assert bool((buf == guard).all())                            # the guards, the padding between rows too
    assert torch.equal(nrm[1:-1].view(n, nb).view(torch.int32), grp.round_norms.view(torch.int32))
    assert float(nrm[0]) == guard and float(nrm[-1]) == guard


@BITS
def test_bf16_models_equal_the_fp32_launch_on_the_widened_gradients(pkg, bits):
    P, X = 4096 + 77, _rows(800, 3, 4096 + 77)
    mixed, twin = _adamw_group(pkg, FLAGS, P, bits, X, dtype=BF16), _adamw_group(pkg, FLAGS, P, bits, X)
    for t, f in enumerate(FLAGS):
        G = rne_bf16(_rows(850 + 3 * t, 3, P))
        _put_bits(mixed.grads, G)
        twin.grads.copy_(torch.from_numpy(upcast(G)))
        for g in (mixed, twin):
            assert g.adamw_step(t, LR) is bool(f.any())
        _same(mixed, twin, STATE, f"iteration {t}")
        assert same_bf16(_bits(mixed.rows), rne_bf16(mixed.master_rows.cpu().numpy()))   # after the step alone too
        assert not _bits(mixed.grads).any()


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_graph_replay_equals_the_host_steps(pkg, dtype):
    """adamw_device_round captured once, replayed with lr_dev set over a schedule with an inactive round and once
    past its end, against adamw_step on a twin"""
    P, T = 3 * 4096 + 5, len(FLAGS)
    a, b = (_adamw_group(pkg, FLAGS, P, 8, _rows(700, 3, P), dtype=dtype) for _ in range(2))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(torch.cuda.Stream()):
        with torch.cuda.graph(graph):
            a.adamw_device_round()
    for t in range(T + 1):
        G = torch.from_numpy(upcast(rne_bf16(F32(0.3) * _rows(3100 + 10 * t, 3, P)))).cuda()
        a.grads.copy_(G)
        b.grads.copy_(G)                                             # past the schedule: g stays as it was written
        a.lr_dev.fill_(LR / (t + 1))
        graph.replay()
        if t < T:
            b.adamw_communicate(LR / (t + 1))
        _same(a, b, STATE + ("rows", "grads"), f"replay {t}")
    assert int(a.iter_dev.item()) == T + 1 == int(a.opt_step_dev.item()) - 1 and bool(a.grads.any())


@pytest.mark.parametrize("step", ["none", "sgd", "adamw"])
def test_inactive_and_out_of_schedule_rounds_per_step(pkg, step):
    """The kernel's no-op rules, once per step policy, through the _at entry points (a device counter).  3 rows,
    P = 257: a bucket of 16-byte accesses and the bucket that holds P.  A counter outside the schedule writes
    nothing, g included; a round of the schedule with no active matching leaves x_hat, s and the norms alone and is
    exactly the reference step (nothing, without a step); an AdamW optimizer step below 1 writes nothing."""
    P, lr, (mom, wd) = 257, 0.05, (0.9, 5e-4)
    flags = np.array([[1, 1, 1], [0, 0, 0]], np.uint8)
    X, G = _rows(500, 3, P), _rows(510, 3, P)
    grp = _group(pkg, flags, P, 4, rows=X, dtype=torch.float32)
    arrays, launch = {"x": grp.x, "x_hat": grp.x_hat, "s": grp.s, "round_norms": grp.round_norms}, grp.device_round
    if step == "sgd":
        grp.attach_sgd(momentum=mom, weight_decay=wd)
        arrays.update(g=grp.grad_arena, m=grp.mom_arena)
        launch = grp.sgd_device_round
    if step == "adamw":
        grp.attach_adamw(betas=BETAS, eps=EPS, weight_decay=HYPERS[0][0], decoupled=HYPERS[0][1])
        arrays.update(g=grp.grad_arena, m=grp.exp_avg_arena, v=grp.exp_avg_sq_arena)
        launch = grp.adamw_device_round
    grp.x_hat[:, :P].copy_(torch.from_numpy(F32(0.5) * _rows(520, 3, P)))
    grp.s[:, :P].copy_(torch.from_numpy(F32(0.25) * _rows(530, 3, P)))
    grp.round_norms.fill_(7.25)
    if step != "none":
        grp.grads.copy_(torch.from_numpy(G))
        grp.lr_dev.fill_(lr)

    def run(counter):
        """the launch at `counter`: the arrays' bits before it and after it"""
        grp.iter_dev.fill_(counter)
        torch.cuda.synchronize()
        before = {k: v.clone() for k, v in arrays.items()}
        launch()
        torch.cuda.synchronize()
        same = lambda k: torch.equal(arrays[k].view(torch.int32), before[k].view(torch.int32))
        return before, {k for k in arrays if not same(k)}

    for counter in (len(flags), -1):                                 # 1: outside the schedule
        assert run(counter)[1] == set(), (step, counter)
    if step == "adamw":                                              # 3: no such optimizer step, on an active round
        grp.opt_step_dev.fill_(0)
        assert run(0)[1] == set(), "optimizer step 0"
        grp.opt_step_dev.fill_(1)
    before, changed = run(1)                                         # 2: a round with no active matching
    if step == "none":
        assert changed == set()
        return
    assert changed == set(arrays) - {"x_hat", "s", "round_norms"}, changed
    if step == "sgd":
        want = dict(zip("xm", sgd_ref(X, G, np.zeros_like(X), lr, wd, mom, False)))
    else:
        Z = np.zeros_like(X)
        want = dict(zip("xmv", adam_ref(X, G, Z, Z, 1, lr, (*BETAS, EPS, *HYPERS[0]), TABLE)))
    want["g"] = np.zeros_like(X)
    for k, w in want.items():                                        # the step's P columns; the padding as it was
        before[k][:, :P].copy_(torch.from_numpy(np.asarray(w, F32)))
        assert torch.equal(arrays[k].view(torch.int32), before[k].view(torch.int32)), (step, k)


def test_refusals_and_checkpoints(pkg):
    topo, P = Topo(PARTNER3, 1 / 3, FLAGS), 777
    mk = lambda **kw: pkg.ChocoWorkerGroup(topo, numel=P, consensus_lr=0.1, **kw)
    one = dict(compressor="quant", one_launch=True, bits=4)
    for kw in (dict(ratio=0.9), dict(compressor="sign"), dict(compressor="quant")):
        with pytest.raises(NotImplementedError, match="no standalone Adam step"):
            mk(**kw).attach_adamw()
    sgd = mk(**one)
    sgd.attach_sgd(0.9)
    with pytest.raises(ValueError, match="one optimizer"):
        sgd.attach_adamw()
    a = _adamw_group(pkg, FLAGS, P, 4, _rows(950, 3, P))
    with pytest.raises(ValueError, match="one optimizer"):
        a.attach_sgd()
    plain = set(mk(**one).state_dict())
    assert set(sgd.state_dict()) - plain == {"momentum_rows"}
    assert set(a.state_dict()) - plain == {"exp_avg_rows", "exp_avg_sq_rows", "opt_step"}
    for t in range(2):
        a.grads.copy_(torch.from_numpy(_rows(960 + t, 3, P)))
        a.adamw_communicate(LR)
    b = _adamw_group(pkg, FLAGS, P, 4, None)
    b.load_state_dict(a.state_dict())
    assert b.opt_step == 2 and int(b.opt_step_dev.item()) == 3 and b.iter == 2
    for g in (a, b):
        g.grads.copy_(torch.from_numpy(_rows(970, 3, P)))
        g.adamw_communicate(LR)
    _same(b, a, STATE, "a resumed checkpoint")
    half = a.state_dict()
    del half["exp_avg_sq_rows"]
    with pytest.raises(ValueError, match="only valid together"):
        b.load_state_dict(half)
    for src, dst in ((sgd, b), (a, mk(**one)), (a, sgd)):            # another optimizer's checkpoint
        with pytest.raises(ValueError, match="does not match"):
            dst.load_state_dict(src.state_dict())


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_virtual_trainer_fused_adamw_with_quant(pkg, dtype):
    H = pkg.harness
    args = H.HarnessArgs(size=8, epoch=1, bs=16, budget=1.0, graphid=0, lr=1e-3, compress=True, compressor="quant")
    model_fn = H.model_factory(args)
    tr = H.VirtualTrainer(args, lambda: model_fn().to(dtype), n_batches=2, fused_adamw=True)
    grp = tr.group
    assert grp.one_launch and grp.dtype == dtype and grp.adamw_hyper["weight_decay"] == 5e-4
    tr.train_epoch()
    assert grp.iter == 2 == grp.opt_step and bool(torch.isfinite(grp.rows).all())
    assert float(grp.x_hat.abs().max()) > 0 and float(grp.exp_avg_sq_rows.max()) > 0 and not grp.grads.any()
    for comp in ("topk", "sign"):
        args.compressor = comp
        with pytest.raises(ValueError, match="fused_adamw"):
            H.VirtualTrainer(args, model_fn, n_batches=2, fused_adamw=True)
