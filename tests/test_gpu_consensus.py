"""The consensus-distance kernel (csrc/consensus.hip, mx_consensus) and its callers, against the specification
in tests/consref.py (never the code under test).

Every output -- dist[r], the consensus distance stats[0], the norm of the mean stats[1] -- is within 1 fp32
ulp of consref (the column arithmetic is pinned, so only the order of the sums over columns differs: see
consref).  Every launch starts from a workspace filled with NaN and outputs filled with -1, so a slot the
kernels fail to write shows, and rows are padded with NaN guard words: nothing past P may count.

Widths, with B = mx_consensus_cols() = 4096 columns per work item (a workgroup's four waves take 1024 each,
in passes of 64 lanes x 1 to 8 columns, by row class and element size): 1-5 (the element path), 255-257,
1023 / 1025 (a wave's seam), B - 1, B, B + 1, 2B + 3, and 257 B + 5 -- the finishing kernel's lanes each add
more than one partial only past 64 B columns and more than four past 256 B.  Row counts 1, 2, 3, 8, 9, 16, 17,
33, 64: each side of every row-class seam (8 | 16 | 32 | 64 rows held per lane) and divisors that are no
power of two (a true division, not a multiplication by 1/n)."""
import ctypes

import numpy as np
import pytest

import bf16ref
import clipref
import consref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
NAN16 = np.uint16(0x7FC0)
NS = [1, 2, 3, 8, 9, 16, 17, 33, 64]


class _Launcher:
    """mx_consensus on a [nseg][n] pointer table (numpy int64), the tables and outputs built once; run()
    refills the workspace with NaN and the outputs with -1 and returns (dist, stats) as numpy float32"""

    def __init__(self, pkg, ptrs, lens, elem):
        E, L = pkg.engine, pkg.lib
        self.pkg = pkg
        ptrs = np.ascontiguousarray(ptrs, np.int64)
        lens = np.ascontiguousarray(lens, np.int64)
        nseg, n = ptrs.shape
        chunks = ctypes.c_int64(-1)
        nbytes = L.mx_consensus_layout(lens.ctypes.data, nseg, n, ctypes.byref(chunks))
        assert nbytes == 8 * (n + 1) * chunks.value
        self.tab, self.sl = torch.from_numpy(ptrs).cuda(), torch.from_numpy(lens).cuda()
        self.work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
        self.dist = torch.empty(n, dtype=torch.float32, device="cuda")
        self.stats = torch.empty(2, dtype=torch.float32, device="cuda")
        self.call = E.ConsensusCall(self.tab.data_ptr(), self.sl.data_ptr(), self.work.data_ptr(), self.dist.data_ptr(),
                                    self.stats.data_ptr(), chunks.value, nseg, n, elem, 0)

    def run(self):
        L = self.pkg.lib
        self.work.fill_(float("nan"))
        self.dist.fill_(-1.0)
        self.stats.fill_(-1.0)
        assert L.mx_consensus(ctypes.addressof(self.call), self.pkg._lib.stream_ptr()) == 0, L.mx_last_error()
        torch.cuda.synchronize()
        return self.dist.cpu().numpy(), self.stats.cpu().numpy()


def _dev(host, elem):
    """a host array (float32, or uint16 bfloat16 bit patterns) on the device; 16-byte aligned rows"""
    t = torch.from_numpy(host if elem == 4 else host.view(np.int16)).cuda()
    assert t.data_ptr() % 16 == 0 and (host.shape[1] * elem) % 16 == 0
    return t


def _padded(vals, elem):
    """[n, P] values in rows padded to a multiple of 8 columns, at least 8 NaN guard words after each"""
    n, P = vals.shape
    ld = (P + 8 + 7) // 8 * 8
    host = np.full((n, ld), np.nan, F32) if elem == 4 else np.full((n, ld), NAN16, np.uint16)
    host[:, :P] = vals
    return host


def _rows(pkg, vals, elem, keep=None):
    """one segment of P columns, row r at its padded row: (dist, stats)"""
    t = _dev(_padded(vals, elem), elem)
    ptrs = np.array([[t[r].data_ptr() for r in range(vals.shape[0])]], np.int64)
    la = _Launcher(pkg, ptrs, [vals.shape[1]], elem)
    if keep is not None:
        keep.extend([t, la])
    return la.run()


def _wide(vals, elem):
    return np.asarray(vals, F32) if elem == 4 else bf16ref.upcast(vals)


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _check(got, vals, elem, where):
    """finite and within 1 ulp of consref, every output"""
    dist, stats = got
    wd, ws = consref.consref(_wide(vals, elem))
    assert np.isfinite(dist).all() and np.isfinite(stats).all(), where
    assert (dist >= 0).all() and (stats >= 0).all(), where
    ud, us = clipref.ulp_diff(dist, wd), clipref.ulp_diff(stats, ws)
    assert int(ud.max()) <= 1 and int(us.max()) <= 1, (where, ud.tolist(), us.tolist())


def _widths(pkg):
    B = pkg.lib.mx_consensus_cols()
    assert B == 4096
    return [1, 3, 4, 5, 255, 256, 257, 1023, 1025, B - 1, B, B + 1, 2 * B + 3]


@pytest.mark.parametrize("kind", consref.KINDS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("elem", [4, 2])
def test_widths(pkg, elem, n, kind):
    rng = np.random.default_rng([elem, n, len(kind)])
    for P in _widths(pkg):
        vals = consref.make_rows(rng, n, P, kind, elem)
        _check(_rows(pkg, vals, elem), vals, elem, f"elem {elem} n {n} {kind} P {P}")


@pytest.mark.parametrize("elem", [4, 2])
def test_long_rows(pkg, elem):
    """257 B + 5 columns, 8 rows: every loop of both kernels runs more than once; and again on a grid of 3
    workgroups, bit-identical"""
    B = pkg.lib.mx_consensus_cols()
    n, P = 8, 257 * B + 5
    vals = consref.make_rows(np.random.default_rng(elem), n, P, "noise", elem)
    keep = []
    got = _rows(pkg, vals, elem, keep)
    _check(got, vals, elem, f"elem {elem}")
    saved = pkg.engine.consensus_tuning()
    try:
        pkg.engine.set_consensus_tuning(grid=3)
        again = keep[1].run()
    finally:
        pkg.engine.set_consensus_tuning(**saved)
    assert _same(got, again)


@pytest.mark.parametrize("n", [16, 32, 64])
@pytest.mark.parametrize("elem", [4, 2])
def test_larger_row_classes_under_every_knob(pkg, elem, n):
    """the largest row count of each larger class at 5 B + 77 columns: right, and the same bits on 1, 7 and
    65536 workgroups and with 1 and 64 workgroups per CU"""
    B = pkg.lib.mx_consensus_cols()
    P = 5 * B + 77
    vals = consref.make_rows(np.random.default_rng([elem, n]), n, P, "ulps", elem)
    keep = []
    base = _rows(pkg, vals, elem, keep)
    _check(base, vals, elem, f"elem {elem} n {n}")
    saved = pkg.engine.consensus_tuning()
    try:
        for knobs in ({"grid": 1}, {"grid": 7}, {"grid": 65536}, {"blocks_per_cu": 1}, {"blocks_per_cu": 64}):
            pkg.engine.set_consensus_tuning(**saved)
            pkg.engine.set_consensus_tuning(**knobs)
            assert _same(base, keep[1].run()), knobs
    finally:
        pkg.engine.set_consensus_tuning(**saved)


@pytest.mark.parametrize("n", [1, 3, 8, 33, 64])
@pytest.mark.parametrize("elem", [4, 2])
def test_identical_rows_give_exactly_zero(pkg, elem, n):
    """k * x is exact in fp64 for k <= 64 and (n * x) / n = x: every distance is 0.0, not -0.0, and the norm
    of the mean is the row's norm"""
    B = pkg.lib.mx_consensus_cols()
    P = 2 * B + 3
    rng = np.random.default_rng([elem, n, 7])
    row = (rng.standard_normal(P) * np.exp(rng.uniform(-20, 20, P))).astype(F32)
    if elem == 4:
        row[:3] = F32([1e-42, -3.4028235e38, -0.0])           # a denormal, the largest magnitude, -0.0
    else:
        row = bf16ref.rne_bf16(row)
        row[:3] = [0x0001, 0xFF7F, 0x8000]
    assert np.isfinite(_wide(row, elem)).all()
    dist, stats = _rows(pkg, np.tile(row, (n, 1)), elem)
    assert (dist == 0).all() and not np.signbit(dist).any()
    assert stats[0] == 0 and not np.signbit(stats[0])
    want = clipref.grad_norm_ref(_wide(row, elem)[None])
    assert np.isfinite(stats[1]) and int(clipref.ulp_diff(stats[1:], want).max()) <= 1


@pytest.mark.parametrize("n", [2, 3, 4, 8, 17])
@pytest.mark.parametrize("elem", [4, 2])
def test_one_displaced_element_is_the_closed_form(pkg, elem, n):
    """Identical rows of small integers, one row moved by 3.0 in ONE column -- column 0, column P - 1, each side
    of every 256-column boundary up to 2 B + 3: that row is 3 (n - 1) / n from the mean, every other row 3 / n,
    and the consensus distance is 3 sqrt(n - 1) / n, all within 1 ulp; exactly for n = 2, 4, 8, where 3 / n and
    its square are exact."""
    B = pkg.lib.mx_consensus_cols()
    P = 2 * B + 3
    rng = np.random.default_rng([elem, n, 11])
    base = rng.integers(-2, 3, P).astype(F32)                 # x and x + 3 are exact in bfloat16 too
    enc = (lambda v: np.asarray(v, F32)) if elem == 4 else (lambda v: bf16ref.rne_bf16(np.asarray(v, F32)))
    host = _padded(np.tile(enc(base), (n, 1)), elem)
    t = _dev(host, elem)
    la = _Launcher(pkg, np.array([[t[r].data_ptr() for r in range(n)]], np.int64), [P], elem)
    tt = t if elem == 4 else t.view(torch.bfloat16)
    pos = sorted({0, P - 1} | {k - 1 for k in range(256, P, 256)} | {k for k in range(256, P, 256)})
    far, near = F32(3.0 * (n - 1) / n), F32(3.0 / n)
    xi = F32(3.0 * np.sqrt(np.float64(n - 1)) / n)
    for i, c in enumerate(pos):
        r = i % n
        tt[r, c] = float(base[c]) + 3.0
        dist, stats = la.run()
        tt[r, c] = float(base[c])
        want = np.full(n, near, F32)
        want[r] = far
        assert np.isfinite(dist).all() and np.isfinite(stats).all()
        if n in (2, 4, 8):
            assert np.array_equal(dist, want), (c, r, dist.tolist())
        assert int(clipref.ulp_diff(dist, want).max()) <= 1, (c, r, dist.tolist())
        assert int(clipref.ulp_diff(stats[:1], xi).max()) <= 1, (c, r, float(stats[0]))
    dist, stats = la.run()                                    # every element restored: consensus again
    assert (dist == 0).all() and stats[0] == 0


@pytest.mark.parametrize("n", [5, 33])
@pytest.mark.parametrize("delta", [0, 1, 2])
@pytest.mark.parametrize("elem", [4, 2])
def test_unaligned_two_segment_tables(pkg, elem, delta, n):
    """Two segments (5 and B + 3 elements) at pointers 0 / 4 / 8 bytes (fp32) or 0 / 2 / 8 bytes (bf16) past a
    16-byte boundary, NaN guard words before and after every row of both: the figures are finite and right,
    and the buffer is unchanged."""
    B = pkg.lib.mx_consensus_cols()
    d = delta if elem == 4 else (0, 1, 4)[delta]
    lens = [5, B + 3]
    off = [8 + d, 32 + d]
    stride = (off[1] + lens[1] + 16 + 7) // 8 * 8
    vals = consref.make_rows(np.random.default_rng([elem, delta, n]), n, sum(lens), "noise", elem)
    host = np.full((n, stride), np.nan, F32) if elem == 4 else np.full((n, stride), NAN16, np.uint16)
    host[:, off[0]:off[0] + lens[0]] = vals[:, :lens[0]]
    host[:, off[1]:off[1] + lens[1]] = vals[:, lens[0]:]
    t = _dev(host, elem)
    ptrs = np.array([[t[r].data_ptr() + elem * off[s] for r in range(n)] for s in range(2)], np.int64)
    assert all(int(p) % 16 == (elem * d) % 16 for p in ptrs.reshape(-1))
    la = _Launcher(pkg, ptrs, lens, elem)
    assert la.call.chunks == 3
    _check(la.run(), vals, elem, f"elem {elem} delta {d} n {n}")
    bits = np.uint32 if elem == 4 else np.uint16
    assert np.array_equal(t.cpu().numpy().view(host.dtype).view(bits), host.view(bits))


@pytest.mark.parametrize("n", [6, 40])
@pytest.mark.parametrize("elem", [4, 2])
def test_special_values(pkg, elem, n):
    """A NaN element, and an Inf element, make the mean of their column non-finite and with it EVERY output.
    Elements of +-the largest finite value stay finite (the squares are fp64) and match consref.  Rows of
    denormals are counted, not flushed: a non-zero distance."""
    P = 4099
    rng = np.random.default_rng([elem, n, 20])
    g = (rng.standard_normal((n, P)) / 64).astype(F32)
    enc = (lambda v: v) if elem == 4 else bf16ref.rne_bf16
    nan, inf = (F32(np.nan), F32(-np.inf)) if elem == 4 else (np.uint16(0xFFC1), np.uint16(0xFF80))
    big = F32([3.4028235e38, -3.4028235e38]) if elem == 4 else np.array([0x7F7F, 0xFF7F], np.uint16)
    for what, (r, c) in ((nan, (n - 1, 1234)), (inf, (0, P - 1))):
        vals = enc(g).copy()
        vals[r, c] = what
        dist, stats = _rows(pkg, vals, elem)
        assert not np.isfinite(dist).any() and not np.isfinite(stats).any()
    vals = enc(g).copy()
    vals[1, 5], vals[n - 1, 5] = big[0], big[1]               # opposite signs in one column: distances of 3.4e38
    vals[:, 4098] = big[1]                                    # the same in every row: a mean of -3.4e38, no distance
    got = _rows(pkg, vals, elem)
    _check(got, vals, elem, "largest finite values")
    assert got[0][1] > 1e38 and got[1][0] > 1e37 and got[1][1] > 1e38
    den = np.zeros((n, P), F32 if elem == 4 else np.uint16)
    den[0, [0, 77, 4097]] = F32([1e-42, -3e-41, 1.4e-45]) if elem == 4 else np.array([0x0001, 0x8003, 0x0040], np.uint16)
    got = _rows(pkg, den, elem)
    _check(got, den, elem, "denormals")
    assert (got[0] > 0).all() and got[1][0] > 0 and got[1][1] > 0


@pytest.mark.parametrize("elem", [4, 2])
def test_launches_reproduce_and_every_distance_depends_on_every_row(pkg, elem):
    """Two launches give the same bits.  Unlike the gradient norm's rows, the distances are NOT independent:
    changing row 3 moves the mean, so every dist changes (and both stats)."""
    B = pkg.lib.mx_consensus_cols()
    n, P = 8, 5 * B + 77
    rng = np.random.default_rng(elem + 10)
    vals = consref.make_rows(rng, n, P, "spread", elem)
    keep = []
    base = _rows(pkg, vals, elem, keep)
    assert _same(base, keep[1].run())
    other = vals.copy()
    other[3] = consref.make_rows(rng, 1, P, "spread", elem)[0]
    moved = _rows(pkg, other, elem)
    _check(moved, other, elem, "moved")
    assert (moved[0].view(np.uint32) != base[0].view(np.uint32)).all()
    assert (moved[1].view(np.uint32) != base[1].view(np.uint32)).all()


# ------------------------------------------------------------------ groups
def _topo(pkg, T=4):
    from conftest import Topo
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    return Topo(partner, 2 / 7, np.ones((T, partner.shape[0]), np.uint8))          # every matching active


def _figures(grp):
    torch.cuda.synchronize()
    return grp.consensus_dists.cpu().numpy(), grp.consensus_stats.cpu().numpy()


def test_group_fp32_round_contracts(pkg):
    """8 workers x 70,001 N(0, 1): consensus_distance() is consref of the rows; one round with every matching
    active brings the workers strictly closer and leaves the mean where it was -- the mixing matrix is doubly
    stochastic, and at most M + 1 <= 9 fp32 roundings per element move ||mean|| by less than 9 * 2^-24 =
    5.4e-7 relative (asserted: 1e-5); the new figures are consref of the new rows."""
    P = 70_001
    grp = pkg.VirtualWorkerGroup(_topo(pkg), numel=P)
    x = np.random.default_rng(1).standard_normal((8, P)).astype(F32)
    grp.rows.copy_(torch.from_numpy(x))
    out = grp.consensus_distance()
    assert out is grp.consensus_dists and out.shape == (8,) and out.dtype == torch.float32 and out.is_cuda
    assert grp.consensus_stats.shape == (2,) and grp.consensus_stats.dtype == torch.float32
    before = _figures(grp)
    _check(before, x, 4, "before")
    grp.communicate()
    grp.consensus_distance()
    after = _figures(grp)
    _check(after, grp.rows.cpu().numpy(), 4, "after")
    assert after[1][0] < before[1][0]
    assert abs(float(after[1][1]) - float(before[1][1])) < 1e-5 * float(before[1][1])


def test_group_after_the_in_place_mean(pkg):
    """harness.sync_rows (mx_mean_rows_to in place) makes the rows identical: the consensus distance is 0.0"""
    P = 70_001
    grp = pkg.VirtualWorkerGroup(_topo(pkg), numel=P)
    grp.rows.copy_(torch.from_numpy(np.random.default_rng(2).standard_normal((8, P)).astype(F32)))
    grp.consensus_distance()
    assert _figures(grp)[1][0] > 0
    pkg.harness.sync_rows(grp.rows)
    grp.consensus_distance()
    dist, stats = _figures(grp)
    assert (dist == 0).all() and stats[0] == 0 and stats[1] > 0


def test_group_bf16_rows_and_masters(pkg):
    """bfloat16 rows are measured by default; once master weights are attached the fp32 masters are, of="rows"
    still measures the bfloat16 rows, and of="masters" without masters is an MXError"""
    P = 4_099
    grp = pkg.VirtualWorkerGroup(_topo(pkg), numel=P, dtype=torch.bfloat16)
    bits = bf16ref.rne_bf16(np.random.default_rng(3).standard_normal((8, P)).astype(F32))
    grp.rows.copy_(torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16))
    with pytest.raises(pkg.MXError, match="master"):
        grp.consensus_distance(of="masters")
    with pytest.raises(ValueError):
        grp.consensus_distance(of="gradients")
    grp.consensus_distance()
    _check(_figures(grp), bits, 2, "bf16 rows")
    grp.attach_sgd(master_weights=True)
    masters = (bf16ref.upcast(bits) + F32(1e-3) * np.random.default_rng(4).standard_normal((8, P))).astype(F32)
    grp.master_rows.copy_(torch.from_numpy(masters))
    grp.consensus_distance()
    default = _figures(grp)
    _check(default, masters, 4, "masters by default")
    grp.consensus_distance(of="masters")
    assert _same(default, _figures(grp))
    grp.consensus_distance(of="rows")
    rows = _figures(grp)
    _check(rows, bits, 2, "of=rows")
    assert not _same(default, rows)


def test_choco_group(pkg):
    P = 4_099
    grp = pkg.ChocoWorkerGroup(_topo(pkg), numel=P, ratio=0.9, consensus_lr=0.3)
    x = np.random.default_rng(5).standard_normal((8, P)).astype(F32)
    grp.rows.copy_(torch.from_numpy(x))
    out = grp.consensus_distance()
    assert out is grp.consensus_dists and out.shape == (8,)
    _check(_figures(grp), x, 4, "choco")


def test_two_rank_layouts_refuse(pkg):
    """the mean needs every worker's rows on this GPU"""
    from conftest import LoopbackHub
    topo = _topo(pkg)
    grp = pkg.VirtualWorkerGroup(topo, numel=100, nranks=2, rank=0, comm=LoopbackHub(2).comm(0))
    with pytest.raises(NotImplementedError, match="every worker's rows on this GPU"):
        grp.consensus_distance()
    ch = pkg.ChocoWorkerGroup(topo, numel=100, ratio=0.9, consensus_lr=0.3, nranks=2, rank=0,
                              comm=LoopbackHub(2).comm(0))
    with pytest.raises(NotImplementedError, match="every worker's rows on this GPU"):
        ch.consensus_distance()


def test_graph_capture_with_device_round(pkg):
    """device_round and consensus_distance captured in one HIP graph (one stream: no parallel branches, the
    default queue count), replayed three times: the figures are consref of the rows after the third round"""
    P = 70_001
    grp = pkg.VirtualWorkerGroup(_topo(pkg, T=8), numel=P)
    x = np.random.default_rng(6).standard_normal((8, P)).astype(F32)
    grp.rows.copy_(torch.from_numpy(x))
    grp.consensus_distance()                                  # builds the state: nothing is allocated under capture
    first = _figures(grp)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            grp.device_round()
            grp.consensus_distance()
    torch.cuda.synchronize()
    assert np.array_equal(grp.rows.cpu().numpy(), x) and _same(first, _figures(grp))      # capture ran nothing
    xi = [float(first[1][0])]
    for _ in range(3):
        g.replay()
        xi.append(float(_figures(grp)[1][0]))
    assert int(grp.iter_dev.item()) == 3 and xi[0] > xi[1] > xi[2] > xi[3]
    _check(_figures(grp), grp.rows.cpu().numpy(), 4, "after three replays")


# ------------------------------------------------------------------ harness
def _args(pkg, **kw):
    base = dict(size=8, epoch=1, bs=16, budget=0.5, graphid=0, lr=0.1)
    base.update(kw)
    return pkg.harness.HarnessArgs(**base)


@pytest.mark.parametrize("mode", ["eager", "batched", "graph", "fused", "choco"])
def test_trainer_logs_the_consensus_distance(pkg, mode):
    """consensus_every=2 over 4 batches: two measurements of length n + 2, finite, the stats carry them"""
    H = pkg.harness
    kw = {"eager": {}, "batched": {"batched": True}, "graph": {"batched": True, "graph": True},
          "fused": {"fused_sgd": True}, "choco": {}}[mode]
    args = _args(pkg, compress=True, budget=1.0, ratio=0.9) if mode == "choco" else _args(pkg, momentum=0.0)
    tr = H.VirtualTrainer(args, H.model_factory(args), n_batches=4, consensus_every=2, **kw)
    stats = tr.train_epoch()
    assert len(tr.consensus_log) == 2
    for row in tr.consensus_log:
        assert row.shape == (10,) and row.dtype == torch.float32 and row.device.type == "cpu"
        assert torch.isfinite(row).all() and (row >= 0).all() and row[-1] > 0
        assert abs(float(row[-2]) - float(row[:8].double().pow(2).mean().sqrt())) <= 1e-6 * float(row[-2]) + 1e-30
    for r, s in enumerate(stats):
        assert s["consensus"] == float(tr.consensus_log[-1][-2])
        assert s["consensus_dist"] == float(tr.consensus_log[-1][r])
    # the last measurement followed the last round: it is consref of the rows as they are now
    dist, st = consref.consref(tr.group.rows.float().cpu().numpy())
    last = tr.consensus_log[-1].numpy()
    assert int(clipref.ulp_diff(last[:8], dist).max()) <= 1 and int(clipref.ulp_diff(last[8:], st).max()) <= 1


def test_trainer_default_measures_nothing(pkg, tmp_path):
    """consensus_every=None (the default): the stats keys and the Recorder's files are what they were"""
    import os
    H = pkg.harness
    args = _args(pkg, save=True, savePath=str(tmp_path) + os.sep)
    tr = H.VirtualTrainer(args, H.model_factory(args), n_batches=2)
    stats = tr.train_epoch()
    tr.finish()
    assert tr.consensus_log == [] and tr.consensus_every is None
    assert set(stats[0]) == {"worker", "loss", "train_acc", "comp_time", "comm_time"}
    assert tr.group.consensus_dists is None
    files = [f for _, _, fs in os.walk(tmp_path) for f in fs]
    logs = sorted({f.rsplit("-", 1)[1] for f in files if f.endswith(".log")})
    assert logs == sorted(s + ".log" for s in ("recordtime", "time", "comptime", "commtime", "acc", "losses", "tacc"))
    assert len(files) == 7 * 8 + 1 and not any("consensus" in f for f in files)
    with pytest.raises(ValueError):
        H.VirtualTrainer(args, H.model_factory(args), n_batches=2, consensus_every=0)
