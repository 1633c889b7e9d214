"""Every Choco kernel variant at the smallest shapes where it can still go wrong: one element, one chunk
less / exactly / more than one element (4095, 4096, 4097), several chunks with a partial last one (3 * 4096 + 5)
and more chunks than one wave owns (40 001); k = 1, about 1 % and P; rows that start on a 16-byte boundary
and one float past it.  Top-k against the CPU oracle (indices, and values as uint32, bit for bit), the apply
pass against the oracle's Choco round (x, x_hat, s bit for bit)."""
import numpy as np
import pytest

from conftest import Topo

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = (1, 4095, 4096, 4097, 3 * 4096 + 5, 40_001)
RATIOS = (1.0, 0.99, 0.0)                      # k = 1, max(1, P // 100), P
VARIANTS = [{}, {"compact_store": 0}, {"compact_pf2": 1}, {"compact_wave": 1}, {"compact_wave": 3}, {"select": 1},
            {"sample_stride": 1}, {"sample_stride": 16, "cand_chunks": 1}]      # cand_chunks 1: 3 blocks at the barrier
# three workers, each pair matched once
PARTNER3 = [[1, 0, -1], [-1, 2, 1], [2, -1, 0]]

_inputs = {}                                   # (seed, P) -> row; (seed, P, k) -> the oracle's (values, indices)


def _row(O, seed, P):
    """uniform [-1, 1) with 22 % of the elements tied at magnitude 0.995, both signs: about 0.4 % of the keys
    lie above the ties, so the k = 1 % threshold is the tied key and only its lowest indices are taken.  From
    piece 16 on, every 16th 1024-element piece holds no ties and is scaled by 1.06 instead -- pieces a sampling
    stride of 16 reads, so at 40 001 elements the sampled floor comes out above the ties, fewer than k keys
    are kept and the fallback compaction (with its row barrier) has to run."""
    if (seed, P) not in _inputs:
        y = O.synth(seed, P)
        x = y.copy()
        x[::7] = np.float32(0.995)
        x[::11] = np.float32(-0.995)
        piece = np.arange(P) // 1024
        big = (piece % 16 == 0) & (piece > 0)
        x[big] = y[big] * np.float32(1.06)
        x.setflags(write=False)
        _inputs[seed, P] = x
    return _inputs[seed, P]


def _want(O, seed, P, k):
    if (seed, P, k) not in _inputs:
        _inputs[seed, P, k] = O.topk_abs(_row(O, seed, P), k)
    return _inputs[seed, P, k]


def _fallbacks(pkg, grp):
    """fallback compactions of each row of the group so far (mx_topk_stats)"""
    out = np.zeros(5 * grp.n_local, np.int64)
    pkg._lib.check(pkg.lib.mx_topk_stats(grp.work.data_ptr(), grp.work_ld, grp.n_local, grp.numel, out.ctypes.data,
                                         None))
    return out[1::5].tolist()


class _knobs:
    def __init__(self, pkg, knobs):
        self.pkg, self.knobs = pkg, knobs

    def __enter__(self):
        L = self.pkg.lib
        self.saved = {k: int(L.mx_topk_get(k.encode())) for k in self.knobs}
        for k, v in self.knobs.items():
            self.pkg._lib.check(L.mx_topk_set(k.encode(), v))

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.pkg.lib.mx_topk_set(k.encode(), v)


@pytest.mark.parametrize("knobs", VARIANTS, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()) or "defaults")
@pytest.mark.parametrize("P", SIZES)
def test_topk_small_shapes(pkg, O, P, knobs):
    """get_top_k (one row: the ballot-ranked kernels) from an aligned and an unaligned start, and a 3-row
    ChocoWorkerGroup.compress (the scan-ranked kernels, x_hat = 0), for every k, under one variant."""
    ks = sorted({O.topk_k(P, r): r for r in RATIOS}.items())
    with _knobs(pkg, knobs):
        for k, ratio in ks:
            ov, oi = _want(O, 100, P, k)
            big = torch.zeros(P + 8, dtype=torch.float32, device="cuda")
            for off in (4, 5):                       # the allocation is 256-byte aligned
                xv = big[off:off + P]
                xv.copy_(torch.tensor(_row(O, 100, P)))
                assert (xv.data_ptr() % 16 == 0) == (off == 4)
                v, i = pkg.get_top_k(xv, ratio)
                assert i.numel() == k
                assert np.array_equal(i.cpu().numpy(), oi), (k, off)
                assert np.array_equal(v.cpu().numpy().view(np.uint32), ov.view(np.uint32)), (k, off)
            pkg.check_top_k()
            topo = Topo(PARTNER3, 1 / 3, np.ones((1, 3), np.uint8))
            grp = pkg.ChocoWorkerGroup(topo, numel=P, ratio=ratio, consensus_lr=0.1)
            assert grp.k == k and grp.n_local == 3
            for r in range(3):
                grp.rows[r].copy_(torch.tensor(_row(O, 100 + r, P)))
            grp.compress(0)
            grp.check_topk()
            if knobs.get("sample_stride") == 16 and P == 40_001 and 1 < k < P:
                assert _fallbacks(pkg, grp) == [1, 1, 1]     # the path this variant is here for
            for r in range(3):
                rv, ri = _want(O, 100 + r, P, k)
                v, i = grp.message(r)
                assert np.array_equal(i.cpu().numpy(), ri), (k, r)
                assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)), (k, r)


@pytest.mark.parametrize("apply_persist", [0, 1])
@pytest.mark.parametrize("apply_nt", [0, 1])
@pytest.mark.parametrize("apply_pf", [0, 1])
def test_apply_small_shapes(pkg, O, apply_pf, apply_nt, apply_persist):
    """Two rounds of a 3-row group, three whole tiles and a 5-element one, under every apply kernel form."""
    P, ratio, n = 3 * 4096 + 5, 0.9, 3
    flags = np.array([[1, 1, 1], [1, 0, 1]], np.uint8)
    topo = Topo(PARTNER3, 1 / 3, flags)
    with _knobs(pkg, {"apply_pf": apply_pf, "apply_nt": apply_nt, "apply_persist": apply_persist}):
        grp = pkg.ChocoWorkerGroup(topo, numel=P, ratio=ratio, consensus_lr=0.1)
        X = np.stack([_row(O, 100 + i, P) for i in range(n)])
        XH, S = np.zeros_like(X), np.zeros_like(X)
        grp.rows.copy_(torch.from_numpy(X))
        k = O.topk_k(P, ratio)
        for t, f in enumerate(flags):
            if t:
                D = np.stack([np.float32(0.01) * _row(O, 200 + i, P) for i in range(n)])
                X += D
                grp.rows.add_(torch.from_numpy(D).cuda())
            grp.communicate()
            O.choco_round(X, XH, S, topo.neighbors_info, f, 1 / 3, k, 0.1)
            assert np.array_equal(grp.rows.cpu().numpy().view(np.uint32), X.view(np.uint32)), f"x {t}"
            assert np.array_equal(grp.x_hat[:, :P].cpu().numpy().view(np.uint32), XH.view(np.uint32)), f"x_hat {t}"
            assert np.array_equal(grp.s[:, :P].cpu().numpy().view(np.uint32), S.view(np.uint32)), f"s {t}"
