"""The consensus distance, the parts that need no GPU: the specification in tests/consref.py on cases worked
by hand and against another summation tree, and the C ABI of csrc/consensus.hip (workspace size, knobs,
host-side refusals, the call record's size)."""
import ctypes
import importlib

import numpy as np
import pytest

import bf16ref
import clipref
import consref

torch = pytest.importorskip("torch")

F32 = np.float32


def test_hand_computed():
    """rows [0, 0] and [2, 0]: the mean is [1, 0], both distances 1, consensus distance 1, ||mean|| 1"""
    dist, stats = consref.consref(F32([[0, 0], [2, 0]]))
    assert dist.dtype == F32 and stats.dtype == F32
    assert dist.tolist() == [1.0, 1.0] and stats.tolist() == [1.0, 1.0]
    # 3 rows, one column: 0, 0, 3 -> mean 1: distances 1, 1, 2; sqrt((1 + 1 + 4) / 3) = sqrt(2)
    dist, stats = consref.consref(F32([[0], [0], [3]]))
    assert dist.tolist() == [1.0, 1.0, 2.0] and stats[0] == F32(np.sqrt(2.0)) and stats[1] == 1.0
    # bfloat16 bit patterns are widened exactly: 0x4000 = 2.0
    dist, stats = consref.consref_bf16(np.array([[0, 0], [0x4000, 0]], np.uint16))
    assert dist.tolist() == [1.0, 1.0] and stats.tolist() == [1.0, 1.0]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 33, 64])
def test_identical_rows_give_zero(n):
    """k * x is exact in fp64 for k <= 64 and (n * x) / n = x: exactly 0.0, not -0.0, whatever x holds"""
    rng = np.random.default_rng(n)
    row = (rng.standard_normal(1001) * np.exp(rng.uniform(-20, 20, 1001))).astype(F32)
    row[:4] = F32([1e-42, -3.4028235e38, 3.4028235e38, -0.0])
    dist, stats = consref.consref(np.tile(row, (n, 1)))
    assert (dist == 0).all() and not np.signbit(dist).any()
    assert stats[0] == 0 and not np.signbit(stats[0])
    assert clipref.ulp_diff(stats[1:], clipref.grad_norm_ref(row[None])).max() <= 1


def test_translation_leaves_the_distances():
    """x_r + t has the same deviations as x_r up to the fp32 rounding of the translated rows: with |x| ~ 1
    and |t| ~ 1 each element moves by at most 2^-23 absolute (one rounding of a value below 4), a relative
    change of the distances of a few 2^-23 / mean|d|; 1e-5 bounds it generously, and the norm of the mean
    moves by the translation"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((8, 4099)).astype(F32)
    t = rng.standard_normal(4099).astype(F32)
    d0, s0 = consref.consref(x)
    d1, s1 = consref.consref((x + t).astype(F32))
    assert np.allclose(d0, d1, rtol=1e-5, atol=0) and np.isclose(s0[0], s1[0], rtol=1e-5, atol=0)
    assert abs(float(s1[1]) - float(s0[1])) > 1.0


def test_special_values():
    x = np.ones((3, 5), F32)
    x[1, 2] = np.nan
    dist, stats = consref.consref(x)
    assert not np.isfinite(dist).any() and not np.isfinite(stats).any()
    x[1, 2] = np.inf
    dist, stats = consref.consref(x)
    assert not np.isfinite(dist).any() and not np.isfinite(stats).any()
    x[1, 2] = 3.4028235e38
    x[2, 2] = -3.4028235e38
    dist, stats = consref.consref(x)
    assert np.isfinite(dist).all() and np.isfinite(stats).all() and dist[1] > 2e38
    den = np.zeros((2, 4), F32)
    den[0, 1] = 1e-42
    dist, stats = consref.consref(den)
    assert (dist > 0).all() and stats[0] > 0


def _other_tree(x):
    """the same column arithmetic, the column sums in another order: 4096-column chunks, within a chunk 256
    interleaved lanes summed one after the other, then the lanes, then the chunks"""
    x64 = np.asarray(x, F32).astype(np.float64)
    n, P = x64.shape
    s = x64[0].copy()
    for r in range(1, n):
        s = s + x64[r]
    m = s / np.float64(n)

    def tree(v):
        pad = np.zeros((P + 4095) // 4096 * 4096)
        pad[:P] = v
        lanes = pad.reshape(-1, 16, 256)
        acc = np.zeros((lanes.shape[0], 256))
        for k in range(16):
            acc = acc + lanes[:, k, :]
        per_chunk = np.zeros(lanes.shape[0])
        for l in range(256):
            per_chunk = per_chunk + acc[:, l]
        out = 0.0
        for v in per_chunk:
            out = out + v
        return out

    D = [tree((x64[r] - m) ** 2) for r in range(n)]
    total = D[0]
    for r in range(1, n):
        total = total + D[r]
    return (np.sqrt(np.array(D)).astype(F32),
            np.array([np.sqrt(total / np.float64(n)), np.sqrt(tree(m * m))]).astype(F32))


@pytest.mark.parametrize("kind", consref.KINDS)
@pytest.mark.parametrize("n", [1, 3, 8, 17, 64])
def test_another_summation_tree_is_within_one_ulp(n, kind):
    """what the 1-ulp tolerance of the GPU tests rests on, on the three input kinds they use"""
    x = consref.make_rows(np.random.default_rng([n, len(kind)]), n, 30_007, kind)
    assert np.isfinite(x).all()
    d0, s0 = consref.consref(x)
    d1, s1 = _other_tree(x)
    assert clipref.ulp_diff(d0, d1).max() <= 1 and clipref.ulp_diff(s0, s1).max() <= 1
    if n == 1:
        assert (d0 == 0).all() and s0[0] == 0


def test_workspace_size(pkg):
    L = pkg.lib
    B = L.mx_consensus_cols()
    assert B == 4096
    chunks = ctypes.c_int64(-1)
    lens = np.array([5, B + 3], np.int64)
    nbytes = L.mx_consensus_layout(lens.ctypes.data, 2, 8, ctypes.byref(chunks))
    assert chunks.value == 3 and nbytes == 8 * (8 + 1) * 3
    lens = np.array([0, 1, B, B + 1, 5, 3 * B - 1], np.int64)
    nbytes = L.mx_consensus_layout(lens.ctypes.data, len(lens), 64, ctypes.byref(chunks))
    assert chunks.value == 0 + 1 + 1 + 2 + 1 + 3 and nbytes == 8 * 65 * 8
    one = np.array([25_600_000], np.int64)
    assert L.mx_consensus_layout(one.ctypes.data, 1, 8, ctypes.byref(chunks)) == 8 * 9 * 6250 and chunks.value == 6250
    assert L.mx_consensus_layout(one.ctypes.data, 1, 1, None) == 8 * 2 * 6250
    assert L.mx_consensus_layout(None, 1, 8, None) < 0 and b"mx_consensus_layout" in L.mx_last_error()
    assert L.mx_consensus_layout(one.ctypes.data, 0, 8, None) < 0
    assert L.mx_consensus_layout(one.ctypes.data, 1, 0, None) < 0
    assert L.mx_consensus_layout(one.ctypes.data, 1, 65, None) < 0 and b"n_local" in L.mx_last_error()
    neg = np.array([4, -1], np.int64)
    assert L.mx_consensus_layout(neg.ctypes.data, 2, 8, None) < 0 and b"negative" in L.mx_last_error()


def test_knobs_round_trip(pkg):
    E = importlib.import_module(pkg.__name__ + ".engine")
    L = pkg.lib
    saved = E.consensus_tuning()
    assert set(saved) == {"blocks_per_cu", "grid"}
    try:
        E.set_consensus_tuning(blocks_per_cu=3, grid=17)
        assert E.consensus_tuning() == {"blocks_per_cu": 3, "grid": 17}
        assert L.mx_consensus_get(b"grid") == 17
        for key, bad in ((b"blocks_per_cu", 0), (b"blocks_per_cu", 65), (b"grid", -1), (b"grid", 65537)):
            assert L.mx_consensus_set(key, bad) == -1
        assert E.consensus_tuning() == {"blocks_per_cu": 3, "grid": 17}
    finally:
        E.set_consensus_tuning(**saved)
    assert E.consensus_tuning() == saved
    assert L.mx_consensus_set(b"nope", 1) == -1 and b"unknown key" in L.mx_last_error()
    assert L.mx_consensus_get(b"nope") == -1 and b"unknown key" in L.mx_last_error()
    assert L.mx_consensus_set(None, 1) == -1 and L.mx_consensus_get(None) == -1
    with pytest.raises(pkg.MXError):
        E.set_consensus_tuning(nope=1)


def test_call_record_and_refusals_need_no_gpu(pkg):
    """every host-side refusal returns MX_ERR_INVALID before anything touches a device (fake addresses)"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    L = pkg.lib
    assert ctypes.sizeof(E.ConsensusCall) == 64
    assert [f[0] for f in E.ConsensusCall._fields_] == ["x_ptrs_dev", "seg_len_dev", "work_dev", "dist_dev", "stats_dev",
                                                        "chunks", "nseg", "n_local", "elem_size", "pad_"]
    fake = 1 << 40

    def rc(**kw):
        a = dict(x_ptrs_dev=fake, seg_len_dev=fake, work_dev=fake, dist_dev=fake, stats_dev=fake, chunks=1, nseg=1,
                 n_local=8, elem_size=4, pad_=0)
        a.update(kw)
        c = E.ConsensusCall(**a)
        return L.mx_consensus(ctypes.addressof(c), None)

    assert L.mx_consensus(None, None) == -1 and b"null" in L.mx_last_error()
    for k in ("x_ptrs_dev", "seg_len_dev", "work_dev", "dist_dev", "stats_dev"):
        assert rc(**{k: None}) == -1 and b"null" in L.mx_last_error(), k
    for es in (0, 1, 3, 8):
        assert rc(elem_size=es) == -1 and b"elem_size" in L.mx_last_error()
    for n in (0, -1, 65):
        assert rc(n_local=n) == -1 and b"n_local" in L.mx_last_error()
    assert rc(nseg=0) == -1 and rc(chunks=-1) == -1 and b"chunks" in L.mx_last_error()


def test_bf16_widening_is_exact():
    """consref_bf16 is consref of the widened values: the same figures as the fp32 rows holding them"""
    rng = np.random.default_rng(9)
    bits = bf16ref.rne_bf16(rng.standard_normal((5, 777)).astype(F32))
    a, b = consref.consref_bf16(bits), consref.consref(bf16ref.upcast(bits))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
