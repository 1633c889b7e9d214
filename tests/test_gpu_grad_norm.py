"""The gradient-norm kernel (csrc/grad_norm.hip, mx_grad_norm): per-row 2-norms and clip factors on the
device, against the specification in tests/clipref.py (never the code under test).

norm_dev is within 1 fp32 ulp of clipref.grad_norm_ref (any fp64 summation order is: see clipref) and
scale_dev equals clipref.clip_scale_ref(norm_dev) bit for bit.  Every launch starts from a workspace
and outputs filled with NaN / -1, so a slot the kernels fail to write shows.

Widths: with B = mx_grad_norm_cols() = 4096 columns per work item (a workgroup's four waves take 1024
each, in 256-column (fp32) / 512-column (bf16) passes): 1-5 (the element path), 255-257, 1023 / 1025 (a
wave's seam), 4097, B - 1, B, B + 1, 2B + 3, and 257 B + 5 = 1,052,677 -- the finishing kernel's 256
threads each add more than one partial only past 256 B columns, so that is the shortest row at which
every loop of both kernels runs more than once (8 rows only: 33 such rows are 139 MB for nothing new;
the 33-row sets end at 70,001 columns, 18 work items per row)."""
import ctypes

import numpy as np
import pytest

import bf16ref
import clipref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
NAN16 = np.uint16(0x7FC0)


def _launch(pkg, ptrs, lens, elem, max_norm=1.0):
    """mx_grad_norm on a [nseg][n] pointer table (numpy int64): (norm, scale) as numpy float32"""
    E, L = pkg.engine, pkg.lib
    ptrs = np.ascontiguousarray(ptrs, np.int64)
    lens = np.ascontiguousarray(lens, np.int64)
    nseg, n = ptrs.shape
    chunks = ctypes.c_int64(-1)
    nbytes = L.mx_grad_norm_layout(lens.ctypes.data, nseg, n, ctypes.byref(chunks))
    assert nbytes == 8 * n * chunks.value
    tab, sl = torch.from_numpy(ptrs).cuda(), torch.from_numpy(lens).cuda()
    work = torch.full((max(nbytes // 8, 1),), float("nan"), dtype=torch.float64, device="cuda")
    norm = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    scale = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    call = E.GradNormCall(tab.data_ptr(), sl.data_ptr(), work.data_ptr(), norm.data_ptr(), scale.data_ptr(),
                          chunks.value, nseg, n, elem, float(F32(max_norm)))
    assert L.mx_grad_norm(ctypes.addressof(call), pkg._lib.stream_ptr()) == 0, L.mx_last_error()
    torch.cuda.synchronize()
    return norm.cpu().numpy(), scale.cpu().numpy()


def _dev(host, elem):
    """a host array (float32, or uint16 bfloat16 bit patterns) on the device; 16-byte aligned rows"""
    t = torch.from_numpy(host if elem == 4 else host.view(np.int16)).cuda()
    assert t.data_ptr() % 16 == 0 and (host.shape[1] * elem) % 16 == 0
    return t


def _rows(pkg, host, P, elem, max_norm=1.0):
    """one segment of P columns, row r at host[r]"""
    t = _dev(host, elem)
    ptrs = np.array([[t[r].data_ptr() for r in range(host.shape[0])]], np.int64)
    return _launch(pkg, ptrs, [P], elem, max_norm)


def _random(rng, n, P, elem):
    """rows of different magnitudes around 1 / sqrt(P): some norms below max_norm = 1, some above; padded to a
    multiple of 8 columns with NaN guard words (nothing past P may count)"""
    ld = (P + 8 + 7) // 8 * 8
    mag = np.exp(rng.uniform(-3, 3, (n, 1))) / np.sqrt(P)
    g = (rng.standard_normal((n, P)) * mag).astype(F32)
    if elem == 4:
        host = np.full((n, ld), np.nan, F32)
        host[:, :P] = g
        return host, g
    bits = bf16ref.rne_bf16(g)
    host = np.full((n, ld), NAN16, np.uint16)
    host[:, :P] = bits
    return host, bf16ref.upcast(bits)


def _check(norm, scale, g, max_norm, where):
    want = clipref.grad_norm_ref(g)
    assert np.isfinite(norm).all() and int(clipref.ulp_diff(norm, want).max()) <= 1, where
    assert np.array_equal(scale.view(np.uint32), clipref.clip_scale_ref(norm, max_norm).view(np.uint32)), where


def _widths(pkg):
    B = pkg.lib.mx_grad_norm_cols()
    assert B == 4096
    return [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4097, B - 1, B, B + 1, 2 * B + 3]


@pytest.mark.parametrize("n", [8, 33])
@pytest.mark.parametrize("elem", [4, 2])
def test_widths(pkg, elem, n):
    rng = np.random.default_rng([elem, n])
    clipped = 0
    for P in _widths(pkg) + ([70_001] if n == 33 else []):
        host, g = _random(rng, n, P, elem)
        norm, scale = _rows(pkg, host, P, elem)
        _check(norm, scale, g, 1.0, f"elem {elem} n {n} P {P}")
        clipped += int((scale < 1.0).sum())
        assert (scale <= 1.0).all()
    assert 0 < clipped < n * (len(_widths(pkg)) + 1)          # some rows clip, some do not


@pytest.mark.parametrize("elem", [4, 2])
def test_long_rows(pkg, elem):
    """257 B + 5 columns: every loop of both kernels runs more than once; and again on a grid of 3 workgroups"""
    B = pkg.lib.mx_grad_norm_cols()
    n, P = 8, 257 * B + 5
    rng = np.random.default_rng(elem)
    host, g = _random(rng, n, P, elem)
    t = _dev(host, elem)
    ptrs = np.array([[t[r].data_ptr() for r in range(n)]], np.int64)
    norm, scale = _launch(pkg, ptrs, [P], elem)
    _check(norm, scale, g, 1.0, f"elem {elem}")
    saved = pkg.engine.grad_norm_tuning()
    try:
        pkg.engine.set_grad_norm_tuning(grid=3)
        norm2, scale2 = _launch(pkg, ptrs, [P], elem)
    finally:
        pkg.engine.set_grad_norm_tuning(**saved)
    assert np.array_equal(norm.view(np.uint32), norm2.view(np.uint32))
    assert np.array_equal(scale.view(np.uint32), scale2.view(np.uint32))


@pytest.mark.parametrize("elem", [4, 2])
def test_single_element_rows_are_exact(pkg, elem):
    """A row of zeros with one 3.0: at column 0, at the last column and on each side of every pass, wave
    and work-item boundary (every multiple of 256 up to 2B + 3 columns) the norm is exactly 3.0; a row
    of zeros has norm 0 and factor 1.0.  64 rows per launch."""
    B = pkg.lib.mx_grad_norm_cols()
    P = 2 * B + 3
    ld = (P + 7) // 8 * 8
    pos = sorted({0, 1, 3, 4, 7, 8, P - 1} | {k - 1 for k in range(256, P, 256)} | {k for k in range(256, P, 256)})
    pos = pos + [None]                                     # the row of zeros
    three = F32(3.0) if elem == 4 else np.uint16(0x4040)
    want_scale = clipref.clip_scale_ref(F32([3.0]), 1.0)[0]
    for lo in range(0, len(pos), 64):
        part = pos[lo:lo + 64]
        host = np.zeros((len(part), ld), F32 if elem == 4 else np.uint16)
        for r, c in enumerate(part):
            if c is not None:
                host[r, c] = three
        norm, scale = _rows(pkg, host, P, elem)
        for r, c in enumerate(part):
            if c is None:
                assert norm[r] == 0.0 and not np.signbit(norm[r]) and scale[r] == 1.0
            else:
                assert norm[r] == F32(3.0) and scale[r] == want_scale, (elem, c)


@pytest.mark.parametrize("delta", [0, 1, 2])
@pytest.mark.parametrize("elem", [4, 2])
def test_unaligned_two_segment_tables(pkg, elem, delta):
    """Two segments (5 and B + 3 elements) at pointers 0 / 4 / 8 bytes (fp32) or 0 / 2 / 8 bytes (bf16) past
    a 16-byte boundary, NaN guard words before and after every row of both: the norms are finite and
    right, and the buffer is unchanged."""
    B = pkg.lib.mx_grad_norm_cols()
    d = delta if elem == 4 else (0, 1, 4)[delta]
    n, lens = 5, [5, B + 3]
    off = [8 + d, 32 + d]
    stride = (off[1] + lens[1] + 16 + 7) // 8 * 8
    rng = np.random.default_rng([elem, delta])
    g = (rng.standard_normal((n, sum(lens))) * np.exp(rng.uniform(-3, 3, (n, 1))) / 64).astype(F32)
    if elem == 4:
        host = np.full((n, stride), np.nan, F32)
        vals = g
    else:
        host = np.full((n, stride), NAN16, np.uint16)
        vals = bf16ref.rne_bf16(g)
        g = bf16ref.upcast(vals)
    host[:, off[0]:off[0] + lens[0]] = vals[:, :lens[0]]
    host[:, off[1]:off[1] + lens[1]] = vals[:, lens[0]:]
    t = _dev(host, elem)
    ptrs = np.array([[t[r].data_ptr() + elem * off[s] for r in range(n)] for s in range(2)], np.int64)
    assert all(int(p) % 16 == (elem * d) % 16 for p in ptrs.reshape(-1))
    norm, scale = _launch(pkg, ptrs, lens, elem, 0.5)
    _check(norm, scale, g, 0.5, f"elem {elem} delta {d}")
    after = t.cpu().numpy().view(host.dtype)
    assert np.array_equal(after.view(np.uint32 if elem == 4 else np.uint16), host.view(np.uint32 if elem == 4 else np.uint16))


@pytest.mark.parametrize("elem", [4, 2])
def test_rows_are_independent_and_launches_reproducible(pkg, elem):
    """row r's bits do not change when the other rows do; two launches, and every knob, give the same bits"""
    B = pkg.lib.mx_grad_norm_cols()
    n, P = 8, 5 * B + 77
    rng = np.random.default_rng(elem + 10)
    host, _ = _random(rng, n, P, elem)
    base = _rows(pkg, host, P, elem)
    again = _rows(pkg, host, P, elem)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base, again))
    other, _ = _random(rng, n, P, elem)
    other[3] = host[3]
    moved = _rows(pkg, other, P, elem)
    assert moved[0].view(np.uint32)[3] == base[0].view(np.uint32)[3]
    assert moved[1].view(np.uint32)[3] == base[1].view(np.uint32)[3]
    assert not np.array_equal(np.delete(moved[0], 3), np.delete(base[0], 3))
    saved = pkg.engine.grad_norm_tuning()
    try:
        for knobs in ({"blocks_per_cu": 1}, {"blocks_per_cu": 64}, {"grid": 1}, {"grid": 7}, {"grid": 65536}):
            pkg.engine.set_grad_norm_tuning(**saved)
            pkg.engine.set_grad_norm_tuning(**knobs)
            got = _rows(pkg, host, P, elem)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base, got)), knobs
    finally:
        pkg.engine.set_grad_norm_tuning(**saved)


@pytest.mark.parametrize("elem", [4, 2])
def test_special_values(pkg, elem):
    """A NaN element: NaN norm and NaN factor.  An Inf element: norm Inf, factor 0.  Elements of the
    largest finite value whose norm exceeds it: Inf.  Denormal elements are counted (their squares are
    normal fp64 numbers).  The other rows stay what they were."""
    P = 4099
    ld = (P + 7) // 8 * 8
    rng = np.random.default_rng(elem + 20)
    g = (rng.standard_normal((6, P)) / 64).astype(F32)
    g[4] = 0.0
    if elem == 4:
        host = np.zeros((6, ld), F32)
        host[:, :P] = g
        host[0, 1234] = np.nan
        host[1, P - 1] = -np.inf
        host[2, [5, 4098]] = [3.4028235e38, -3.4028235e38]
        host[4, [0, 77, 4097]] = F32([1e-42, -3e-41, 1.4e-45])
        vals = host[:, :P]
    else:
        host = np.zeros((6, ld), np.uint16)
        host[:, :P] = bf16ref.rne_bf16(g)
        host[0, 1234] = 0xFFC1
        host[1, P - 1] = 0xFF80
        host[2, [5, 4098]] = [0x7F7F, 0xFF7F]
        host[4, [0, 77, 4097]] = [0x0001, 0x8003, 0x0040]
        vals = bf16ref.upcast(host[:, :P])
    norm, scale = _rows(pkg, host, P, elem)
    assert np.isnan(norm[0]) and np.isnan(scale[0])
    assert np.isposinf(norm[1]) and scale[1] == 0.0
    assert np.isposinf(norm[2]) and scale[2] == 0.0
    want = clipref.grad_norm_ref(vals[3:])
    assert 0 < want[1] < 1.2e-38 and norm[4] > 0                         # a denormal norm, not flushed
    assert int(clipref.ulp_diff(norm[3:], want).max()) <= 1
    assert np.array_equal(scale[3:].view(np.uint32), clipref.clip_scale_ref(norm[3:], 1.0).view(np.uint32))
    assert scale[4] == 1.0
