"""Global-norm gradient clipping, the parts that need no GPU: the specification in tests/clipref.py
against torch on the CPU, and the new C ABI (workspace size, host-side refusals; the call record's layout
is checked in tests/test_native_abi.py)."""
import ctypes
import importlib

import numpy as np
import pytest

import clipref

torch = pytest.importorskip("torch")

F32 = np.float32


def test_grad_norm_ref_matches_fp64_torch():
    """grad_norm_ref against torch.linalg.vector_norm of the fp64 copy, cast to fp32: within 1 ulp (the
    two fp64 sums differ by their order only)."""
    rng = np.random.default_rng(3)
    for P in (1, 5, 257, 4097, 70_001):
        g = (rng.standard_normal((8, P)) * np.exp(rng.uniform(-8, 8, (8, 1)))).astype(F32)
        want = torch.linalg.vector_norm(torch.from_numpy(g).double(), dim=1).float().numpy()
        got = clipref.grad_norm_ref(g)
        assert got.dtype == F32 and int(clipref.ulp_diff(got, want).max()) <= 1, P
    bits = rng.integers(0x3000, 0x4400, (4, 1025)).astype(np.uint16)
    g = (bits.astype(np.uint32) << 16).view(F32)
    want = torch.linalg.vector_norm(torch.from_numpy(g).double(), dim=1).float().numpy()
    assert int(clipref.ulp_diff(clipref.grad_norm_ref_bf16(bits), want).max()) <= 1
    with np.errstate(all="ignore"):
        special = np.zeros((4, 9), F32)
        special[0, 3] = np.nan
        special[1, 8] = -np.inf
        special[2, :] = 3.4028235e38
        special[3, 0], special[3, 5] = 1e-42, -3e-41
        got = clipref.grad_norm_ref(special)
    assert np.isnan(got[0]) and np.isposinf(got[1]) and np.isposinf(got[2])
    assert got[3] == F32(np.sqrt(np.float64(F32(1e-42)) ** 2 + np.float64(F32(-3e-41)) ** 2)) and got[3] > 0


def test_clip_scale_ref_is_torchs_expression():
    """bit for bit torch's fp32 clamp(max_norm / (norm + 1e-6), max=1.0) on the same fp32 norms"""
    rng = np.random.default_rng(4)
    norms = np.concatenate([np.float32([0.0, 0.5, 0.999999, 1.0, 1.0000001, 2.0, 3.0, 1e-7, 1e30, 3.4028235e38,
                                        np.inf, np.nan]),
                            np.exp(rng.uniform(-20, 20, 500)).astype(F32)])
    for max_norm in (1.0, 0.1, 2.5, 1e30):
        got = clipref.clip_scale_ref(norms, max_norm)
        t = torch.from_numpy(norms)
        want = torch.clamp(max_norm / (t + 1e-6), max=1.0).numpy()
        assert want.dtype == F32
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), max_norm
    s = clipref.clip_scale_ref(np.float32([0.5, 0.0, np.inf, np.nan, 2.0]), 1.0)
    assert s[0] == 1.0 and s[1] == 1.0 and s[2] == 0.0 and np.isnan(s[3]) and s[4] == F32(1.0) / (F32(2.0) + F32(1e-6)) * F32(1.0)


def test_end_to_end_against_clip_grad_norm_cpu():
    """8 x 4097 fp32 on the CPU: torch's total norm (an fp32 sum, order unspecified) agrees with the
    specification within P * 2^-24 relative -- the worst case of any fp32 summation order of P
    non-negative terms -- and the clipped gradient within the same bound of scale_grad's."""
    n, P = 8, 4097
    rng = np.random.default_rng(5)
    g = (rng.standard_normal((n, P)) * np.float32([0.001, 0.01, 0.015, 0.02, 0.1, 1.0, 10.0, 0.0])[:, None]).astype(F32)
    norms = clipref.grad_norm_ref(g)
    scales = clipref.clip_scale_ref(norms, 1.0)
    assert (scales[:3] == 1.0).all() and (scales[3:7] < 1.0).all() and scales[7] == 1.0 and norms[7] == 0.0
    bound = P * 2.0 ** -24
    worst = 0.0
    for r in range(n):
        p = torch.nn.Parameter(torch.zeros(P))
        p.grad = torch.from_numpy(g[r].copy())
        total = float(torch.nn.utils.clip_grad_norm_([p], 1.0))
        rel = abs(total - float(norms[r])) / float(norms[r]) if norms[r] else abs(total)
        worst = max(worst, rel)
        assert rel <= bound, (r, rel)
        want = clipref.scale_grad(g[r:r + 1], scales[r:r + 1])[0]
        got = p.grad.numpy()
        assert np.all(np.abs(got - want) <= 2 * bound * np.abs(want) + 1e-45), r
    print(f"clip_grad_norm_ vs specification, 8 x 4097: max relative norm difference {worst:.3e} (bound {bound:.3e})")


def test_workspace_size(pkg):
    L = pkg.lib
    B = L.mx_grad_norm_cols()
    assert B == 4096
    lens = np.array([0, 1, B, B + 1, 5, 3 * B - 1], np.int64)
    chunks = ctypes.c_int64(-1)
    nbytes = L.mx_grad_norm_layout(lens.ctypes.data, len(lens), 8, ctypes.byref(chunks))
    assert chunks.value == 0 + 1 + 1 + 2 + 1 + 3 and nbytes == 8 * chunks.value * 8
    assert L.mx_grad_norm_layout(lens.ctypes.data, len(lens), 64, None) == 64 * 8 * 8
    one = np.array([25_600_000], np.int64)
    assert L.mx_grad_norm_layout(one.ctypes.data, 1, 8, ctypes.byref(chunks)) == 8 * 6250 * 8 and chunks.value == 6250
    assert L.mx_grad_norm_layout(None, 1, 8, None) == -1
    assert L.mx_grad_norm_layout(one.ctypes.data, 1, 0, None) == -1
    assert L.mx_grad_norm_layout(one.ctypes.data, 1, 65, None) == -1 and b"n_local" in L.mx_last_error()
    neg = np.array([-1], np.int64)
    assert L.mx_grad_norm_layout(neg.ctypes.data, 1, 8, None) == -1


def test_grad_norm_refusals_need_no_gpu(pkg):
    """every host-side refusal returns MX_ERR_INVALID before anything touches a device (fake addresses)"""
    E = importlib.import_module(pkg.__name__ + ".engine")
    L = pkg.lib
    fake = 1 << 40

    def rc(**kw):
        a = dict(g_ptrs_dev=fake, seg_len_dev=fake, work_dev=fake, norm_dev=fake, scale_dev=fake, chunks=1, nseg=1,
                 n_local=8, elem_size=4, max_norm=1.0)
        a.update(kw)
        c = E.GradNormCall(**a)
        return L.mx_grad_norm(ctypes.addressof(c), None)

    assert L.mx_grad_norm(None, None) == -1 and b"null" in L.mx_last_error()
    for k in ("g_ptrs_dev", "seg_len_dev", "work_dev", "norm_dev", "scale_dev"):
        assert rc(**{k: None}) == -1 and b"null" in L.mx_last_error(), k
    for es in (0, 1, 3, 8):
        assert rc(elem_size=es) == -1 and b"elem_size" in L.mx_last_error()
    for n in (0, -1, 65):
        assert rc(n_local=n) == -1 and b"n_local" in L.mx_last_error()
    for mn in (0.0, -1.0, float("inf"), float("nan")):
        assert rc(max_norm=mn) == -1 and b"max_norm" in L.mx_last_error()
    assert L.mx_grad_norm_set(b"nope", 1) == -1 and L.mx_grad_norm_get(b"nope") == -1
    assert L.mx_grad_norm_get(b"blocks_per_cu") == 8 and L.mx_grad_norm_get(b"grid") == 0
    # the scaled fused entry points refuse what the unscaled ones refuse
    for name in ("mx_sgd_mix_scaled", "mx_sgd_mix_bf16_scaled"):
        assert getattr(L, name)(None, fake, 0, 0.1, None, None) == -1 and b"null" in L.mx_last_error()
        assert getattr(L, name + "_at")(None, fake, fake, 4, 0.1, None, None) == -1
    for name in ("mx_adamw_mix_scaled", "mx_adamw_mix_bf16_scaled"):
        assert getattr(L, name)(None, fake, 0, 1, 0.1, None, None) == -1 and b"null" in L.mx_last_error()
        assert getattr(L, name + "_at")(None, fake, fake, 4, fake, 0.1, None, None) == -1


def test_clip_value_validation(pkg):
    E = importlib.import_module(pkg.__name__ + ".engine")
    assert E.clip_value(None, "t") is None and E.clip_value(1, "t") == 1.0 and E.clip_value(0.25, "t") == 0.25
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50, "x", [1.0]):
        with pytest.raises(ValueError):
            E.clip_value(bad, "t")
