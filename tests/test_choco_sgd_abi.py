"""The Choco SGD-step entry points of the C ABI, host side only: argument validation before any launch
(fake device addresses)."""
import ctypes

import pytest

FAKE = ctypes.c_void_p(1 << 40)


def _fused(L, x=FAKE, g=FAKE, m=None, xh=FAKE, ld=8, nrows=1, P=8, msgs=FAKE, msg_ld=256, work=FAKE, mom=0.0,
           nesterov=0, iter_dev=None, n_iters=0):
    return L.mx_choco_sign_sgd_compress(x, g, m, xh, ld, nrows, P, msgs, msg_ld, work, 0.1, None, 5e-4, mom, nesterov,
                                        1, iter_dev, n_iters, None)


def _step(L, x=FAKE, g=FAKE, m=None, xh=None, ld=8, nrows=1, P=8, mom=0.0, nesterov=0, iter_dev=None, n_iters=0,
          **unused):
    return L.mx_choco_sgd_step(x, g, m, ld, nrows, P, 0.1, None, 5e-4, mom, nesterov, 1, iter_dev, n_iters, None)


@pytest.mark.parametrize("call,name", [(_fused, b"mx_choco_sign_sgd_compress"), (_step, b"mx_choco_sgd_step")])
def test_entry_points_refuse_bad_arguments(pkg, call, name):
    L = pkg.lib
    nulls = [dict(x=None), dict(g=None)] + ([dict(xh=None), dict(msgs=None), dict(work=None)] if call is _fused else [])
    for bad in nulls:
        assert call(L, **bad) == -1 and L.mx_last_error() == name + b": null pointer", bad
    for bad in (dict(m=FAKE), dict(mom=0.9)):                      # m exactly when momentum != 0
        assert call(L, **bad) == -1 and b"momentum rows" in L.mx_last_error(), bad
    assert call(L, nesterov=1) == -1 and b"nesterov needs momentum" in L.mx_last_error()
    for bad, text in ((dict(P=0), b"P=0"), (dict(nrows=0), b"nrows=0"), (dict(ld=7, nrows=2), b"ld=7")):
        assert call(L, **bad) == -1 and text in L.mx_last_error() and name in L.mx_last_error(), bad
    assert call(L, iter_dev=FAKE, n_iters=-1) == -1 and b"iteration counter" in L.mx_last_error()
    if call is _fused:
        odd = ctypes.c_void_p((1 << 40) + 4)
        for bad in (dict(msgs=odd), dict(work=odd), dict(nrows=2, msg_ld=64), dict(nrows=2, msg_ld=76)):
            assert call(L, **bad) == -1 and b"msg_ld" in L.mx_last_error(), bad
