"""The mixed-precision one-launch quantized round's C ABI, host side only: the fp32 entry points' refusals plus a null
image, all before any launch (fake addresses)"""
import ctypes

import pytest

FAKE = ctypes.c_void_p(1 << 40)


def _call(L, at, sgd, x=FAKE, g=FAKE, m=FAKE, xh=FAKE, s=FAKE, p=FAKE, ld=512, n=2, P=300, bits=8, plan=FAKE, it=0,
          idev=FAKE, n_iters=4, norms=FAKE, norm_ld=2, mom=0.9, nesterov=0):
    fn = getattr(L, "mx_choco_quant" + ("_sgd" if sgd else "") + "_round_bf16" + ("_at" if at else ""))
    head = (x, g, m, xh, s, p) if sgd else (x, xh, s, p)
    tail = (0.1, None, 0.0, mom, nesterov, 1) if sgd else ()
    return fn(*head, ld, n, P, bits, plan, *((idev, n_iters) if at else (it,)), 1, 0.5, 0.1, 7, 0, norms, norm_ld,
              *tail, None)


@pytest.mark.parametrize("at", [False, True])
@pytest.mark.parametrize("sgd", [False, True])
def test_entry_points_refuse_bad_arguments(pkg, at, sgd):
    L = pkg.lib
    bad = [(dict(x=None), b"null"), (dict(xh=None), b"null"), (dict(s=None), b"null"), (dict(p=None), b"null"),
           (dict(plan=None), b"null"), (dict(bits=5), b"bits=5"), (dict(bits=1), b"bits=1"), (dict(n=0), b"n_local=0"),
           (dict(n=17), b"n_local=17"), (dict(ld=299), b"ld=299"), (dict(P=0), b"P=0"), (dict(norm_ld=1), b"norm_ld=1")]
    bad += [(dict(idev=None), b"iteration counter"), (dict(n_iters=-1), b"iteration counter")] if at else \
           [(dict(it=-1), b"iter < 0")]
    if sgd:
        bad += [(dict(g=None), b"null"), (dict(m=None), b"momentum"), (dict(mom=0.0), b"momentum"),
                (dict(m=None, mom=0.0, nesterov=1), b"nesterov")]
    for kw, word in bad:
        assert _call(L, at, sgd, **kw) == -1 and word in L.mx_last_error(), kw
