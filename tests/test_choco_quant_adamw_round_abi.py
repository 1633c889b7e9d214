"""The one-launch AdamW + quantized round's C ABI, host side only: the sgd entry points' refusals plus the optimizer's
own, all before any launch (fake addresses)"""
import ctypes

import pytest

FAKE = ctypes.c_void_p(1 << 40)


def _call(L, at, bf, x=FAKE, g=FAKE, m=FAKE, v=FAKE, xh=FAKE, s=FAKE, p=FAKE, ld=512, n=2, P=300, bits=8, plan=FAKE,
          it=0, idev=FAKE, n_iters=4, norms=FAKE, norm_ld=2, bias=FAKE, n_bias=5, step=1, sdev=None):
    fn = getattr(L, "mx_choco_quant_adamw_round" + ("_bf16" if bf else "") + ("_at" if at else ""))
    return fn(x, g, m, v, xh, s, *((p,) if bf else ()), ld, n, P, bits, plan, *((idev, n_iters) if at else (it,)), 1,
              0.5, 0.1, 7, 0, norms, norm_ld, 1e-3, None, 0.1, 0.999, 1e-3, 1e-8, 1e-2, 1, 1, bias, n_bias, step, sdev,
              None)


@pytest.mark.parametrize("at", [False, True])
@pytest.mark.parametrize("bf", [False, True])
def test_entry_points_refuse_bad_arguments(pkg, at, bf):
    L = pkg.lib
    bad = [(dict(x=None), b"null"), (dict(g=None), b"null"), (dict(m=None), b"null"), (dict(v=None), b"null"),
           (dict(xh=None), b"null"), (dict(s=None), b"null"), (dict(plan=None), b"null"), (dict(bias=None), b"null"),
           (dict(n_bias=0), b"n_bias=0"), (dict(step=0), b"optimizer step 0"), (dict(bits=5), b"bits=5"),
           (dict(n=0), b"n_local=0"), (dict(n=17), b"n_local=17"), (dict(ld=299), b"ld=299"), (dict(P=0), b"P=0"),
           (dict(norm_ld=1), b"norm_ld=1")]
    bad += [(dict(idev=None), b"iteration counter"), (dict(n_iters=-1), b"iteration counter")] if at else \
           [(dict(it=-1), b"iter < 0")]
    bad += [(dict(p=None), b"null")] if bf else []
    for kw, word in bad:
        assert _call(L, at, bf, **kw) == -1 and word in L.mx_last_error(), kw
