"""mx_choco_randk_compress, host side only: the refusals before any launch (fake addresses)"""
import ctypes

import pytest

FAKE = ctypes.c_void_p(1 << 40)


@pytest.mark.parametrize("bad, word", [
    (dict(x=None), b"null"), (dict(msgs=None), b"null"), (dict(P=0), b"P=0"), (dict(P=1 << 31, ld=1 << 31), b"P=2147483648"),
    (dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(nrows=0), b"nrows=0"), (dict(nrows=2, ld=7), b"ld=7"),
    (dict(base=-1), b"row_base=-1"), (dict(nrows=2, msg_ld=40), b"msg_ld"), (dict(nrows=2, msg_ld=52), b"msg_ld"),
    (dict(msgs=ctypes.c_void_p((1 << 40) + 4)), b"unaligned"), (dict(rdev=FAKE, n_rounds=-1), b"round counter")])
def test_compress_refuses_bad_arguments(pkg, bad, word):
    def comp(x=FAKE, ld=8, nrows=1, P=8, k=3, msgs=FAKE, msg_ld=48, rdev=None, n_rounds=0, base=0):
        return pkg.lib.mx_choco_randk_compress(x, None, ld, nrows, P, k, msgs, msg_ld, 0, 0, rdev, n_rounds, base, None)

    assert pkg.lib.mx_choco_msg_bytes(8, 3) == 48                     # msg_ld 40: short; 52: no multiple of 8
    assert comp(**bad) == -1 and word in pkg.lib.mx_last_error(), bad
