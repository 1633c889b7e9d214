"""The quantizer's C ABI, host side only: message sizes and the refusals before any launch (fake addresses)"""
import ctypes

import pytest

import quantref

@pytest.mark.parametrize("bits", [4, 8])
def test_message_sizes(pkg, bits):
    L = pkg.lib
    for P in (1, 255, 256, 257, 4096, 4097, 14_774_436):
        assert L.mx_choco_quant_msg_bytes(P, bits) == quantref.msg_bytes(P, bits), P
    assert L.mx_choco_quant_msg_bytes(0, bits) == -1 and b"mx_choco_quant_msg_bytes" in L.mx_last_error()
    assert L.mx_choco_quant_msg_bytes(100, bits + 1) == -1 and b"bits" in L.mx_last_error()


def test_entry_points_refuse_bad_arguments(pkg):
    L = pkg.lib
    fake = ctypes.c_void_p(1 << 40)

    def comp(x=fake, ld=8, nrows=1, P=8, bits=8, msgs=fake, msg_ld=256, rdev=None, n_rounds=0, base=0):
        return L.mx_choco_quant_compress(x, None, ld, nrows, P, bits, msgs, msg_ld, 0, 0, rdev, n_rounds, base, None)

    def apply(x=fake, xh=fake, s=fake, ld=8, P=8, bits=8, msgs=fake, msg_ld=256, n_slots=2, plan=fake, it=0,
              n_local=2, M=1):
        return L.mx_choco_quant_apply(x, xh, s, ld, P, bits, msgs, msg_ld, n_slots, plan, it, n_local, M, 0.5, 0.1,
                                      None)

    def apply_at(iter_dev=fake, n_iters=4, plan=fake, bits=4):
        return L.mx_choco_quant_apply_at(fake, fake, fake, 8, 8, bits, fake, 256, 2, plan, iter_dev, n_iters, 2, 1,
                                         0.5, 0.1, None)

    for bad, word in ((dict(x=None), b"null"), (dict(msgs=None), b"null"), (dict(bits=5), b"bits=5"), (dict(P=-1), b"P=-1"),
                      (dict(bits=0), b"bits=0"), (dict(nrows=0), b"nrows=0"), (dict(nrows=2, ld=7), b"ld=7"), (dict(base=-1), b"row_base=-1"),
                      (dict(nrows=2, msg_ld=128), b"msg_ld"), (dict(nrows=2, msg_ld=388), b"msg_ld"),    # < 384; % 8
                      (dict(msgs=ctypes.c_void_p((1 << 40) + 4)), b"unaligned"),
                      (dict(rdev=fake, n_rounds=-1), b"round counter")):
        assert comp(**bad) == -1 and word in L.mx_last_error(), bad
    for bad in (dict(x=None), dict(xh=None), dict(s=None), dict(msgs=None), dict(plan=None)):
        assert apply(**bad) == -1 and b"null" in L.mx_last_error(), bad
    for bad in (dict(P=0), dict(ld=7), dict(it=-1), dict(n_local=0), dict(n_slots=1), dict(M=0), dict(bits=1),
                dict(bits=16), dict(msg_ld=128), dict(bits=4, msg_ld=252), dict(msg_ld=-256)):
        assert apply(**bad) == -1 and b"mx_choco_quant_apply:" in L.mx_last_error(), bad
    assert apply_at(iter_dev=None) == -1 and b"iteration counter" in L.mx_last_error()
    assert apply_at(n_iters=-1) == -1 and b"iteration counter" in L.mx_last_error()
    assert apply_at(bits=2) == -1 and b"mx_choco_quant_apply_at: bits=2" in L.mx_last_error()

