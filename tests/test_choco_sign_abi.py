"""The scaled-sign entry points of the C ABI, host side only: message and workspace sizes, argument
validation before any launch (fake device addresses), and the knobs."""
import ctypes


def test_message_and_workspace_sizes(pkg):
    L = pkg.lib
    assert L.mx_choco_sign_msg_bytes(1) == 72 and L.mx_choco_sign_msg_bytes(64) == 72
    assert L.mx_choco_sign_msg_bytes(65) == 80 and L.mx_choco_sign_msg_bytes(4097) == 64 + 8 * 65
    assert L.mx_choco_sign_msg_bytes(0) == -1 and b"mx_choco_sign_msg_bytes" in L.mx_last_error()
    assert L.mx_choco_sign_msg_bytes(-5) == -1
    assert L.mx_choco_sign_work_bytes(1, 1) == 8 and L.mx_choco_sign_work_bytes(4096, 3) == 24
    assert L.mx_choco_sign_work_bytes(4097, 3) == 48
    assert L.mx_choco_sign_work_bytes(0, 1) == 0 and b"mx_choco_sign_work_bytes" in L.mx_last_error()
    assert L.mx_choco_sign_work_bytes(10, -1) == 0


def test_entry_points_refuse_bad_arguments(pkg):
    L = pkg.lib
    fake = ctypes.c_void_p(1 << 40)
    comp = L.mx_choco_sign_compress
    assert comp(None, None, 8, 1, 8, fake, 256, fake, None) == -1 and b"null" in L.mx_last_error()
    assert comp(fake, None, 8, 1, 8, None, 256, fake, None) == -1 and b"null" in L.mx_last_error()
    assert comp(fake, None, 8, 1, 8, fake, 256, None, None) == -1 and b"null" in L.mx_last_error()
    assert comp(fake, None, 8, 1, -1, fake, 256, fake, None) == -1 and b"P=-1" in L.mx_last_error()
    assert comp(fake, None, 8, 0, 8, fake, 256, fake, None) == -1 and b"nrows=0" in L.mx_last_error()
    assert comp(fake, None, 7, 2, 8, fake, 256, fake, None) == -1 and b"ld=7" in L.mx_last_error()
    assert comp(fake, None, 8, 2, 8, fake, 64, fake, None) == -1 and b"msg_ld" in L.mx_last_error()     # < 72
    assert comp(fake, None, 8, 2, 8, fake, 76, fake, None) == -1 and b"msg_ld" in L.mx_last_error()     # % 8
    assert comp(fake, None, 8, 1, 8, ctypes.c_void_p((1 << 40) + 4), 256, fake, None) == -1

    def apply(x=fake, xh=fake, s=fake, ld=8, P=8, msgs=fake, msg_ld=256, n_slots=2, plan=fake, it=0, n_local=2,
              M=1):
        return L.mx_choco_sign_apply(x, xh, s, ld, P, msgs, msg_ld, n_slots, plan, it, n_local, M, 0.5, 0.1, None)

    def apply_at(iter_dev=fake, n_iters=4, plan=fake, P=8):
        return L.mx_choco_sign_apply_at(fake, fake, fake, 8, P, fake, 256, 2, plan, iter_dev, n_iters, 2, 1, 0.5,
                                        0.1, None)

    for bad in (dict(x=None), dict(xh=None), dict(s=None), dict(msgs=None), dict(plan=None)):
        assert apply(**bad) == -1 and b"null" in L.mx_last_error(), bad
    for bad in (dict(P=0), dict(P=-3), dict(ld=7), dict(it=-1), dict(n_local=0), dict(n_slots=1), dict(M=0),
                dict(msg_ld=64), dict(msg_ld=100), dict(msg_ld=-256)):
        assert apply(**bad) == -1 and b"mx_choco_sign_apply" in L.mx_last_error(), bad
    assert apply_at(iter_dev=None) == -1 and b"iteration counter" in L.mx_last_error()
    assert apply_at(n_iters=-1) == -1 and b"iteration counter" in L.mx_last_error()
    assert apply_at(plan=None) == -1 and b"null" in L.mx_last_error()
    assert apply_at(P=-1) == -1


SIGN_KNOBS = {"apply_nt": (-1, -1, 1), "blocks_per_cu": (8, 1, 64), "grid": (0, 0, 65536)}


def test_knobs_round_trip(pkg):
    L = pkg.lib
    INV = pkg._lib.MX_ERR_INVALID

    def get(k):
        return L.mx_choco_sign_get(k.encode())

    def put(k, v):
        return L.mx_choco_sign_set(k.encode(), v)

    saved = {k: get(k) for k in SIGN_KNOBS}
    try:
        assert saved == {k: d for k, (d, _, _) in SIGN_KNOBS.items()}
        for k, (default, lo, hi) in SIGN_KNOBS.items():
            for v in (lo, hi):
                assert put(k, v) == 0 and get(k) == v, (k, v)
            for v in (lo - 1, hi + 1):
                assert put(k, v) == INV and get(k) == hi, (k, v)
                assert L.mx_last_error() == f"mx_choco_sign_set: {k} {v}".encode()
            assert put(k, default) == 0 and get(k) == default
        assert put("no_such_knob", 1) == INV and L.mx_last_error() == b"mx_choco_sign_set: unknown key 'no_such_knob'"
        assert get("no_such_knob") == INV and L.mx_last_error() == b"mx_choco_sign_get: unknown key 'no_such_knob'"
        assert L.mx_choco_sign_set(None, 1) == INV and b"null key" in L.mx_last_error()
        assert L.mx_choco_sign_get(None) == INV
    finally:
        for k, v in saved.items():
            put(k, v)
