"""ChocoSGD with the scaled-sign (1-bit) compressor Q(v) = (|v|_1 / P) sign(v): the specification, restated
in numpy for the tests (never the code under test).  It follows the oracle's Choco round
(choco_round_impl, oracle/matcha_oracle.c) line by line with the dense message in place of the sparse one.
For worker i with fp32 state rows x_i, x_hat_i, s_i:

    d_i[c]   = x_i[c] - x_hat_i[c]                            one fp32 subtraction
    L_i      = sum_c f64(|d_i[c]|)                            fp64 sum of exact widenings
    scale_i  = f32(L_i / f64(P))                              fp64 division, one rounding to fp32
    neg_i[c] = d_i[c] < 0                                     false for +0, -0 and NaN
    q_i[c]   = -scale_i if neg_i[c] else +scale_i

    a32 = f32(alpha); g32 = f32(gamma)
    for each active partner j of i, ascending matching:       s_i[c] = f32(s_i[c] + f32(a32 * q_j[c]))
    s_i[c]  = f32(s_i[c] + f32(f32(1 - deg_i * alpha) * q_i[c]))
    x_hat_i[c] = f32(x_hat_i[c] + q_i[c])
    x_i[c]  = fmaf(g32, s_i[c], x_i[c]);  x_i[c] = fmaf(-g32, x_hat_i[c], x_i[c])

Every message is formed from the state before the round.  A 1-bit message has no zero: a zero difference
(either sign) travels as +scale, where torch.sign would give 0.  NaN and Inf need no special case: one in
d makes scale NaN or Inf, and the arithmetic above propagates it.

The summation order of L is free: any fp64 order over P <= 2^26 non-negative terms is within P * 2^-53 of
the exact sum (clipref.py), so a conforming scale is within 1 fp32 ulp of sign_message's.  Everything else
is exact given the scale: sign_round takes the scales a device produced (`scale=`) and is then bit for bit
what the device must hold.

Wire format of a message slot (64 + 8 ceil(P / 64) bytes): float32 scale at 0, float64 L at 8, int64 P at
16, zeros up to 64, then np.packbits(d < 0, bitorder="little") with the padding bits zero."""
import math

import numpy as np

from sgdref import fmaf32

F32 = np.float32
HEADER = 64


def msg_bytes(P):
    return HEADER + 8 * ((int(P) + 63) // 64)


def abs_sum(d):
    """fp64: the exactly rounded sum of the exact widenings |d[c]| (math.fsum); NaN / Inf as they fall"""
    a = np.abs(np.asarray(d, F32)).astype(np.float64)
    if not np.isfinite(a).all():
        with np.errstate(all="ignore"):
            return float(a.sum())                          # NaN or Inf whatever the order
    return math.fsum(a.tolist())


def sign_message(d):
    """(scale float32, bits uint8[ceil(P/8)]) of one float32 row d"""
    d = np.asarray(d, F32).reshape(-1)
    with np.errstate(all="ignore"):
        scale = F32(np.float64(abs_sum(d)) / np.float64(d.size))
    return scale, np.packbits(d < 0, bitorder="little")


def unpack(bits, P):
    """bool [P]: the sign bits of a message"""
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:P].astype(bool)


def dense(scale, neg):
    """q = -scale where neg else +scale (float32; a NaN scale keeps its payload, the sign bit flips)"""
    s = np.full(neg.shape, F32(scale), F32)
    return (s.view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))).view(F32)


def sign_round(X, XH, S, partner, flags, alpha, gamma, scale=None):
    """One round on float32 [n, P] arrays X, XH, S, IN PLACE, with no skip: a round with no active matching
    applies every worker's own message with self weight 1 (ChocoWorkerGroup.average called directly;
    communicate() and step() skip such rounds before they get here).  partner int [M][n] (-1: unmatched),
    flags [M].  scale: float32 [n] to use in place of this file's (a device's, within 1 ulp).  Returns
    (the scales used float32 [n], the sign bits bool [n, P])."""
    n, P = X.shape
    assert X.dtype == XH.dtype == S.dtype == F32
    partner = np.asarray(partner, np.int64)
    flags = np.asarray(flags).astype(bool)
    a32, g32 = F32(alpha), F32(gamma)
    with np.errstate(all="ignore"):
        D = (X - XH).astype(F32)
        neg = D < 0
        sc = np.array([sign_message(D[i])[0] for i in range(n)], F32) if scale is None else \
            np.asarray(scale, F32).reshape(n).copy()
        Q = np.stack([dense(sc[i], neg[i]) for i in range(n)])
        for i in range(n):
            deg = 0
            for m in range(partner.shape[0]):
                j = int(partner[m, i])
                if not flags[m] or j < 0:
                    continue
                deg += 1
                S[i] = (S[i] + (a32 * Q[j]).astype(F32)).astype(F32)
            sw = F32(1.0 - float(deg) * float(alpha))      # Python float arithmetic, then f32 (the plan record's)
            S[i] = (S[i] + (sw * Q[i]).astype(F32)).astype(F32)
            XH[i] = (XH[i] + Q[i]).astype(F32)
            X[i] = fmaf32(g32, S[i], X[i])
            X[i] = fmaf32(-g32, XH[i], X[i])
    return sc, neg


def same_bits(a, b):
    """float32 arrays equal as uint32, NaNs equal where both are NaN (payloads are the hardware's)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def consensus_distance(X):
    """sqrt(mean_i |x_i - mean|^2), fp64"""
    X = np.asarray(X, np.float64)
    return float(np.sqrt(((X - X.mean(0)) ** 2).sum(1).mean()))
