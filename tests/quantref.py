"""ChocoSGD's bucketed stochastic quantizer (B = 256, bits 4 or 8): the specification of DESIGN.md section 6n in
numpy, never the code under test.  Any fp64 order over 256 non-negative terms is within 256 * 2^-53 of the exact
sum, so a conforming norm is within 1 fp32 ulp of norms(); the rest is exact given a device's norms (`norm=`)."""
import math

import numpy as np

from sgdref import fmaf32

F32, U32, B = np.float32, np.uint32, 256


def consts(bits):
    s = 2 ** (bits - 1) - 1
    return s, F32(1 / (s * (1 + min(B / s ** 2, math.sqrt(B) / s))))


def mix32(h):
    h = np.asarray(h).astype(U32)
    with np.errstate(over="ignore"):
        for shift, mul in ((16, 0x7feb352d), (15, 0x846ca68b)):
            h = (h ^ (h >> U32(shift))) * U32(mul)
        return h ^ (h >> U32(16))


def xi(seed, rnd, row, n):
    key = mix32(mix32(mix32(seed & 0xffffffff) ^ U32(rnd & 0xffffffff)) ^ U32(row & 0xffffffff))
    with np.errstate(over="ignore"):
        h = mix32(key + np.arange(n, dtype=U32))
    return (h >> U32(8)).astype(F32) * F32(2.0 ** -24)


def msg_bytes(P, bits):
    nb = (P + B - 1) // B
    return 64 + 64 * ((nb + 15) // 16) + 32 * bits * nb


def norms(d):
    sq = d.astype(np.float64).reshape(-1, B) ** 2
    with np.errstate(all="ignore"):
        n2 = [math.fsum(r) if np.isfinite(r).all() else float(r.sum()) for r in sq]
        return np.sqrt(np.array(n2, np.float64)).astype(F32)


def quantize(d, bits, seed, rnd, row, norm=None):
    """(norm float32 [nb], code uint8 [nb * 256], q float32 [P]) of one float32 row d"""
    d = np.asarray(d, F32).reshape(-1)
    P, (s, c) = d.size, consts(bits)
    dp = np.pad(d, (0, -P % B))                               # +0 at and past P
    norm = norms(dp) if norm is None else np.asarray(norm, F32)
    with np.errstate(all="ignore"):
        inv = np.where(norm == 0, F32(0), F32(s) / norm).astype(F32)
        v = (np.abs(dp) * np.repeat(inv, B)).astype(F32) + xi(seed, rnd, row, dp.size)
        level = np.where(v >= 1, np.minimum(F32(s), np.floor(v)), F32(0)).astype(F32)
        neg = dp < 0
        mag = level * np.repeat((norm * c).astype(F32), B)
    q = (mag.view(U32) ^ (neg.astype(U32) << U32(31))).view(F32)
    return norm, (level.astype(np.uint8) | (neg.astype(np.uint8) << (bits - 1))), q[:P]


def pack(code, bits):
    return code if bits == 8 else (code[0::2] | (code[1::2] << 4)).astype(np.uint8)


def unpack(packed, bits):
    return packed if bits == 8 else np.stack([packed & 15, packed >> 4], 1).reshape(-1)


def slot(P, bits, norm, code):
    out = np.zeros(msg_bytes(P, bits), np.uint8)
    out[16:24] = np.array([P], np.int64).view(np.uint8)
    out[24:32] = np.array([bits, B], np.int32).view(np.uint8)
    out[64:64 + 4 * norm.size] = norm.view(np.uint8)
    out[out.size - 32 * bits * norm.size:] = pack(code, bits)
    return out


def quant_round(X, XH, S, partner, flags, alpha, gamma, bits, seed, rnd, row_base=0, norm=None):
    """One round on float32 [n, P] arrays IN PLACE (signref.sign_round's contract); returns the norms [n, nb]"""
    n, P = X.shape
    partner, flags = np.asarray(partner, np.int64), np.asarray(flags).astype(bool)
    a32, g32 = F32(alpha), F32(gamma)
    with np.errstate(all="ignore"):
        D = (X - XH).astype(F32)
        msg = [quantize(D[i], bits, seed, rnd, row_base + i, None if norm is None else norm[i]) for i in range(n)]
        for i in range(n):
            deg = 0
            for m in range(partner.shape[0]):
                j = int(partner[m, i])
                if flags[m] and j >= 0:
                    deg += 1
                    S[i] = (S[i] + (a32 * msg[j][2]).astype(F32)).astype(F32)
            sw = F32(1.0 - float(deg) * float(alpha))      # Python float arithmetic, then f32 (the plan record's)
            S[i] = (S[i] + (sw * msg[i][2]).astype(F32)).astype(F32)
            XH[i] = (XH[i] + msg[i][2]).astype(F32)
            X[i] = fmaf32(-g32, XH[i], fmaf32(g32, S[i], X[i]))
    return np.stack([m[0] for m in msg])
