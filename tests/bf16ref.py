"""The bfloat16 round's specification, restated in numpy for the tests (never the code under test):

    out_bits == rne_bf16(O.decen_round(upcast(X), partner, flags, alpha))

upcast is the exact widening (bits << 16); the oracle runs its fp32 FMA chain (partners in ascending
matching order, self term last); rne_bf16 rounds once, to nearest even.  Non-NaN results compare
uint16 for uint16; a NaN compares equal to any NaN (neither torch's cast nor v_cvt_pk_bf16_f32 pins
the payload)."""
import numpy as np


def rne_bf16(f):
    """float32 array -> bfloat16 bit patterns (uint16), round to nearest even:
    (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bits u.  NaN inputs are kept out of the integer
    formula: its carry runs through the exponent, which is what rounds the largest finite values up
    to Inf, but it would also turn a NaN whose upper mantissa bits are all ones into +-0 or Inf
    (0x7FFF8000 -> 0x8000).  A NaN gives its own upper half with the quiet bit set."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r[nan] = ((u[nan] >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16)
    return r


def upcast(bits):
    """bfloat16 bit patterns (uint16) -> the float32 array of the same values (bits << 16)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def is_nan16(bits):
    return (np.asarray(bits, np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def same_bf16(got, want):
    """uint16-exact where `want` is not a NaN, a NaN of any payload where it is."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    wn = is_nan16(want)
    return bool(np.array_equal(is_nan16(got), wn) and np.array_equal(got[~wn], want[~wn]))


def spec_round(O, bits, partner, flags, alpha, idle_rows="skip"):
    """One bfloat16 round of every worker by the specification.  An all-zero flags row leaves the
    rows alone; with idle_rows="skip" so do rows without an active partner (their 16-bit patterns
    untouched), with "canonical" they are rewritten as bf16(0 + 1.0 * x) like every other row."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    flags = np.asarray(flags, np.uint8)
    if not flags.any():
        return bits.copy()
    partner = np.asarray(partner, np.int32)
    out = rne_bf16(O.decen_round(upcast(bits), partner, flags, alpha))
    if idle_rows == "skip":
        deg = (partner[flags.astype(bool)] >= 0).sum(axis=0)
        out[deg == 0] = bits[deg == 0]
    return out


SPECIALS = np.array([0x0000, 0x8000,                      # +-0
                     0x0001, 0x807F, 0x0040, 0x8001,      # subnormals
                     0x7F80, 0xFF80,                      # +-Inf
                     0x7FC0, 0xFFC1, 0x7F81, 0xFFFF,      # NaNs (quiet, signalling, all ones)
                     0x7F7F, 0xFF7F, 0x7F7E, 0xFF7E],     # the largest finite values
                    np.uint16)


def random_bits(rng, shape, specials=True):
    """Random bfloat16 bit patterns with exponents within about +-2^20 (sums stay finite), and --
    unless specials=False -- every pattern of SPECIALS planted a few times at random places."""
    sign = rng.integers(0, 2, shape, dtype=np.uint16) << np.uint16(15)
    exp = rng.integers(127 - 20, 127 + 21, shape).astype(np.uint16) << np.uint16(7)
    man = rng.integers(0, 128, shape, dtype=np.uint16)
    bits = (sign | exp | man).astype(np.uint16)
    if specials:
        flat = bits.reshape(-1)
        k = min(flat.size // 2, 4 * SPECIALS.size)
        pos = rng.permutation(flat.size)[:k]
        flat[pos] = SPECIALS[np.arange(k) % SPECIALS.size]
    return bits
