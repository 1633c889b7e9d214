"""Topologies by hand for the LDS row kernels (csrc/mix_bf16.hip, csrc/fused_round.h) -- test helper, no GPU.

The graphs of topologies.py fill a row class exactly or nearly so, have about ten matchings and degrees
that differ by a few.  These tables reach what they leave out: any number of rows 1-64 (partly filled
classes), M = 32 matchings (the largest plan record, src[r * M + e] at stride 32), chains of 32 partners
(round_robin) and chains of 32 next to chains of 1 and 0 in one work item (star).

A partner may occur twice in a row's chain (round_robin cycles its rounds): include/matcha_gossip.h puts
no distinctness requirement on partner_dev, the oracle takes the matchings as listed, and so does the
reference's loop over the matchings."""
import numpy as np

N_ALL = [1, 2, 5, 8, 9, 12, 16, 17, 24, 32, 33, 48, 63, 64]
M_MAX = 32
# degree <= 32: every weight alpha, and the self weight 1 - degree * alpha >= 1/2, is non-negative and they
# sum to 1 -- a round is a convex combination, so values never grow from round to round
ALPHA = 1.0 / 64.0


def round_robin(n, M=M_MAX):
    """partner int32 [M][n]: matching g is round g mod (m - 1) of the circle method on m = n + (n & 1) nodes
    (node m - 1 fixed, the others rotating); an odd n drops the pair of the bye node m - 1 = n."""
    m = n + (n & 1)
    partner = np.full((M, n), -1, np.int32)
    for g in range(M):
        r = g % (m - 1)
        pairs = [(m - 1, r)] + [((r + k) % (m - 1), (r - k) % (m - 1)) for k in range(1, m // 2)]
        for a, b in pairs:
            if a < n and b < n:
                partner[g, a], partner[g, b] = b, a
    return partner


def star(n):
    """partner int32 [min(32, n - 1)][n]: matching g is the single pair (0, g + 1).  The hub has degree M,
    the leaves 1 .. M degree 1, and for n > 33 the remaining rows degree 0."""
    M = min(M_MAX, n - 1)
    partner = np.full((M, n), -1, np.int32)
    for g in range(M):
        partner[g, 0], partner[g, g + 1] = g + 1, 0
    return partner


def single():
    """one worker, one matching, no partner"""
    return np.array([[-1]], np.int32)


def table(name, n):
    """the topology `name` ("rr" / "star") on n workers; single() for n = 1 whatever the name"""
    if n == 1:
        return single()
    return round_robin(n) if name == "rr" else star(n)


def cases(ns):
    """(n, name) over both topologies; n = 1 once"""
    return [(n, name) for n in ns for name in (("single",) if n == 1 else ("rr", "star"))]


def degrees(partner, flags):
    """the direct count: active partners per row"""
    partner, flags = np.asarray(partner, np.int32), np.asarray(flags, np.uint8)
    return (partner[flags.astype(bool)] >= 0).sum(axis=0).astype(np.int64)


def flag_rounds(partner, seed):
    """uint8 [4][M]: every matching, a random half with at least one flag set, the one matching with the
    fewest pairs, all zero"""
    M = partner.shape[0]
    rng = np.random.default_rng(seed)
    rand = (rng.random(M) < 0.5).astype(np.uint8)
    rand[rng.integers(M)] = 1
    one = np.zeros(M, np.uint8)
    one[min(range(M), key=lambda g: int((partner[g] >= 0).sum()))] = 1
    return np.stack([np.ones(M, np.uint8), rand, one, np.zeros(M, np.uint8)])
