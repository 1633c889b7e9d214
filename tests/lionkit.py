"""What tests/test_gpu_lion_mix.py and tests/test_gpu_lion_mix_bf16.py share -- test helper: the three
forms of the fused Lion round behind one description (Kind), the topologies and shapes, and the test
bodies, which the two files parametrise.

    f32    csrc/lion_mix.hip        x, g, m fp32
    mp32   csrc/lion_mix_bf16.hip   fp32 masters w, bf16 g and p, fp32 momentum
    mp16   csrc/lion_mix_bf16.hip   the same with bfloat16 momentum

Every comparison is against tests/lionref.py, never the code under test: w / x / fp32 m uint32 for uint32,
p and a bfloat16 m uint16 for uint16.  A NaN of any payload passes where the specification is a NaN in
run_special_values only (nan_ok)."""
import ctypes
import random

import numpy as np
import torch

import bf16ref
import clipref
import lionref
from abitables import PaddedTables
from conftest import Topo, special_values
from sgdref import is_nan32, same_f32

LR = 0.01
HYPERS = {"H0": (0.9, 0.99, 0.0), "H1": (0.9, 0.99, 1e-2), "H2": (0.95, 0.98, 0.1)}      # beta1, beta2, wd
DEFAULT_KNOBS = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0}
_TOPOS = {}


class Kind:
    def __init__(self, name):
        assert name in ("f32", "mp32", "mp16")
        self.name, self.mixed, self.m16 = name, name != "f32", name == "mp16"
        self.base = "mx_lion_mix_bf16" if self.mixed else "mx_lion_mix"
        self.x = "w" if self.mixed else "x"
        self.tables = ("w", "g", "m", "p") if self.mixed else ("x", "g", "m")
        self.dtype = torch.bfloat16 if self.mixed else torch.float32
        self.mdtype = torch.bfloat16 if self.m16 else torch.float32

    def bits(self, k):
        """array k travels as bfloat16 bit patterns (uint16)"""
        return (self.mixed and k in "gp") or (self.m16 and k == "m")

    def tuning(self, pkg):
        E = pkg.engine
        return (E.lion_mix_bf16_tuning, E.set_lion_mix_bf16_tuning) if self.mixed else \
            (E.lion_mix_tuning, E.set_lion_mix_tuning)

    def __repr__(self):
        return self.name


KINDS = {k: Kind(k) for k in ("f32", "mp32", "mp16")}


def topology(pkg, name):
    """(partner int32 [M][n], alpha) of the five topologies, built once"""
    if name not in _TOPOS:
        if name == "g0":                           # graph 0, 8 workers: the 8-row class
            gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 2 / 7)
        elif name == "g16":                        # a 16-worker graph: the 16-row class
            gp = pkg.GraphProcessor(pkg.select_graph(2), 1.0, 0, 16, 4, True)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), 0.2)
        elif name == "ring32":                     # a ring of 32 by hand: the 32-row class, two matchings
            idx = np.arange(32)
            _TOPOS[name] = (np.stack([idx ^ 1, np.where(idx & 1, (idx + 1) % 32, (idx - 1) % 32)]).astype(np.int32), 0.25)
        elif name == "er64":                       # ER(64, 0.1, seed 1234): the 64-row class
            random.seed(0)
            base = pkg.erdos_renyi(64, 0.1, 1234)
            np.random.seed(1234)
            gp = pkg.MatchaProcessor(base, 0.5, 0, 64, 4, False)
            _TOPOS[name] = (np.asarray(gp.neighbors_info, np.int32), float(gp.neighbor_weight))
        else:                                      # 3 workers by hand: the 8-row class with unused rows
            _TOPOS[name] = (np.array([[1, 0, -1], [-1, 2, 1]], np.int32), -2.0 ** -8)
    partner, alpha = _TOPOS[name]
    assert partner.shape[0] <= 32
    for g in range(partner.shape[0]):              # matchings: symmetric
        for i, j in enumerate(partner[g]):
            assert j < 0 or (j != i and partner[g, j] == i)
    return partner, alpha


def flag_kinds(partner, seed):
    """four kinds of rounds, three consecutive rounds each: all zero, the matching with the fewest pairs,
    every matching, random 0.5"""
    M = partner.shape[0]
    rng = np.random.default_rng(seed)
    one = np.zeros(M, np.uint8)
    one[min(range(M), key=lambda g: int((partner[g] >= 0).sum()))] = 1
    rand = (rng.random((3, M)) < 0.5).astype(np.uint8)
    rand[0, rng.integers(M)] = 1
    return np.concatenate([np.zeros((3, M), np.uint8), np.tile(one, (3, 1)), np.ones((3, M), np.uint8), rand])


def tile(pkg, K, n):
    T = int(getattr(pkg.lib, K.base + "_tile")(n))
    assert T > 0
    return T


def shapes(pkg, K, n):
    T = tile(pkg, K, n)
    return [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, T - 1, T, T + 9, 3 * T + 5]


def group(pkg, K, topo, P, hyper, zero, idle_rows="skip", **kw):
    b1, b2, wd = HYPERS[hyper] if isinstance(hyper, str) else hyper
    grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows, dtype=K.dtype)
    grp.attach_lion(betas=(b1, b2), weight_decay=wd, zero_grads=zero, master_weights=K.mixed,
                    momentum_dtype=K.mdtype, **kw)
    return grp


def _arr(grp, K, k):
    return {"x": grp.rows, "w": grp.master_rows, "g": grp.grads, "m": grp.lion_exp_avg_rows, "p": grp.rows}[k]


def put(grp, K, **arrays):
    """x= (fp32 values: the rows, or the masters), g=, m= (fp32 values or bfloat16 bit patterns, by kind)"""
    for k, a in arrays.items():
        name = K.x if k == "x" else k
        t = _arr(grp, K, name)
        if K.bits(name):
            t.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)))
        else:
            t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


def state(grp, K):
    """host copies {x, g, m, p}: fp32 arrays or bit patterns by kind; p None for the fp32 kind"""
    torch.cuda.synchronize()
    out = {}
    for k in ("x", "g", "m", "p"):
        name = K.x if k == "x" else k
        if k == "p" and not K.mixed:
            out[k] = None
            continue
        t = _arr(grp, K, name)
        out[k] = t.view(torch.int16).cpu().numpy().view(np.uint16) if K.bits(name) else t.cpu().numpy()
    return out


def same(K, got, want, keys="xmp", nan_ok=False):
    for k in keys:
        name = K.x if k == "x" else k
        if want[k] is None:
            continue
        if K.bits(name):
            ok = bf16ref.same_bf16(got[k], want[k]) if nan_ok else np.array_equal(got[k], want[k])
        else:
            ok = same_f32(got[k], want[k]) if nan_ok else lionref.eq32(got[k], want[k])
        if not ok:
            return False
    return True


def same_state(K, a, b):
    return same(K, a, b, "xmp") and np.array_equal(lionref.u32(a["g"]) if not K.mixed else a["g"],
                                                   lionref.u32(b["g"]) if not K.mixed else b["g"])


def tails_zero(grp, K, P):
    arenas = [grp.arena, grp.grad_arena, grp.lion_exp_avg_arena] + ([grp.master_arena] if K.mixed else [])
    return all(not a[:, P:].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32).any().item() for a in arenas)


def g32(K, G):
    return bf16ref.upcast(G) if K.mixed else np.asarray(G, np.float32)


def rand_g(K, rng, shape, zeros=None, rowscale=None):
    """a gradient in the kind's format; exact zeros where `zeros`"""
    if K.mixed:
        if rowscale is None:
            G = bf16ref.random_bits(rng, shape, specials=False)
        else:
            G = bf16ref.rne_bf16((rng.standard_normal(shape) * rowscale[:, None]).astype(np.float32))
    else:
        G = rng.standard_normal(shape).astype(np.float32)
        if rowscale is not None:
            G = (G * rowscale[:, None]).astype(np.float32)
    if zeros is not None:
        G[zeros] = 0
    return G


def zero_m(K, shape):
    return np.zeros(shape, np.uint16 if K.m16 else np.float32)


def spec(O, K, s, G, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None):
    """the specification's {x, m, p, xp} after one round from state s with gradient G"""
    hyper = HYPERS[hyper] if isinstance(hyper, str) else hyper
    if K.mixed:
        x, m, p, xp = lionref.spec_round_bf16(O, s["x"], G, s["m"], partner, flags, alpha, lr, hyper, idle_rows, scale,
                                              runs, m_bf16=K.m16)
    else:
        x, m, xp = lionref.spec_round(O, s["x"], G, s["m"], partner, flags, alpha, lr, hyper, idle_rows, scale, runs)
        p = None
    return {"x": x, "m": m, "p": p, "xp": xp}


def g_after(K, got, G, zero):
    return (not got["g"].any()) if zero else np.array_equal(lionref.u32(got["g"]) if not K.mixed else got["g"],
                                                            lionref.u32(G) if not K.mixed else G)


# ---------------------------------------------------------------------------------------------- test bodies
def run_rounds(pkg, O, K, name, idle_rows, hyper):
    """three consecutive rounds of each flag kind at every shape, state carried; about 5 % of the gradients
    are exact zeros on momentum that stays zero, so c == 0 occurs in every round"""
    partner, alpha = topology(pkg, name)
    n = partner.shape[1]
    flags = flag_kinds(partner, 5)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([len(name), len(idle_rows), n, int(hyper[1]), len(K.name)])
    Ps = shapes(pkg, K, n)
    zero_dirs = 0
    for pi, P in enumerate(Ps[-3:] if name == "er64" else Ps):
        zero = bool(pi & 1)                          # both settings of zero_grads, alternating by P
        grp = group(pkg, K, topo, P, hyper, zero, idle_rows)
        assert tuple(grp.lion_exp_avg_rows.shape) == (n, P) and grp.lion_exp_avg_arena.dtype == K.mdtype
        assert tuple(grp.lion_exp_avg_arena.shape) == (n, grp.ld) and grp.grad_arena.dtype == K.dtype
        zeros = rng.random((n, P)) < 0.05
        zeros[0, 0] = True
        s = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": zero_m(K, (n, P))}
        put(grp, K, x=s["x"])
        for it in range(len(flags)):
            G = rand_g(K, rng, (n, P), zeros)
            put(grp, K, g=G)
            ran = grp.lion_step(it, LR)
            got = state(grp, K)
            want = spec(O, K, s, G, partner, flags[it], alpha, LR, hyper, idle_rows)
            where = f"{K} {name} {idle_rows} {hyper} P={P} round {it}"
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the Lion step alone: not a no-op
                assert lionref.eq32(got["x"], want["xp"]) and not lionref.eq32(got["x"], s["x"]), where
                wd = HYPERS[hyper][2]
                if wd == 0:                          # a zero direction kept x bit for bit
                    assert np.array_equal(lionref.u32(got["x"])[zeros], lionref.u32(s["x"])[zeros]), where
                zero_dirs += int(zeros.sum())
            for k in "xmp":
                assert same(K, got, want, k), where + ": " + k
            assert g_after(K, got, G, zero), where + ": g"
            assert tails_zero(grp, K, P), where + ": wrote past the row"
            s = got
        assert not np.asarray(s["m"])[zeros].any(), "momentum under zero gradients stays zero"
    assert zero_dirs > 0


def run_signed_zero(pkg, O, K):
    """x = -0.0, g = 0, m = 0: the direction is a zero and x keeps 0x80000000, with and without decay (the
    Lion step alone; the step under an active round is held to the specification, whose mix turns it +0)"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    flags = np.stack([np.zeros(M, np.uint8), np.ones(M, np.uint8)])
    n, P = 8, 1033
    for hyper in ("H0", "H2"):
        grp = group(pkg, K, Topo(partner, alpha, flags), P, hyper, False)
        s = {"x": np.full((n, P), -0.0, np.float32), "m": zero_m(K, (n, P))}
        G = np.zeros((n, P), np.uint16 if K.mixed else np.float32)
        put(grp, K, x=s["x"], g=G, m=s["m"])
        assert grp.lion_step(0, LR) is False
        got = state(grp, K)
        assert (lionref.u32(got["x"]) == 0x80000000).all(), hyper
        assert not np.asarray(got["m"]).view(np.uint16 if K.m16 else np.uint32).any(), hyper
        if K.mixed:
            assert (got["p"] == 0x8000).all(), hyper
        assert same(K, got, spec(O, K, s, G, partner, flags[0], alpha, LR, hyper)), hyper
        assert grp.lion_step(1, LR) is True
        got2 = state(grp, K)
        assert same(K, got2, spec(O, K, got, G, partner, flags[1], alpha, LR, hyper)), hyper


def run_special_values(pkg, O, K, where):
    """NaNs, +-Inf, +-0, subnormals and the largest finite values planted in x, then g, then m"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    n, P = 8, 4099
    rng = np.random.default_rng(31)
    s = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": zero_m(K, (n, P))}
    G = rand_g(K, rng, (n, P))
    if where == "x":
        s["x"] = np.stack([special_values(P, 100 + r) for r in range(n)])
    elif where == "g":
        G = bf16ref.random_bits(rng, (n, P), specials=True) if K.mixed else \
            np.stack([special_values(P, 200 + r) for r in range(n)])
    else:
        s["m"] = bf16ref.random_bits(rng, (n, P), specials=True) if K.m16 else \
            np.stack([special_values(P, 300 + r) for r in range(n)])
    for fl in (np.ones(M, np.uint8), np.zeros(M, np.uint8)):
        grp = group(pkg, K, Topo(partner, alpha, fl[None, :]), P, "H1", False)
        put(grp, K, x=s["x"], g=G, m=s["m"])
        assert grp.lion_step(0, LR) == bool(fl.any())
        got = state(grp, K)
        want = spec(O, K, s, G, partner, fl, alpha, LR, "H1")
        nan = int(is_nan32(want["x"]).sum())
        print(f"{K} special {where} flags {int(fl.any())}: {nan} NaN outputs of {n * P} in the specification")
        assert 0 < nan <= 0.05 * n * P               # on the spec itself: the comparison below compares something
        for k in "xmp":
            assert same(K, got, want, k, nan_ok=True), f"{where} {k}"
        assert g_after(K, got, G, False) and tails_zero(grp, K, P)


def _abi_offsets(K):
    """element offsets 0-7 per (array, segment, row): row 0 all aligned (the vector path); row 1 the 2-byte
    arrays 8-byte but not 16-byte aligned, the rest aligned (the vector path); row 2 every array one element
    off; row 3 one array alone off; from row 4 on every offset 0-7 in turn"""
    def off(k, s, r):
        narrow = K.bits(k)
        if r == 0:
            return 0
        if r == 1:
            return 4 if narrow else 0
        if r == 2:
            return 1
        if r == 3:
            return (2 if narrow else 1) if k == "m" else 0
        return (r + 3 * s + 2 * K.tables.index(k)) % 8
    return off


def run_abi(pkg, O, K):
    """the raw entry point on four-segment tables (5, 0, T + 3, 130 elements) over padded buffers: bit-equal
    to the specification, guard words around every segment untouched -- with zero_grads, so g is stored to"""
    E = pkg.engine
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    flags = np.stack([np.ones(M, np.uint8), flag_kinds(partner, 3)[3], np.zeros(M, np.uint8)])
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    n = 8
    T = tile(pkg, K, n)
    lens = [5, 0, T + 3, 130]
    dtypes = {k: np.uint16 if K.bits(k) else np.float32 for k in K.tables}
    pt = PaddedTables(n, lens, dtypes, _abi_offsets(K))
    for k in K.tables:                             # every offset occurs; 8-byte-not-16 and odd ones for 2-byte arrays
        offs = set(int(v) for v in (pt.start[k] - np.array(pt.base)).reshape(-1))
        assert offs == set(range(8)), (k, offs)
    cls = E.LionBf16Layout if K.mixed else E.LionLayout
    lay = cls(lens, *[pt.ptrs(k) for k in K.tables], n)
    assert lay.total_tiles == 4
    b1, b2, wd = HYPERS["H2"]
    call = lay.call(eng, (b1, b2), wd, True, K.m16) if K.mixed else lay.call(eng, (b1, b2), wd, True)
    fn = getattr(pkg.lib, K.base)
    rng = np.random.default_rng(41)
    s = {"x": rng.standard_normal((n, pt.P)).astype(np.float32), "m": zero_m(K, (n, pt.P))}
    pt.put(K.x, s["x"])
    pt.put("m", s["m"])
    zeros = rng.random((n, pt.P)) < 0.05
    for it in range(3):
        G = rand_g(K, rng, (n, pt.P), zeros)
        pt.put("g", G)
        assert fn(ctypes.addressof(call), it, LR, None, pkg._lib.stream_ptr()) == 0, pkg.lib.mx_last_error()
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, "H2")
        got = {"x": pt.get(K.x), "m": pt.get("m"), "p": pt.get("p") if K.mixed else None}
        where = f"{K} round {it}"
        for k in "xmp":
            assert same(K, got, want, k), where + ": " + k
        assert not pt.get("g").any(), where + ": g not zeroed within the lengths"
        for k in K.tables:
            assert pt.guards_intact(k), where + f": guard words of {k}"
        s = got


def run_scaled_grouped(pkg, O, K, mode):
    """clip_grad_norm (the _scaled entry points, against clipref), param_groups (_grouped, against groupref's
    run rule) and both: a run boundary inside a 4-element chunk, one at a work-item seam and one at the tile
    seam, a run of one column, lr_scale 0; one row below the clip norm, the others above"""
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 8)[[6, 3, 0]]
    n = 8
    T = tile(pkg, K, n)
    P = 3 * T + 5
    b1, b2, wd = HYPERS["H1"]
    kw, runs = {}, None
    if mode != "clip":
        kw["param_groups"] = [{"columns": [(0, 2)], "weight_decay": 0.0},
                              {"columns": [(2, 3)], "lr_scale": 0.5},
                              {"columns": [(7, 512)], "weight_decay": 0.1, "lr_scale": 2.0},
                              {"columns": [(512, T)], "weight_decay": 0.0, "lr_scale": 0.0},
                              {"columns": [(T, T + 1)], "weight_decay": 0.25},
                              {"columns": [(2 * T + 7, P)], "lr_scale": 0.0}]
        f = lambda v: float(np.float32(v))
        runs = [(0, 2, 0.0, 1.0), (2, 3, f(wd), 0.5), (3, 7, f(wd), 1.0), (7, 512, f(0.1), 2.0), (512, T, 0.0, 0.0),
                (T, T + 1, 0.25, 1.0), (T + 1, 2 * T + 7, f(wd), 1.0), (2 * T + 7, P, f(wd), 0.0)]
    if mode != "groups":
        kw["clip_grad_norm"] = 1.0
    grp = group(pkg, K, Topo(partner, alpha, flags), P, "H1", True, **kw)
    if runs is not None:
        assert grp.param_runs == runs
    rng = np.random.default_rng([P, len(mode), len(K.name)])
    s = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": zero_m(K, (n, P))}
    put(grp, K, x=s["x"])
    rowscale = np.ones(n)
    rowscale[0] = 1e-4                               # row 0 stays below the norm, the others are clipped
    zeros = rng.random((n, P)) < 0.05
    for it in range(3):
        G = rand_g(K, rng, (n, P), zeros, rowscale)
        put(grp, K, g=G)
        grp.lion_step(it, LR)
        got = state(grp, K)
        scale = None
        if mode != "groups":
            norms, scale = grp.grad_norms.cpu().numpy(), grp.grad_scales.cpu().numpy()
            ref = clipref.grad_norm_ref(g32(K, G))                       # the norm before clipping
            assert int(clipref.ulp_diff(norms, ref).max()) <= 1
            assert lionref.eq32(scale, clipref.clip_scale_ref(norms, 1.0))
            assert scale[0] == 1.0 and (scale[1:] < 1.0).all()
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, "H1", scale=scale, runs=runs)
        for k in "xmp":
            assert same(K, got, want, k), f"{K} {mode} round {it}: {k}"
        assert not got["g"].any() and tails_zero(grp, K, P)
        if runs is not None and not flags[it].any():                     # lr_scale 0 and wd 0: the weights are frozen
            assert lionref.eq32(got["x"][:, 512:T], s["x"][:, 512:T])
        s = got


def run_graph_replay(pkg, O, K):
    """lion_device_round captured once and replayed over a 6-round schedule with fresh gradients and a
    learning rate changed after round 3 through lr_dev == six lion_step calls on a twin (themselves the
    specification's); two replays past the schedule write nothing"""
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    n, P = 8, 2 * tile(pkg, K, 8) + 77
    rng = np.random.default_rng(61)
    X0 = rng.standard_normal((n, P)).astype(np.float32)
    zeros = rng.random((n, P)) < 0.05
    Gs = [rand_g(K, rng, (n, P), zeros) for _ in range(7)]
    lrs = [0.01, 0.01, 0.01, 0.01, 0.0025, 0.0025]
    eager = group(pkg, K, topo, P, "H1", True)
    put(eager, K, x=X0)
    s = {"x": X0, "m": zero_m(K, (n, P))}
    for it in range(6):
        put(eager, K, g=Gs[it])
        eager.lion_step(it, lrs[it])
        s = spec(O, K, s, Gs[it], partner, flags[it], alpha, lrs[it], "H1")
    want = state(eager, K)
    assert same(K, want, s) and not want["g"].any()

    grp = group(pkg, K, topo, P, "H1", True)
    put(grp, K, x=X0)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            grp.lion_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and lionref.eq32(state(grp, K)["x"], X0)      # capture ran nothing
    for it in range(6):
        put(grp, K, g=Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = state(grp, K)
    assert same_state(K, got, want)
    put(grp, K, g=Gs[6])                             # past the schedule: no mix, no Lion step, g not zeroed
    for _ in range(2):
        g.replay()
    past = state(grp, K)
    assert int(grp.iter_dev.item()) == 8
    assert same(K, past, want) and g_after(K, past, Gs[6], False)


_KNOB_BASE = {}


def _knob_run(pkg, K, name):
    """three rounds (every matching, the sparsest, random) on 3T + 5 columns with decay, zeroing"""
    partner, alpha = topology(pkg, name)
    n = partner.shape[1]
    flags = flag_kinds(partner, 6)[[6, 3, 9]]
    P = 3 * tile(pkg, K, n) + 5
    rng = np.random.default_rng([P, n])
    grp = group(pkg, K, Topo(partner, alpha, flags), P, "H2", True)
    put(grp, K, x=rng.standard_normal((n, P)).astype(np.float32))
    zeros = rng.random((n, P)) < 0.05
    for it in range(3):
        put(grp, K, g=rand_g(K, rng, (n, P), zeros))
        grp.lion_step(it, LR)
    assert tails_zero(grp, K, P)
    return state(grp, K)


def run_knobs(pkg, K, knobs):
    """the family's knobs tune speed only: the 8-row and 64-row classes give the default's bits under each;
    the default itself is held to the specification by run_rounds"""
    tuning, set_tuning = K.tuning(pkg)
    for name in ("g0", "er64"):
        if (K.name, name) not in _KNOB_BASE:
            assert tuning() == DEFAULT_KNOBS
            _KNOB_BASE[K.name, name] = _knob_run(pkg, K, name)
    saved = {k: v for k, v in tuning().items() if k in knobs}
    try:
        set_tuning(**knobs)
        assert all(tuning()[k] == v for k, v in knobs.items())
        got = {name: _knob_run(pkg, K, name) for name in ("g0", "er64")}
    finally:
        set_tuning(**saved)
    assert tuning() == DEFAULT_KNOBS
    for name in ("g0", "er64"):
        assert same_state(K, got[name], _KNOB_BASE[K.name, name]), f"{K} {knobs} {name}"
    assert pkg.engine.sgd_mix_tuning()["grid"] == 0 and pkg.engine.sgd_mix_bf16_tuning()["grid"] == 0


def run_checkpoints(pkg, O, K):
    """a round trip continues bit for bit; a Lion checkpoint is refused by an SGD group, an SGD or AdamW
    checkpoint by a Lion group; the key is the arena's dtype; without the key the buffer is zeroed"""
    partner, alpha = topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((4, partner.shape[0]), np.uint8))
    n, P = 8, 1300
    rng = np.random.default_rng(71)
    zeros = rng.random((n, P)) < 0.05
    Gs = [rand_g(K, rng, (n, P), zeros) for _ in range(4)]

    def steps(g, its):
        for it in its:
            put(g, K, g=Gs[it])
            g.lion_step(it, LR)

    grp = group(pkg, K, topo, P, "H1", True)
    put(grp, K, x=rng.standard_normal((n, P)).astype(np.float32))
    steps(grp, range(2))
    grp.iter = 2
    ckpt = grp.state_dict()
    keys = {"kind", "iter", "row_base", "workers", "rows", "lion_exp_avg_rows"} | ({"master_rows"} if K.mixed else set())
    assert set(ckpt) == keys and ckpt["lion_exp_avg_rows"].dtype == K.mdtype
    assert tuple(ckpt["lion_exp_avg_rows"].shape) == (n, P) and ckpt["lion_exp_avg_rows"].abs().max().item() > 0
    twin = group(pkg, K, topo, P, "H1", True)
    twin.load_state_dict(ckpt)
    assert twin.iter == 2 and same_state(K, state(twin, K), state(grp, K))
    steps(grp, range(2, 4))
    steps(twin, range(2, 4))
    assert same_state(K, state(twin, K), state(grp, K))              # continues bit for bit
    twin.load_state_dict({k: v for k, v in ckpt.items() if k != "lion_exp_avg_rows"})
    assert not twin.lion_exp_avg_rows.view(torch.int16 if K.m16 else torch.int32).any().item()
    # the other optimizers' groups refuse Lion state, and a Lion group theirs
    kw = {"dtype": K.dtype}
    sgd = pkg.VirtualWorkerGroup(topo, numel=P, **kw)
    sgd.attach_sgd(momentum=0.9, master_weights=K.mixed)
    with pytest_raises(ValueError, "Lion"):
        sgd.load_state_dict(ckpt)
    adamw = pkg.VirtualWorkerGroup(topo, numel=P, **kw)
    adamw.attach_adamw(master_weights=K.mixed)
    with pytest_raises(ValueError, "Lion"):
        adamw.load_state_dict(ckpt)
    with pytest_raises(ValueError, "Lion"):
        pkg.VirtualWorkerGroup(topo, numel=P, **kw).load_state_dict({k: v for k, v in ckpt.items() if k != "master_rows"})
    with pytest_raises(ValueError, "momentum"):
        twin.load_state_dict(sgd.state_dict())
    with pytest_raises(ValueError, "Adam"):
        twin.load_state_dict(adamw.state_dict())
    assert set(sgd.state_dict()) == (keys - {"lion_exp_avg_rows"}) | {"momentum_rows"}      # untouched
    with pytest_raises(ValueError, "Lion"):                          # another shape
        group(pkg, K, topo, P + 1, "H1", True).load_state_dict({**ckpt, "rows": twin.arena[:, :P + 1].clone(), **(
            {"master_rows": twin.master_arena[:, :P + 1].clone()} if K.mixed else {})})
    return ckpt, topo, P


def run_attach_errors(pkg, K):
    partner, alpha = topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))

    def fresh():
        return pkg.VirtualWorkerGroup(topo, numel=100, dtype=K.dtype)

    mw = {"master_weights": K.mixed}
    grp = fresh()
    with pytest_raises(pkg.MXError, r"no Lion state: call attach_lion\(\) first"):
        grp.lion_step(0, LR)
    grp.attach_lion(momentum_dtype=K.mdtype, **mw)
    assert grp.lion_hyper == {"betas": (0.9, 0.99), "weight_decay": 0.0, "zero_grads": True, "momentum_dtype": K.mdtype}
    with pytest_raises(RuntimeError, "attach_lion: already attached"):
        grp.attach_lion(**mw)
    with pytest_raises(RuntimeError, r"attach_sgd: the group already carries Lion state \(attach_lion\)"):
        grp.attach_sgd(**mw)
    with pytest_raises(RuntimeError, r"attach_adamw: the group already carries Lion state \(attach_lion\)"):
        grp.attach_adamw(**mw)
    with pytest_raises(pkg.MXError, "no SGD state"):
        grp.sgd_step(0, LR)
    g = fresh()
    g.attach_sgd(**mw)
    with pytest_raises(RuntimeError, r"attach_lion: the group already carries SGD state \(attach_sgd\)"):
        g.attach_lion(**mw)
    with pytest_raises(RuntimeError, r"attach_adamw: the group already carries SGD state \(attach_sgd\)"):
        g.attach_adamw(**mw)                          # the existing pair's text
    g = fresh()
    g.attach_adamw(**mw)
    with pytest_raises(RuntimeError, r"attach_lion: the group already carries AdamW state \(attach_adamw\)"):
        g.attach_lion(**mw)
    with pytest_raises(RuntimeError, r"attach_sgd: the group already carries AdamW state \(attach_adamw\)"):
        g.attach_sgd(**mw)
    for bad in ({"betas": (1.0, 0.99)}, {"betas": (0.9, -0.1)}, {"weight_decay": -1.0},
                {"momentum_dtype": torch.float16}, {"clip_grad_norm": 0.0}):
        with pytest_raises(ValueError, "attach_lion"):
            fresh().attach_lion(**{**mw, **bad})
    if K.mixed:
        with pytest_raises(NotImplementedError, "bfloat16 groups need fp32 master weights under Lion"):
            fresh().attach_lion()
    else:
        with pytest_raises(ValueError, "master_weights"):
            fresh().attach_lion(master_weights=True)
        with pytest_raises(ValueError, "bfloat16 momentum"):
            fresh().attach_lion(momentum_dtype=torch.bfloat16)


def run_trainer(pkg, O, K):
    """harness.VirtualTrainer(fused_lion=True): every iteration's fused launch by the specification from the
    rows, gradients and momentum the backward passes left, with clipping and a no-decay group honoured; the
    torch optimizers never step; a checkpoint resumed in a new trainer continues bit for bit"""
    H = pkg.harness
    hyper = {"betas": (0.95, 0.98), "weight_decay": 1e-2, "momentum_dtype": K.mdtype}
    groups = [{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}]

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=1e-3, matcha=True, warmup=False)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        fn = H.model_factory(args)
        return H.VirtualTrainer(args, (lambda: fn().to(torch.bfloat16)) if K.mixed else fn, n_batches=3,
                                **{"fused_lion": True, "lion_hyper": hyper, "clip_grad_norm": 0.5,
                                   "param_groups": groups, **kw})

    tr = make()
    grp = tr.group
    assert grp.dtype == K.dtype and grp.lion_exp_avg_arena.dtype == K.mdtype and (grp.master_rows is not None) == K.mixed
    assert grp.lion_hyper["betas"] == (0.95, 0.98) and grp.lion_hyper["weight_decay"] == 1e-2
    runs = grp.param_runs
    assert len(runs) > 1 and {r[2] for r in runs} == {0.0, float(np.float32(1e-2))} and grp.clip_grad_norm == 0.5
    partner = np.asarray(tr.GP.neighbors_info, np.int32)
    seen, before = {"rounds": 0}, {}

    def hook(when, t):
        if when == "before":
            before["s"], before["it"] = state(t.group, K), t.group.iter
            assert before["s"]["g"].any()                            # backward() filled the gradient arena
            return
        flags = np.asarray(tr.GP.active_flags[before["it"]], np.uint8)
        lr = t.optimizers[0].param_groups[0]["lr"]
        got = state(t.group, K)
        scale = t.group.grad_scales.cpu().numpy()
        want = spec(O, K, before["s"], before["s"]["g"], partner[:len(flags)], flags, tr.GP.neighbor_weight, lr,
                    (0.95, 0.98, 1e-2), scale=scale, runs=runs)
        assert same(K, got, want) and not got["g"].any(), f"round {before['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats) and "grad_norm" in stats[0]
    assert seen["rounds"] == 3 and grp.iter == 3 and len(tr.grad_norm_log) == 3
    assert all(not o.state for o in tr.optimizers)                   # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert "lion_exp_avg_rows" in ckpt["group"]
    tr2 = make()
    tr2.load_state_dict(ckpt)
    tr.train_epoch()
    tr2.train_epoch()
    assert same_state(K, state(tr.group, K), state(tr2.group, K)) and tr.group.iter == tr2.group.iter == 6
    for kw in ({"fused_sgd": True}, {"fused_adamw": True}):
        with pytest_raises(ValueError, "mutually exclusive"):
            make(**kw)
    with pytest_raises(ValueError, "fused_lion"):
        make(batched=True)
    with pytest_raises(ValueError, "fused_lion"):
        make(args={"compress": True})


def pytest_raises(exc, match):
    import pytest
    return pytest.raises(exc, match=match)
