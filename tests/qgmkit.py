"""What tests/test_gpu_qgm_mix.py and tests/test_gpu_qgm_mix_bf16.py share -- test helper: the two forms of
the fused quasi-global-momentum round behind one description (Kind) and the test bodies, which the two files
parametrise.  The topologies, the flag kinds and the gradient generator are tests/lionkit.py's.

    f32    csrc/qgm_mix.hip        x, g, mh fp32
    mp32   csrc/qgm_mix_bf16.hip   fp32 masters w, bf16 g and p, fp32 buffer mh

Every comparison is against tests/qgmref.py, never the code under test: w / x / mh uint32 for uint32, p
uint16 for uint16.  A NaN of any payload passes where the specification is a NaN in run_special_values only
(nan_ok)."""
import ctypes

import numpy as np
import torch

import bf16ref
import clipref
import qgmref
from abitables import PaddedTables
from conftest import Topo, special_values
from lionkit import flag_kinds, pytest_raises, topology
from sgdref import is_nan32, same_f32

LR = 0.01
# beta, mu, wd, nesterov: the paper's mu = beta; Nesterov with mu != beta and decay; a small mu with strong decay
HYPERS = {"H0": (0.9, 0.9, 0.0, False), "H1": (0.9, 0.8, 1e-2, True), "H2": (0.95, 0.5, 0.1, False)}
DEFAULT_KNOBS = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0, "stage_plain": 1}


class Kind:
    def __init__(self, name):
        assert name in ("f32", "mp32")
        self.name, self.mixed = name, name != "f32"
        self.base = "mx_qgm_mix_bf16" if self.mixed else "mx_qgm_mix"
        self.x = "w" if self.mixed else "x"
        self.tables = ("w", "g", "m", "p") if self.mixed else ("x", "g", "m")
        self.dtype = torch.bfloat16 if self.mixed else torch.float32

    def bits(self, k):
        """array k travels as bfloat16 bit patterns (uint16)"""
        return self.mixed and k in "gp"

    def tuning(self, pkg):
        E = pkg.engine
        return (E.qgm_mix_bf16_tuning, E.set_qgm_mix_bf16_tuning) if self.mixed else \
            (E.qgm_mix_tuning, E.set_qgm_mix_tuning)

    def __repr__(self):
        return self.name


KINDS = {k: Kind(k) for k in ("f32", "mp32")}


def tile(pkg, K, n):
    T = int(getattr(pkg.lib, K.base + "_tile")(n))
    assert T > 0
    return T


def shapes(pkg, K, n):
    T = tile(pkg, K, n)
    return [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, T - 1, T, T + 9, 3 * T + 5]


def hyper_of(hyper):
    return HYPERS[hyper] if isinstance(hyper, str) else hyper


def group(pkg, K, topo, P, hyper, zero, idle_rows="skip", **kw):
    beta, mu, wd, nesterov = hyper_of(hyper)
    grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows, dtype=K.dtype)
    grp.attach_qgm(momentum=beta, mu=mu, weight_decay=wd, nesterov=nesterov, zero_grads=zero,
                   master_weights=K.mixed, **kw)
    return grp


def _arr(grp, k):
    return {"x": grp.rows, "w": grp.master_rows, "g": grp.grads, "m": grp.qgm_buffer_rows, "p": grp.rows}[k]


def put(grp, K, **arrays):
    """x= (fp32 values: the rows, or the masters), g= (fp32 values or bfloat16 bit patterns, by kind), m="""
    for k, a in arrays.items():
        name = K.x if k == "x" else k
        t = _arr(grp, name)
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
        t = _arr(grp, name)
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
            ok = same_f32(got[k], want[k]) if nan_ok else qgmref.eq32(got[k], want[k])
        if not ok:
            return False
    return True


def g_bits(K, a):
    return a if K.mixed else qgmref.u32(a)


def same_state(K, a, b):
    return same(K, a, b, "xmp") and np.array_equal(g_bits(K, a["g"]), g_bits(K, b["g"]))


def tails_zero(grp, K, P):
    arenas = [grp.arena, grp.grad_arena, grp.qgm_buffer_arena] + ([grp.master_arena] if K.mixed else [])
    return all(not a[:, P:].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32).any().item() for a in arenas)


def g32(K, G):
    return bf16ref.upcast(G) if K.mixed else np.asarray(G, np.float32)


def rand_g(K, rng, shape, rowscale=None):
    """a gradient in the kind's format"""
    G = rng.standard_normal(shape).astype(np.float32)
    if rowscale is not None:
        G = (G * rowscale[:, None]).astype(np.float32)
    return bf16ref.rne_bf16(G) if K.mixed else G


def spec(O, K, s, G, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None):
    """the specification's {x, m, p, xp} after one round from state s with gradient G"""
    hyper = hyper_of(hyper)
    if K.mixed:
        x, m, p, xp = qgmref.spec_round_bf16(O, s["x"], G, s["m"], partner, flags, alpha, lr, hyper, idle_rows, scale,
                                             runs)
    else:
        x, m, xp = qgmref.spec_round(O, s["x"], G, s["m"], partner, flags, alpha, lr, hyper, idle_rows, scale, runs)
        p = None
    return {"x": x, "m": m, "p": p, "xp": xp}


def g_after(K, got, G, zero):
    return (not got["g"].any()) if zero else np.array_equal(g_bits(K, got["g"]), g_bits(K, G))


def special_case(K, where):
    """run_special_values' inputs: NaNs, +-Inf, +-0, subnormals and the largest finite values, with the counts
    of conftest.special_values (15 per row, 11 of which can make a NaN), planted in x, in g or in mh of an
    8 x 4099 group.  (s, G): the state {x, m} and the gradient in the kind's format."""
    n, P = 8, 4099
    rng = np.random.default_rng(31)
    s = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": rng.standard_normal((n, P)).astype(np.float32)}
    G = rand_g(K, rng, (n, P))
    if where == "x":
        s["x"] = np.stack([special_values(P, 100 + r) for r in range(n)])
    elif where == "g":
        G = np.stack([special_values(P, 200 + r) for r in range(n)])
        G = bf16ref.rne_bf16(G) if K.mixed else G        # NaN stays NaN, Inf Inf; +-FLT_MAX round to +-Inf
    else:
        s["m"] = np.stack([special_values(P, 300 + r) for r in range(n)])
    return s, G


def nan_outputs(want):
    """NaNs among the specification's x outputs"""
    return int(is_nan32(want["x"]).sum())


# 11 values per row can make a NaN (5 NaNs, 4 Infs, +-FLT_MAX), 8 rows, and each reaches at most the 8 rows of
# its column through the mix
NAN_BOUND = 11 * 8 * 8


# ---------------------------------------------------------------------------------------------- test bodies
def run_rounds(pkg, O, K, name, idle_rows, hyper):
    """three consecutive rounds of each flag kind at every shape, state carried, both zero_grads settings
    (alternating by shape); ring32 and er64 run the persistent grids, on two workgroups ("grid": 2), so that at
    the widths above one tile a workgroup finishes one work item with the next one's loads in flight: a buffer
    stored by the wrong lane, or a run taken from the prefetched item, shows there"""
    if name in ("ring32", "er64"):
        tuning, set_tuning = K.tuning(pkg)
        assert tuning()["grid"] == 0
        try:
            set_tuning(grid=2)
            _run_rounds(pkg, O, K, name, idle_rows, hyper)
        finally:
            set_tuning(grid=0)
    else:
        _run_rounds(pkg, O, K, name, idle_rows, hyper)


def _run_rounds(pkg, O, K, name, idle_rows, hyper):
    partner, alpha = topology(pkg, name)
    n = partner.shape[1]
    flags = flag_kinds(partner, 5)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([len(name), len(idle_rows), n, int(hyper[1]), len(K.name)])
    Ps = shapes(pkg, K, n)
    for pi, P in enumerate(Ps[-3:] if name == "er64" else Ps):
        zero = bool(pi & 1)
        grp = group(pkg, K, topo, P, hyper, zero, idle_rows)
        assert tuple(grp.qgm_buffer_rows.shape) == (n, P) and grp.qgm_buffer_arena.dtype == torch.float32
        assert tuple(grp.qgm_buffer_arena.shape) == (n, grp.ld) and grp.grad_arena.dtype == K.dtype
        s = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": np.zeros((n, P), np.float32)}
        put(grp, K, x=s["x"])
        for it in range(len(flags)):
            G = rand_g(K, rng, (n, P))
            put(grp, K, g=G)
            ran = grp.qgm_step(it, LR)
            got = state(grp, K)
            want = spec(O, K, s, G, partner, flags[it], alpha, LR, hyper, idle_rows)
            where = f"{K} {name} {idle_rows} {hyper} P={P} round {it}"
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the local step plus the buffer update: not a no-op
                assert qgmref.eq32(got["x"], want["xp"]) and not qgmref.eq32(got["x"], s["x"]), where
                assert not qgmref.eq32(got["m"], s["m"]), where
            for k in "xmp":
                assert same(K, got, want, k), where + ": " + k
            assert g_after(K, got, G, zero), where + ": g"
            assert tails_zero(grp, K, P), where + ": wrote past the row"
            s = got


def run_lr_zero(pkg, O, K):
    """lr = 0, and a run of lr_scale 0: the buffer keeps its bits while x is still mixed; the other columns of
    the grouped launch follow the specification"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    n = 8
    T = tile(pkg, K, n)
    P = 2 * T + 5
    flags = np.stack([np.ones(M, np.uint8), np.zeros(M, np.uint8)])
    rng = np.random.default_rng(17)
    s0 = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": rng.standard_normal((n, P)).astype(np.float32)}
    for mode in ("lr", "scale"):
        kw, runs, lr = {}, None, 0.0
        if mode == "scale":                          # a frozen run over a chunk, a work-item seam and the tile seam
            kw["param_groups"] = [{"columns": [(5, T + 3)], "lr_scale": 0.0}]
            wd = float(np.float32(HYPERS["H1"][2]))
            runs, lr = [(0, 5, wd, 1.0), (5, T + 3, wd, 0.0), (T + 3, P, wd, 1.0)], LR
        grp = group(pkg, K, Topo(partner, alpha, flags), P, "H1", True, **kw)
        put(grp, K, x=s0["x"], m=s0["m"])
        s = dict(s0)
        for it in range(2):
            G = rand_g(K, rng, (n, P))
            put(grp, K, g=G)
            grp.qgm_step(it, lr)
            got = state(grp, K)
            want = spec(O, K, s, G, partner, flags[it], alpha, lr, "H1", runs=runs)
            assert same(K, got, want), f"{K} {mode} round {it}"
            frozen = slice(0, P) if mode == "lr" else slice(5, T + 3)
            assert qgmref.eq32(got["m"][:, frozen], s["m"][:, frozen]), f"{K} {mode} round {it}: the buffer moved"
            if it == 0:                              # the active round still mixes the frozen columns
                assert not qgmref.eq32(got["x"][:, frozen], s["x"][:, frozen])
            else:                                    # the all-zero round at lr_r = 0 keeps x too
                assert qgmref.eq32(got["x"][:, frozen], s["x"][:, frozen])
            if mode == "scale":
                assert not qgmref.eq32(got["m"][:, :5], s["m"][:, :5])
            assert not got["g"].any() and tails_zero(grp, K, P)
            s = got


def run_noops(pkg, K):
    """a device counter outside the schedule and a peer-reads plan record: nothing is written -- x, the buffer
    and g compared bit for bit -- in the plain, the clipping and the grouped mode"""
    L = pkg.lib
    partner, alpha = topology(pkg, "g0")
    n, P = 8, 1300
    rng = np.random.default_rng(23)
    X = rng.standard_normal((n, P)).astype(np.float32)
    for kw in ({}, {"clip_grad_norm": 1.0}, {"param_groups": [{"columns": [(3, 700)], "lr_scale": 0.5}]}):
        grp = group(pkg, K, Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8)), P, "H1", True, **kw)
        put(grp, K, x=X, m=X * np.float32(0.5), g=rand_g(K, rng, (n, P)))
        before = state(grp, K)
        for counter in (2, 7, -1):                   # outside [0, T)
            grp.iter_dev.fill_(counter)
            grp.qgm_device_round()
        assert same_state(K, state(grp, K), before), f"{K} {kw}: past the schedule"
        args = (grp.engine.plan.data_ptr(), grp.engine.T + 1, grp.n_local, grp.engine.M)
        pkg._lib.check(L.mx_plan_set_peer_reads(*args, 1, pkg._lib.stream_ptr()))
        grp.qgm_step(0, LR)
        grp.iter_dev.fill_(0)
        grp.qgm_device_round()
        assert same_state(K, state(grp, K), before), f"{K} {kw}: peer-reads record"
        pkg._lib.check(L.mx_plan_set_peer_reads(*args, 0, pkg._lib.stream_ptr()))
        assert grp.qgm_step(0, LR)                   # the bit cleared: the same launch now writes
        after = state(grp, K)
        assert not same(K, after, before, "x") and not same(K, after, before, "m") and not after["g"].any()


def run_refusals(pkg, K):
    """the host-side refusals of the raw entry points: MX_ERR_INVALID, nothing written"""
    L, INVALID = pkg.lib, pkg._lib.MX_ERR_INVALID
    partner, alpha = topology(pkg, "g0")
    grp = group(pkg, K, Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8)), 300, "H1", True)
    rng = np.random.default_rng(51)
    X = rng.standard_normal((8, 300)).astype(np.float32)
    put(grp, K, x=X, m=X * np.float32(0.5), g=rand_g(K, rng, (8, 300)))
    before = state(grp, K)
    lay = grp._qgm.layout
    run, run_at = getattr(L, K.base), getattr(L, K.base + "_at")

    def refused(**fields):
        call = lay.call(grp.engine, 0.9, 0.8, 1e-2, True, True)
        for k, v in fields.items():
            setattr(call, k, v)
        s = pkg._lib.stream_ptr()
        return run(ctypes.addressof(call), 0, LR, None, s) == INVALID and \
            run_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, LR, None, s) == INVALID

    assert refused(n_slots=9) and refused(n_local=65, n_slots=65) and refused(M=33)
    assert refused(m_ptrs_dev=None) and b"buffer" in L.mx_last_error()
    assert refused(**{K.x + "_ptrs_dev": None}) and refused(g_ptrs_dev=None)
    if K.mixed:
        assert refused(p_ptrs_dev=None)
    call = lay.call(grp.engine, 0.9, 0.8, 1e-2, True, True)
    assert run_at(ctypes.addressof(call), None, 2, LR, None, pkg._lib.stream_ptr()) == INVALID
    assert same_state(K, state(grp, K), before)


def run_special_values(pkg, O, K, where):
    """NaNs, +-Inf, +-0, subnormals and the largest finite values planted in x, then g, then mh"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    s, G = special_case(K, where)
    n, P = s["x"].shape
    for fl in (np.ones(M, np.uint8), np.zeros(M, np.uint8)):
        grp = group(pkg, K, Topo(partner, alpha, fl[None, :]), P, "H1", False)
        put(grp, K, x=s["x"], g=G, m=s["m"])
        assert grp.qgm_step(0, LR) == bool(fl.any())
        got = state(grp, K)
        want = spec(O, K, s, G, partner, fl, alpha, LR, "H1")
        nan = nan_outputs(want)
        print(f"{K} special {where} flags {int(fl.any())}: {nan} NaN outputs of {n * P} in the specification")
        assert 0 < nan <= NAN_BOUND <= 0.05 * n * P     # on the spec itself: the comparison below compares something
        for k in "xmp":
            assert same(K, got, want, k, nan_ok=True), f"{where} {k}"
        assert g_after(K, got, G, False) and tails_zero(grp, K, P)


def _abi_offsets(K):
    """element offsets 0-7 per (array, segment, row): row 0 all aligned (the vector path); row 1 the 2-byte
    arrays 8-byte but not 16-byte aligned, the rest aligned (the vector path); row 2 every array one element
    off; row 3 the buffer alone off (the reload's own array); from row 4 on every offset 0-7 in turn"""
    def off(k, s, r):
        narrow = K.bits(k)
        if r == 0:
            return 0
        if r == 1:
            return 4 if narrow else 0
        if r == 2:
            return 1
        if r == 3:
            return 1 if k == "m" else 0
        return (r + 3 * s + 2 * K.tables.index(k)) % 8
    return off


def run_abi(pkg, O, K):
    """the raw entry point on four-segment tables (5, 0, T + 3, 130 elements) over padded buffers: bit-equal
    to the specification, guard words around every segment of x, g, mh and p untouched -- with zero_grads,
    so g is stored to; the reload after the round reads x and mh through the same tables"""
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
    for k in K.tables:
        offs = set(int(v) for v in (pt.start[k] - np.array(pt.base)).reshape(-1))
        assert offs == set(range(8)), (k, offs)
    cls = E.QgmBf16Layout if K.mixed else E.QgmLayout
    lay = cls(lens, *[pt.ptrs(k) for k in K.tables], n)
    assert lay.total_tiles == 4
    beta, mu, wd, nesterov = HYPERS["H1"]
    call = lay.call(eng, beta, mu, wd, nesterov, True)
    fn = getattr(pkg.lib, K.base)
    rng = np.random.default_rng(41)
    s = {"x": rng.standard_normal((n, pt.P)).astype(np.float32), "m": np.zeros((n, pt.P), np.float32)}
    pt.put(K.x, s["x"])
    pt.put("m", s["m"])
    for it in range(3):
        G = rand_g(K, rng, (n, pt.P))
        pt.put("g", G)
        assert fn(ctypes.addressof(call), it, LR, None, pkg._lib.stream_ptr()) == 0, pkg.lib.mx_last_error()
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, "H1")
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
    run rule) and both, with lionkit.run_scaled_grouped's run boundaries: one inside a 4-element chunk, one at
    a work-item seam and one at the tile seam, a run of one column, lr_scale 0; one row below the clip norm"""
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 8)[[6, 3, 0]]
    n = 8
    T = tile(pkg, K, n)
    P = 3 * T + 5
    wd = HYPERS["H1"][2]
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
    s = {"x": rng.standard_normal((n, P)).astype(np.float32), "m": np.zeros((n, P), np.float32)}
    put(grp, K, x=s["x"])
    rowscale = np.ones(n)
    rowscale[0] = 1e-4                               # row 0 stays below the norm, the others are clipped
    for it in range(3):
        G = rand_g(K, rng, (n, P), rowscale)
        put(grp, K, g=G)
        grp.qgm_step(it, LR)
        got = state(grp, K)
        scale = None
        if mode != "groups":
            norms, scale = grp.grad_norms.cpu().numpy(), grp.grad_scales.cpu().numpy()
            ref = clipref.grad_norm_ref(g32(K, G))                       # the norm before clipping
            assert int(clipref.ulp_diff(norms, ref).max()) <= 1
            assert qgmref.eq32(scale, clipref.clip_scale_ref(norms, 1.0))
            assert scale[0] == 1.0 and (scale[1:] < 1.0).all()
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, "H1", scale=scale, runs=runs)
        for k in "xmp":
            assert same(K, got, want, k), f"{K} {mode} round {it}: {k}"
        assert not got["g"].any() and tails_zero(grp, K, P)
        if runs is not None:                                             # lr_scale 0: the buffer is frozen
            assert qgmref.eq32(got["m"][:, 512:T], s["m"][:, 512:T])
        s = got


def run_graph_replay(pkg, O, K):
    """qgm_device_round captured once and replayed over a 6-round schedule with fresh gradients and a
    learning rate changed after round 3 through lr_dev == six qgm_step calls on a twin (themselves the
    specification's); two replays past the schedule write nothing"""
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    n, P = 8, 2 * tile(pkg, K, 8) + 77
    rng = np.random.default_rng(61)
    X0 = rng.standard_normal((n, P)).astype(np.float32)
    Gs = [rand_g(K, rng, (n, P)) for _ in range(7)]
    lrs = [0.01, 0.01, 0.01, 0.01, 0.0025, 0.0025]
    eager = group(pkg, K, topo, P, "H1", True)
    put(eager, K, x=X0)
    s = {"x": X0, "m": np.zeros((n, P), np.float32)}
    for it in range(6):
        put(eager, K, g=Gs[it])
        eager.qgm_step(it, lrs[it])
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
            grp.qgm_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and qgmref.eq32(state(grp, K)["x"], X0)      # capture ran nothing
    for it in range(6):
        put(grp, K, g=Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = state(grp, K)
    assert same_state(K, got, want)
    put(grp, K, g=Gs[6])                             # past the schedule: no step, the buffer and g untouched
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
    grp = group(pkg, K, Topo(partner, alpha, flags), P, "H1", True)
    put(grp, K, x=rng.standard_normal((n, P)).astype(np.float32))
    for it in range(3):
        put(grp, K, g=rand_g(K, rng, (n, P)))
        grp.qgm_step(it, LR)
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
    """a round trip continues bit for bit; a QGM checkpoint is refused by the other optimizers' groups, by a
    group without an optimizer and by a QGM group of another shape, and a QGM group refuses theirs; without
    the key the buffer is zeroed"""
    partner, alpha = topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((4, partner.shape[0]), np.uint8))
    n, P = 8, 1300
    rng = np.random.default_rng(71)
    Gs = [rand_g(K, rng, (n, P)) for _ in range(4)]

    def steps(g, its):
        for it in its:
            put(g, K, g=Gs[it])
            g.qgm_step(it, LR)

    grp = group(pkg, K, topo, P, "H1", True)
    put(grp, K, x=rng.standard_normal((n, P)).astype(np.float32))
    steps(grp, range(2))
    grp.iter = 2
    ckpt = grp.state_dict()
    keys = {"kind", "iter", "row_base", "workers", "rows", "qgm_buffer_rows"} | ({"master_rows"} if K.mixed else set())
    assert set(ckpt) == keys and ckpt["qgm_buffer_rows"].dtype == torch.float32
    assert tuple(ckpt["qgm_buffer_rows"].shape) == (n, P) and ckpt["qgm_buffer_rows"].abs().max().item() > 0
    twin = group(pkg, K, topo, P, "H1", True)
    twin.load_state_dict(ckpt)
    assert twin.iter == 2 and same_state(K, state(twin, K), state(grp, K))
    steps(grp, range(2, 4))
    steps(twin, range(2, 4))
    assert same_state(K, state(twin, K), state(grp, K))              # continues bit for bit
    twin.load_state_dict({k: v for k, v in ckpt.items() if k != "qgm_buffer_rows"})
    assert not twin.qgm_buffer_rows.view(torch.int32).any().item()
    kw = {"dtype": K.dtype}
    others = {}
    for opt, attach in (("sgd", {"momentum": 0.9}), ("adamw", {}), ("lion", {})):
        g = pkg.VirtualWorkerGroup(topo, numel=P, **kw)
        getattr(g, "attach_" + opt)(master_weights=K.mixed, **attach)
        with pytest_raises(ValueError, "quasi-global momentum"):
            g.load_state_dict(ckpt)
        others[opt] = g
    with pytest_raises(ValueError, "quasi-global momentum"):
        pkg.VirtualWorkerGroup(topo, numel=P, **kw).load_state_dict({k: v for k, v in ckpt.items() if k != "master_rows"})
    for opt, word in (("sgd", "momentum"), ("adamw", "Adam"), ("lion", "Lion")):
        with pytest_raises(ValueError, word):
            twin.load_state_dict(others[opt].state_dict())
    assert set(others["sgd"].state_dict()) == (keys - {"qgm_buffer_rows"}) | {"momentum_rows"}      # untouched
    with pytest_raises(ValueError, "quasi-global momentum"):         # another shape
        group(pkg, K, topo, P + 1, "H1", True).load_state_dict({**ckpt, "rows": twin.arena[:, :P + 1].clone(), **(
            {"master_rows": twin.master_arena[:, :P + 1].clone()} if K.mixed else {})})


def run_attach_errors(pkg, K):
    partner, alpha = topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))

    def fresh():
        return pkg.VirtualWorkerGroup(topo, numel=100, dtype=K.dtype)

    mw = {"master_weights": K.mixed}
    grp = fresh()
    with pytest_raises(pkg.MXError, r"no QGM state: call attach_qgm\(\) first"):
        grp.qgm_step(0, LR)
    grp.attach_qgm(**mw)
    assert grp.qgm_hyper == {"momentum": 0.9, "mu": 0.9, "weight_decay": 0.0, "nesterov": False, "zero_grads": True}
    with pytest_raises(RuntimeError, "attach_qgm: already attached"):
        grp.attach_qgm(**mw)
    for opt in ("sgd", "adamw", "lion"):
        with pytest_raises(RuntimeError, rf"attach_{opt}: the group already carries QGM state \(attach_qgm\)"):
            getattr(grp, "attach_" + opt)(**mw)
    with pytest_raises(pkg.MXError, "no SGD state"):
        grp.sgd_step(0, LR)
    for opt, name in (("sgd", "SGD"), ("adamw", "AdamW"), ("lion", "Lion")):
        g = fresh()
        getattr(g, "attach_" + opt)(**mw)
        with pytest_raises(RuntimeError, rf"attach_qgm: the group already carries {name} state \(attach_{opt}\)"):
            g.attach_qgm(**mw)
    g = fresh()                                      # the existing pairs' texts are as they were
    g.attach_sgd(**mw)
    with pytest_raises(RuntimeError, r"attach_adamw: the group already carries SGD state \(attach_sgd\)"):
        g.attach_adamw(**mw)
    with pytest_raises(RuntimeError, r"attach_lion: the group already carries SGD state \(attach_sgd\)"):
        g.attach_lion(**mw)
    for bad in ({"momentum": 1.0}, {"momentum": -0.1}, {"mu": 1.0}, {"mu": -0.5}, {"weight_decay": -1.0},
                {"clip_grad_norm": 0.0}):
        with pytest_raises(ValueError, "attach_qgm"):
            fresh().attach_qgm(**{**mw, **bad})
    if K.mixed:
        with pytest_raises(NotImplementedError, "bfloat16 groups need fp32 master weights under quasi-global momentum"):
            fresh().attach_qgm()
    else:
        with pytest_raises(ValueError, "master_weights"):
            fresh().attach_qgm(master_weights=True)


def run_trainer(pkg, O, K):
    """harness.VirtualTrainer(fused_qgm=True): every iteration's fused launch by the specification from the
    rows, gradients and buffer the backward passes left, with clipping and a no-decay group honoured; the
    torch optimizers never step; a checkpoint resumed in a new trainer continues bit for bit"""
    H = pkg.harness
    hyper = {"momentum": 0.9, "mu": 0.8, "weight_decay": 1e-2, "nesterov": True}
    groups = [{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}]

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=1e-3, matcha=True, warmup=False)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        fn = H.model_factory(args)
        return H.VirtualTrainer(args, (lambda: fn().to(torch.bfloat16)) if K.mixed else fn, n_batches=3,
                                **{"fused_qgm": True, "qgm_hyper": hyper, "clip_grad_norm": 0.5,
                                   "param_groups": groups, **kw})

    tr = make()
    grp = tr.group
    assert grp.dtype == K.dtype and grp.qgm_buffer_arena.dtype == torch.float32 and (grp.master_rows is not None) == K.mixed
    assert grp.qgm_hyper["momentum"] == 0.9 and grp.qgm_hyper["mu"] == 0.8 and grp.qgm_hyper["nesterov"] is True
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
                    (0.9, 0.8, 1e-2, True), scale=scale, runs=runs)
        assert same(K, got, want) and not got["g"].any(), f"round {before['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats) and "grad_norm" in stats[0]
    assert seen["rounds"] == 3 and grp.iter == 3 and len(tr.grad_norm_log) == 3
    assert all(not o.state for o in tr.optimizers)                   # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert "qgm_buffer_rows" in ckpt["group"]
    tr2 = make()
    tr2.load_state_dict(ckpt)
    tr.train_epoch()
    tr2.train_epoch()
    assert same_state(K, state(tr.group, K), state(tr2.group, K)) and tr.group.iter == tr2.group.iter == 6
    for kw in ({"fused_sgd": True}, {"fused_adamw": True}, {"fused_lion": True}):
        with pytest_raises(ValueError, "mutually exclusive"):
            make(**kw)
    with pytest_raises(ValueError, "fused_qgm"):
        make(batched=True)
    with pytest_raises(ValueError, "fused_qgm"):
        make(args={"compress": True})
