"""What tests/test_gpu_gt_mix.py and tests/test_gpu_gt_mix_bf16.py share -- test helper: the two forms of gradient
tracking's launch pair behind one description (Kind) and the test bodies, which the two files parametrise.  The
topologies and the flag kinds are tests/lionkit.py's.

    f32    csrc/gt_track.hip + the fused SGD kernel (mx_sgd_mix) over the trackers    x, g, y, gp, m fp32
    mp32   csrc/gt_track_bf16.hip + csrc/gt_step_bf16.hip    fp32 masters w, bf16 g and p, fp32 y, gp, m

State keys: x (the rows, or the masters), y (the tracker), gp (the previous gradient), m (the momentum; None
without), g, p (the bfloat16 rows; None for f32).  Every comparison is against tests/gtref.py, never the code
under test: x / y / gp / m uint32 for uint32, p uint16 for uint16.  A NaN of any payload passes where the
specification is a NaN in run_special_values only (nan_ok)."""
import ctypes

import numpy as np
import torch

import bf16ref
import clipref
import gtref
from abitables import PaddedTables
from conftest import Topo, special_values
from lionkit import flag_kinds, pytest_raises, topology
from sgdref import is_nan32, same_f32

LR = 0.01
# wd, mom, nesterov: plain tracking; momentum with decay; Nesterov
HYPERS = {"H0": (0.0, 0.0, False), "H1": (1e-2, 0.9, False), "H2": (1e-2, 0.9, True)}
DEFAULT_KNOBS = {"nontemporal": 2, "wgpc": 0, "blocks_per_cu": 2, "flat_small": 256, "grid": 0}
STATE = ("x", "y", "gp", "m", "p")
_IDX = np.arange(8)
RING8 = np.stack([_IDX ^ 1, np.where(_IDX & 1, (_IDX + 1) % 8, (_IDX - 1) % 8)]).astype(np.int32)


class Kind:
    def __init__(self, name):
        assert name in ("f32", "mp32")
        self.name, self.mixed = name, name != "f32"
        self.track = "mx_gt_track_bf16" if self.mixed else "mx_gt_track"
        self.step = "mx_gt_step_bf16" if self.mixed else "mx_sgd_mix"
        self.base = self.track                       # the tile is every fused family's
        self.dtype = torch.bfloat16 if self.mixed else torch.float32
        self.arrays = ("x", "g", "y", "gp", "m", "p") if self.mixed else ("x", "g", "y", "gp", "m")

    def bits(self, k):
        """array k travels as bfloat16 bit patterns (uint16)"""
        return self.mixed and k in ("g", "p")

    def tunings(self, pkg):
        """(tuning, set_tuning) of the new families this kind launches"""
        E = pkg.engine
        if self.mixed:
            return [(E.gt_track_bf16_tuning, E.set_gt_track_bf16_tuning), (E.gt_step_bf16_tuning, E.set_gt_step_bf16_tuning)]
        return [(E.gt_track_tuning, E.set_gt_track_tuning)]

    def layouts(self, pkg):
        E = pkg.engine
        return (E.GtTrackBf16Layout, E.GtStepBf16Layout) if self.mixed else (E.GtTrackLayout, E.SgdLayout)

    def step_call(self, lay, eng, hyper):
        wd, mom, nesterov = hyper
        return lay.call(eng, wd, mom, nesterov) if self.mixed else lay.call(eng, wd, mom, nesterov, False)

    def __repr__(self):
        return self.name


KINDS = {k: Kind(k) for k in ("f32", "mp32")}


def tile(pkg, K, n):
    T = int(getattr(pkg.lib, K.base + "_tile")(n))
    assert T > 0 and T == int(getattr(pkg.lib, K.step + "_tile")(n))
    return T


def shapes(pkg, K, n):
    T = tile(pkg, K, n)
    return [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, T - 1, T, T + 9, 3 * T + 5]


def hyper_of(hyper):
    return HYPERS[hyper] if isinstance(hyper, str) else hyper


def group(pkg, K, topo, P, hyper, zero, idle_rows="skip", **kw):
    wd, mom, nesterov = hyper_of(hyper)
    grp = pkg.VirtualWorkerGroup(topo, numel=P, idle_rows=idle_rows, dtype=K.dtype)
    grp.attach_gt(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=zero, master_weights=K.mixed, **kw)
    return grp


def _arr(grp, K, k):
    return {"x": grp.master_rows if K.mixed else grp.rows, "g": grp.grads, "y": grp.gt_tracker_rows,
            "gp": grp.gt_prev_grad_rows, "m": grp.momentum_rows, "p": grp.rows}[k]


def put(grp, K, **arrays):
    """x= (fp32 values: the rows, or the masters), g= (fp32 values or bfloat16 bit patterns, by kind), y=, gp=,
    m= (None is skipped: a group without momentum)"""
    for k, a in arrays.items():
        if a is None:
            continue
        t = _arr(grp, K, k)
        if K.bits(k):
            t.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)))
        else:
            t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


def state(grp, K):
    """host copies {x, y, gp, m, g, p}: fp32 arrays or bit patterns by kind"""
    torch.cuda.synchronize()
    out = {}
    for k in ("x", "y", "gp", "m", "g", "p"):
        t = _arr(grp, K, k) if (k != "p" or K.mixed) else None
        if t is None:
            out[k] = None
        else:
            out[k] = t.view(torch.int16).cpu().numpy().view(np.uint16) if K.bits(k) else t.cpu().numpy()
    return out


def same(K, got, want, keys=STATE, nan_ok=False):
    for k in keys:
        if want[k] is None:
            if got[k] is not None and k != "p":
                return False
            continue
        if K.bits(k):
            ok = bf16ref.same_bf16(got[k], want[k]) if nan_ok else np.array_equal(got[k], want[k])
        else:
            ok = same_f32(got[k], want[k]) if nan_ok else gtref.eq32(got[k], want[k])
        if not ok:
            return False
    return True


def g_bits(K, a):
    return a if K.mixed else gtref.u32(a)


def same_state(K, a, b):
    return same(K, a, b) and np.array_equal(g_bits(K, a["g"]), g_bits(K, b["g"]))


def _arenas(grp, K):
    out = [grp.arena, grp.grad_arena, grp.gt_tracker_arena, grp.gt_prev_grad_arena]
    return out + ([grp.mom_arena] if grp.mom_arena is not None else []) + ([grp.master_arena] if K.mixed else [])


def tails_zero(grp, K, P):
    return all(not a[:, P:].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32).any().item()
               for a in _arenas(grp, K))


def g32(K, G):
    return bf16ref.upcast(G) if K.mixed else np.asarray(G, np.float32)


def rand_g(K, rng, shape, rowscale=None):
    """a gradient in the kind's format"""
    G = rng.standard_normal(shape).astype(np.float32)
    if rowscale is not None:
        G = (G * rowscale[:, None]).astype(np.float32)
    return bf16ref.rne_bf16(G) if K.mixed else G


def zero_state(n, P, hyper, x):
    mom = hyper_of(hyper)[1]
    z = np.zeros((n, P), np.float32)
    return {"x": x, "y": z.copy(), "gp": z.copy(), "m": z.copy() if mom != 0 else None}


def spec(O, K, s, G, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None):
    """the specification's {x, y, gp, m, p, yp, xp} after one iteration from state s with gradient G"""
    return gtref.spec_round(O, s, G, partner, flags, alpha, lr, hyper_of(hyper), idle_rows, scale, runs, K.mixed)


def g_after(K, got, G, zero):
    return (not got["g"].any()) if zero else np.array_equal(g_bits(K, got["g"]), g_bits(K, G))


def launch_track(pkg, grp, it):
    st = grp._gt.track
    pkg._lib.check(st.run(st.addr, it, LR, None, pkg._lib.stream_ptr()), st.base)


def launch_step(pkg, grp, it, lr):
    st = grp._gt.step
    pkg._lib.check(st.run(st.addr, it, lr, None, pkg._lib.stream_ptr()), st.base)


# ---------------------------------------------------------------------------------------------- test bodies
def run_rounds(pkg, O, K, name, idle_rows, hyper):
    """three consecutive rounds of each flag kind at every shape, y, gp and m carried, both zero_grads settings
    (alternating by shape); ring32 and er64 run the persistent grids, on two workgroups ("grid": 2), so that at
    the widths above one tile a workgroup finishes one work item with the next one's loads in flight"""
    if name in ("ring32", "er64"):
        pairs = K.tunings(pkg) + ([] if K.mixed else [(pkg.engine.sgd_mix_tuning, pkg.engine.set_sgd_mix_tuning)])
        assert all(t()["grid"] == 0 for t, _ in pairs)
        try:
            for _, set_tuning in pairs:
                set_tuning(grid=2)
            _run_rounds(pkg, O, K, name, idle_rows, hyper)
        finally:
            for _, set_tuning in pairs:
                set_tuning(grid=0)
    else:
        _run_rounds(pkg, O, K, name, idle_rows, hyper)


def _run_rounds(pkg, O, K, name, idle_rows, hyper):
    partner, alpha = topology(pkg, name)
    n = partner.shape[1]
    flags = flag_kinds(partner, 5)
    topo = Topo(partner, alpha, flags)
    rng = np.random.default_rng([len(name), len(idle_rows), n, int(hyper[1]), len(K.name), 7])
    Ps = shapes(pkg, K, n)
    mom = hyper_of(hyper)[1]
    for pi, P in enumerate(Ps[-3:] if name == "er64" else Ps):
        zero = bool(pi & 1)
        grp = group(pkg, K, topo, P, hyper, zero, idle_rows)
        for a in (grp.gt_tracker_arena, grp.gt_prev_grad_arena):
            assert tuple(a.shape) == (n, grp.ld) and a.dtype == torch.float32 and not a.any().item()
        assert tuple(grp.gt_tracker_rows.shape) == tuple(grp.gt_prev_grad_rows.shape) == (n, P)
        assert grp.grad_arena.dtype == K.dtype and (grp.momentum_rows is not None) == (mom != 0)
        s = zero_state(n, P, hyper, rng.standard_normal((n, P)).astype(np.float32))
        put(grp, K, x=s["x"])
        for it in range(len(flags)):
            G = rand_g(K, rng, (n, P))
            put(grp, K, g=G)
            want = spec(O, K, s, G, partner, flags[it], alpha, LR, hyper, idle_rows)
            where = f"{K} {name} {idle_rows} {hyper} P={P} round {it}"
            if it % 3 == 1:                          # the two launches one by one, the state between them looked at
                launch_track(pkg, grp, it)
                mid = state(grp, K)
                assert same(K, mid, want, ("y", "gp")), where + ": after the track launch"
                assert same(K, mid, s, ("x", "m")), where + ": the track launch wrote x or m"
                assert g_after(K, mid, G, zero), where + ": g after the track launch"
                launch_step(pkg, grp, it, LR)
                ran = bool(flags[it].any())
            else:
                ran = grp.gt_step(it, LR)
            got = state(grp, K)
            assert ran == bool(flags[it].any()), where
            if not flags[it].any():                  # the tracker takes in g and x steps: not a no-op
                assert gtref.eq32(got["y"], want["yp"]) and gtref.eq32(got["x"], want["xp"]), where
                assert not gtref.eq32(got["x"], s["x"]) and not gtref.eq32(got["y"], s["y"]), where
            if it == 0:                              # from zeros the tracker's first value is the gradient itself
                assert gtref.eq32(want["yp"], g32(K, G))
            for k in STATE:
                assert same(K, got, want, (k,)), where + ": " + k
            assert g_after(K, got, G, zero), where + ": g"
            assert tails_zero(grp, K, P), where + ": wrote past the row"
            s = got


def run_lr_scale_zero(pkg, O, K):
    """a run of lr_scale 0 freezes x (bit for bit on an all-zero round; still mixed on an active one) while its
    tracker still moves; the other columns follow the specification"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    n = 8
    T = tile(pkg, K, n)
    P = 2 * T + 5
    flags = np.stack([np.ones(M, np.uint8), np.zeros(M, np.uint8)])
    rng = np.random.default_rng(17)
    wd = float(np.float32(HYPERS["H1"][0]))
    runs = [(0, 5, wd, 1.0), (5, T + 3, wd, 0.0), (T + 3, P, wd, 1.0)]   # frozen over a chunk, a work-item seam, the tile seam
    grp = group(pkg, K, Topo(partner, alpha, flags), P, "H1", True, param_groups=[{"columns": [(5, T + 3)], "lr_scale": 0.0}])
    assert grp.param_runs == runs
    s = {k: rng.standard_normal((n, P)).astype(np.float32) for k in ("x", "y", "gp", "m")}
    put(grp, K, **s)
    frozen = slice(5, T + 3)
    for it in range(2):
        G = rand_g(K, rng, (n, P))
        put(grp, K, g=G)
        grp.gt_step(it, LR)
        got = state(grp, K)
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, "H1", runs=runs)
        assert same(K, got, want), f"{K} round {it}"
        assert not gtref.eq32(got["y"][:, frozen], s["y"][:, frozen]), f"{K} round {it}: the tracker stood still"
        if it == 0:                                  # the active round still mixes the frozen columns
            assert not gtref.eq32(got["x"][:, frozen], s["x"][:, frozen])
        else:                                        # the all-zero round at lr_r = 0 keeps x
            assert gtref.eq32(got["x"][:, frozen], s["x"][:, frozen])
        assert not gtref.eq32(got["x"][:, :5], s["x"][:, :5])
        assert not got["g"].any() and tails_zero(grp, K, P)
        s = got


def run_noops(pkg, K):
    """a device counter outside the schedule and a peer-reads plan record: nothing is written by either launch --
    x, y, gp, m and g compared bit for bit -- in the plain, the clipping and the grouped mode"""
    L = pkg.lib
    partner, alpha = topology(pkg, "g0")
    n, P = 8, 1300
    rng = np.random.default_rng(23)
    for kw in ({}, {"clip_grad_norm": 1.0}, {"param_groups": [{"columns": [(3, 700)], "lr_scale": 0.5}]}):
        grp = group(pkg, K, Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8)), P, "H1", True, **kw)
        put(grp, K, g=rand_g(K, rng, (n, P)), **{k: rng.standard_normal((n, P)).astype(np.float32) for k in ("x", "y", "gp", "m")})
        before = state(grp, K)
        for counter in (2, 7, -1):                   # outside [0, T)
            grp.iter_dev.fill_(counter)
            grp.gt_device_round()
        assert same_state(K, state(grp, K), before), f"{K} {kw}: past the schedule"
        args = (grp.engine.plan.data_ptr(), grp.engine.T + 1, grp.n_local, grp.engine.M)
        pkg._lib.check(L.mx_plan_set_peer_reads(*args, 1, pkg._lib.stream_ptr()))
        grp.gt_step(0, LR)
        grp.iter_dev.fill_(0)
        grp.gt_device_round()
        assert same_state(K, state(grp, K), before), f"{K} {kw}: peer-reads record"
        pkg._lib.check(L.mx_plan_set_peer_reads(*args, 0, pkg._lib.stream_ptr()))
        assert grp.gt_step(0, LR)                    # the bit cleared: the same launches now write
        after = state(grp, K)
        assert not any(same(K, after, before, (k,)) for k in ("x", "y", "gp", "m")) and not after["g"].any()


def run_refusals(pkg, K):
    """the host-side refusals of the raw entry points: MX_ERR_INVALID, nothing written"""
    L, INVALID = pkg.lib, pkg._lib.MX_ERR_INVALID
    partner, alpha = topology(pkg, "g0")
    grp = group(pkg, K, Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8)), 300, "H1", True)
    rng = np.random.default_rng(51)
    put(grp, K, g=rand_g(K, rng, (8, 300)), **{k: rng.standard_normal((8, 300)).astype(np.float32) for k in ("x", "y", "gp", "m")})
    before = state(grp, K)
    s = pkg._lib.stream_ptr()
    scale = torch.ones(8, dtype=torch.float32, device="cuda")

    def refused(base, make, it=0, **fields):
        call = make()
        for k, v in fields.items():
            setattr(call, k, v)
        return getattr(L, base)(ctypes.addressof(call), it, LR, None, s) == INVALID and \
            getattr(L, base + "_at")(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, LR, None, s) == INVALID and \
            getattr(L, base + "_scaled")(ctypes.addressof(call), None, it, LR, None, s) == INVALID

    track = lambda: grp._gt.track.layout.call(grp.engine, True)
    assert refused(K.track, track, n_slots=9) and refused(K.track, track, n_local=65, n_slots=65)
    assert refused(K.track, track, M=33) and refused(K.track, track, M=0)
    for t in ("x_ptrs_dev", "g_ptrs_dev", "gp_ptrs_dev", "seg_len_dev", "plan_dev"):
        assert refused(K.track, track, **{t: None}) and b"null pointer" in L.mx_last_error(), t
    call = track()
    assert getattr(L, K.track)(ctypes.addressof(call), -1, LR, None, s) == INVALID and b"iter < 0" in L.mx_last_error()
    assert getattr(L, K.track + "_at")(ctypes.addressof(call), None, 2, LR, None, s) == INVALID
    if K.mixed:                                      # the fp32 step launch is mx_sgd_mix, whose refusals have their tests
        step = lambda: grp._gt.step.layout.call(grp.engine, 1e-2, 0.9, False)
        assert refused(K.step, step, zero_grads=1) and b"zero_grads" in L.mx_last_error()
        assert refused(K.step, step, n_slots=9) and refused(K.step, step, M=33)
        for t in ("w_ptrs_dev", "g_ptrs_dev", "m_ptrs_dev", "p_ptrs_dev"):
            assert refused(K.step, step, **{t: None}), t
        call = step()
        assert getattr(L, K.step)(ctypes.addressof(call), -1, LR, None, s) == INVALID and b"iter < 0" in L.mx_last_error()
        assert getattr(L, K.step + "_scaled")(ctypes.addressof(call), scale.data_ptr(), 0, LR, None, s) == INVALID
        assert b"clip factors" in L.mx_last_error()
    assert same_state(K, state(grp, K), before)


def special_case(K, where):
    """run_special_values' inputs: NaNs, +-Inf, +-0, subnormals and the largest finite values, with the counts of
    conftest.special_values (15 per row, 11 of which can make a NaN), planted in g, gp, y or x of an 8 x 4099
    group.  (s, G): the state {x, y, gp, m} and the gradient in the kind's format."""
    n, P = 8, 4099
    rng = np.random.default_rng(31)
    s = {k: rng.standard_normal((n, P)).astype(np.float32) for k in ("x", "y", "gp", "m")}
    G = rand_g(K, rng, (n, P))
    seed = {"x": 100, "g": 200, "gp": 300, "y": 400}[where]
    planted = np.stack([special_values(P, seed + r) for r in range(n)])
    if where == "g":
        G = bf16ref.rne_bf16(planted) if K.mixed else planted      # NaN stays NaN, Inf Inf; +-FLT_MAX round to +-Inf
    else:
        s[where] = planted
    return s, G


# 11 values per row can make a NaN (5 NaNs, 4 Infs, +-FLT_MAX), 8 rows, and each reaches at most the 8 rows of its
# column through the two mixes
NAN_BOUND = 11 * 8 * 8


def nan_outputs(want):
    """NaNs among the specification's outputs: the most in any of y and x"""
    return max(int(is_nan32(want["x"]).sum()), int(is_nan32(want["y"]).sum()))


def run_special_values(pkg, O, K, where):
    """NaNs, +-Inf, +-0, subnormals and the largest finite values planted in g, gp, y or x"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    s, G = special_case(K, where)
    n, P = s["x"].shape
    for fl in (np.ones(M, np.uint8), np.zeros(M, np.uint8)):
        grp = group(pkg, K, Topo(partner, alpha, fl[None, :]), P, "H2", False)
        put(grp, K, g=G, **s)
        assert grp.gt_step(0, LR) == bool(fl.any())
        got = state(grp, K)
        want = spec(O, K, s, G, partner, fl, alpha, LR, "H2")
        nan = nan_outputs(want)
        print(f"{K} special {where} flags {int(fl.any())}: {nan} NaN outputs of {n * P} in the specification")
        assert 0 < nan <= NAN_BOUND <= 0.05 * n * P     # on the spec itself: the comparison below compares something
        for k in STATE:
            assert same(K, got, want, (k,), nan_ok=True), f"{where} {k}"
        assert g_after(K, got, G, False) and tails_zero(grp, K, P)


def _abi_offsets(K):
    """element offsets 0-7 per (array, segment, row): row 0 all aligned (the vector path); row 1 the 2-byte arrays
    8-byte but not 16-byte aligned, the rest aligned (the vector path); row 2 every array one element off; row 3
    the previous gradient alone off, row 4 the tracker alone (the fp32 "gradient" of the step launch); from row 5
    on every offset 0-7 in turn"""
    def off(k, s, r):
        if r == 0:
            return 0
        if r == 1:
            return 4 if K.bits(k) else 0
        if r == 2:
            return 1
        if r == 3:
            return 1 if k == "gp" else 0
        if r == 4:
            return 2 if k == "y" else 0
        return (r + 3 * s + 2 * K.arrays.index(k)) % 8
    return off


def run_abi(pkg, O, K):
    """the raw entry points on four-segment tables (5, 0, T + 3, 130 elements) over padded buffers, rows at every
    alignment (so the per-element path of the bf16-gradient and fp32-gradient forms runs beside the vector path):
    bit-equal to the specification after each launch, guard words around every segment of every array -- the
    one after gp included -- untouched, with zero_grads, so g is stored to"""
    partner, alpha = topology(pkg, "g0")
    M = partner.shape[0]
    flags = np.stack([np.ones(M, np.uint8), flag_kinds(partner, 3)[3], np.zeros(M, np.uint8)])
    eng = pkg.GossipEngine(Topo(partner, alpha, flags))
    n = 8
    T = tile(pkg, K, n)
    lens = [5, 0, T + 3, 130]
    pt = PaddedTables(n, lens, {k: np.uint16 if K.bits(k) else np.float32 for k in K.arrays}, _abi_offsets(K))
    for k in K.arrays:
        offs = set(int(v) for v in (pt.start[k] - np.array(pt.base)).reshape(-1))
        assert offs == set(range(8)), (k, offs)
    track_cls, step_cls = K.layouts(pkg)
    tlay = track_cls(lens, pt.ptrs("y"), pt.ptrs("g"), pt.ptrs("gp"), n)
    slay = step_cls(lens, pt.ptrs("x"), pt.ptrs("y"), pt.ptrs("m"), *([pt.ptrs("p")] if K.mixed else []), n)
    assert tlay.total_tiles == slay.total_tiles == 4
    hyper = HYPERS["H2"]
    tcall, scall = tlay.call(eng, True), K.step_call(slay, eng, hyper)
    track, step = getattr(pkg.lib, K.track), getattr(pkg.lib, K.step)
    rng = np.random.default_rng(41)
    s = zero_state(n, pt.P, hyper, rng.standard_normal((n, pt.P)).astype(np.float32))
    for k in ("x", "y", "gp", "m"):
        pt.put(k, s[k])

    def held():
        return {"x": pt.get("x"), "y": pt.get("y"), "gp": pt.get("gp"), "m": pt.get("m"), "p": pt.get("p") if K.mixed else None}

    for it in range(3):
        G = rand_g(K, rng, (n, pt.P))
        pt.put("g", G)
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, hyper)
        where = f"{K} round {it}"
        assert track(ctypes.addressof(tcall), it, LR, None, pkg._lib.stream_ptr()) == 0, pkg.lib.mx_last_error()
        mid = held()
        assert same(K, mid, want, ("y", "gp")) and same(K, mid, s, ("x", "m")), where + ": after the track launch"
        assert not pt.get("g").any(), where + ": g not zeroed within the lengths"
        assert step(ctypes.addressof(scall), it, LR, None, pkg._lib.stream_ptr()) == 0, pkg.lib.mx_last_error()
        got = held()
        for k in STATE:
            assert same(K, got, want, (k,)), where + ": " + k
        for k in K.arrays:
            assert pt.guards_intact(k), where + f": guard words of {k}"
        s = got


def run_scaled_grouped(pkg, O, K, mode):
    """clip_grad_norm (the track launch's _scaled entry points, against clipref: the factor enters gs and gp),
    param_groups (the step launch's _grouped, against groupref's run rule: the runs change only the step) and
    both, with lionkit.run_scaled_grouped's run boundaries"""
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 8)[[6, 3, 0]]
    n = 8
    T = tile(pkg, K, n)
    P = 3 * T + 5
    wd = HYPERS["H1"][0]
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
    s = zero_state(n, P, "H1", rng.standard_normal((n, P)).astype(np.float32))
    put(grp, K, x=s["x"])
    rowscale = np.ones(n)
    rowscale[0] = 1e-4                               # row 0 stays below the norm, the others are clipped
    for it in range(3):
        G = rand_g(K, rng, (n, P), rowscale)
        put(grp, K, g=G)
        grp.gt_step(it, LR)
        got = state(grp, K)
        scale = None
        if mode != "groups":
            norms, scale = grp.grad_norms.cpu().numpy(), grp.grad_scales.cpu().numpy()
            ref = clipref.grad_norm_ref(g32(K, G))                       # the norm before clipping
            assert int(clipref.ulp_diff(norms, ref).max()) <= 1
            assert gtref.eq32(scale, clipref.clip_scale_ref(norms, 1.0))
            assert scale[0] == 1.0 and (scale[1:] < 1.0).all()
            assert gtref.eq32(got["gp"], clipref.scale_grad(g32(K, G), scale))      # gp holds the clipped value
        else:
            assert gtref.eq32(got["gp"], g32(K, G))
        want = spec(O, K, s, G, partner, flags[it], alpha, LR, "H1", scale=scale, runs=runs)
        for k in STATE:
            assert same(K, got, want, (k,)), f"{K} {mode} round {it}: {k}"
        if runs is not None:                         # the runs change only the step: the tracker is the ungrouped one's
            plain = spec(O, K, s, G, partner, flags[it], alpha, LR, "H1", scale=scale)
            assert same(K, got, plain, ("y", "gp")) and not same(K, got, plain, ("x",))
        assert not got["g"].any() and tails_zero(grp, K, P)
        s = got


def run_graph_replay(pkg, O, K):
    """gt_device_round captured once and replayed over a 6-round schedule with fresh gradients and a learning rate
    changed after round 3 through lr_dev == six gt_step calls on a twin (themselves the specification's); two
    replays past the schedule write nothing"""
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 4)[[6, 3, 0, 9, 10, 7]]
    topo = Topo(partner, alpha, flags)
    n, P = 8, 2 * tile(pkg, K, 8) + 77
    rng = np.random.default_rng(61)
    X0 = rng.standard_normal((n, P)).astype(np.float32)
    Gs = [rand_g(K, rng, (n, P)) for _ in range(7)]
    lrs = [0.01, 0.01, 0.01, 0.01, 0.0025, 0.0025]
    eager = group(pkg, K, topo, P, "H2", True)
    put(eager, K, x=X0)
    s = zero_state(n, P, "H2", X0)
    for it in range(6):
        put(eager, K, g=Gs[it])
        eager.gt_step(it, lrs[it])
        s = spec(O, K, s, Gs[it], partner, flags[it], alpha, lrs[it], "H2")
    want = state(eager, K)
    assert same(K, want, s) and not want["g"].any()

    grp = group(pkg, K, topo, P, "H2", True)
    put(grp, K, x=X0)
    grp.iter_dev.fill_(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            grp.gt_device_round()
    torch.cuda.synchronize()
    assert int(grp.iter_dev.item()) == 0 and gtref.eq32(state(grp, K)["x"], X0)      # capture ran nothing
    for it in range(6):
        put(grp, K, g=Gs[it])
        grp.lr_dev.fill_(lrs[it])
        g.replay()
    got = state(grp, K)
    assert same_state(K, got, want)
    put(grp, K, g=Gs[6])                             # past the schedule: no step, nothing tracked, g untouched
    for _ in range(2):
        g.replay()
    past = state(grp, K)
    assert int(grp.iter_dev.item()) == 8
    assert same(K, past, want) and g_after(K, past, Gs[6], False)


_KNOB_BASE = {}


def _knob_run(pkg, K, name):
    """three rounds (every matching, the sparsest, random) on 3T + 5 columns with momentum, decay, zeroing"""
    partner, alpha = topology(pkg, name)
    n = partner.shape[1]
    flags = flag_kinds(partner, 6)[[6, 3, 9]]
    P = 3 * tile(pkg, K, n) + 5
    rng = np.random.default_rng([P, n])
    grp = group(pkg, K, Topo(partner, alpha, flags), P, "H2", True)
    put(grp, K, x=rng.standard_normal((n, P)).astype(np.float32))
    for it in range(3):
        put(grp, K, g=rand_g(K, rng, (n, P)))
        grp.gt_step(it, LR)
    assert tails_zero(grp, K, P)
    return state(grp, K)


def run_knobs(pkg, K, knobs):
    """the new families' knobs tune speed only: the 8-row and 64-row classes give the default's bits under each
    (set on every new family the kind launches); the default itself is held to the specification by run_rounds"""
    pairs = K.tunings(pkg)
    for name in ("g0", "er64"):
        if (K.name, name) not in _KNOB_BASE:
            assert all(t() == DEFAULT_KNOBS for t, _ in pairs)
            _KNOB_BASE[K.name, name] = _knob_run(pkg, K, name)
    try:
        for tuning, set_tuning in pairs:
            set_tuning(**knobs)
            assert all(tuning()[k] == v for k, v in knobs.items())
        got = {name: _knob_run(pkg, K, name) for name in ("g0", "er64")}
    finally:
        for _, set_tuning in pairs:
            set_tuning(**{k: DEFAULT_KNOBS[k] for k in knobs})
    assert all(t() == DEFAULT_KNOBS for t, _ in pairs)
    for name in ("g0", "er64"):
        assert same_state(K, got[name], _KNOB_BASE[K.name, name]), f"{K} {knobs} {name}"
    assert pkg.engine.sgd_mix_tuning()["grid"] == 0 and pkg.engine.sgd_mix_bf16_tuning()["grid"] == 0


def run_checkpoints(pkg, O, K):
    """a round trip continues bit for bit; a tracker without its previous gradient (or the reverse) is an error;
    a gradient-tracking checkpoint is refused by the other optimizers' groups and by a group of another shape;
    without the keys tracker and previous gradient are zeroed"""
    partner, alpha = topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((4, partner.shape[0]), np.uint8))
    n, P = 8, 1300
    rng = np.random.default_rng(71)
    Gs = [rand_g(K, rng, (n, P)) for _ in range(4)]

    def steps(g, its):
        for it in its:
            put(g, K, g=Gs[it])
            g.gt_step(it, LR)

    grp = group(pkg, K, topo, P, "H2", True)
    put(grp, K, x=rng.standard_normal((n, P)).astype(np.float32))
    steps(grp, range(2))
    grp.iter = 2
    ckpt = grp.state_dict()
    own = {"gt_tracker_rows", "gt_prev_grad_rows", "momentum_rows"}
    keys = {"kind", "iter", "row_base", "workers", "rows"} | own | ({"master_rows"} if K.mixed else set())
    assert set(ckpt) == keys
    for k in own:
        assert ckpt[k].dtype == torch.float32 and tuple(ckpt[k].shape) == (n, P) and ckpt[k].abs().max().item() > 0
    twin = group(pkg, K, topo, P, "H2", True)
    twin.load_state_dict(ckpt)
    assert twin.iter == 2 and same_state(K, state(twin, K), state(grp, K))
    steps(grp, range(2, 4))
    steps(twin, range(2, 4))
    assert same_state(K, state(twin, K), state(grp, K))              # continues bit for bit
    for half in ("gt_tracker_rows", "gt_prev_grad_rows"):
        before = state(twin, K)
        with pytest_raises(ValueError, "only valid together"):
            twin.load_state_dict({k: v for k, v in ckpt.items() if k != half})
        assert same_state(K, state(twin, K), before)                 # the refused load wrote nothing
    twin.load_state_dict({k: v for k, v in ckpt.items() if k not in own})
    for rows in (twin.gt_tracker_rows, twin.gt_prev_grad_rows, twin.momentum_rows):
        assert not rows.view(torch.int32).any().item()
    plain = group(pkg, K, topo, P, "H0", True)                       # no momentum: no momentum rows either
    assert "momentum_rows" not in plain.state_dict() and "gt_tracker_rows" in plain.state_dict()
    kw = {"dtype": K.dtype}
    for opt, attach in (("sgd", {"momentum": 0.9}), ("adamw", {}), ("lion", {}), ("qgm", {})):
        g = pkg.VirtualWorkerGroup(topo, numel=P, **kw)
        getattr(g, "attach_" + opt)(master_weights=K.mixed, **attach)
        with pytest_raises(ValueError, "gradient-tracking state"):
            g.load_state_dict({k: v for k, v in ckpt.items() if k != "momentum_rows"})
        if opt != "sgd":
            with pytest_raises(ValueError, {"adamw": "Adam", "lion": "Lion", "qgm": "quasi-global"}[opt]):
                twin.load_state_dict(g.state_dict())
    with pytest_raises(ValueError, "gradient-tracking state"):       # another shape
        group(pkg, K, topo, P + 1, "H0", True).load_state_dict({
            **{k: v for k, v in ckpt.items() if k != "momentum_rows"}, "rows": twin.arena[:, :P + 1].clone(),
            **({"master_rows": twin.master_arena[:, :P + 1].clone()} if K.mixed else {})})


def run_attach_errors(pkg, K):
    partner, alpha = topology(pkg, "g0")
    topo = Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8))

    def fresh(**kw):
        return pkg.VirtualWorkerGroup(topo, numel=100, dtype=K.dtype, **kw)

    mw = {"master_weights": K.mixed}
    grp = fresh()
    with pytest_raises(pkg.MXError, r"no gradient-tracking state: call attach_gt\(\) first"):
        grp.gt_step(0, LR)
    with pytest_raises(pkg.MXError, "no gradient-tracking state"):
        grp.gt_device_round()
    with pytest_raises(pkg.MXError, "no tracker"):
        grp.consensus_distance(of="tracker")
    grp.attach_gt(**mw)
    assert grp.gt_hyper == {"momentum": 0.0, "weight_decay": 0.0, "nesterov": False, "zero_grads": True}
    assert grp.momentum_rows is None and (grp.master_rows is not None) == K.mixed
    with pytest_raises(RuntimeError, "attach_gt: already attached"):
        grp.attach_gt(**mw)
    for opt in ("sgd", "adamw", "lion", "qgm"):
        with pytest_raises(RuntimeError, rf"attach_{opt}: the group already carries gradient-tracking state \(attach_gt\)"):
            getattr(grp, "attach_" + opt)(**mw)
    with pytest_raises(pkg.MXError, "no SGD state"):
        grp.sgd_step(0, LR)
    for opt, name in (("sgd", "SGD"), ("adamw", "AdamW"), ("lion", "Lion"), ("qgm", "QGM")):
        g = fresh()
        getattr(g, "attach_" + opt)(**mw)
        with pytest_raises(RuntimeError, rf"attach_gt: the group already carries {name} state \(attach_{opt}\)"):
            g.attach_gt(**mw)
    g = fresh()                                      # the existing pairs' texts are as they were
    g.attach_sgd(**mw)
    with pytest_raises(RuntimeError, r"attach_adamw: the group already carries SGD state \(attach_sgd\)"):
        g.attach_adamw(**mw)
    for bad in ({"momentum": 1.0}, {"momentum": -0.1}, {"weight_decay": -1.0}, {"nesterov": True},
                {"clip_grad_norm": 0.0}):
        with pytest_raises(ValueError, "attach_gt"):
            fresh().attach_gt(**{**mw, **bad})
    if K.mixed:
        with pytest_raises(NotImplementedError, "bfloat16 groups need fp32 master weights under gradient tracking"):
            fresh().attach_gt()
    else:
        with pytest_raises(ValueError, "master_weights"):
            fresh().attach_gt(master_weights=True)


def run_trainer(pkg, O, K):
    """harness.VirtualTrainer(fused_gt=True) on the MLP toy: every iteration's launch pair by the specification
    from the rows, gradients, tracker, previous gradient and momentum the backward passes left, with clipping
    and a no-decay group honoured; the torch optimizers never step; a checkpoint resumed in a new trainer
    continues bit for bit"""
    H = pkg.harness
    hyper = {"momentum": 0.9, "weight_decay": 1e-2, "nesterov": True}
    groups = [{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}]

    def make(**kw):
        args = H.HarnessArgs(size=8, epoch=2, bs=16, budget=0.5, graphid=0, lr=1e-3, matcha=True, warmup=False)
        for k, v in kw.pop("args", {}).items():
            setattr(args, k, v)
        fn = H.model_factory(args)
        return H.VirtualTrainer(args, (lambda: fn().to(torch.bfloat16)) if K.mixed else fn, n_batches=3,
                                **{"fused_gt": True, "gt_hyper": hyper, "clip_grad_norm": 0.5,
                                   "param_groups": groups, **kw})

    tr = make()
    grp = tr.group
    assert grp.dtype == K.dtype and grp.gt_tracker_arena.dtype == torch.float32 and (grp.master_rows is not None) == K.mixed
    assert grp.gt_hyper["momentum"] == 0.9 and grp.gt_hyper["nesterov"] is True
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
                    (1e-2, 0.9, True), scale=scale, runs=runs)
        assert same(K, got, want) and not got["g"].any(), f"round {before['it']}"
        seen["rounds"] += 1

    stats = tr.train_epoch(on_round=hook)
    assert len(stats) == 8 and all(np.isfinite(s["loss"]) for s in stats) and "grad_norm" in stats[0]
    assert seen["rounds"] == 3 and grp.iter == 3 and len(tr.grad_norm_log) == 3
    assert all(not o.state for o in tr.optimizers)                   # the torch optimizers never stepped
    ckpt = tr.state_dict()
    assert {"gt_tracker_rows", "gt_prev_grad_rows", "momentum_rows"} <= set(ckpt["group"])
    tr2 = make()
    tr2.load_state_dict(ckpt)
    tr.train_epoch()
    tr2.train_epoch()
    assert same_state(K, state(tr.group, K), state(tr2.group, K)) and tr.group.iter == tr2.group.iter == 6
    for kw in ({"fused_sgd": True}, {"fused_adamw": True}, {"fused_lion": True}, {"fused_qgm": True}):
        with pytest_raises(ValueError, "mutually exclusive"):
            make(**kw)
    with pytest_raises(ValueError, "fused_gt"):
        make(batched=True)
    with pytest_raises(ValueError, "fused_gt"):
        make(args={"compress": True})


def run_fp32_step_is_sgd(pkg, O):
    """the fp32 step launch IS the fused SGD kernel: its entry points are the ("sgd", False) family's, and an fp32
    gt_step leaves x and m with the bits of sgd_step on an attach_sgd group whose gradient arena was loaded with
    the tracker"""
    K = KINDS["f32"]
    E = pkg.engine
    partner, alpha = topology(pkg, "g0")
    flags = flag_kinds(partner, 9)[[6, 9, 0]]
    topo = Topo(partner, alpha, flags)
    n, P = 8, 2 * tile(pkg, K, 8) + 11
    wd, mom, nesterov = HYPERS["H2"]
    grp = group(pkg, K, topo, P, "H2", True)
    sgd_fam = E.FAMILIES["sgd", False]
    assert grp._gt.step.base == "mx_sgd_mix" and grp._gt.step.run is sgd_fam.run and grp._gt.step.grouped is sgd_fam.grouped
    assert grp._gt.step.run_at is sgd_fam.run_at and type(grp._gt.step.call) is E.SgdMixCall
    assert grp._gt.step.call.zero_grads == 0 and torch.equal(grp._gt.step.layout.g_ptrs, grp._gt.track.layout.x_ptrs)
    twin = pkg.VirtualWorkerGroup(topo, numel=P)
    twin.attach_sgd(momentum=mom, weight_decay=wd, nesterov=nesterov, zero_grads=False)
    rng = np.random.default_rng(81)
    X0 = rng.standard_normal((n, P)).astype(np.float32)
    put(grp, K, x=X0)
    twin.rows.copy_(torch.from_numpy(X0))
    for it in range(3):
        put(grp, K, g=rand_g(K, rng, (n, P)))
        grp.gt_step(it, LR)
        twin.grads.copy_(grp.gt_tracker_rows)        # what the step launch read: it does not write y
        twin.sgd_step(it, LR)
        torch.cuda.synchronize()
        assert torch.equal(grp.rows.view(torch.int32), twin.rows.view(torch.int32)), f"round {it}: x"
        assert torch.equal(grp.momentum_rows.view(torch.int32), twin.momentum_rows.view(torch.int32)), f"round {it}: m"
        assert torch.equal(grp.gt_tracker_rows.view(torch.int32), twin.grads.view(torch.int32))   # y is not written


def run_end_to_end(pkg, O):
    """tests/test_gt_ref.py's heterogeneous quadratics through the public API: f_i(x) = 0.5 |x - b_i|^2, b ~ N(0, 1)
    of shape (8, 16), a ring of 8, alpha 1/3, every matching active, lr 0.1, 200 iterations, gradients rows - b
    written into group.grads by torch.  Gradient tracking's max |x_i - mean b| is at most 1e-3 of D-SGD's
    (sgd_communicate on an attach_sgd group), the issue's cap.  consensus_distance(of="tracker") after the third
    iteration, where the mean gradient is still O(1): consensus_stats[1] equals |mean g| in fp64 to fp32 rounding."""
    n, P, iters, lr, alpha = 8, 16, 200, 0.1, 1.0 / 3.0
    b_host = np.random.default_rng(2024).standard_normal((n, P)).astype(np.float32)
    b = torch.from_numpy(b_host).cuda()
    topo = Topo(RING8, alpha, np.ones((iters, 2), np.uint8))
    gt = pkg.VirtualWorkerGroup(topo, numel=P)
    gt.attach_gt()
    sgd = pkg.VirtualWorkerGroup(topo, numel=P)
    sgd.attach_sgd()
    for grp in (gt, sgd):
        grp.rows.zero_()
    s = zero_state(n, P, "H0", np.zeros((n, P), np.float32))
    fl = np.ones(2, np.uint8)
    for it in range(iters):
        g = gt.rows - b
        gt.grads.copy_(g)
        sgd.grads.copy_(sgd.rows - b)
        gt.gt_communicate(lr)
        sgd.sgd_communicate(lr)
        if it < 3:                                   # the specification beside it, for the bound's scale
            s = spec(O, KINDS["f32"], s, g.cpu().numpy(), RING8, fl, alpha, lr, "H0")
        if it == 2:
            gt.consensus_distance(of="tracker")
            torch.cuda.synchronize()
            got = float(gt.consensus_stats[1].item())
            want = float(g.double().mean(dim=0).norm().item())
            assert gtref.eq32(gt.gt_tracker_rows.cpu().numpy(), s["y"])
            # The bound, from n, the row length P and the iterations k = 3 so far, with u = 2^-24 (half an fp32 ulp
            # of 1) and V the largest magnitude among the gradients and the specification's trackers:
            #   the tracker: every iteration rounds each element 5 times (fsub, fadd, and the ring's three fma), each
            #     by at most u V, so a column's mean tracker is off its mean gradient by at most 5 k u V;
            #   the kernel's mean over n rows: at most n roundings of at most u V each;
            #   the norm over P columns turns a per-column error e into at most sqrt(P) e;
            #   the sum of P squares, the square root and the fp32 result: at most (P + 4) u relative.
            u = 2.0 ** -24
            V = max(float(np.abs(s["y"]).max()), float(np.abs(s["yp"]).max()), float(g.abs().max().item()))
            tol = np.sqrt(P) * (5 * 3 + n) * u * V + (P + 4) * u * want
            print(f"mean tracker norm {got:.9g}, |mean g| {want:.9g}, difference {abs(got - want):.3e}, bound {tol:.3e}")
            assert want > 0.05 and abs(got - want) <= tol
    torch.cuda.synchronize()
    opt = b.double().mean(dim=0)
    d_gt = float((gt.rows.double() - opt).abs().max().item())
    d_sgd = float((sgd.rows.double() - opt).abs().max().item())
    print(f"max|x_i - mean b|: gradient tracking {d_gt:.3e}, D-SGD {d_sgd:.3e}, ratio {d_gt / d_sgd:.3e}")
    assert d_sgd > 0.05 and d_gt <= 1e-3 * d_sgd
