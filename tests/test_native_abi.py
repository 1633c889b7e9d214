"""The C ABI: the library loads and exports every symbol include/matcha_gossip.h declares; host-side
entry points and argument validation work without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _declared():
    txt = open(os.path.join(ROOT, "include", "matcha_gossip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", txt)))


def test_exports_every_declared_symbol(pkg):
    names = _declared()
    assert len(names) >= 20
    so = ctypes.CDLL(pkg._lib.LIB_PATH)
    for n in names:
        assert hasattr(so, n), n
    assert set(names) == set(pkg._lib.SIGNATURES), "ctypes table out of sync with the header"


def test_version_and_plan_geometry(pkg):
    L = pkg.lib
    assert L.mx_version().startswith(b"matcha-gossip")
    assert L.mx_plan_words(8, 5) == 4 + 2 * 8 + 8 * 5
    assert L.mx_mix_tile(8) == 1024 and L.mx_mix_tile(16) == 1024
    assert L.mx_mix_tile(32) == 512 and L.mx_mix_tile(64) == 256 and L.mx_mix_tile(65) == 256
    assert L.mx_mix_tile(156) == 256 and L.mx_mix_tile(157) == 0          # mix_kernel_wide up to 156 slots
    assert L.mx_choco_msg_bytes(10, 3) == 4 * 4 + 8 * 3 + 4 * 2          # + tile bounds [1 tile + 1]
    assert L.mx_choco_msg_bytes(8193, 4) == 4 * 4 + 8 * 4 + 4 * 4        # 3 tiles of 4096
    assert L.mx_choco_apply_work_bytes(1 << 20, 8) == 0


def test_mix_layout(pkg):
    L = pkg.lib
    lens = np.array([0, 1, 1024, 1025, 5], np.int64)
    off = np.zeros(6, np.int64)
    assert L.mx_mix_layout(lens.ctypes.data, 5, 8, off.ctypes.data) == 0
    assert off.tolist() == [0, 0, 1, 2, 4, 5]


def test_invalid_arguments_report_errors(pkg):
    L = pkg.lib
    rc = L.mx_gossip_mix(None, None, None, None, 1, 1, 8, None, 0, 8, 5, 0.25, None)
    assert rc == -1 and b"null" in L.mx_last_error()
    key = np.zeros(624, np.uint32)
    p = np.array([1.5])
    out = np.zeros(624, np.uint32)
    pos = ctypes.c_int(0)
    rc = L.mx_flags_binomial(key.ctypes.data, 624, p.ctypes.data, 1, 10, ctypes.c_void_p(16),
                             out.ctypes.data, ctypes.byref(pos), None)
    assert rc == -1 and b"> 1" in L.mx_last_error()
    assert L.mx_topk_abs_diff(None, None, 10, 11, None, None, None, None) == -1
    # the pull transport's Choco entries validate before touching a device
    assert L.mx_pull_fetch(None, 1, 2, None, None, 256, 100, None) == -1 and b"null" in L.mx_last_error()
    fake = ctypes.c_void_p(256)
    assert L.mx_pull_fetch(fake, 1, 2, fake, fake, 96, 100, None) == -1 and b"dst_ld" in L.mx_last_error()
    assert L.mx_choco_apply_slots(fake, fake, fake, 8, 8, 1, None, 2, fake, 0, 1, 1, 0.5, 0.1, None) == -1
    assert b"slot table" in L.mx_last_error()


def test_dropin_shims_resolve(pkg):
    import importlib.util
    import sys
    d = os.path.join(ROOT, pkg.__name__, "dropin")
    sys.path.insert(0, d)
    try:
        for mod in ("graph_manager", "communicator", "comm_helpers", "compressors"):
            spec = importlib.util.spec_from_file_location("dropin_" + mod, os.path.join(d, mod + ".py"))
            m = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(m)
        assert m.get_top_k is pkg.get_top_k
    finally:
        sys.path.remove(d)


def test_exchange_plan_moves_each_row_once_per_link(pkg):
    """Graph 0 split over 2 GPUs ({0-3}, {4-7}), every matching active: 6 cross edges, but workers
    0 (partners 4, 7), 1 (5, 7) and 3 (6, 7) each cross the link once, and 7 (partners 0, 1, 3)
    once the other way -- 3 rows 0 -> 1 and 4 rows 1 -> 0 instead of 6 + 6 (mx_exchange_plan)."""
    import ctypes
    import numpy as np
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, 8, 4, True)
    partner = np.ascontiguousarray(np.asarray(gp.neighbors_info, np.int32))
    M = partner.shape[0]
    owner = pkg.engine.owner_table(8, 2)
    flags = np.ones(M, np.uint8)
    for rank, (base, nl) in enumerate(pkg.partition(8, 2)):
        cnt = ctypes.c_int(0)
        assert pkg.lib.mx_exchange_plan(flags.ctypes.data, M, partner.ctypes.data, 8, owner.ctypes.data, rank,
                                        base, nl, None, 0, ctypes.byref(cnt)) == 0
        ops = np.zeros((cnt.value, 4), np.int32)
        assert pkg.lib.mx_exchange_plan(flags.ctypes.data, M, partner.ctypes.data, 8, owner.ctypes.data, rank,
                                        base, nl, ops.ctypes.data, cnt.value, ctypes.byref(cnt)) == 0
        sends = sorted(int(o[3]) for o in ops if o[0] == 0)
        recvs = [int(o[3]) for o in ops if o[0] == 1]
        assert len(set(sends)) == len(sends) and len(set(recvs)) == len(recvs)
        assert [int(o[2]) for o in ops if o[0] == 1] == list(range(len(recvs)))    # slab slots
        assert (len(sends), len(recvs)) == ((3, 4) if rank == 0 else (4, 3))
        assert sends == ([0, 1, 3] if rank == 0 else [4, 5, 6, 7])
        assert pkg.engine.max_incoming_remote(partner, base, nl) == len(recvs)


def test_mix_kernel_dispatch_names(pkg):
    """mx_mix_kernel_name mirrors mx_gossip_mix's dispatch under the knobs (host-only)."""
    E = pkg.engine
    saved = E.mix_tuning()
    try:
        assert saved["rows"] == 2
        assert [E.mix_kernel_name(s) for s in (1, 8, 9, 16, 33, 64)] == ["mix_kernel_rows"] * 6
        assert E.mix_kernel_name(65) == E.mix_kernel_name(156) == "mix_kernel_wide"
        assert E.mix_kernel_name(157) == ""
        E.set_mix_tuning(rows=1)
        assert [E.mix_kernel_name(s) for s in (8, 16, 64)] == ["mix_kernel_reg", "mix_kernel_rows", "mix_kernel_rows"]
        E.set_mix_tuning(rows=0, regidx=0)
        assert [E.mix_kernel_name(s) for s in (8, 16)] == ["mix_kernel", "mix_kernel"]
        E.set_mix_tuning(rows=2, regidx=1, unroll=4)
        assert [E.mix_kernel_name(s) for s in (8, 16)] == ["mix_kernel_reg", "mix_kernel_rows"]
        assert pkg.lib.mx_mix_set(b"rows", 3) != 0
    finally:
        E.set_mix_tuning(**saved)


# mx_mix_set's knobs: key -> (default, accepted values as (set, read back), first values outside the range)
_BOOL = ((0, 0), (1, 1), (7, 1), (-1, 1))
_TPB = ((256, 256), (512, 512), (1024, 1024))
MIX_KNOBS = {
    "blocks_per_cu": (2, ((1, 1), (64, 64)), (0, 65)),
    "unroll": (1, ((1, 1), (2, 2), (4, 4)), (0, 3, 5)),
    "nontemporal": (2, ((0, 0), (1, 1), (2, 2), (5, 1), (-1, 1)), ()),
    "prefetch": (0, _BOOL, ()),
    "regidx": (1, _BOOL, ()),
    "chunked": (0, _BOOL, ()),
    "grid": (0, ((0, 0), (65536, 65536)), (-1, 65537)),
    "readlane_min": (32, ((8, 8), (128, 128)), (7, 129)),
    "rows": (2, ((0, 0), (1, 1), (2, 2)), (-1, 3)),
    "split": (0, ((0, 0), (1, 1), (2, 2), (4, 4)), (-1, 3, 5)),
    "flat_small": (256, ((0, 0), (4096, 4096)), (-1, 4097)),
    "ns48": (0, _BOOL, ()),
    "rows_pf2": (2, ((0, 0), (1, 1), (2, 2)), (-1, 3)),
    "wide_lds_kb": (158, ((8, 8), (158, 158)), (7, 159)),
    "wide_plan_lds": (1, ((0, 0), (1, 1)), (-1, 2)),
    "wide_per_cu": (0, ((0, 0), (8, 8)), (-1, 9)),
    "wide_tpb": (1024, _TPB, (128, 255, 2048)),
    "rows_tpb": (256, _TPB, (128, 255, 2048)),
    "mid_bpc": (4, ((0, 0), (16, 16)), (-1, 17)),
    "mid_tiles": (8, ((0, 0), (1024, 1024)), (-1, 1025)),
    "wide_pf2": (1, ((0, 0), (1, 1)), (-1, 2)),
    "spec": (1, _BOOL, ()),
    "spec_wgpc": (5, ((0, 0), (32, 32)), (-1, 33)),
    "spec_glds": (1, _BOOL, ()),
    "mean_wgpc": (3, ((0, 0), (32, 32)), (-1, 33)),
    "store_policy": (0, ((0, 0), (4, 4)), (-1, 5)),
}


def test_mix_knobs_defaults_ranges_and_refusals(pkg):
    """mx_mix_set / mx_mix_get, every key of TUNE_KEYS: the default, each accepted boundary value read back
    as stored (booleans and nontemporal normalised), each first value outside the range refused with the key
    in mx_last_error and the knob left as it was; spec_launches reads and cannot be set (host-only)."""
    L, E = pkg.lib, pkg.engine
    INV = pkg._lib.MX_ERR_INVALID
    assert set(MIX_KNOBS) == set(E.TUNE_KEYS) and len(E.TUNE_KEYS) == 26

    def get(k):
        return L.mx_mix_get(k.encode())

    def put(k, v):
        return L.mx_mix_set(k.encode(), v)

    saved = {k: get(k) for k in MIX_KNOBS}
    try:
        for k, (default, _, _) in MIX_KNOBS.items():
            assert put(k, default) == 0, k
        assert {k: get(k) for k in MIX_KNOBS} == {k: d for k, (d, _, _) in MIX_KNOBS.items()}
        for k, (default, accepted, refused) in MIX_KNOBS.items():
            for v, back in accepted:
                assert put(k, v) == 0 and get(k) == back, (k, v)
            before = get(k)
            for v in refused:
                assert put(k, v) == INV, (k, v)
                err = L.mx_last_error()
                assert b"mx_mix_set:" in err and k.encode() in err and str(v).encode() in err, (k, v, err)
                assert get(k) == before, (k, v)
            assert put(k, default) == 0 and get(k) == default, k
        n = get("spec_launches")
        assert n >= 0
        assert put("spec_launches", 0) == INV and b"spec_launches" in L.mx_last_error()
        assert get("spec_launches") == n
        assert put("no_such_knob", 1) == INV and L.mx_last_error() == b"mx_mix_set: unknown key 'no_such_knob'"
        assert get("no_such_knob") == INV and L.mx_last_error() == b"mx_mix_get: unknown key 'no_such_knob'"
        assert L.mx_mix_set(None, 1) == INV and b"null key" in L.mx_last_error()
        assert L.mx_mix_get(None) == INV
    finally:
        for k, v in saved.items():
            put(k, v)


# mx_topk_set's table knobs: key -> (default, lowest accepted, highest accepted).  spin_ticks and compact_trace
# write a device symbol (they need a GPU) and are not in the table.
_INT_MAX = 2 ** 31 - 1
TOPK_KNOBS = {
    "sample_stride": (0, 0, _INT_MAX),
    "compact_blocks": (0, 0, 1 << 20),
    "cand_chunks": (0, 0, 4096),
    "apply_nt": (-1, -1, 1),
    "apply_persist": (-1, -1, 1),
    "apply_pf": (1, 0, 1),
    "compact_store": (1, 0, 1),
    "compact_wave": (0, 0, 1024),
    "compact_pf2": (0, 0, 1),
    "select": (0, 0, 1),
    "fine_floor": (1, 0, 1),
    "floor_hint": (-1, -1, 64),
    "select_blocks": (0, 0, 32),
    "sample_pieces": (1, 1, 1024),
}


def test_topk_knobs_defaults_ranges_and_refusals(pkg):
    """mx_topk_set / mx_topk_get, every host-side knob: the default, both bounds read back as stored, one value
    past each bound refused (-1, the knob left as it was, key and value in mx_last_error); select_trace
    normalised to 0 / 1; hist_grid and hist_capacity read and are unknown to set; unknown and null keys; a
    value outside the int range (sample_stride = 2^32 would narrow to 0) refused."""
    L = pkg.lib
    INV = pkg._lib.MX_ERR_INVALID

    def get(k):
        return L.mx_topk_get(k.encode())

    def put(k, v):
        return L.mx_topk_set(k.encode(), v)

    keys = list(TOPK_KNOBS) + ["select_trace"]
    saved = {k: get(k) for k in keys}
    try:
        assert saved == {**{k: d for k, (d, _, _) in TOPK_KNOBS.items()}, "select_trace": 0}
        for k, (default, lo, hi) in TOPK_KNOBS.items():
            for v in (lo, hi):
                assert put(k, v) == 0 and get(k) == v, (k, v)
            for v in (lo - 1, hi + 1):
                assert put(k, v) == INV, (k, v)
                assert get(k) == hi, (k, v)
                if -_INT_MAX - 1 <= v <= _INT_MAX:
                    err = L.mx_last_error()
                    assert err == f"mx_topk_set: {k} {v}".encode() or \
                        (k == "floor_hint" and err.startswith(f"mx_topk_set: {k} {v} ".encode())), (k, v, err)
            assert put(k, default) == 0 and get(k) == default, k
        for v, back in ((1, 1), (0, 0), (7, 1), (-1, 1), (0, 0)):
            assert put("select_trace", v) == 0 and get("select_trace") == back, v
        for k in ("hist_grid", "hist_capacity"):
            n = get(k)
            assert n >= 0
            assert put(k, 0) == INV and L.mx_last_error() == f"mx_topk_set: unknown key '{k}'".encode()
            assert get(k) == n
        assert put("no_such_knob", 1) == INV and L.mx_last_error() == b"mx_topk_set: unknown key 'no_such_knob'"
        assert get("no_such_knob") == INV and L.mx_last_error() == b"mx_topk_get: unknown key 'no_such_knob'"
        assert L.mx_topk_set(None, 1) == INV and b"null key" in L.mx_last_error()
        assert L.mx_topk_get(None) == INV
        for k in TOPK_KNOBS:                       # no silent narrowing: 2^32 is not 0, 2^32 + 1 is not 1
            for v in (2 ** 32, 2 ** 32 + 1, -2 ** 32, 2 ** 31, -2 ** 31 - 1):
                assert put(k, v) == INV and get(k) == TOPK_KNOBS[k][0], (k, v)
    finally:
        for k, v in saved.items():
            put(k, v)


def test_mean_rows_to_refuses_partial_overlap_and_names_kernels(pkg):
    """a destination overlapping the rows at a column offset is refused before any
    launch (host-side validation, fake device addresses); whole-row aliasing passes validation.
    mx_mean_kernel_name follows the launch dispatch (the bench's centralized figure)."""
    L = pkg.lib
    base, ld, count = 1 << 40, 1024, 1000
    rc = L.mx_mean_rows_to(base, 8, ld, count, 0, base + 4 * 16, 8, ld, None)   # 16 columns in
    assert rc == -1 and b"column offset" in L.mx_last_error()
    rc = L.mx_mean_rows_to(base, 8, ld, count, 0, base + 4 * (3 * ld + 5), 1, count, None)
    assert rc == -1 and b"column offset" in L.mx_last_error()
    A = 1 << 40                                       # 16-byte aligned fake addresses (nothing launched)

    def name(nrows, count, order, ld=None, base=A, dst_ld=None):
        ld = ld if ld is not None else (count + 63) // 64 * 64
        return L.mx_mean_kernel_name(base, nrows, ld, count, order, base, nrows, dst_ld if dst_ld else ld)
    assert name(8, 25_600_000, 0) == b"mean_tile_kernel<1>"
    assert name(8, 25_600_000, 1) == b"mean_tile_kernel<0>"
    assert name(8, 400, 0) == b"mean4_kernel<1, 4>"
    assert name(16, 4096, 1) == b"mean4_kernel<0, 4>"
    assert name(16, 4096, 0) == b"mean_to_kernel<float, 1, 64>"
    assert name(65, 4096, 0) == b"mean_to_kernel<float, 2, 1>"
    # the dispatch's alignment conditions -- unaligned rows / ld / dst_ld take the scalar path
    assert name(8, 25_600_000, 0, base=A + 4) == b"mean_to_kernel<float, 1, 8>"
    assert name(8, 25_600_000, 1, ld=25_600_002) == b"mean_to_kernel<float, 0, 1>"
    assert name(8, 25_600_000, 0, dst_ld=25_600_006) == b"mean_to_kernel<float, 1, 8>"
    assert name(8, 100, 0, ld=50) == b"invalid"


def test_ipc_knobs_and_publish_rows_validation(pkg):
    """mx_ipc_set / mx_ipc_get (the export probe's knobs, include/matcha_gossip.h) and the host-side
    argument checks of mx_snapshot_publish_rows (no launch: fake device addresses)."""
    import ctypes
    L = pkg.lib
    g0 = L.mx_ipc_get(b"granule")
    assert g0 == 2 << 20 and L.mx_ipc_get(b"tries") == -1 and L.mx_ipc_get(b"nope") == -1
    try:
        assert L.mx_ipc_set(b"granule", 1) == 0 and L.mx_ipc_get(b"granule") == 1
        assert L.mx_ipc_set(b"granule", 0) != 0 and L.mx_ipc_set(b"tries", 2) != 0
        assert L.mx_ipc_set(b"nope", 1) != 0 and b"unknown" in L.mx_last_error()
    finally:
        L.mx_ipc_set(b"granule", g0)
    ex, ref = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.mx_ipc_stats(ctypes.byref(ex), ctypes.byref(ref)) == 0 and ex.value >= 0 and ref.value >= 0
    fake = 1 << 40
    assert L.mx_snapshot_publish_rows(fake, 8, fake, 8, 6, 2, fake, 5, fake, 8, 0, None) != 0      # n % 4
    assert L.mx_snapshot_publish_rows(fake, 8, fake, 8, 8, 2, fake, 5, fake, 8, 7, None) != 0      # block
    assert L.mx_snapshot_publish_rows(None, 8, fake, 8, 8, 2, fake, 5, fake, 8, 0, None) != 0      # null
    assert L.mx_snapshot_publish_rows(fake, 8, fake, 8, 0, 2, fake, 5, fake, 8, 0, None) == 0      # nothing to do


FUSED = ("mx_sgd_mix", "mx_sgd_mix_bf16", "mx_adamw_mix", "mx_adamw_mix_bf16")
FUSED_DEFAULTS = {b"nontemporal": 2, b"wgpc": 0, b"blocks_per_cu": 2, b"flat_small": 256, b"grid": 0}


def test_fused_round_knobs_are_per_family(pkg):
    """mx_*_set / _get of the four fused optimizer rounds: the defaults, every key set on one family read
    back from that family alone, the refusals (naming the entry point called), values restored."""
    L = pkg.lib
    INV = pkg._lib.MX_ERR_INVALID
    get = {f: getattr(L, f + "_get") for f in FUSED}
    put = {f: getattr(L, f + "_set") for f in FUSED}
    for f in FUSED:
        assert {k: get[f](k) for k in FUSED_DEFAULTS} == FUSED_DEFAULTS, f
    changed = {b"nontemporal": 0, b"wgpc": 5, b"blocks_per_cu": 3, b"flat_small": 17, b"grid": 7}
    try:
        for f in FUSED:
            for k, v in changed.items():
                assert put[f](k, v) == 0 and get[f](k) == v, (f, k)
                for o in FUSED:
                    if o != f:
                        assert get[o](k) == FUSED_DEFAULTS[k], (f, k, o)
                assert put[f](k, FUSED_DEFAULTS[k]) == 0 and get[f](k) == FUSED_DEFAULTS[k], (f, k)
            for k, v in ((b"wgpc", 33), (b"blocks_per_cu", 0), (b"flat_small", 4097), (b"grid", 65537), (b"no_such_knob", 1)):
                assert put[f](k, v) == INV, (f, k)
                assert (f + "_set:").encode() in L.mx_last_error(), (f, k, L.mx_last_error())
            assert {k: get[f](k) for k in FUSED_DEFAULTS} == FUSED_DEFAULTS, f     # a refusal changes nothing
            assert get[f](b"no_such_knob") == INV
    finally:
        for f in FUSED:
            for k, v in FUSED_DEFAULTS.items():
                put[f](k, v)


def test_fused_round_layouts_agree(pkg):
    """mx_*_tile / mx_*_layout of the four fused optimizer rounds: 1024 / 1024 / 512 / 256 columns by row
    class, the same offsets from all four -- ceil(len / tile) accumulated -- and the refusals."""
    L = pkg.lib
    INV = pkg._lib.MX_ERR_INVALID
    lens = np.array([0, 1, 1023, 1024, 1025, 4097], np.int64)
    for n_slots in (1, 8, 9, 16, 17, 32, 33, 64):
        tile = 1024 if n_slots <= 16 else 512 if n_slots <= 32 else 256
        want = [0] + np.cumsum((lens + tile - 1) // tile).tolist()
        for f in FUSED:
            assert getattr(L, f + "_tile")(n_slots) == tile, (f, n_slots)
            off = np.full(len(lens) + 1, -1, np.int64)
            assert getattr(L, f + "_layout")(lens.ctypes.data, len(lens), n_slots, off.ctypes.data) == 0
            assert off.tolist() == want, (f, n_slots)
    off = np.zeros(len(lens) + 1, np.int64)
    neg = np.array([5, -1], np.int64)
    for f in FUSED:
        lay = getattr(L, f + "_layout")
        for n_slots in (0, 65):
            assert getattr(L, f + "_tile")(n_slots) == 0
            assert lay(lens.ctypes.data, len(lens), n_slots, off.ctypes.data) == INV
            assert (f + "_layout:").encode() in L.mx_last_error()
        assert lay(neg.ctypes.data, 2, 8, off.ctypes.data) == INV
        assert (f + "_layout:").encode() in L.mx_last_error()


# C record -> (its ctypes mirror in engine, sizeof by the header's field list on an LP64 target)
CALL_RECORDS = {"mx_mix_call": ("MixCall", 88), "mx_sgd_mix_call": ("SgdMixCall", 96),
                "mx_sgd_mix_bf16_call": ("SgdBf16Call", 104), "mx_adamw_mix_call": ("AdamwMixCall", 128),
                "mx_adamw_mix_bf16_call": ("AdamwBf16Call", 136), "mx_grad_norm_call": ("GradNormCall", 64),
                "mx_param_runs": ("ParamRunsRec", 40)}


def _header_fields(struct):
    """the member names of `typedef struct <struct> { ... }` in include/matcha_gossip.h, in order"""
    txt = open(os.path.join(ROOT, "include", "matcha_gossip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), txt, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        names += [re.search(r"(\w+)\s*$", part).group(1) for part in decl.split(",") if part.strip()]
    return names


@pytest.mark.parametrize("struct", sorted(CALL_RECORDS))
def test_call_struct_layout_matches_header(pkg, tmp_path, struct):
    """Every ctypes mirror of a call record has the C struct's members -- all of them, by name and in
    order, so a field dropped from the mirror's tail shows -- and its size and field offsets, which a C
    program built against include/matcha_gossip.h prints."""
    import subprocess
    import importlib
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, CALL_RECORDS[struct][0])
    fields = [f for f, _ in cls._fields_]
    assert fields == _header_fields(struct)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "matcha_gossip.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({struct}));\n'
                   + "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want and got[0] == CALL_RECORDS[struct][1]


class _Addr:
    """stands in for a device tensor: only its address is read"""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


class _Engine:
    """stands in for a GossipEngine: what a call record takes from it"""
    _plan_ptr, n_slots, n_local, M, alpha32 = (1 << 40) + 99, 9, 8, 5, float(np.float32(2 / 7))


@pytest.mark.parametrize("family,momentum", [("SgdLayout", True), ("SgdLayout", False), ("SgdBf16Layout", True),
                                             ("SgdBf16Layout", False), ("AdamwLayout", True),
                                             ("AdamwBf16Layout", True)])
def test_call_records_are_packed_as_specified(pkg, family, momentum):
    """layout.call(engine, ...) of the four fused layouts over distinct fake addresses: every field of the
    record -- each pointer table in its own field (an absent momentum table NULL), the geometry (n_slots /
    n_local / M the engine's, not the layout's), the hyperparameters as fp32 roundings with omb1 / omb2
    rounded from the fp64 1 - beta, the flags 0 or 1 for any truthy input, pad_ 0."""
    import importlib
    E = importlib.import_module(pkg.__name__ + ".engine")
    cls = getattr(E, family)
    fam = cls.family
    adam = "Adamw" in family
    assert fam is E.FAMILIES["adamw" if adam else "sgd", "Bf16" in family] and fam.adam == adam
    assert fam.tables == {"SgdLayout": ("x", "g", "m"), "SgdBf16Layout": ("w", "g", "m", "p"),
                          "AdamwLayout": ("x", "g", "m", "v"), "AdamwBf16Layout": ("w", "g", "m", "v", "p")}[family]
    assert fam.optional == (None if adam else "m")                         # only SGD's momentum may be absent

    def f32(v):
        return float(np.float32(v))

    lay = object.__new__(cls)                     # the constructor uploads tables: only call() is under test
    want = {}
    k = 1 << 40
    for t in fam.tables + ("seg_len", "tile_off", "bias"):
        k += 1
        absent = t == "m" and not momentum
        name = t + "_ptrs" if t in fam.tables else t
        setattr(lay, name, None if absent else _Addr(k))
        if t != "bias" or adam:
            want[name + "_dev"] = None if absent else k
    lay.total_tiles, lay.nseg, lay.n_local, lay.n_bias = 77, 3, 64, 4321 if adam else 0
    want.update(plan_dev=_Engine._plan_ptr, total_tiles=77, nseg=3, n_slots=9, n_local=8, M=5,
                alpha=_Engine.alpha32, wd=f32(0.1), zero_grads=1)
    if adam:
        call = lay.call(_Engine, (0.9, 0.999), 1e-8, 0.1, "x", 2)
        want.update(n_bias=4321, omb1=f32(1.0 - 0.9), beta2=f32(0.999), omb2=f32(1.0 - 0.999), eps=f32(1e-8),
                    decoupled=1)
        assert f32(1.0 - 0.9) != 1 - f32(0.9) and f32(1.0 - 0.9) != f32(1 - f32(0.9))     # the roundings differ
    else:
        call = lay.call(_Engine, 0.1, 0.9, "x", 2)
        want.update(mom=f32(0.9), nesterov=1, pad_=0)
    assert type(call) is fam.rec
    got = {f: getattr(call, f) for f, _ in fam.rec._fields_}
    assert got == want
    ptrs = [v for f, v in got.items() if f.endswith("_dev") and v is not None]
    assert len(set(ptrs)) == len(ptrs)
    zero = lay.call(_Engine, (0.9, 0.999), 1e-8, 0.1, 0, "") if adam else lay.call(_Engine, 0.1, 0.9, 0, None)
    assert zero.zero_grads == 0 and (zero.decoupled if adam else zero.nesterov) == 0
