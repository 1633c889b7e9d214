"""Gossip engine: the device-resident schedule, round plans, worker layout and transport.

One process drives one GPU and a contiguous block of the topology's workers
(rows [row_base, row_base + n_local)).  With one process (the "virtual worker" mode) the
block is every worker; with N processes (torch.distributed, one per GPU) the workers are split
into N contiguous blocks and edges that cross blocks go over RCCL (xGMI).

Per round (reference: decenCommunicator.communicate, communicator.py:133-158):
    1. [N > 1] mx_exchange_round: one ncclGroupStart/End with a send of every local row whose
       active partner is remote and a receive of every remote partner row into the slab;
    2. mx_gossip_mix: the in-place FMA-chain mixing kernel over local rows + slab rows, driven
       by the precomputed plan record of this iteration.
Everything is enqueued on one HIP stream; nothing is copied to or from the host per round.
"""
import collections
import contextlib
import ctypes
import math
import sys
import time
import weakref

import numpy as np
import torch

from ._lib import MX_ERR_RCCL, MXError, check, lib, require_device, stream_ptr

ROW_ALIGN = 64  # arena rows padded to 256 B

TUNE_KEYS = ("blocks_per_cu", "unroll", "nontemporal", "prefetch", "regidx", "chunked", "grid", "readlane_min",
             "rows", "split", "flat_small", "ns48", "rows_pf2", "wide_lds_kb", "wide_plan_lds", "wide_per_cu", "wide_tpb", "rows_tpb", "mid_bpc", "mid_tiles", "wide_pf2", "spec", "spec_wgpc", "spec_glds", "mean_wgpc", "store_policy")


def mix_tuning():
    """Current mixing-kernel knobs (include/matcha_gossip.h, mx_mix_set)."""
    return {k: int(lib.mx_mix_get(k.encode())) for k in TUNE_KEYS}


def mix_kernel_name(n_slots):
    """The kernel mx_gossip_mix launches for n_slots under the current knobs."""
    return lib.mx_mix_kernel_name(int(n_slots)).decode()


# bumped by set_mix_tuning alone: the mixing kernel's tile depends on its knobs (unroll), so a Layout
# re-checks its tile after a change.  The fused rounds' tile depends on the row count only
_TUNE_GEN = [0]
_mix_packed = lib.mx_gossip_mix_packed
_mix_bf16_packed = lib.mx_gossip_mix_bf16_packed

# row element types the mixing kernels take: float32 everywhere; bfloat16 on one GPU with every
# partner local (csrc/mix_bf16.hip: an fp32 FMA chain over exactly widened inputs, rounded to
# nearest even once at the store)
ROW_DTYPES = (torch.float32, torch.bfloat16)


def row_dtype(dtype):
    if dtype not in ROW_DTYPES:
        raise TypeError(f"worker rows are float32 or bfloat16, not {dtype}")
    return dtype


def set_mix_tuning(**knobs):
    _TUNE_GEN[0] += 1
    for k, v in knobs.items():
        check(lib.mx_mix_set(k.encode(), int(v)), "mx_mix_set")


GRAD_NORM_TUNE_KEYS = ("blocks_per_cu", "grid")


def grad_norm_tuning():
    """Current knobs of the gradient-norm kernel (mx_grad_norm_set)."""
    return {k: int(lib.mx_grad_norm_get(k.encode())) for k in GRAD_NORM_TUNE_KEYS}


def set_grad_norm_tuning(**knobs):
    for k, v in knobs.items():
        check(lib.mx_grad_norm_set(k.encode(), int(v)), "mx_grad_norm_set")


CONSENSUS_TUNE_KEYS = ("blocks_per_cu", "grid")


def consensus_tuning():
    """Current knobs of the consensus-distance kernel (mx_consensus_set)."""
    return {k: int(lib.mx_consensus_get(k.encode())) for k in CONSENSUS_TUNE_KEYS}


def set_consensus_tuning(**knobs):
    for k, v in knobs.items():
        check(lib.mx_consensus_set(k.encode(), int(v)), "mx_consensus_set")


SLOWMO_TUNE_KEYS = ("store_policy", "wgpc")


def slowmo_tuning():
    """Current knobs of the SlowMo outer-step kernel (mx_slowmo_set)."""
    return {k: int(lib.mx_slowmo_get(k.encode())) for k in SLOWMO_TUNE_KEYS}


def set_slowmo_tuning(**knobs):
    for k, v in knobs.items():
        check(lib.mx_slowmo_set(k.encode(), int(v)), "mx_slowmo_set")


def clip_value(clip_grad_norm, who):
    """The clip_grad_norm keyword of attach_sgd / attach_adamw: None (off) or a positive finite float."""
    if clip_grad_norm is None:
        return None
    try:
        v = float(clip_grad_norm)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: clip_grad_norm must be None or a positive finite number") from None
    with np.errstate(over="ignore", under="ignore"):
        v32 = float(np.float32(v)) if math.isfinite(v) else v      # the kernel takes the fp32 rounding
    if not (math.isfinite(v32) and v32 > 0.0):
        raise ValueError(f"{who}: clip_grad_norm must be None or a positive finite number, not {clip_grad_norm!r}")
    return v


class ParamShape:
    """What a param_groups predicate sees for a parameter known by its shape only (param_runs on the host)."""

    def __init__(self, shape):
        self.shape = tuple(int(d) for d in shape)
        self.ndim = len(self.shape)

    def numel(self):
        return int(math.prod(self.shape))

    def dim(self):
        return self.ndim


PARAM_GROUP_KEYS = ("params", "columns", "weight_decay", "lr_scale")


def _group_value(v, what):
    """A weight decay or lr scale of a parameter group: the fp32 rounding of a finite Python float >= 0."""
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"param_groups: {what} must be a finite number >= 0") from None
    with np.errstate(over="ignore", under="ignore"):
        v32 = float(np.float32(v)) if math.isfinite(v) else v
    if not (math.isfinite(v32) and v32 >= 0.0):
        raise ValueError(f"param_groups: {what} must be a finite number >= 0, not {v!r}")
    return v32


def param_runs(numel, named_shapes, param_groups, default_wd):
    """Resolve torch-style parameter groups to the run list of the fused launches (mx_param_runs):
    [(start, end, weight_decay, lr_scale), ...], half-open column ranges that cover [0, numel) in
    order, adjacent ranges with equal pairs merged.  A pure host function.

    numel         -- columns of a worker row
    named_shapes  -- [(name, parameter or shape), ...] in the order the row is laid out
                     (models[0].named_parameters()), or None for a group built from numel alone
    param_groups  -- a list of dicts with exactly one selector each:
                       "params":  a list of names, or a predicate fn(name, param) -> bool (param is what
                                  named_shapes carries; a bare shape is wrapped as a ParamShape)
                       "columns": a list of half-open (start, end) column ranges
                     and optionally "weight_decay" (default: default_wd) and "lr_scale" (default 1.0);
                     columns no group selects take the defaults
    ValueError: overlapping groups, an unknown name, an empty or out-of-range column range, a negative
    or non-finite value, an unknown key, no or two selectors, "params" without named_shapes, and
    named_shapes that do not add up to numel."""
    numel = int(numel)
    if numel < 1:
        raise ValueError(f"param_runs: numel={numel} < 1")
    default = (_group_value(default_wd, "the default weight_decay"), 1.0)
    spans = None
    if named_shapes is not None:
        spans, off = {}, 0
        order = []
        for name, par in named_shapes:
            if not hasattr(par, "shape"):
                par = ParamShape(par)
            k = int(math.prod(tuple(par.shape)))
            if name in spans:
                raise ValueError(f"param_runs: parameter name {name!r} appears twice")
            spans[name] = (off, off + k)
            order.append((name, par))
            off += k
        if off != numel:
            raise ValueError(f"param_runs: the named parameters hold {off} elements, the row {numel}")
    pieces = []                              # (start, end, wd, scale) of every selected range
    for gi, g in enumerate(param_groups):
        if not isinstance(g, dict):
            raise ValueError(f"param_groups[{gi}]: a group is a dict")
        for key in g:
            if key not in PARAM_GROUP_KEYS:
                raise ValueError(f"param_groups[{gi}]: unknown key {key!r} (known: {', '.join(PARAM_GROUP_KEYS)})")
        if ("params" in g) == ("columns" in g):
            raise ValueError(f"param_groups[{gi}]: give exactly one of 'params' and 'columns'")
        pair = (_group_value(g.get("weight_decay", default[0]), f"weight_decay of group {gi}"),
                _group_value(g.get("lr_scale", 1.0), f"lr_scale of group {gi}"))
        if "params" in g:
            if spans is None:
                raise ValueError(f"param_groups[{gi}]: 'params' needs a group built from models; a numel-only "
                                 "group selects by 'columns'")
            sel = g["params"]
            if callable(sel):
                names = [name for name, par in order if sel(name, par)]
            else:
                names = list(sel)
                for name in names:
                    if name not in spans:
                        raise ValueError(f"param_groups[{gi}]: unknown parameter name {name!r}")
            ranges = [spans[name] for name in names]
            ranges = [r for r in ranges if r[1] > r[0]]          # a parameter without elements selects nothing
        else:
            ranges = []
            for rg in g["columns"]:
                try:
                    a, b = (int(v) for v in rg)
                except (TypeError, ValueError):
                    raise ValueError(f"param_groups[{gi}]: a column range is a (start, end) pair") from None
                if not (0 <= a < b <= numel):
                    raise ValueError(f"param_groups[{gi}]: column range [{a}, {b}) is empty or outside [0, {numel})")
                ranges.append((a, b))
        pieces += [(a, b) + pair for a, b in ranges]
    pieces.sort(key=lambda t: (t[0], t[1]))
    runs, at = [], 0

    def push(a, b, pair):
        if runs and runs[-1][2:] == pair:
            runs[-1] = (runs[-1][0], b) + pair
        else:
            runs.append((a, b) + pair)

    for a, b, wd, sc in pieces:
        if a < at:
            raise ValueError(f"param_groups: columns [{a}, {min(b, at)}) are selected twice (overlapping groups)")
        if a > at:
            push(at, a, default)
        push(a, b, (wd, sc))
        at = b
    if at < numel:
        push(at, numel, default)
    return runs


class ParamRunsRec(ctypes.Structure):
    """mx_param_runs (include/matcha_gossip.h): the run tables of a grouped fused launch."""
    _fields_ = [("run_off_dev", ctypes.c_void_p), ("run_end_dev", ctypes.c_void_p), ("wd_dev", ctypes.c_void_p),
                ("lr_scale_dev", ctypes.c_void_p), ("nruns", ctypes.c_int32)]


class ParamRuns:
    """The device tables of a run list (param_runs) over ONE segment of `numel` columns, checked by
    mx_param_runs_check on the host before they are uploaded, and the record the _grouped entry points
    take.  Built once by attach_sgd / attach_adamw(param_groups=...); keeps the tables alive."""

    def __init__(self, numel, runs):
        self.runs = list(runs)
        seg_len = np.asarray([int(numel)], dtype=np.int64)
        off = np.asarray([0, len(self.runs)], dtype=np.int32)
        end = np.asarray([r[1] for r in self.runs], dtype=np.int64)
        wd = np.asarray([r[2] for r in self.runs], dtype=np.float32)
        scale = np.asarray([r[3] for r in self.runs], dtype=np.float32)
        check(lib.mx_param_runs_check(seg_len.ctypes.data, 1, off.ctypes.data, end.ctypes.data, wd.ctypes.data,
                                      scale.ctypes.data), "mx_param_runs_check")
        self.run_off = torch.from_numpy(off).cuda()
        self.run_end = torch.from_numpy(end).cuda()
        self.wd = torch.from_numpy(wd).cuda()
        self.lr_scale = torch.from_numpy(scale).cuda()
        self.rec = ParamRunsRec(self.run_off.data_ptr(), self.run_end.data_ptr(), self.wd.data_ptr(),
                                self.lr_scale.data_ptr(), len(self.runs))
        self.addr = ctypes.addressof(self.rec)


ADAM_BIAS_MAX = 1 << 21     # entries (16 MB): reached at beta2 ~ 0.99999


def adam_bias_table(beta1, beta2):
    """Adam's bias corrections as the fused kernel reads them (include/matcha_gossip.h, mx_adamw_mix):
    float32 [n_bias, 2], row t-1 = (f32(1 - beta1**t), f32(sqrt(1 - beta2**t))) in Python floats, as
    torch.optim.Adam computes them, ending at the first row where both are exactly 1.0f -- every later
    step uses that row, exactly.  ValueError for betas outside [0, 1) or that do not get there within
    2^21 rows."""
    beta1, beta2 = float(beta1), float(beta2)
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError(f"adam_bias_table: betas ({beta1}, {beta2}) outside [0, 1)")
    one = np.float32(1.0)

    def row(t):
        return np.float32(1.0 - beta1 ** t), np.float32(math.sqrt(1.0 - beta2 ** t))

    # both columns are non-decreasing in t, so the last admissible row decides before anything is built
    if row(ADAM_BIAS_MAX) != (one, one):
        raise ValueError(f"adam_bias_table: betas ({beta1}, {beta2}) do not saturate within {ADAM_BIAS_MAX} steps")
    rows = []
    for t in range(1, ADAM_BIAS_MAX + 1):
        rows.append(row(t))
        if rows[-1] == (one, one):
            break
    return np.array(rows, dtype=np.float32).reshape(-1, 2)


def partition(n, nranks):
    """Contiguous worker blocks [(row_base, n_local)] per rank (sizes differ by at most 1)."""
    base, extra = divmod(n, nranks)
    out, start = [], 0
    for r in range(nranks):
        cnt = base + (1 if r < extra else 0)
        out.append((start, cnt))
        start += cnt
    return out


def owner_table(n, nranks):
    own = np.empty(n, np.int32)
    for r, (b, c) in enumerate(partition(n, nranks)):
        own[b:b + c] = r
    return own


def validate_partner(partner):
    """The drawer's table must describe matchings: symmetric, in range (graph_manager.py:157-180)."""
    M, n = partner.shape
    for g in range(M):
        for i in range(n):
            j = int(partner[g, i])
            if j == -1:
                continue
            if not (0 <= j < n) or j == i or int(partner[g, j]) != i:
                raise ValueError(f"neighbors_info[{g}] is not a matching at worker {i} -> {j}")


def max_incoming_remote(partner, row_base, n_local):
    """Receive-slab rows needed when every matching is active (upper bound over all rounds): the
    distinct remote workers that partner a local worker in some matching -- each is received
    once per round however many local partners it has (mx_exchange_plan / plan_kernel)."""
    M, n = partner.shape
    remote = set()
    for g in range(M):
        for p in range(n):
            q = int(partner[g, p])
            if q < 0:
                continue
            if row_base <= q < row_base + n_local and not (row_base <= p < row_base + n_local):
                remote.add(p)
    return len(remote)


class RcclComm:
    """An RCCL communicator owned by the C library (one per process), bootstrapped through
    torch.distributed (which must be initialised; any backend) for the unique-id broadcast.

    The communicator is non-blocking with a deadline (mx_rccl_init_timeout): if a peer never
    joins the init, or the connection setup of a later exchange / all-reduce, the call raises
    MXError ("timed out") after `timeout_s` (default $MX_RCCL_TIMEOUT_S or 300 s) instead of
    hanging; abort() then releases the communicator.  A peer that dies or skips an exchange
    AFTER the connections exist leaves the RCCL kernel waiting on the GPU: wait() is the stream
    synchronisation with the same deadline (mx_rccl_wait: on expiry the communicator is aborted
    and MXError raised) -- use it instead of torch.cuda.synchronize() where a peer may be gone."""

    def __init__(self, group=None, timeout_s=None):
        import os
        import torch.distributed as dist
        require_device()
        self.rank = dist.get_rank(group)
        self.nranks = dist.get_world_size(group)
        if timeout_s is None:
            timeout_s = float(os.environ.get("MX_RCCL_TIMEOUT_S") or 300.0)
        self.timeout_s = float(timeout_s)
        uid = (ctypes.c_char * 128)()
        if self.rank == 0:
            check(lib.mx_rccl_unique_id(ctypes.cast(uid, ctypes.c_void_p)), "mx_rccl_unique_id")
        obj = [bytes(uid)]
        dist.broadcast_object_list(obj, src=0, group=group)
        buf = (ctypes.c_char * 128).from_buffer_copy(obj[0])
        h = ctypes.c_void_p()
        nb = ctypes.c_int(0)
        check(lib.mx_rccl_init_timeout(ctypes.cast(buf, ctypes.c_void_p), self.nranks, self.rank,
                                       int(self.timeout_s * 1000), ctypes.byref(h), ctypes.byref(nb)),
              "mx_rccl_init_timeout")
        self.handle = h
        self.nonblocking = bool(nb.value)

    def count(self):
        """ncclCommCount: the ranks RCCL holds in this communicator."""
        n = ctypes.c_int(0)
        check(lib.mx_rccl_count(self.handle, ctypes.byref(n)), "mx_rccl_count")
        return int(n.value)

    def wait(self, stream=None, timeout_s=None):
        """Block until everything enqueued on `stream` (default: the current stream) has run, or
        raise MXError after timeout_s (default: the communicator's deadline) -- the communicator is
        then aborted (mx_rccl_wait)."""
        if not self.handle:
            raise MXError("RcclComm.wait: communicator closed or aborted")
        ms = int(1000 * (self.timeout_s if timeout_s is None else float(timeout_s)))
        rc = lib.mx_rccl_wait(self.handle, stream_ptr(stream), max(1, ms))
        if rc:
            if rc == MX_ERR_RCCL:
                self.handle = None              # only the timeout path aborts the communicator
            check(rc, "mx_rccl_wait")

    def abort(self):
        """Release a communicator whose peers are gone (ncclCommAbort; after a timed-out call)."""
        if self.handle:
            lib.mx_rccl_abort(self.handle)
            self.handle = None

    def close(self):
        if self.handle:
            rc = lib.mx_rccl_destroy(self.handle)
            self.handle = None
            check(rc, "mx_rccl_destroy")


class PullTransport:
    """Cross-GPU partner rows without RCCL: every rank publishes a snapshot of its rows in an
    IPC-shared device buffer (mx_ipc_alloc); its peers map it (mx_ipc_open) and their mixing
    kernel reads the partner rows straight from this GPU's HBM over xGMI (communicator.py:110's
    sendrecv becomes a remote load inside the FMA chain).  A round is three launches on one
    stream and nothing on the host (VirtualWorkerGroup._step_pull):
        1. mx_snapshot_publish_rows: the local rows a peer reads this round (an active partner in
           another block) into snapshot `round % 2` of the buffer, every workgroup ending with a
           system-scope release (the bytes reach HBM, not only this GPU's write-back L2);
        2. mx_pull_gate (one wave): this rank's epoch = round + 1 (system-scope release), then a
           bounded wait for the epochs of the ranks owning this round's and the previous round's
           remote partners, then the receive slots pointed at their snapshot rows (csrc/pull.hip);
        3. the mixing kernel; the plan records carry the peer-reads bit
           (mx_plan_set_peer_reads), so every workgroup first acquires at system scope: lines of
           the same snapshot buffer cached on THIS GPU in round r - 2 are not served.
    Snapshots alternate between two buffers; a rank overwrites snapshot r % 2 in round r + 2 only
    after its gate of round r + 1 saw every reader of round r past its mix.  A
    peer that stops publishing makes the gate expire after `timeout_s` (default
    $MX_PULL_TIMEOUT_S or 300 s): sticky error words, MXError at the end of the round
    (VirtualWorkerGroup.wait_round) or at the next step.  Needs one process per GPU of ONE node
    (the peers' HBM must be mappable) -- or, for tests, several processes sharing a GPU.
    Bootstrap uses torch.distributed (any backend).  VirtualWorkerGroup.close() is collective
    under this transport (a barrier before the buffers are freed)."""

    handle = None

    def __init__(self, group=None, timeout_s=None):
        import os
        import torch.distributed as dist
        require_device()
        self.group = group
        self.rank = dist.get_rank(group)
        self.nranks = dist.get_world_size(group)
        if self.nranks > 64:
            raise ValueError("PullTransport: at most 64 ranks")
        if timeout_s is None:
            timeout_s = float(os.environ.get("MX_PULL_TIMEOUT_S") or 300.0)
        if not timeout_s > 0:
            raise ValueError("PullTransport: timeout_s must be > 0")
        self.timeout_s = float(timeout_s)

    def bind(self, vwg, row_bytes=None):
        """Collective: allocate vwg's snapshot buffer, exchange handles, map the peers'.  Every
        rank takes part in every exchange even when its own step failed, and all ranks raise
        together (MXError naming the first failing rank) if any failed, so a refusal on one GPU
        cannot leave the others waiting.  No retry: a refused export is counted by the library
        (mx_ipc_stats -> pull_stats()) and reported, never absorbed (DESIGN.md "IPC exports").
        row_bytes: the stride of one worker's snapshot (default: a whole row, vwg.ld floats; a
        ChocoWorkerGroup passes its message stride)."""
        import torch.distributed as dist
        hb = int(lib.mx_ipc_handle_bytes())
        half = vwg.n_local * (int(row_bytes) if row_bytes is not None else vwg.ld * 4)
        _BIND_STATS["binds"] += 1
        own = ctypes.c_void_p()
        handle = (ctypes.c_char * hb)()
        err = None
        try:
            check(lib.mx_ipc_alloc(PULL_HEADER + 2 * half, ctypes.byref(own), ctypes.cast(handle, ctypes.c_void_p)),
                  "mx_ipc_alloc")
        except MXError as e:
            err = str(e)
        objs = [None] * self.nranks
        dist.all_gather_object(objs, (self.rank, None if err else bytes(handle)), group=self.group)
        peers = [0] * self.nranks
        opened = []
        if err is None and all(h is not None for _, h in objs):
            try:
                for r, h in objs:
                    if r == self.rank:
                        peers[r] = own.value
                        continue
                    buf = (ctypes.c_char * hb).from_buffer_copy(h)
                    p = ctypes.c_void_p()
                    check(lib.mx_ipc_open(ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(p)), "mx_ipc_open")
                    peers[r] = p.value
                    opened.append(p.value)
            except MXError as e:
                err = str(e)
        elif err is None:
            err = "a peer could not allocate its snapshot buffer"
        oks = [None] * self.nranks
        dist.all_gather_object(oks, err, group=self.group)
        bad = [(r, e) for r, e in enumerate(oks) if e is not None]
        if bad:
            for p in opened:
                lib.mx_ipc_close(p)
            if own.value:
                lib.mx_ipc_free(own.value)
            _BIND_STATS["failed"] += 1
            sys.stderr.write(f"[matcha_gossip] PullTransport.bind: rank {self.rank}: failed: {bad}\n")
            raise MXError(f"pull transport unavailable: rank {bad[0][0]}: {bad[0][1]}")
        return _PullState(self, vwg, own.value, peers, opened, half)


PULL_HEADER = 256          # MX_PULL_HEADER_BYTES: the epoch word ahead of the two snapshots

# this process's pull-transport binds: how many, how many failed (on any rank of the group)
# (with mx_ipc_stats' refused exports, reported by bench.py's line and checked
# to be zero by the multi-process tests -- never absorbed silently)
_BIND_STATS = {"binds": 0, "failed": 0}


def ipc_stats():
    """(hipIpcGetMemHandle calls, refusals) of this process so far (mx_ipc_stats)."""
    ex, ref = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.mx_ipc_stats(ctypes.byref(ex), ctypes.byref(ref)), "mx_ipc_stats")
    return int(ex.value), int(ref.value)


def pull_stats():
    """{"binds", "bind_failures", "ipc_exports", "ipc_refused", "ipc_recovered"} of this process so
    far: every PullTransport.bind, every hipIpcGetMemHandle call, every mx_ipc_alloc that returned no
    exported block, and every refused block a second allocation recovered (the address range of a
    just-closed import reused: mx_ipc_alloc, tools/ipc_reuse_probe.py)."""
    ex, ref = ipc_stats()
    return {"binds": _BIND_STATS["binds"], "bind_failures": _BIND_STATS["failed"], "ipc_exports": ex,
            "ipc_refused": ref, "ipc_recovered": int(lib.mx_ipc_get(b"recovered"))}


class _PullState:
    """One group's bound pull buffers: the device table of every rank's snapshot buffer
    (mx_pull_rank), the previous round's flags row, and the gate's sticky error words."""

    def __init__(self, transport, vwg, own, peers, opened, half):
        self.transport, self.own, self.peers, self.opened, self.half = transport, own, peers, opened, half
        self.round = 0
        blocks = partition(int(vwg.topology.size), transport.nranks)
        tab = np.zeros((transport.nranks, 2), np.int64)
        for r, (b, c) in enumerate(blocks):
            tab[r, 0] = peers[r]
            tab[r, 1] = (int(b) & 0xFFFFFFFF) | (int(c) << 32)      # int32 row_base, int32 n_local
        self.ranks_dev = torch.from_numpy(tab).to("cuda")
        self.owner_dev = torch.from_numpy(np.ascontiguousarray(vwg.engine.owner)).to("cuda")
        self.prev_row = torch.zeros(vwg.engine.M, dtype=torch.uint8, device="cuda")
        host, dev = ctypes.POINTER(ctypes.c_int32)(), ctypes.c_void_p()
        check(lib.mx_host_words(4, ctypes.byref(host), ctypes.byref(dev)), "mx_host_words")
        self.err_host, self.err_dev = host, dev.value

    def error(self):
        """None, or the gate's message once one of its waits expired (sticky)."""
        if not self.err_host or self.err_host[0] == 0:
            return None
        e = [int(self.err_host[i]) for i in range(4)]
        if e[0] == 2:
            return "pull gate: more distinct remote partners than receive slots"
        return (f"pull gate: rank {e[1]} did not publish round epoch {e[2]} within "
                f"{self.transport.timeout_s:g} s (last seen {e[3]}); the round's result is undefined")

    def close(self):
        for p in self.opened:
            lib.mx_ipc_close(p)
        self.opened = []
        if self.own:
            lib.mx_ipc_free(self.own)
            self.own = 0
        if self.err_host:
            lib.mx_host_words_free(ctypes.cast(self.err_host, ctypes.c_void_p))
            self.err_host = None


def wait_round(comm, stream=None):
    """The end-of-round synchronisation of communicate(): with the library's RCCL communicator a
    deadline-bounded wait (RcclComm.wait -- a peer gone mid-exchange raises instead of hanging),
    otherwise torch.cuda.synchronize().  An RcclComm that was aborted raises: its kernels may
    still be queued, and an unbounded synchronize could hang on them."""
    if isinstance(comm, RcclComm):
        if not comm.handle:
            raise MXError("the RCCL communicator was aborted or closed (an earlier exchange timed out)")
        comm.wait(stream)
    else:
        torch.cuda.synchronize()


_DEFAULT_COMM = None


def default_comm():
    """Process-wide RCCL communicator over the default torch.distributed group."""
    global _DEFAULT_COMM
    if _DEFAULT_COMM is None:
        _DEFAULT_COMM = RcclComm()
    return _DEFAULT_COMM


def topology_flags(topology):
    """Device flag table uint8 [T][M] of a processor, consistent with its host active_flags."""
    host = np.asarray(topology.active_flags, dtype=np.uint8)
    if host.ndim != 2:
        raise ValueError("active_flags must be a rectangular [iterations][matchings] table")
    dev = getattr(topology, "flags_dev", None)
    if dev is not None and tuple(dev.shape) == host.shape:
        if np.array_equal(dev.cpu().numpy(), host):
            return dev, host
    return torch.from_numpy(np.ascontiguousarray(host)).to("cuda"), host


def flags_row(active_flags, M):
    """A flags row as uint8[M]: a shorter row (FixedProcessor's two columns) names the first
    matchings only, like the reference's enumerate(active_flags) walk (communicator.py:99-110); a
    longer one names matchings that do not exist (neighbors_info[graph_id] would fail there too)."""
    f = np.asarray(active_flags)
    if f.ndim != 1 or f.shape[0] > M:
        raise IndexError(f"active_flags must hold at most one entry per matching ({M}), got shape {f.shape}")
    row = np.zeros(M, np.uint8)
    row[:f.shape[0]] = f != 0
    return row


class MixCall(ctypes.Structure):
    """mx_mix_call (include/matcha_gossip.h): a group's mixing arguments packed once, so an eager
    round converts 3 ctypes arguments instead of 13 (mx_gossip_mix_packed)."""
    _fields_ = [("seg_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p),
                ("tile_off_dev", ctypes.c_void_p), ("seg_vec_dev", ctypes.c_void_p),
                ("plan_dev", ctypes.c_void_p), ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32),
                ("n_slots", ctypes.c_int32), ("n_local", ctypes.c_int32), ("M", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("pad_", ctypes.c_int32), ("need_host", ctypes.c_void_p),
                ("n_iters", ctypes.c_int64)]


class Layout:
    """Pointer table of the mixing kernel: slot k's copy of segment s (include/matcha_gossip.h).
    Lengths are in elements of `dtype` (float32, or bfloat16: the mx_mix_bf16_* tiles and kernels)."""

    def __init__(self, seg_lens, slot_ptrs, n_slots, dtype=torch.float32):
        self.dtype = row_dtype(dtype)
        self.bf16 = dtype == torch.bfloat16
        self.elem = 2 if self.bf16 else 4
        self._tile_fn = lib.mx_mix_bf16_tile if self.bf16 else lib.mx_mix_tile
        nseg = len(seg_lens)
        seg_len = np.asarray(seg_lens, dtype=np.int64)
        table = np.zeros((nseg, n_slots), dtype=np.int64)
        vec = np.ones(nseg, dtype=np.uint8)
        for k, ptrs in enumerate(slot_ptrs):
            for s in range(nseg):
                table[s, k] = ptrs[s]
                if ptrs[s] % 16:
                    vec[s] = 0
        tile_off = np.zeros(nseg + 1, dtype=np.int64)
        if self.bf16:
            check(lib.mx_mix_bf16_layout(seg_len.ctypes.data, nseg, n_slots, tile_off.ctypes.data),
                  "mx_mix_bf16_layout")
        else:
            check(lib.mx_mix_layout(seg_len.ctypes.data, nseg, n_slots, tile_off.ctypes.data), "mx_mix_layout")
        self.nseg = nseg
        self.n_slots = n_slots
        self.tile = int(self._tile_fn(n_slots))
        self.total_tiles = int(tile_off[-1])
        self.seg_ptrs = torch.from_numpy(table).to("cuda")
        self.seg_len = torch.from_numpy(seg_len).to("cuda")
        self.tile_off = torch.from_numpy(tile_off).to("cuda")
        self.seg_vec = torch.from_numpy(vec).to("cuda")
        self.tune_gen = _TUNE_GEN[0]
        self._args = (self.seg_ptrs.data_ptr(), self.seg_len.data_ptr(), self.tile_off.data_ptr(),
                      self.seg_vec.data_ptr(), nseg, self.total_tiles, n_slots)
        # engine -> (MixCall, its address).  Keyed by the engine object, weakly: a freed engine's
        # record goes with it, so a later engine whose plan tensor reuses the same device address
        # never inherits its n_local / M / alpha or its need_host pointer
        self._calls = weakref.WeakKeyDictionary()

    def call_for(self, engine):
        """The packed mx_mix_call of this layout under `engine` (built once, kept while both live)."""
        rec = self._calls.get(engine)
        if rec is None:
            need = engine.need_host
            c = MixCall(self._args[0], self._args[1], self._args[2], self._args[3], engine._plan_ptr,
                        self.total_tiles, self.nseg, self.n_slots, engine.n_local, engine.M, engine.alpha32, 0,
                        need.ctypes.data if need is not None else None, len(need) if need is not None else 0)
            rec = self._calls[engine] = (c, ctypes.addressof(c))
        return rec[1]


class SgdMixCall(ctypes.Structure):
    """mx_sgd_mix_call (include/matcha_gossip.h): the fused SGD + mixing launch's arguments, packed once."""
    _fields_ = [("x_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p), ("plan_dev", ctypes.c_void_p),
                ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("n_local", ctypes.c_int32), ("M", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("wd", ctypes.c_float), ("mom", ctypes.c_float), ("nesterov", ctypes.c_int32),
                ("zero_grads", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class AdamwMixCall(ctypes.Structure):
    """mx_adamw_mix_call (include/matcha_gossip.h): the fused AdamW + mixing launch's arguments, packed once."""
    _fields_ = [("x_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("v_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p),
                ("plan_dev", ctypes.c_void_p), ("bias_dev", ctypes.c_void_p), ("total_tiles", ctypes.c_int64),
                ("n_bias", ctypes.c_int64), ("nseg", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("n_local", ctypes.c_int32), ("M", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("wd", ctypes.c_float), ("omb1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("omb2", ctypes.c_float), ("eps", ctypes.c_float), ("decoupled", ctypes.c_int32),
                ("zero_grads", ctypes.c_int32)]


class SgdBf16Call(ctypes.Structure):
    """mx_sgd_mix_bf16_call (include/matcha_gossip.h): the mixed-precision fused launch's arguments."""
    _fields_ = [("w_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("p_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p),
                ("plan_dev", ctypes.c_void_p), ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32),
                ("n_slots", ctypes.c_int32), ("n_local", ctypes.c_int32), ("M", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("wd", ctypes.c_float), ("mom", ctypes.c_float),
                ("nesterov", ctypes.c_int32), ("zero_grads", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class AdamwBf16Call(ctypes.Structure):
    """mx_adamw_mix_bf16_call (include/matcha_gossip.h): the mixed-precision fused AdamW launch's arguments."""
    _fields_ = [("w_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("v_ptrs_dev", ctypes.c_void_p), ("p_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p),
                ("tile_off_dev", ctypes.c_void_p), ("plan_dev", ctypes.c_void_p), ("bias_dev", ctypes.c_void_p),
                ("total_tiles", ctypes.c_int64), ("n_bias", ctypes.c_int64), ("nseg", ctypes.c_int32),
                ("n_slots", ctypes.c_int32), ("n_local", ctypes.c_int32), ("M", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("wd", ctypes.c_float), ("omb1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("omb2", ctypes.c_float), ("eps", ctypes.c_float),
                ("decoupled", ctypes.c_int32), ("zero_grads", ctypes.c_int32)]


class LionMixCall(ctypes.Structure):
    """mx_lion_mix_call (include/matcha_gossip.h): the fused Lion + mixing launch's arguments, packed once."""
    _fields_ = [("x_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p), ("plan_dev", ctypes.c_void_p),
                ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("n_local", ctypes.c_int32), ("M", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("wd", ctypes.c_float), ("omb1", ctypes.c_float), ("omb2", ctypes.c_float),
                ("zero_grads", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class LionBf16Call(ctypes.Structure):
    """mx_lion_mix_bf16_call (include/matcha_gossip.h): the mixed-precision fused Lion launch's arguments."""
    _fields_ = [("w_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("p_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p),
                ("plan_dev", ctypes.c_void_p), ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32),
                ("n_slots", ctypes.c_int32), ("n_local", ctypes.c_int32), ("M", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("wd", ctypes.c_float), ("omb1", ctypes.c_float),
                ("omb2", ctypes.c_float), ("zero_grads", ctypes.c_int32), ("m_bf16", ctypes.c_int32)]


class QgmMixCall(ctypes.Structure):
    """mx_qgm_mix_call (include/matcha_gossip.h): the fused quasi-global-momentum launch's arguments, packed once."""
    _fields_ = [("x_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p), ("plan_dev", ctypes.c_void_p),
                ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("n_local", ctypes.c_int32), ("M", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("wd", ctypes.c_float), ("beta", ctypes.c_float), ("omu", ctypes.c_float),
                ("nesterov", ctypes.c_int32), ("zero_grads", ctypes.c_int32)]


class QgmBf16Call(ctypes.Structure):
    """mx_qgm_mix_bf16_call (include/matcha_gossip.h): the mixed-precision fused QG-momentum launch's arguments."""
    _fields_ = [("w_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("m_ptrs_dev", ctypes.c_void_p),
                ("p_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p),
                ("plan_dev", ctypes.c_void_p), ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32),
                ("n_slots", ctypes.c_int32), ("n_local", ctypes.c_int32), ("M", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("wd", ctypes.c_float), ("beta", ctypes.c_float),
                ("omu", ctypes.c_float), ("nesterov", ctypes.c_int32), ("zero_grads", ctypes.c_int32)]


class GtTrackCall(ctypes.Structure):
    """mx_gt_track_call (include/matcha_gossip.h): the gradient-tracking track launch's arguments, packed once.
    x_ptrs_dev is the tracker's table (the row the round mixes), gp_ptrs_dev the previous gradient's."""
    _fields_ = [("x_ptrs_dev", ctypes.c_void_p), ("g_ptrs_dev", ctypes.c_void_p), ("gp_ptrs_dev", ctypes.c_void_p),
                ("seg_len_dev", ctypes.c_void_p), ("tile_off_dev", ctypes.c_void_p), ("plan_dev", ctypes.c_void_p),
                ("total_tiles", ctypes.c_int64), ("nseg", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("n_local", ctypes.c_int32), ("M", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("zero_grads", ctypes.c_int32)]


class GtTrackBf16Call(ctypes.Structure):
    """mx_gt_track_bf16_call (include/matcha_gossip.h): the track launch's arguments with bfloat16 gradients."""
    _fields_ = list(GtTrackCall._fields_)


class GtStepBf16Call(ctypes.Structure):
    """mx_gt_step_bf16_call (include/matcha_gossip.h): the mixed-precision gradient-tracking step launch's
    arguments: mx_sgd_mix_bf16_call's fields, g_ptrs_dev being the fp32 tracker's table."""
    _fields_ = list(SgdBf16Call._fields_)


SGD_TUNE_KEYS = ("nontemporal", "wgpc", "blocks_per_cu", "flat_small", "grid")
# the QG-momentum families' own knob on top: x and mh staged with plain loads (include/matcha_gossip.h)
QGM_TUNE_KEYS = SGD_TUNE_KEYS + ("stage_plain",)

# the ten entry points of a fused family, as suffixes of its C base name, in FusedFamily's field order
_FUSED_ENTRIES = ("_tile", "_layout", "_set", "_get", "", "_at", "_scaled", "_scaled_at", "_grouped", "_grouped_at")

FusedFamily = collections.namedtuple(
    "FusedFamily", "base rec tables optional adam words "
                   "tile tile_prefix set get run run_at scaled scaled_at grouped grouped_at")


def _family(base, rec, tables, optional, adam, words):
    """base     -- the C base name: every entry point is base + a suffix of _FUSED_ENTRIES
    rec      -- the ctypes mirror of its call record (mx_<family>_call)
    tables   -- its pointer tables in the record's order: table t is the layout's `t_ptrs` and the
                record's `t_ptrs_dev`
    optional -- the table that may be absent (None -> NULL): SGD's momentum
    adam     -- the record carries a bias table and the launches an optimizer-step argument
    words    -- what its messages call the kernel"""
    return FusedFamily(base, rec, tuple(tables.split()), optional, adam, words,
                       *(getattr(lib, base + suffix) for suffix in _FUSED_ENTRIES))


# (optimizer, mixed precision) -> family; everything below reads this table
FAMILIES = {
    ("sgd", False): _family("mx_sgd_mix", SgdMixCall, "x g m", "m", False, "fused SGD + mixing"),
    ("sgd", True): _family("mx_sgd_mix_bf16", SgdBf16Call, "w g m p", "m", False,
                           "mixed-precision fused SGD + mixing"),
    ("adamw", False): _family("mx_adamw_mix", AdamwMixCall, "x g m v", None, True, "fused AdamW + mixing"),
    ("adamw", True): _family("mx_adamw_mix_bf16", AdamwBf16Call, "w g m v p", None, True,
                             "mixed-precision fused AdamW + mixing"),
    ("lion", False): _family("mx_lion_mix", LionMixCall, "x g m", None, False, "fused Lion + mixing"),
    ("lion", True): _family("mx_lion_mix_bf16", LionBf16Call, "w g m p", None, False,
                            "mixed-precision fused Lion + mixing"),
    ("qgm", False): _family("mx_qgm_mix", QgmMixCall, "x g m", None, False, "fused quasi-global momentum + mixing"),
    ("qgm", True): _family("mx_qgm_mix_bf16", QgmBf16Call, "w g m p", None, False,
                           "mixed-precision fused quasi-global momentum + mixing"),
    # gradient tracking: the track launch in both gradient storages, and the mixed-precision step launch (the
    # fp32 step launch is the ("sgd", False) family over the tracker's table)
    ("gt", False): _family("mx_gt_track", GtTrackCall, "x g gp", None, False, "gradient-tracking track + mixing"),
    ("gt", True): _family("mx_gt_track_bf16", GtTrackBf16Call, "x g gp", None, False,
                          "gradient-tracking track + mixing over bfloat16 gradients"),
    ("gt_step", True): _family("mx_gt_step_bf16", GtStepBf16Call, "w g m p", "m", False,
                               "mixed-precision gradient-tracking step + mixing"),
}


def _tuning_pair(fam, keys=SGD_TUNE_KEYS):
    """(<family>_tuning, set_<family>_tuning) of a fused family.  None of the knobs changes the tile
    (include/matcha_gossip.h), so a set invalidates no layout."""
    def tuning():
        return {k: int(fam.get(k.encode())) for k in keys}

    def set_tuning(**knobs):
        for k, v in knobs.items():
            check(fam.set(k.encode(), int(v)), fam.base + "_set")

    stem = fam.base[len("mx_"):]
    tuning.__name__ = tuning.__qualname__ = stem + "_tuning"
    set_tuning.__name__ = set_tuning.__qualname__ = "set_" + stem + "_tuning"
    tuning.__doc__ = f"Current knobs of the {fam.words} kernel (include/matcha_gossip.h, {fam.base}_set)."
    return tuning, set_tuning


sgd_mix_tuning, set_sgd_mix_tuning = _tuning_pair(FAMILIES["sgd", False])
sgd_mix_bf16_tuning, set_sgd_mix_bf16_tuning = _tuning_pair(FAMILIES["sgd", True])
adamw_mix_tuning, set_adamw_mix_tuning = _tuning_pair(FAMILIES["adamw", False])
adamw_mix_bf16_tuning, set_adamw_mix_bf16_tuning = _tuning_pair(FAMILIES["adamw", True])
lion_mix_tuning, set_lion_mix_tuning = _tuning_pair(FAMILIES["lion", False])
lion_mix_bf16_tuning, set_lion_mix_bf16_tuning = _tuning_pair(FAMILIES["lion", True])
qgm_mix_tuning, set_qgm_mix_tuning = _tuning_pair(FAMILIES["qgm", False], QGM_TUNE_KEYS)
qgm_mix_bf16_tuning, set_qgm_mix_bf16_tuning = _tuning_pair(FAMILIES["qgm", True], QGM_TUNE_KEYS)
gt_track_tuning, set_gt_track_tuning = _tuning_pair(FAMILIES["gt", False])
gt_track_bf16_tuning, set_gt_track_bf16_tuning = _tuning_pair(FAMILIES["gt", True])
gt_step_bf16_tuning, set_gt_step_bf16_tuning = _tuning_pair(FAMILIES["gt_step", True])


def _f32(v):
    return float(np.float32(v))


def sgd_hyper(wd, mom, nesterov, zero_grads):
    """The SGD records' words after alpha: wd, mom, nesterov, zero_grads, pad_."""
    return _f32(wd), _f32(mom), int(bool(nesterov)), int(bool(zero_grads)), 0


def adam_hyper(betas, eps, wd, decoupled, zero_grads):
    """The Adam records' words after alpha: wd, omb1, beta2, omb2, eps, decoupled, zero_grads.  betas are
    the Python floats: omb1 / omb2 are rounded from the fp64 values 1 - beta."""
    b1, b2 = float(betas[0]), float(betas[1])
    return (_f32(wd), _f32(1.0 - b1), _f32(b2), _f32(1.0 - b2), _f32(eps), int(bool(decoupled)),
            int(bool(zero_grads)))


def lion_hyper(betas, wd, zero_grads, m_bf16=None):
    """The Lion records' words after alpha: wd, omb1, omb2, zero_grads, then pad_ (fp32 record) or, with
    m_bf16 given, m_bf16 (mixed-precision record).  betas are the Python floats: omb1 / omb2 are rounded
    from the fp64 values 1 - beta, as adam_hyper's."""
    b1, b2 = float(betas[0]), float(betas[1])
    return (_f32(wd), _f32(1.0 - b1), _f32(1.0 - b2), int(bool(zero_grads)), 0 if m_bf16 is None else int(bool(m_bf16)))


def lion_arguments(betas, weight_decay, momentum_dtype, master_weights):
    """attach_lion's own argument checks, a pure host function: (betas, weight_decay, m_bf16).  ValueError
    for betas outside [0, 1), a negative weight decay, a momentum dtype other than float32 / bfloat16, and
    bfloat16 momentum without master weights."""
    betas = (float(betas[0]), float(betas[1]))
    weight_decay = float(weight_decay)
    if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
        raise ValueError(f"attach_lion: betas {betas} outside [0, 1)")
    if not weight_decay >= 0.0:
        raise ValueError("attach_lion: weight_decay must not be negative")
    if momentum_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"attach_lion: momentum_dtype is torch.float32 or torch.bfloat16, not {momentum_dtype}")
    m_bf16 = momentum_dtype == torch.bfloat16
    if m_bf16 and not master_weights:
        raise ValueError("attach_lion: bfloat16 momentum is the mixed-precision round's (a bfloat16 group with "
                         "master_weights=True)")
    return betas, weight_decay, m_bf16


def qgm_hyper(beta, mu, wd, nesterov, zero_grads):
    """The QG-momentum records' words after alpha: wd, beta, omu, nesterov, zero_grads.  beta and mu are the
    Python floats: omu is rounded from the fp64 value 1 - mu, as adam_hyper's omb1."""
    return _f32(wd), _f32(beta), _f32(1.0 - float(mu)), int(bool(nesterov)), int(bool(zero_grads))


def qgm_arguments(momentum, mu, weight_decay):
    """attach_qgm's own argument checks, a pure host function: (momentum, mu, weight_decay) with mu = momentum
    when None (the paper's setting).  ValueError for a momentum or mu outside [0, 1) and a negative weight
    decay."""
    momentum = float(momentum)
    mu = momentum if mu is None else float(mu)
    weight_decay = float(weight_decay)
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"attach_qgm: momentum {momentum} outside [0, 1)")
    if not 0.0 <= mu < 1.0:
        raise ValueError(f"attach_qgm: mu {mu} outside [0, 1)")
    if not weight_decay >= 0.0:
        raise ValueError("attach_qgm: weight_decay must not be negative")
    return momentum, mu, weight_decay


def gt_track_hyper(zero_grads):
    """The track records' one word after alpha: zero_grads."""
    return (int(bool(zero_grads)),)


def gt_arguments(momentum, weight_decay, nesterov):
    """attach_gt's own argument checks, a pure host function: (momentum, weight_decay, nesterov).  ValueError for
    a momentum outside [0, 1), a negative weight decay and Nesterov without momentum."""
    momentum, weight_decay, nesterov = float(momentum), float(weight_decay), bool(nesterov)
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"attach_gt: momentum {momentum} outside [0, 1)")
    if not weight_decay >= 0.0:
        raise ValueError("attach_gt: weight_decay must not be negative")
    if nesterov and momentum == 0.0:
        raise ValueError("attach_gt: Nesterov momentum requires a momentum")
    return momentum, weight_decay, nesterov


def pack_call(fam, tables, seg_len, tile_off, plan, bias, total_tiles, n_bias, nseg, n_slots, n_local, M, alpha32,
              hyper):
    """The call record of family `fam`, a pure function of integers and floats: `tables` are the device
    addresses of its pointer tables in fam.tables order (None: an absent table, NULL), seg_len / tile_off
    / plan / bias device addresses (bias and n_bias count for the Adam families only), `hyper` the words
    of sgd_hyper / adam_hyper / lion_hyper."""
    head = (*tables, seg_len, tile_off, plan)
    if fam.adam:
        return fam.rec(*head, bias, total_tiles, n_bias, nseg, n_slots, n_local, M, alpha32, *hyper)
    return fam.rec(*head, total_tiles, nseg, n_slots, n_local, M, alpha32, *hyper)


class FusedLayout:
    """Pointer tables of a fused optimizer + mixing kernel (`family`, set by the six classes below): one
    int64 device table [nseg, n_local] per pointer list -- row r's copy of segment s -- as `<t>_ptrs` for
    t in family.tables, the segment lengths (in elements) and the tile prefix; for the Adam families the
    bias-correction table (adam_bias_table) too.  The tile depends on n_local alone (no knob enters it), so
    a layout stays valid for its lifetime."""
    family = None

    def __init__(self, seg_lens, tables, n_local, bias=None):
        fam = self.family
        nseg = len(seg_lens)
        seg_len = np.asarray(seg_lens, dtype=np.int64)
        tile_off = np.zeros(nseg + 1, dtype=np.int64)
        check(fam.tile_prefix(seg_len.ctypes.data, nseg, n_local, tile_off.ctypes.data), fam.base + "_layout")

        def table(rows):
            t = np.zeros((nseg, n_local), dtype=np.int64)
            for r, ptrs in enumerate(rows):
                t[:, r] = ptrs
            return torch.from_numpy(t).to("cuda")

        self.nseg, self.n_local = nseg, n_local
        self.tile = int(fam.tile(n_local))
        self.total_tiles = int(tile_off[-1])
        for t, rows in zip(fam.tables, tables):
            setattr(self, t + "_ptrs", None if rows is None and t == fam.optional else table(rows))
        self.seg_len = torch.from_numpy(seg_len).to("cuda")
        self.tile_off = torch.from_numpy(tile_off).to("cuda")
        self.bias, self.n_bias = None, 0
        if fam.adam:
            bias = np.ascontiguousarray(bias, dtype=np.float32)
            if bias.ndim != 2 or bias.shape[1] != 2 or bias.shape[0] < 1:
                raise ValueError("bias table: float32 [n_bias, 2]")
            self.n_bias = int(bias.shape[0])
            self.bias = torch.from_numpy(bias).to("cuda")

    def _pack(self, engine, hyper):
        """pack_call over this layout's addresses; n_slots, n_local and M are the engine's"""
        fam = self.family
        tables = [getattr(self, t + "_ptrs") for t in fam.tables]
        return pack_call(fam, [t.data_ptr() if t is not None else None for t in tables], self.seg_len.data_ptr(),
                         self.tile_off.data_ptr(), engine._plan_ptr, self.bias.data_ptr() if fam.adam else None,
                         self.total_tiles, self.n_bias, self.nseg, engine.n_slots, engine.n_local, engine.M,
                         engine.alpha32, hyper)


class SgdLayout(FusedLayout):
    """csrc/sgd_mix.hip: row r's copy of segment s, its gradient and -- unless m_ptrs is None (no momentum)
    -- its momentum buffer, fp32, lengths in floats.  x_ptrs / g_ptrs / m_ptrs are lists over the rows of
    per-segment device addresses."""
    family = FAMILIES["sgd", False]

    def __init__(self, seg_lens, x_ptrs, g_ptrs, m_ptrs, n_local):
        super().__init__(seg_lens, (x_ptrs, g_ptrs, m_ptrs), n_local)

    def call(self, engine, wd, mom, nesterov, zero_grads):
        return self._pack(engine, sgd_hyper(wd, mom, nesterov, zero_grads))


class SgdBf16Layout(FusedLayout):
    """csrc/sgd_mix_bf16.hip: row r's fp32 master of segment s, its bfloat16 gradient, its fp32 momentum
    buffer (m_ptrs None without momentum) and its bfloat16 model row, lengths in elements."""
    family = FAMILIES["sgd", True]

    def __init__(self, seg_lens, w_ptrs, g_ptrs, m_ptrs, p_ptrs, n_local):
        super().__init__(seg_lens, (w_ptrs, g_ptrs, m_ptrs, p_ptrs), n_local)

    call = SgdLayout.call


class AdamwLayout(FusedLayout):
    """csrc/adamw_mix.hip: row r's copy of segment s, its gradient, exp_avg and exp_avg_sq, fp32, lengths
    in floats, and the bias-correction table on the device."""
    family = FAMILIES["adamw", False]

    def __init__(self, seg_lens, x_ptrs, g_ptrs, m_ptrs, v_ptrs, n_local, bias):
        super().__init__(seg_lens, (x_ptrs, g_ptrs, m_ptrs, v_ptrs), n_local, bias)

    def call(self, engine, betas, eps, wd, decoupled, zero_grads):
        """betas are the Python floats (adam_hyper)"""
        return self._pack(engine, adam_hyper(betas, eps, wd, decoupled, zero_grads))


class AdamwBf16Layout(FusedLayout):
    """csrc/adamw_mix_bf16.hip: row r's fp32 master of segment s, its bfloat16 gradient, its fp32 exp_avg
    and exp_avg_sq and its bfloat16 model row, lengths in elements, and the bias-correction table."""
    family = FAMILIES["adamw", True]

    def __init__(self, seg_lens, w_ptrs, g_ptrs, m_ptrs, v_ptrs, p_ptrs, n_local, bias):
        super().__init__(seg_lens, (w_ptrs, g_ptrs, m_ptrs, v_ptrs, p_ptrs), n_local, bias)

    call = AdamwLayout.call


class LionLayout(FusedLayout):
    """csrc/lion_mix.hip: row r's copy of segment s, its gradient and its momentum buffer, fp32, lengths in
    floats."""
    family = FAMILIES["lion", False]

    def __init__(self, seg_lens, x_ptrs, g_ptrs, m_ptrs, n_local):
        super().__init__(seg_lens, (x_ptrs, g_ptrs, m_ptrs), n_local)

    def call(self, engine, betas, wd, zero_grads):
        """betas are the Python floats (lion_hyper)"""
        return self._pack(engine, lion_hyper(betas, wd, zero_grads))


class LionBf16Layout(FusedLayout):
    """csrc/lion_mix_bf16.hip: row r's fp32 master of segment s, its bfloat16 gradient, its momentum buffer
    (fp32, or bfloat16 when the call is packed with m_bf16) and its bfloat16 model row, lengths in elements."""
    family = FAMILIES["lion", True]

    def __init__(self, seg_lens, w_ptrs, g_ptrs, m_ptrs, p_ptrs, n_local):
        super().__init__(seg_lens, (w_ptrs, g_ptrs, m_ptrs, p_ptrs), n_local)

    def call(self, engine, betas, wd, zero_grads, m_bf16=False):
        return self._pack(engine, lion_hyper(betas, wd, zero_grads, m_bf16))


class QgmLayout(FusedLayout):
    """csrc/qgm_mix.hip: row r's copy of segment s, its gradient and its quasi-global momentum buffer (the
    `m` table), fp32, lengths in floats."""
    family = FAMILIES["qgm", False]

    def __init__(self, seg_lens, x_ptrs, g_ptrs, m_ptrs, n_local):
        super().__init__(seg_lens, (x_ptrs, g_ptrs, m_ptrs), n_local)

    def call(self, engine, beta, mu, wd, nesterov, zero_grads):
        """beta and mu are the Python floats (qgm_hyper)"""
        return self._pack(engine, qgm_hyper(beta, mu, wd, nesterov, zero_grads))


class QgmBf16Layout(FusedLayout):
    """csrc/qgm_mix_bf16.hip: row r's fp32 master of segment s, its bfloat16 gradient, its fp32 quasi-global
    momentum buffer and its bfloat16 model row, lengths in elements."""
    family = FAMILIES["qgm", True]

    def __init__(self, seg_lens, w_ptrs, g_ptrs, m_ptrs, p_ptrs, n_local):
        super().__init__(seg_lens, (w_ptrs, g_ptrs, m_ptrs, p_ptrs), n_local)

    call = QgmLayout.call


class GtTrackLayout(FusedLayout):
    """csrc/gt_track.hip: row r's tracker of segment s (the `x` table: the row the round mixes), its gradient
    and its previous gradient, fp32, lengths in floats."""
    family = FAMILIES["gt", False]

    def __init__(self, seg_lens, x_ptrs, g_ptrs, gp_ptrs, n_local):
        super().__init__(seg_lens, (x_ptrs, g_ptrs, gp_ptrs), n_local)

    def call(self, engine, zero_grads):
        return self._pack(engine, gt_track_hyper(zero_grads))


class GtTrackBf16Layout(FusedLayout):
    """csrc/gt_track_bf16.hip: row r's fp32 tracker of segment s, its bfloat16 gradient and its fp32 previous
    gradient, lengths in elements."""
    family = FAMILIES["gt", True]

    def __init__(self, seg_lens, x_ptrs, g_ptrs, gp_ptrs, n_local):
        super().__init__(seg_lens, (x_ptrs, g_ptrs, gp_ptrs), n_local)

    call = GtTrackLayout.call


class GtStepBf16Layout(FusedLayout):
    """csrc/gt_step_bf16.hip: row r's fp32 master of segment s, its fp32 tracker (the `g` table, read only), its
    fp32 momentum buffer (m_ptrs None without momentum) and its bfloat16 model row, lengths in elements."""
    family = FAMILIES["gt_step", True]

    def __init__(self, seg_lens, w_ptrs, g_ptrs, m_ptrs, p_ptrs, n_local):
        super().__init__(seg_lens, (w_ptrs, g_ptrs, m_ptrs, p_ptrs), n_local)

    def call(self, engine, wd, mom, nesterov):
        """no zero_grads: the step launch never writes the tracker (the record refuses the flag)"""
        return self._pack(engine, sgd_hyper(wd, mom, nesterov, False))


FUSED_LAYOUTS = {("sgd", False): SgdLayout, ("sgd", True): SgdBf16Layout,          # keyed as FAMILIES
                 ("adamw", False): AdamwLayout, ("adamw", True): AdamwBf16Layout,
                 ("lion", False): LionLayout, ("lion", True): LionBf16Layout,
                 ("qgm", False): QgmLayout, ("qgm", True): QgmBf16Layout,
                 ("gt", False): GtTrackLayout, ("gt", True): GtTrackBf16Layout,
                 ("gt_step", False): SgdLayout, ("gt_step", True): GtStepBf16Layout}

# what attach_gt holds in _gt: the FusedState of its track launch and of its step launch
GtState = collections.namedtuple("GtState", "track step")

# what attach_sgd / attach_adamw / attach_lion hold in _sgd / _adamw / _lion: the layout, the packed call record and its address,
# then the family's own fields side by side, so that a step reads its launch functions in one lookup
FusedState = collections.namedtuple("FusedState", ("layout", "call", "addr") + FusedFamily._fields)

# optimizer -> its name in messages, the other optimizer, and how attach_* says that bfloat16 rows need masters
# (the conflict check covers every other entry; the named one is looked at first)
_OPTIMIZER_WORDS = {
    "sgd": ("SGD", "adamw", "a bfloat16 group needs fp32 master weights for its SGD step"),
    "adamw": ("AdamW", "sgd", "bfloat16 groups need fp32 master weights under AdamW"),
    "lion": ("Lion", "adamw", "bfloat16 groups need fp32 master weights under Lion"),
}
# every slot a group has (_sgd / _adamw / _lion / _qgm): the three above, then quasi-global momentum, which
# comes last in every other optimizer's conflict check
_FUSED_WORDS = {**_OPTIMIZER_WORDS,
                "qgm": ("QGM", "sgd", "bfloat16 groups need fp32 master weights under quasi-global momentum")}


# ... and gradient tracking, whose slot (_gt) holds a launch PAIR; it comes last in the others' conflict check.
# _FUSED_WORDS keeps its four entries: they are the optimizers whose slot is one FusedState
_GROUP_WORDS = {**_FUSED_WORDS,
                "gt": ("gradient-tracking", "sgd", "bfloat16 groups need fp32 master weights under gradient tracking")}


def _attached(state, opt):
    """The state in a group's _sgd / _adamw / _lion / _qgm / _gt slot, or the error of a group without one."""
    if state is None:
        raise MXError(f"no {_GROUP_WORDS[opt][0]} state: call attach_{opt}() first")
    return state


class GradNormCall(ctypes.Structure):
    """mx_grad_norm_call (include/matcha_gossip.h): the gradient-norm launches' arguments, packed once."""
    _fields_ = [("g_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p), ("work_dev", ctypes.c_void_p),
                ("norm_dev", ctypes.c_void_p), ("scale_dev", ctypes.c_void_p), ("chunks", ctypes.c_int64),
                ("nseg", ctypes.c_int32), ("n_local", ctypes.c_int32), ("elem_size", ctypes.c_int32),
                ("max_norm", ctypes.c_float)]


class GradNorm:
    """Per-worker gradient 2-norms and clip factors on the device (csrc/grad_norm.hip; torch's
    clip_grad_norm_ per row): `norms` and `scales` (fp32 CUDA [n_local]) and the fp64 workspace, over
    the gradient table of a fused layout (SgdLayout / AdamwLayout / their bf16 forms: `layout.g_ptrs`,
    `layout.seg_len`).  elem_size 4 = fp32 gradients, 2 = bfloat16."""

    def __init__(self, seg_lens, layout, elem_size, max_norm):
        seg_len = np.asarray(seg_lens, dtype=np.int64)
        chunks = ctypes.c_int64(0)
        nbytes = int(lib.mx_grad_norm_layout(seg_len.ctypes.data, len(seg_len), layout.n_local, ctypes.byref(chunks)))
        if nbytes < 0:
            check(nbytes, "mx_grad_norm_layout")
        self.layout = layout                                   # keeps the tables alive
        self.max_norm = float(np.float32(max_norm))
        self.work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
        self.norms = torch.zeros(layout.n_local, dtype=torch.float32, device="cuda")
        self.scales = torch.ones(layout.n_local, dtype=torch.float32, device="cuda")
        self.call = GradNormCall(layout.g_ptrs.data_ptr(), layout.seg_len.data_ptr(), self.work.data_ptr(),
                                 self.norms.data_ptr(), self.scales.data_ptr(), chunks.value, len(seg_len),
                                 layout.n_local, int(elem_size), self.max_norm)
        self._addr = ctypes.addressof(self.call)
        self.scale_ptr = self.scales.data_ptr()

    def enqueue(self, s):
        """The two norm launches on raw stream `s`: no host synchronisation, graph-capturable."""
        rc = lib.mx_grad_norm(self._addr, s)
        if rc:
            check(rc, "mx_grad_norm")


class ConsensusCall(ctypes.Structure):
    """mx_consensus_call (include/matcha_gossip.h): the consensus-distance launches' arguments, packed once."""
    _fields_ = [("x_ptrs_dev", ctypes.c_void_p), ("seg_len_dev", ctypes.c_void_p), ("work_dev", ctypes.c_void_p),
                ("dist_dev", ctypes.c_void_p), ("stats_dev", ctypes.c_void_p), ("chunks", ctypes.c_int64),
                ("nseg", ctypes.c_int32), ("n_local", ctypes.c_int32), ("elem_size", ctypes.c_int32),
                ("pad_", ctypes.c_int32)]


class Consensus:
    """Every worker's distance from the mean of the rows, the consensus distance and the norm of the mean on
    the device (csrc/consensus.hip): `dists` (fp32 CUDA [n]), `stats` (fp32 CUDA [2]: the consensus
    distance, the norm of the mean) and the fp64 workspace, over the rows at `row_ptrs` ([nseg][n] device
    addresses, segment s of seg_lens[s] elements).  elem_size 4 = fp32 rows, 2 = bfloat16.  `dists` /
    `stats`: output tensors to write instead of new ones (a group's sources share one pair)."""

    def __init__(self, seg_lens, row_ptrs, elem_size, dists=None, stats=None):
        seg_len = np.asarray(seg_lens, dtype=np.int64)
        ptrs = np.ascontiguousarray(row_ptrs, dtype=np.int64).reshape(len(seg_len), -1)
        n = ptrs.shape[1]
        chunks = ctypes.c_int64(0)
        nbytes = int(lib.mx_consensus_layout(seg_len.ctypes.data, len(seg_len), n, ctypes.byref(chunks)))
        if nbytes < 0:
            check(nbytes, "mx_consensus_layout")
        self.x_ptrs = torch.from_numpy(ptrs).cuda()
        self.seg_len = torch.from_numpy(seg_len).cuda()
        self.work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
        self.dists = torch.zeros(n, dtype=torch.float32, device="cuda") if dists is None else dists
        self.stats = torch.zeros(2, dtype=torch.float32, device="cuda") if stats is None else stats
        self.call = ConsensusCall(self.x_ptrs.data_ptr(), self.seg_len.data_ptr(), self.work.data_ptr(),
                                  self.dists.data_ptr(), self.stats.data_ptr(), chunks.value, len(seg_len), n,
                                  int(elem_size), 0)
        self._addr = ctypes.addressof(self.call)

    def enqueue(self, s):
        """The two launches on raw stream `s`: no host synchronisation, graph-capturable."""
        rc = lib.mx_consensus(self._addr, s)
        if rc:
            check(rc, "mx_consensus")


class SlowmoCall(ctypes.Structure):
    """mx_slowmo_call (include/matcha_gossip.h): the SlowMo outer step's arguments, packed once."""
    _fields_ = [("rows", ctypes.c_void_p), ("a", ctypes.c_void_p), ("u", ctypes.c_void_p), ("p", ctypes.c_void_p),
                ("ld", ctypes.c_int64), ("p_ld", ctypes.c_int64), ("count", ctypes.c_int64),
                ("n_local", ctypes.c_int32), ("order", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("beta", ctypes.c_float)]


SLOWMO_BUFFERS = ("maintain", "reset", "average")
# fused family (a group's slot) -> the arenas that count as its momentum-like state at an outer step, by
# attribute name.  Gradient tracking's tracker and previous gradient are not among them: the mean tracker is
# what that algorithm preserves
_SLOWMO_STATE = {
    "sgd": ("mom_arena",),
    "gt": ("mom_arena",),
    "adamw": ("exp_avg_arena", "exp_avg_sq_arena"),
    "lion": ("lion_exp_avg_arena",),
    "qgm": ("qgm_buffer_arena",),
}

# what attach_slowmo holds in _slowmo: the call record and its address, the buffer strategy, the state arenas
# it acts on and whether the family counts optimizer steps (AdamW: "reset" restarts the count)
SlowmoState = collections.namedtuple("SlowmoState", ("call", "addr", "buffers", "arenas", "adam", "order"))


IDLE_MODES = {"skip": 0, "canonical": 1}


class GossipEngine:
    """Schedule + plans for one block of workers of a FixedProcessor / MatchaProcessor.

    idle_rows -- workers with no active partner in an active round: "skip" (default; not read or
    written) or "canonical" (rewritten as 0 + 1.0 * x like the reference's averaging, which turns
    -0.0 into +0.0 -- bit-identical to the reference at the cost of streaming those rows;
    mx_plan_set_idle)."""

    def __init__(self, topology, row_base=0, n_local=None, comm=None, owner=None, idle_rows="skip"):
        require_device()
        if idle_rows not in IDLE_MODES:
            raise ValueError(f"idle_rows must be one of {sorted(IDLE_MODES)}")
        self.idle_rows = idle_rows
        self.topology = topology
        self.n = int(topology.size)
        partner_all = np.asarray(topology.neighbors_info, dtype=np.int32).reshape(-1, self.n)
        self.flags_dev, self.flags_host = topology_flags(topology)
        self.T, self.M = self.flags_host.shape
        if self.M > partner_all.shape[0]:
            raise IndexError(f"active_flags has {self.M} columns but only {partner_all.shape[0]} "
                             "matchings exist (neighbors_info[graph_id] would fail)")
        if self.M < partner_all.shape[0]:
            # FixedProcessor's table has two columns (graph_manager.py:208-225) while the
            # reference's averaging(active_flags) walks whatever row it is given over
            # neighbors_info: the table is padded with zero columns, so a round over every
            # matching (adhoc) is expressible; schedule rounds are unchanged
            pad = partner_all.shape[0] - self.M
            self.flags_host = np.hstack([self.flags_host, np.zeros((self.T, pad), np.uint8)])
            self.flags_dev = torch.from_numpy(np.ascontiguousarray(self.flags_host)).to("cuda")
            self.M = partner_all.shape[0]
        self.partner = np.ascontiguousarray(partner_all[:self.M])
        validate_partner(self.partner)
        self.alpha = float(topology.neighbor_weight)
        self.alpha32 = float(np.float32(self.alpha))
        self.row_base = int(row_base)
        self.n_local = self.n if n_local is None else int(n_local)
        self.comm = comm
        self.rank = comm.rank if comm is not None else 0
        if comm is not None and owner is not None and int(owner[self.row_base]) != self.rank:
            raise ValueError("worker block does not belong to this rank")
        self.owner = (np.zeros(self.n, np.int32) if owner is None
                      else np.ascontiguousarray(owner, dtype=np.int32))
        self.max_remote = max_incoming_remote(self.partner, self.row_base, self.n_local)
        if self.max_remote and comm is None:
            raise ValueError("workers outside this block have partners inside it: an RCCL "
                             "communicator is required")
        self.n_slots = self.n_local + self.max_remote
        if lib.mx_mix_tile(self.n_slots) <= 0:   # 1-64 slots: tuned kernels; 65-156: mix_kernel_wide
            raise MXError(f"{self.n_slots} slots per GPU (local workers + distinct remote partners) exceed "
                          "the 156 a mixing tile holds in LDS: spread the workers over more GPUs")
        self.plan_words = int(lib.mx_plan_words(self.n_local, self.M))
        self.partner_dev = torch.from_numpy(self.partner).to("cuda")
        # the schedule's T records + one scratch record (index T) for a round of arbitrary flags (adhoc)
        self.plan = torch.empty((self.T + 1) * self.plan_words, dtype=torch.int32, device="cuda")
        check(lib.mx_plan_build(self.flags_dev.data_ptr(), self.T, self.M, self.partner_dev.data_ptr(),
                                self.n, None, self.rank, self.row_base, self.n_local, self.alpha,
                                self.plan.data_ptr(), stream_ptr()), "mx_plan_build")
        if IDLE_MODES[idle_rows]:
            check(lib.mx_plan_set_idle(self.plan.data_ptr(), self.T, self.n_local, self.M, IDLE_MODES[idle_rows],
                                       stream_ptr()), "mx_plan_set_idle")
        self.flags_host = np.vstack([self.flags_host, np.zeros((1, self.M), np.uint8)])
        self.any_active = self.flags_host.any(axis=1).tolist()
        # per round, the local rows the mixing kernel reads and writes (the plan record's own row
        # set, from the host's copy of the flags): mx_mix_call.need_host, the kernel's load hint
        self._has_partner = (self.partner[:, self.row_base:self.row_base + self.n_local] >= 0).astype(np.int32)
        self.need_host = None
        if self.n_local <= 64:
            self.need_host = np.zeros(self.T + 1, np.uint64)
            self.need_host[:] = self._need_bits(self.flags_host)
        self._plan_ptr = self.plan.data_ptr()
        self.peer_reads = False                  # set by a pull-transport group: applied to adhoc records too
        self._adhoc_ready = False
        self._adhoc_flags = None
        self._row_index = None                   # flags bytes -> first schedule iteration (record_for)

    def adhoc(self, active_flags):
        """A round for an arbitrary flags row -- the reference's averaging(active_flags) takes any
        row, not only the schedule's (communicator.py:92-122, 200-230): its plan record is built
        into the scratch record after the schedule's T rows (stream-ordered, on the current
        stream) and its index, T, returned; valid until the next adhoc() call.  Collective like the
        reference's sendrecv: with N > 1 every rank passes the same row."""
        f = self.flags_row(active_flags)
        self.flags_host[self.T] = f
        self.any_active[self.T] = bool(f.any())
        if self.need_host is not None:
            self.need_host[self.T] = self._need_bits(f[None, :])[0]
        self._adhoc_flags = torch.from_numpy(f.copy()).to("cuda")
        rec = self._plan_ptr + 4 * self.T * self.plan_words
        check(lib.mx_plan_build(self._adhoc_flags.data_ptr(), 1, self.M, self.partner_dev.data_ptr(), self.n, None,
                                self.rank, self.row_base, self.n_local, self.alpha, rec, stream_ptr()),
              "mx_plan_build")
        if IDLE_MODES[self.idle_rows]:
            check(lib.mx_plan_set_idle(rec, 1, self.n_local, self.M, IDLE_MODES[self.idle_rows], stream_ptr()),
                  "mx_plan_set_idle")
        if self.peer_reads:
            check(lib.mx_plan_set_peer_reads(rec, 1, self.n_local, self.M, 1, stream_ptr()), "mx_plan_set_peer_reads")
        self._adhoc_ready = True
        return self.T

    def _need_bits(self, flags):
        """uint64 row masks of rounds `flags` [t][M]: bit r = local row r has an active partner
        (every row of an active round in idle mode "canonical"), as plan_kernel decides."""
        flags = np.asarray(flags, np.int32)
        rows = (flags @ self._has_partner) > 0
        if IDLE_MODES[self.idle_rows]:
            rows = np.repeat(flags.any(axis=1)[:, None], self.n_local, axis=1)
        weights = np.left_shift(np.uint64(1), np.arange(self.n_local, dtype=np.uint64))
        return (rows.astype(np.uint64) * weights[None, :]).sum(axis=1, dtype=np.uint64)

    def record_for(self, active_flags):
        """The plan record of an arbitrary flags row without rebuilding when one exists: a record
        depends only on the row (partners and alpha are fixed), so any schedule iteration with the
        same row -- or the scratch record when it already holds this row -- serves it; otherwise
        adhoc() builds it.  (The reference's averaging(active_flags) sub-step, communicator.py:92-122,
        driven directly: at most 2^M distinct rows, so rebuilds stop after the first of each.)"""
        f = self.flags_row(active_flags)
        key = f.tobytes()
        if self._row_index is None:
            self._row_index = {}
            for t in range(self.T - 1, -1, -1):          # the first iteration holding each row
                self._row_index[self.flags_host[t].tobytes()] = t
        t = self._row_index.get(key)
        if t is not None:
            return t
        if self._adhoc_ready and self.flags_host[self.T].tobytes() == key:
            return self.T
        return self.adhoc(f)

    def flags_row(self, active_flags):
        return flags_row(active_flags, self.M)

    def round_index(self, it):
        """`it` checked against the plan table: a schedule row, or T after adhoc()."""
        it = int(it)
        if not (0 <= it < self.T or (it == self.T and self._adhoc_ready)):
            raise IndexError(f"iteration {it} outside the schedule's {self.T} rows")
        return it

    # ------------------------------------------------------------------ per round
    def exchange_plan(self, it):
        """The ordered point-to-point operations of round `it` for this block (native
        mx_exchange_plan): int32 [n_ops][4] = (0 send / 1 recv, peer, local row / slab slot,
        worker whose row travels)."""
        fr = np.ascontiguousarray(self.flags_host[it])
        cnt = ctypes.c_int(0)
        check(lib.mx_exchange_plan(fr.ctypes.data, self.M, self.partner.ctypes.data, self.n,
                                   self.owner.ctypes.data, self.rank, self.row_base, self.n_local,
                                   None, 0, ctypes.byref(cnt)), "mx_exchange_plan")
        ops = np.zeros((max(1, cnt.value), 4), np.int32)
        check(lib.mx_exchange_plan(fr.ctypes.data, self.M, self.partner.ctypes.data, self.n,
                                   self.owner.ctypes.data, self.rank, self.row_base, self.n_local,
                                   ops.ctypes.data, cnt.value, ctypes.byref(cnt)), "mx_exchange_plan")
        return ops[:cnt.value]

    def exchange(self, it, row_ptrs, slab_ptr, slab_ld_bytes, row_bytes, stream=None):
        """Sends/receives of iteration `it` (no-op with one process).  The transport is the RCCL
        communicator (mx_exchange_round); an object with an ``exchange_round`` method may stand
        in for it (tests use an in-process loopback to drive N ranks on one GPU)."""
        if self.comm is None:
            return 0
        if hasattr(self.comm, "exchange_round"):
            return self.comm.exchange_round(self, it, row_ptrs, slab_ptr, slab_ld_bytes, row_bytes)
        row_arr = (ctypes.c_void_p * self.n_local)(*row_ptrs)
        nrem = ctypes.c_int(0)
        fr = np.ascontiguousarray(self.flags_host[it])
        check(lib.mx_exchange_round(self.comm.handle, fr.ctypes.data, self.M, self.partner.ctypes.data,
                                    self.n, self.owner.ctypes.data, self.rank, self.row_base,
                                    self.n_local, row_arr, slab_ptr, int(slab_ld_bytes), int(row_bytes),
                                    ctypes.byref(nrem), stream_ptr(stream)), "mx_exchange_round")
        return nrem.value

    def mix(self, it, layout, stream=None):
        it = self.round_index(it)                # the kernel indexes the plan table by `it`
        if layout.tune_gen != _TUNE_GEN[0]:
            if layout.tile != layout._tile_fn(layout.n_slots):
                raise MXError("layout built for another mixing tile size (the unroll knob changed it)")
            layout.tune_gen = _TUNE_GEN[0]
        # one ctypes call per round with the group's arguments packed once (small rows are
        # launch-bound: tools/launch_overhead.py)
        rc = (_mix_bf16_packed if layout.bf16 else _mix_packed)(layout.call_for(self), it, stream_ptr(stream))
        if rc:
            check(rc, "mx_gossip_mix_bf16_packed" if layout.bf16 else "mx_gossip_mix_packed")


    def mix_at(self, iter_dev, layout, stream=None):
        """Graph-replayable round: the kernel reads the iteration from the int64 device tensor
        `iter_dev` when it runs (mx_gossip_mix_at) and the counter is advanced by one on the same
        stream, so a captured launch pair serves every iteration (a counter past the schedule
        makes the launch a no-op)."""
        if layout.tune_gen != _TUNE_GEN[0]:
            if layout.tile != layout._tile_fn(layout.n_slots):
                raise MXError("layout built for another mixing tile size (the unroll knob changed it)")
            layout.tune_gen = _TUNE_GEN[0]
        if iter_dev.dtype != torch.int64 or iter_dev.device.type != "cuda" or iter_dev.numel() != 1:
            raise TypeError("iter_dev must be a one-element int64 CUDA tensor")
        s = stream_ptr(stream)
        mix_at = lib.mx_gossip_mix_bf16_at if layout.bf16 else lib.mx_gossip_mix_at
        check(mix_at(*layout._args, self._plan_ptr, iter_dev.data_ptr(), self.T, self.n_local,
                     self.M, self.alpha32, s), "mx_gossip_mix_bf16_at" if layout.bf16 else "mx_gossip_mix_at")
        check(lib.mx_iter_advance(iter_dev.data_ptr(), 1, s), "mx_iter_advance")

    def mix_rounds_at(self, iter_dev, ctrs, layout, stream=None):
        """len(ctrs) graph-replayable rounds with one bookkeeping launch (mx_iter_expand: ctrs[j] =
        *iter_dev + j, *iter_dev += K), then one mixing launch per round reading its own counter --
        the same rounds as K mix_at calls, without the K counter bumps."""
        if layout.tune_gen != _TUNE_GEN[0]:
            if layout.tile != layout._tile_fn(layout.n_slots):
                raise MXError("layout built for another mixing tile size (the unroll knob changed it)")
            layout.tune_gen = _TUNE_GEN[0]
        for t in (iter_dev, ctrs):
            if t.dtype != torch.int64 or t.device.type != "cuda" or not t.is_contiguous():
                raise TypeError("iteration counters must be contiguous int64 CUDA tensors")
        K = ctrs.numel()
        s = stream_ptr(stream)
        check(lib.mx_iter_expand(iter_dev.data_ptr(), ctrs.data_ptr(), K, s), "mx_iter_expand")
        mix_at = lib.mx_gossip_mix_bf16_at if layout.bf16 else lib.mx_gossip_mix_at
        for j in range(K):
            check(mix_at(*layout._args, self._plan_ptr, ctrs.data_ptr() + 8 * j, self.T,
                         self.n_local, self.M, self.alpha32, s),
                  "mx_gossip_mix_bf16_at" if layout.bf16 else "mx_gossip_mix_at")


def _params(model):
    return [p for p in model.parameters()]


class VirtualWorkerGroup:
    """A block of the topology's workers resident on this process's GPU as rows of an
    [n_local, P] HBM arena (the "all virtual workers on one MI355X" mode, and each rank's share
    in the multi-GPU mode).

    models  -- optional list of n_local torch modules on the GPU (identical architectures);
               with adopt=True their parameters are re-homed into the arena as views (identity
               and shapes kept, so optimizers stay valid) and every round mixes them in place.
    numel   -- arena width when no models are given (synthetic workloads / benchmarks).
    placement -- which workers share a GPU when nranks > 1: None / "contiguous" (blocks of
               consecutive ids), "auto" (placement.best_placement: fewest rows over the busiest
               xGMI pair) or an explicit worker order.  `workers` lists the worker id of each
               local row (models are given in that order).
    idle_rows -- "skip" (default) or "canonical": see GossipEngine.
    dtype   -- torch.float32 (default) or torch.bfloat16: the arena's (and every adopted
               parameter's) element type.  A bfloat16 round runs the fp32 FMA chain over exactly
               widened inputs and rounds to nearest even once at the store (csrc/mix_bf16.hip); it
               moves half the bytes.  bfloat16 groups live on one GPU with every partner local:
               nranks > 1, a transport (comm) and chunk_cols raise NotImplementedError -- the
               exchange, publish and ChocoSGD kernels are fp32-only.
    """

    def __init__(self, topology, models=None, numel=None, *, rank=0, nranks=1, comm=None, adopt=True,
                 chunk_cols=None, placement=None, idle_rows="skip", dtype=torch.float32):
        require_device()
        self.dtype = row_dtype(dtype)
        self.elem = 2 if dtype == torch.bfloat16 else 4
        if dtype == torch.bfloat16:
            if nranks > 1 or comm is not None:
                raise NotImplementedError("bfloat16 worker rows are mixed on one GPU only (nranks = 1, no transport): "
                                          "the RCCL exchange and the pull transport move fp32 rows")
            if chunk_cols:
                raise NotImplementedError("bfloat16 worker rows: chunk_cols pipelines the fp32 cross-GPU exchange, "
                                          "which bfloat16 groups do not have")
        if models is not None:
            # before anything is built or launched
            kind = "bfloat16" if dtype == torch.bfloat16 else "float32"
            for m in models:
                for p in _params(m):
                    if p.dtype != dtype or p.device.type != "cuda":
                        raise TypeError(f"worker parameters must be {kind} CUDA tensors")
        from .placement import block_workers, place
        n = int(topology.size)
        topology, self.placement = place(topology, nranks, placement)
        blocks = partition(n, nranks)
        self.row_base, self.n_local = blocks[rank]
        self.workers = block_workers(self.placement, self.row_base, self.n_local)
        if nranks > 1 and comm is None:
            comm = default_comm()
        self.engine = GossipEngine(topology, self.row_base, self.n_local, comm=comm,
                                   owner=owner_table(n, nranks), idle_rows=idle_rows)
        self.topology = topology
        self.iter = 0
        self.iter_dev = torch.zeros(1, dtype=torch.int64, device="cuda")   # device_round's counter
        self._chunk_cols = chunk_cols
        self._adopted = models if (models is not None and adopt) else None
        self._sgd = None                     # attach_sgd: the fused SGD + mixing launch's state
        self.master_arena = self.master_rows = None   # attach_sgd(master_weights=True): fp32 masters of bf16 rows
        self._adamw = None                   # attach_adamw: the fused AdamW + mixing launch's state
        self._lion = None                    # attach_lion: the fused Lion + mixing launch's state
        self._qgm = None                     # attach_qgm: the fused quasi-global-momentum launch's state
        self._gt = None                      # attach_gt: the gradient-tracking launch pair's state (GtState)
        self._slowmo = None                  # attach_slowmo: the outer step's state (SlowmoState)
        self.slowmo_anchor = self.slowmo_momentum = None
        self.lr_dev = None                   # the device rounds' learning rate (attach_*: a 1-element fp32 CUDA tensor)
        self._clip = None                    # attach_*(clip_grad_norm=...): the norm launch's state (GradNorm)
        self._runs = None                    # attach_*(param_groups=...): the run tables (ParamRuns)
        self.param_runs = None               # ... and the merged run list [(start, end, weight_decay, lr_scale)]
        self._named = list(models[0].named_parameters()) if models is not None else None
        self.clip_grad_norm = None
        self.grad_norms = self.grad_scales = None
        self._round_ctrs = {}                # device_rounds(K): per-round counters, one tensor per K
        self._consensus = {}                 # consensus_distance(): source -> (arena address, Consensus)
        self.consensus_dists = self.consensus_stats = None
        self._one_gpu = nranks == 1 and comm is None
        if models is not None:
            if len(models) != self.n_local:
                raise ValueError(f"{len(models)} models for {self.n_local} local workers")
            shapes = [tuple(p.shape) for p in _params(models[0])]
            for m in models[1:]:
                if [tuple(p.shape) for p in _params(m)] != shapes:
                    raise ValueError("all workers must share one architecture")
            self.numel = int(sum(p.numel() for p in _params(models[0])))
        else:
            if numel is None:
                raise ValueError("give models or numel")
            self.numel = int(numel)
        self.ld = (self.numel + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
        self.arena = torch.zeros((self.n_local, self.ld), dtype=self.dtype, device="cuda")
        # column pipelining of the cross-GPU exchange (N > 1): chunk c+1 travels over RCCL on a side
        # stream while chunk c is mixed; the receive slab is two chunk-wide buffers
        self._pull = None
        self.chunked = bool(self.engine.max_remote and chunk_cols and int(chunk_cols) < self.numel
                            and not isinstance(comm, PullTransport))
        if self.chunked:
            W = (int(chunk_cols) + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
            self.chunk_w = W
            self.chunks = [(c0, min(self.numel, c0 + W)) for c0 in range(0, self.numel, W)]
            self.slab = torch.empty((2, self.engine.max_remote, W), dtype=torch.float32, device="cuda")
            self.comm_stream = torch.cuda.Stream()
        else:
            self.slab = (torch.empty((self.engine.max_remote, self.ld), dtype=torch.float32, device="cuda")
                         if self.engine.max_remote and not isinstance(comm, PullTransport) else None)
        if models is not None:
            for r, m in enumerate(models):
                off = 0
                for p in _params(m):
                    k = p.numel()
                    view = self.arena[r, off:off + k].view(p.shape)
                    view.copy_(p.data)
                    if adopt:
                        p.data = view
                    off += k
        self._row_ptrs = [self.arena[r].data_ptr() for r in range(self.n_local)]
        if self.chunked:
            self.chunk_layouts = []
            for ci, (c0, c1) in enumerate(self.chunks):
                buf = self.slab[ci % 2]
                ptrs = [[p + 4 * c0] for p in self._row_ptrs]
                ptrs += [[buf[k].data_ptr()] for k in range(self.engine.max_remote)]
                self.chunk_layouts.append(Layout([c1 - c0], ptrs, self.engine.n_slots))
            self.layout = Layout([self.numel], [[p] for p in self._row_ptrs] +
                                 [[self.slab[0, 0].data_ptr()]] * self.engine.max_remote, self.engine.n_slots)
        elif isinstance(comm, PullTransport):
            # receive slots point at the peers' snapshot rows, set per round (_step_pull); no slab
            self._pull = comm.bind(self)
            # receive slots will be peers' memory: the mixing kernels acquire at system scope first
            check(lib.mx_plan_set_peer_reads(self.engine.plan.data_ptr(), self.engine.T + 1, self.n_local,
                                             self.engine.M, 1, stream_ptr()), "mx_plan_set_peer_reads")
            self.engine.peer_reads = True
            # receive slots start at this rank's own snapshot 0 (valid memory); every round's gate
            # points them at the partners' snapshot rows on the device (mx_pull_gate)
            slot_ptrs = [[p] for p in self._row_ptrs]
            slot_ptrs += [[self._pull.own + PULL_HEADER]] * self.engine.max_remote
            self.layout = Layout([self.numel], slot_ptrs, self.engine.n_slots)
        else:
            slot_ptrs = [[p] for p in self._row_ptrs]
            if self.slab is not None:
                slot_ptrs += [[self.slab[k].data_ptr()] for k in range(self.engine.max_remote)]
            self.layout = Layout([self.numel], slot_ptrs, self.engine.n_slots, dtype=self.dtype)

    @property
    def rows(self):
        """[n_local, P] view of the workers' flat parameter vectors."""
        return self.arena[:, :self.numel]

    @property
    def publish_cols(self):
        """Floats of a row the pull round publishes (the P the mixing kernel reads, rounded up to 4)."""
        return (self.numel + 3) // 4 * 4

    def step(self, it, stream=None):
        """Enqueue round `it` (exchange + mix) on `stream`; returns False for an all-zero round."""
        if not self.engine.any_active[it]:
            return False
        if self.chunked:
            return self._step_chunked(it, stream)
        if self._pull is not None:
            return self._step_pull(it, stream)
        if self.engine.comm is not None:
            self.engine.exchange(it, self._row_ptrs,
                                 self.slab.data_ptr() if self.slab is not None else None,
                                 self.ld * self.elem, self.numel * self.elem, stream)
        self.engine.mix(it, self.layout, stream)
        return True

    def _step_pull(self, it, stream=None):
        """PullTransport round, three launches on one stream and no host wait: snapshot publish,
        the gate (epoch out, bounded epoch waits, receive slots -> the partners' snapshot rows),
        mix.  A gate that expired in an earlier round raises here (sticky)."""
        st = self._pull
        msg = st.error()
        if msg:
            raise MXError(msg)
        eng = self.engine
        it = eng.round_index(it)
        par = st.round & 1
        st.round += 1
        s = stream_ptr(stream)
        frow = (eng._adhoc_flags.data_ptr() if it == eng.T else eng.flags_dev.data_ptr() + it * eng.M)
        # only the rows a peer reads this round (an active partner in another block), each ending
        # with a system-scope release per workgroup (visible to the peers' loads); a row not
        # published in round k is read by no peer in round k
        check(lib.mx_snapshot_publish_rows(self.arena.data_ptr(), self.ld, st.own + PULL_HEADER + par * st.half,
                                           self.ld, self.publish_cols, self.n_local, frow, eng.M,
                                           eng.partner_dev.data_ptr(), eng.n, self.row_base, s),
              "mx_snapshot_publish_rows")
        tr = st.transport
        check(lib.mx_pull_gate(frow, st.prev_row.data_ptr(), eng.M, eng.partner_dev.data_ptr(), eng.n,
                               st.owner_dev.data_ptr(), st.ranks_dev.data_ptr(), tr.nranks, tr.rank, self.row_base,
                               self.n_local, self.ld * 4, par, st.round, self.layout.seg_ptrs.data_ptr(),
                               eng.n_slots, tr.timeout_s, st.err_dev, s), "mx_pull_gate")
        eng.mix(it, self.layout, stream)
        return True

    def wait_round(self, stream=None):
        """The end of a round for communicate(): the transport's wait (engine.wait_round), then
        the pull gate's sticky error, if any, as MXError."""
        wait_round(self.engine.comm, stream)
        if self._pull is not None:
            msg = self._pull.error()
            if msg:
                raise MXError(msg)

    @property
    def pulls(self):
        """True when the receive slots are peers' IPC-mapped snapshots (PullTransport)."""
        return self._pull is not None

    def close(self):
        """Release the pull transport's shared buffers.  COLLECTIVE under PullTransport: every
        rank's snapshot buffer may still be read by a slower peer's last round, so all ranks first
        meet at a barrier (after their own last mix has finished), then unmap and free.  Not to be
        called from a finalizer (decenCommunicator.__del__ leaves a pull group to process exit)."""
        if self._pull is not None:
            import torch.distributed as dist
            torch.cuda.synchronize()
            dist.barrier(group=self._pull.transport.group)
            self._pull.close()
            self._pull = None

    def _step_chunked(self, it, stream=None):
        cur = stream if stream is not None else torch.cuda.current_stream()
        cs = self.comm_stream
        start = torch.cuda.Event()
        start.record(cur)
        cs.wait_event(start)                 # rows are final (previous round, optimizer) before sending
        mixed = [None, None]
        for ci, (c0, c1) in enumerate(self.chunks):
            b = ci % 2
            if mixed[b] is not None:
                cs.wait_event(mixed[b])      # slab buffer b is free once chunk ci-2 has been mixed
            self.engine.exchange(it, [p + 4 * c0 for p in self._row_ptrs], self.slab[b].data_ptr(),
                                 self.chunk_w * 4, (c1 - c0) * 4, cs)
            arrived = torch.cuda.Event()
            arrived.record(cs)
            cur.wait_event(arrived)
            self.engine.mix(it, self.chunk_layouts[ci], cur)
            mixed[b] = torch.cuda.Event()
            mixed[b].record(cur)
        return True

    def device_round(self, stream=None):
        """Enqueue the round at the device-side counter `self.iter_dev` and advance it (no host
        work depends on the round, so the pair can be captured once in a HIP graph --
        torch.cuda.graph -- and replayed every iteration).  One GPU only: a cross-GPU exchange's
        operation list depends on the round's flags on the host.  Set the counter with
        `self.iter_dev.fill_(it)`; `self.iter` (the host counter of communicate()) is not touched."""
        if self.engine.comm is not None:
            raise MXError("device_round: graph-replayable rounds need all partners on this GPU (nranks = 1)")
        if self.chunked:
            raise MXError("device_round: not with chunk_cols")
        self.engine.mix_at(self.iter_dev, self.layout, stream)

    def device_rounds(self, K, stream=None):
        """K device_round()s in K + 1 launches instead of 2 K (for capture in one HIP graph): the
        rounds at the counter `self.iter_dev` .. + K - 1, counter advanced by K."""
        if self.engine.comm is not None:
            raise MXError("device_rounds: graph-replayable rounds need all partners on this GPU (nranks = 1)")
        if self.chunked:
            raise MXError("device_rounds: not with chunk_cols")
        K = int(K)
        if K < 1:
            raise ValueError("device_rounds: K >= 1")
        ctrs = self._round_ctrs.get(K)
        if ctrs is None:
            ctrs = self._round_ctrs[K] = torch.zeros(K, dtype=torch.int64, device="cuda")
        self.engine.mix_rounds_at(self.iter_dev, ctrs, self.layout, stream)

    # ------------------------------------------------------------------ fused SGD + mixing
    def _attach_clip(self, lay, clip):
        """attach_*(clip_grad_norm=clip): the norm launch's state over the fused layout's gradient table"""
        self.clip_grad_norm = clip
        if clip is None:
            return
        self._clip = GradNorm([self.numel], lay, self.grad_arena.element_size(), clip)
        self.grad_norms, self.grad_scales = self._clip.norms, self._clip.scales

    def _attach_groups(self, param_groups, default_wd, who):
        """attach_*(param_groups=...): None keeps the ungrouped launches (no tables); otherwise the
        groups are resolved (param_runs), checked and uploaded once"""
        if param_groups is None:
            return
        try:
            runs = param_runs(self.numel, self._named, list(param_groups), default_wd)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        self._runs = ParamRuns(self.numel, runs)
        self.param_runs = runs

    def grad_norm(self, stream=None):
        """Enqueue the norm launches alone (csrc/grad_norm.hip) and return `grad_norms`: every worker's
        gradient 2-norm, fp32 CUDA [n_local], valid once the stream reaches it; `grad_scales` holds the
        clip factors.  Needs attach_sgd / attach_adamw with clip_grad_norm set."""
        if self._clip is None:
            raise MXError("grad_norm: no clipping state: attach_sgd / attach_adamw with clip_grad_norm=...")
        self._clip.enqueue(stream_ptr(stream))
        return self.grad_norms

    def consensus_distance(self, stream=None, of=None):
        """Enqueue the consensus-distance launches (csrc/consensus.hip: one read of the rows, no host
        synchronisation, graph-capturable) and return `consensus_dists`: every worker's distance from the
        mean of the rows, fp32 CUDA [n_local], valid once the stream reaches it.  `consensus_stats`
        (fp32 CUDA [2]) then holds the consensus distance sqrt(mean_r dist[r]^2) and the norm of the mean
        row.  of=None measures the fp32 masters where master weights are attached and the group's rows
        (fp32 or bfloat16) otherwise; of="rows" the model rows; of="masters" the masters (MXError
        without them); of="tracker" the gradient trackers of attach_gt (MXError without them): the norm of the
        mean row is then the norm of the mean tracker, which equals the norm of the workers' mean gradient --
        the quantity that goes to zero at a stationary point of the average loss.  The state is built on first use, per source; every source writes the same two
        output tensors.  One GPU only: the mean needs every worker's rows on this GPU."""
        if not self._one_gpu:
            raise NotImplementedError("consensus_distance: the mean needs every worker's rows on this GPU "
                                      "(nranks = 1, no transport); a cross-GPU consensus distance is not built")
        if of not in (None, "rows", "masters", "tracker"):
            raise ValueError(f"consensus_distance: of is None, 'rows', 'masters' or 'tracker', not {of!r}")
        if of == "tracker" and self._gt is None:
            raise MXError("consensus_distance: no tracker: attach_gt() first")
        if of == "masters" and self.master_arena is None:
            raise MXError("consensus_distance: no master weights: attach_sgd / attach_adamw / attach_lion with "
                          "master_weights=True")
        masters = of == "masters" or (of is None and self.master_arena is not None)
        arena = self.master_arena if masters else self.arena
        if of == "tracker":
            masters, arena = "tracker", self.gt_tracker_arena
        if self.consensus_dists is None:
            self.consensus_dists = torch.zeros(self.n_local, dtype=torch.float32, device="cuda")
            self.consensus_stats = torch.zeros(2, dtype=torch.float32, device="cuda")
        held = self._consensus.get(masters)
        if held is None or held[0] != arena.data_ptr():
            state = Consensus([self.numel], [[arena[r].data_ptr() for r in range(self.n_local)]],
                              arena.element_size(), dists=self.consensus_dists, stats=self.consensus_stats)
            held = self._consensus[masters] = (arena.data_ptr(), state)
        held[1].enqueue(stream_ptr(stream))
        return self.consensus_dists

    def _fused_family(self, opt, master_weights, clip_grad_norm):
        """What attach_sgd / attach_adamw refuse alike, before anything is allocated; returns the layout
        class of (opt, mixed precision) and the checked clip norm."""
        who = "attach_" + opt
        name, other, needs_master = _GROUP_WORDS[opt]
        clip = clip_value(clip_grad_norm, who)
        if getattr(self, "_" + opt) is not None:
            raise RuntimeError(f"{who}: already attached")
        if self._slowmo is not None:
            raise RuntimeError(f"{who}: the group already carries SlowMo state: attach_slowmo() comes after the "
                               "base optimizer (it resolves the optimizer's state arenas and masters once)")
        for o in [other] + [k for k in _GROUP_WORDS if k not in (opt, other)]:
            if getattr(self, "_" + o) is not None:
                raise RuntimeError(f"{who}: the group already carries {_GROUP_WORDS[o][0]} state (attach_{o})")
        if master_weights and self.dtype != torch.bfloat16:
            raise ValueError(f"{who}: master_weights=True is for bfloat16 groups; fp32 rows are their own masters")
        if self.dtype != torch.float32 and not master_weights:
            raise NotImplementedError(f"{who}: {needs_master}: pass master_weights=True (the fp32 fused kernel does "
                                      "not take bfloat16 rows)")
        if self.engine.comm is not None or self.engine.max_remote:
            raise NotImplementedError(f"{who}: one GPU only (nranks = 1, no transport): the partners' updated "
                                      "rows must exist before any exchange")
        if self._chunk_cols:
            raise NotImplementedError(f"{who}: not with chunk_cols (the column-pipelined cross-GPU exchange)")
        cls = FUSED_LAYOUTS[opt, bool(master_weights)]
        if cls.family.tile(self.n_local) <= 0 or self.engine.M > 32:
            raise NotImplementedError(f"{who}: {self.n_local} local rows / {self.engine.M} matchings exceed the "
                                      "fused kernel's 64 rows / 32 matchings")
        return who, cls, clip

    def _state_arena(self, dtype=torch.float32):
        return torch.zeros((self.n_local, self.ld), dtype=dtype, device="cuda")

    def _attach_fused(self, checked, param_groups, state, bias, hyper, call_args, mixed_row=None):
        """What attach_sgd / attach_adamw build alike once their own hyperparameters are checked (`checked`
        is what _fused_family returned): the gradient arena, the masters of a mixed-precision group, the
        layout over them and the optimizer's `state` arenas ({table name: arena or None}), the parameter
        groups, the call record (layout.call(engine, *call_args)), the adopted parameters' .grad views,
        lr_dev and the clip state.  Returns the FusedState for _sgd / _adamw.  mixed_row: the arena in the `x`
        table's place where the launch mixes something other than the group's rows (attach_gt's tracker)."""
        who, cls, clip = checked
        fam = cls.family
        self.grad_arena = torch.zeros((self.n_local, self.ld), dtype=self.dtype, device="cuda")
        self.grads = self.grad_arena[:, :self.numel]
        self.master_arena = self.master_rows = None
        # x: the fp32 group's rows, their own masters; w / p: a bfloat16 group's fp32 masters and its rows
        arenas = dict(state, g=self.grad_arena, x=self.arena if mixed_row is None else mixed_row, p=self.arena)
        if "w" in fam.tables:
            self.master_arena = self.arena.to(torch.float32)          # the exact widening, tails (zeros) included
            self.master_rows = self.master_arena[:, :self.numel]
            arenas["w"] = self.master_arena
        tables = [arenas[t] for t in fam.tables]
        tables = [None if a is None else [[a[r].data_ptr()] for r in range(self.n_local)] for a in tables]
        lay = cls([self.numel], *tables, self.n_local, *([bias] if fam.adam else []))
        self._attach_groups(param_groups, hyper["weight_decay"], who)
        call = lay.call(self.engine, *call_args)
        if self._adopted is not None:
            for r, m in enumerate(self._adopted):
                off = 0
                for p in _params(m):
                    k = p.numel()
                    p.grad = self.grad_arena[r, off:off + k].view(p.shape)
                    off += k
        self.lr_dev = torch.zeros(1, dtype=torch.float32, device="cuda")   # the device rounds' learning rate
        if self.param_runs is not None:      # groups are hyperparameters too; without them the dict is as before
            hyper["param_groups"] = self.param_runs
        self._attach_clip(lay, clip)
        return FusedState(lay, call, ctypes.addressof(call), *fam)

    def _fused_step(self, st, it, lr, stream):
        """sgd_step / adamw_step: the norm launches of a clipping group, then ONE fused launch through the
        entry point of the group's mode -- parameter groups (_grouped, with the clip factors or NULL),
        else clipping (_scaled), else the plain one.  The mode is read at call time."""
        it = self.engine.round_index(it)
        s = stream_ptr(stream)
        args = (it, self.opt_step + 1, lr, None, s) if st.adam else (it, lr, None, s)
        clip = self._clip
        if self._runs is not None:               # per-group decay / lr scale (with the clip factors, if any)
            if clip is not None:
                clip.enqueue(s)
            rc = st.grouped(st.addr, self._runs.addr, clip.scale_ptr if clip is not None else None, *args)
        elif clip is not None:                   # the norm launches, then the launch that applies the factors
            clip.enqueue(s)
            rc = st.scaled(st.addr, clip.scale_ptr, *args)
        else:
            rc = st.run(st.addr, *args)
        if rc:
            check(rc, st.base)
        if st.adam:
            self.opt_step += 1
        return bool(self.engine.any_active[it])

    def _fused_device_round(self, st, stream):
        """sgd_device_round / adamw_device_round: _fused_step's three modes through the _at entry points,
        then the counters' advance."""
        s = stream_ptr(stream)
        it = self.iter_dev.data_ptr()
        lr = self.lr_dev.data_ptr()
        args = (it, self.engine.T, self.opt_step_dev.data_ptr(), 0.0, lr, s) if st.adam else \
               (it, self.engine.T, 0.0, lr, s)
        clip = self._clip
        if self._runs is not None:
            if clip is not None:
                clip.enqueue(s)
            check(st.grouped_at(st.addr, self._runs.addr, clip.scale_ptr if clip is not None else None, *args),
                  st.base + "_grouped_at")
        elif clip is not None:
            clip.enqueue(s)
            check(st.scaled_at(st.addr, clip.scale_ptr, *args), st.base + "_scaled_at")
        else:
            check(st.run_at(st.addr, *args), st.base + "_at")
        check(lib.mx_iter_advance(it, 1, s), "mx_iter_advance")
        if st.adam:
            check(lib.mx_iter_advance(self.opt_step_dev.data_ptr(), 1, s), "mx_iter_advance")

    def _fused_communicate(self, step, lr):
        it = self.iter
        self.iter += 1
        torch.cuda.synchronize()
        tic = time.time()
        step(it, lr)
        self.wait_round()
        return time.time() - tic

    def attach_sgd(self, momentum=0.0, weight_decay=0.0, nesterov=False, zero_grads=True, master_weights=False,
                   clip_grad_norm=None, param_groups=None):
        """Give the group torch.optim.SGD's state (dampening 0) so that one launch per iteration
        applies every worker's update and the round's mix (csrc/sgd_mix.hip; the reference's
        optimizer.step() + zero_grad() + communicate(), train_mpi.py:131-142).

        Allocates `grad_arena` ([n_local, ld] fp32 zeros; `grads` is its [:, :numel] view) and, with
        momentum, `mom_arena` / `momentum_rows`.  For adopted models every parameter's .grad becomes
        the matching view of the gradient arena, so backward() accumulates in place.
        zero_grads=True (default) has the launch zero the gradients it consumed, which makes
        optimizer.zero_grad() unnecessary -- and zero_grad(set_to_none=True), torch's default,
        would DETACH those views (later gradients would land in fresh tensors the kernel never
        reads): do not call it on an attached group, or pass set_to_none=False.
        One GPU only: every partner's updated row must exist before any exchange, so a cross-GPU
        group is a different design.

        master_weights=True is the bfloat16 group's form (csrc/sgd_mix_bf16.hip; a ValueError on an
        fp32 group, and a bfloat16 group refuses to attach without it): `master_arena` /
        `master_rows` hold an fp32 master of every row, starting as the exact widening of `rows`;
        the gradient arena is bfloat16 (each adopted parameter's .grad a bf16 view of it), the
        momentum arena fp32.  The launch updates and mixes the MASTERS and rewrites `rows` as
        bf16(master), rounded once to nearest even, so updates below half a bf16 ulp accumulate
        instead of rounding away.  `rows` is write-only to the launch: anything written to `rows`
        directly (sync_rows, a checkpoint without masters) is overwritten by bf16(master) at the
        next step unless master_from_rows() is called after it.

        clip_grad_norm=X (a positive finite float; anything else but None is a ValueError) is
        torch.nn.utils.clip_grad_norm_(model.parameters(), X) -- 2-norm, error_if_nonfinite=False --
        per worker, without its passes over the gradients: every step first enqueues the norm
        launches (csrc/grad_norm.hip: one read of the gradient arena), then the fused launch with
        each row's factor multiplied into its gradient on the way into the update.  `grad_norms`
        (fp32 CUDA [n_local]) holds the norms BEFORE clipping -- what torch's function returns -- and
        `grad_scales` the factors, after every step and after grad_norm().  Unlike torch, the gradients
        in memory are never rewritten scaled: they are zeroed under zero_grads and otherwise left as
        backward wrote them.  Clipping has no state: checkpoints are unchanged and load either way.

        param_groups=[{...}, ...] is torch.optim's param_groups for the two hyperparameters recipes
        vary per parameter: every group selects parameters ("params": names of
        models[0].named_parameters(), or a predicate fn(name, param) -> bool) or columns ("columns":
        half-open ranges, the only selector of a numel-only group) and gives them their own
        "weight_decay" (default: this call's) and / or "lr_scale" (default 1.0: the step's learning
        rate is multiplied by it, one fp32 rounding).  Columns no group selects take this call's
        values.  See param_runs for the errors.  The groups are resolved once to column runs
        (`param_runs`: [(start, end, weight_decay, lr_scale)]) whose tables live on the device, and
        every step then goes through the _grouped entry points; None keeps today's launches.  Groups
        are hyperparameters, not state: checkpoints are unchanged.  Momentum, nesterov and the clip
        norm (one per worker over all its groups) are the whole row's."""
        checked = self._fused_family("sgd", master_weights, clip_grad_norm)
        momentum, weight_decay = float(momentum), float(weight_decay)
        if nesterov and momentum == 0.0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.mom_arena = self.momentum_rows = None
        if momentum != 0.0:
            self.mom_arena = self._state_arena()
            self.momentum_rows = self.mom_arena[:, :self.numel]
        self.sgd_hyper = {"momentum": momentum, "weight_decay": weight_decay, "nesterov": bool(nesterov),
                          "zero_grads": bool(zero_grads)}
        self._sgd = self._attach_fused(checked, param_groups, {"m": self.mom_arena}, None, self.sgd_hyper,
                                       (weight_decay, momentum, nesterov, zero_grads))

    def master_from_rows(self):
        """Redo the masters as the exact widening of `rows` (attach_sgd / attach_adamw(master_weights=True) groups).
        Call it after anything that writes `rows` directly -- sync_rows, loading a checkpoint that
        has no masters: the launch never reads `rows`, so such a write is otherwise overwritten by
        bf16(master) at the next step."""
        if self.master_rows is None:
            raise MXError("master_from_rows: no master weights (attach_sgd(master_weights=True) or "
                          "attach_adamw(master_weights=True) on a bfloat16 group)")
        with torch.no_grad():
            self.master_rows.copy_(self.rows)

    def _sgd_state(self):
        return _attached(self._sgd, "sgd").addr

    def sgd_step(self, it, lr, stream=None):
        """Enqueue ONE launch: every local worker's SGD update at learning rate `lr`, then round
        `it`'s mix of the updated rows.  Always launches -- an all-zero round is the SGD step
        alone -- and returns whether the round mixed."""
        return self._fused_step(_attached(self._sgd, "sgd"), it, lr, stream)

    def sgd_device_round(self, stream=None):
        """Graph-replayable sgd_step: the round is read from `self.iter_dev` and the learning rate
        from `self.lr_dev` (a 1-element fp32 CUDA tensor) when the kernel runs, then the counter is
        advanced, so one captured launch pair serves every iteration and every learning rate.  A
        counter outside the schedule makes the launch a no-op: no SGD step either."""
        self._fused_device_round(_attached(self._sgd, "sgd"), stream)

    def sgd_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker at the group's own
        iteration counter, as one launch; returns seconds like communicate()."""
        return self._fused_communicate(self.sgd_step, lr)

    # ------------------------------------------------------------------ fused AdamW + mixing
    def attach_adamw(self, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True, zero_grads=True,
                     master_weights=False, clip_grad_norm=None, param_groups=None):
        """Give the group torch.optim.AdamW's state (decoupled=False: torch.optim.Adam's, the decay as
        an L2 term in the gradient; no amsgrad, no maximize) so that one launch per iteration applies
        every worker's update and the round's mix (csrc/adamw_mix.hip).

        Allocates `grad_arena` / `grads` as attach_sgd does (adopted parameters' .grad become views
        of it; see attach_sgd on zero_grad), `exp_avg_arena` / `exp_avg_rows` and `exp_avg_sq_arena`
        / `exp_avg_sq_rows` (fp32 zeros), and the bias-correction table (adam_bias_table) on the
        device.  `opt_step` counts the optimizer steps taken (adamw_step runs step opt_step + 1);
        `opt_step_dev` (int64 CUDA) is the NEXT step of adamw_device_round, and `lr_dev` its
        learning rate.  One GPU only.

        master_weights=True is the bfloat16 group's form (csrc/adamw_mix_bf16.hip; a ValueError on an
        fp32 group, and a bfloat16 group refuses to attach without it), as attach_sgd's: `master_arena`
        / `master_rows` hold an fp32 master of every row, starting as the exact widening of `rows`;
        the gradient arena is bfloat16 (each adopted parameter's .grad a bf16 view of it), exp_avg
        and exp_avg_sq stay fp32.  The launch updates and mixes the MASTERS and rewrites `rows` as
        bf16(master), rounded once to nearest even.  `rows` is write-only to the launch: call
        master_from_rows() after anything that writes `rows` directly.

        clip_grad_norm=X is attach_sgd's: torch.nn.utils.clip_grad_norm_(model.parameters(), X) per
        worker as one extra read of the gradient arena; exp_avg and exp_avg_sq see the clipped
        gradient, `grad_norms` / `grad_scales` hold the pre-clip norms and the factors, and the
        gradients in memory are never rewritten scaled.

        param_groups=[{...}, ...] is attach_sgd's: per-group "weight_decay" (default: this call's) and
        "lr_scale" over parameters selected by name, by predicate or by column range -- the usual
        "no decay for biases and normalisation scales" is
        [{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}].  Betas and eps are the whole
        row's.  `param_runs` holds the resolved runs; None keeps today's launches."""
        checked = self._fused_family("adamw", master_weights, clip_grad_norm)
        betas = (float(betas[0]), float(betas[1]))
        eps, weight_decay = float(eps), float(weight_decay)
        if eps < 0.0 or weight_decay < 0.0:
            raise ValueError("attach_adamw: eps and weight_decay must not be negative")
        bias = adam_bias_table(*betas)                               # ValueError for betas it cannot serve
        self.exp_avg_arena, self.exp_avg_sq_arena = self._state_arena(), self._state_arena()
        self.exp_avg_rows = self.exp_avg_arena[:, :self.numel]
        self.exp_avg_sq_rows = self.exp_avg_sq_arena[:, :self.numel]
        self.adamw_hyper = {"betas": betas, "eps": eps, "weight_decay": weight_decay, "decoupled": bool(decoupled),
                            "zero_grads": bool(zero_grads)}
        state = self._attach_fused(checked, param_groups, {"m": self.exp_avg_arena, "v": self.exp_avg_sq_arena},
                                   bias, self.adamw_hyper, (betas, eps, weight_decay, decoupled, zero_grads))
        self.opt_step = 0
        self.opt_step_dev = torch.ones(1, dtype=torch.int64, device="cuda")
        self._adamw = state

    def _adamw_state(self):
        return _attached(self._adamw, "adamw").addr

    def adamw_step(self, it, lr, stream=None):
        """Enqueue ONE launch: every local worker's AdamW update number opt_step + 1 at learning rate
        `lr`, then round `it`'s mix of the updated rows; opt_step += 1.  Always launches -- an
        all-zero round is the optimizer step alone -- and returns whether the round mixed."""
        return self._fused_step(_attached(self._adamw, "adamw"), it, lr, stream)

    def adamw_device_round(self, stream=None):
        """Graph-replayable adamw_step: the round is read from `self.iter_dev`, the optimizer step from
        `self.opt_step_dev` and the learning rate from `self.lr_dev` when the kernel runs, then both
        counters are advanced (unconditionally, as sgd_device_round advances iter_dev), so one
        captured launch triple serves every iteration.  A round counter outside the schedule or a
        step below 1 makes the launch a no-op.  `self.opt_step` (adamw_step's host counter) is not
        touched."""
        self._fused_device_round(_attached(self._adamw, "adamw"), stream)

    def adamw_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker at the group's own
        iteration counter, as one launch; returns seconds like communicate()."""
        return self._fused_communicate(self.adamw_step, lr)

    # ------------------------------------------------------------------ fused Lion + mixing
    def attach_lion(self, betas=(0.9, 0.99), weight_decay=0.0, zero_grads=True, master_weights=False,
                    momentum_dtype=torch.float32, clip_grad_norm=None, param_groups=None):
        """Give the group Lion's state (Chen et al. 2023: the weights step by +-lr along the sign of
        (1 - beta1) g + beta1 m, the momentum follows (1 - beta2) g + beta2 m, the weight decay is
        decoupled as AdamW's) so that one launch per iteration applies every worker's update and the
        round's mix (csrc/lion_mix.hip).  Lion keeps ONE state array and has no step counter: it moves
        the bytes of SGD with momentum.

        Allocates `grad_arena` / `grads` as attach_sgd does (adopted parameters' .grad become views of
        it; see attach_sgd on zero_grad) and `lion_exp_avg_arena` / `lion_exp_avg_rows` (zeros).  One
        GPU only.

        master_weights=True is the bfloat16 group's form (csrc/lion_mix_bf16.hip; a ValueError on an
        fp32 group, and a bfloat16 group refuses to attach without it), as attach_sgd's: `master_arena`
        / `master_rows` hold an fp32 master of every row, the gradient arena is bfloat16, and the launch
        updates and mixes the MASTERS and rewrites `rows` as bf16(master).  momentum_dtype=torch.bfloat16
        (mixed-precision groups only) keeps the momentum in bfloat16 as well: it is widened exactly for
        the update and rounded to nearest even once at the store, which takes the round from 22 to 18
        bytes per parameter and the state from 12 to 10 bytes per parameter and worker.  It is a
        different optimizer from the fp32-momentum one by design: its checkpoints load only into groups
        of the same momentum dtype.

        clip_grad_norm and param_groups are attach_sgd's (the momentum sees the clipped gradient; a
        group's "lr_scale" scales the +-lr step, its "weight_decay" the decoupled decay)."""
        checked = self._fused_family("lion", master_weights, clip_grad_norm)
        betas, weight_decay, m_bf16 = lion_arguments(betas, weight_decay, momentum_dtype, master_weights)
        self.lion_exp_avg_arena = self._state_arena(momentum_dtype)
        self.lion_exp_avg_rows = self.lion_exp_avg_arena[:, :self.numel]
        self.lion_hyper = {"betas": betas, "weight_decay": weight_decay, "zero_grads": bool(zero_grads),
                           "momentum_dtype": momentum_dtype}
        call_args = (betas, weight_decay, zero_grads) + ((m_bf16,) if master_weights else ())
        self._lion = self._attach_fused(checked, param_groups, {"m": self.lion_exp_avg_arena}, None, self.lion_hyper,
                                        call_args)

    def lion_step(self, it, lr, stream=None):
        """Enqueue ONE launch: every local worker's Lion update at learning rate `lr`, then round `it`'s
        mix of the updated rows.  Always launches -- an all-zero round is the Lion step alone -- and
        returns whether the round mixed."""
        return self._fused_step(_attached(self._lion, "lion"), it, lr, stream)

    def lion_device_round(self, stream=None):
        """Graph-replayable lion_step, as sgd_device_round: the round is read from `self.iter_dev` and the
        learning rate from `self.lr_dev` when the kernel runs, then the counter is advanced.  A counter
        outside the schedule makes the launch a no-op: no Lion step either."""
        self._fused_device_round(_attached(self._lion, "lion"), stream)

    def lion_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker at the group's own
        iteration counter, as one launch; returns seconds like communicate()."""
        return self._fused_communicate(self.lion_step, lr)

    # ------------------------------------------------------------------ fused quasi-global momentum + mixing
    def attach_qgm(self, momentum=0.9, mu=None, weight_decay=0.0, nesterov=False, zero_grads=True,
                   master_weights=False, clip_grad_norm=None, param_groups=None):
        """Give the group quasi-global momentum (QG-DSGDm: Lin et al., ICML 2021): SGD with momentum whose
        buffer is fed by the displacement of the worker's row AFTER the gossip round, (x_t - x_{t+1}) / lr,
        not by its own gradient, so that it follows the direction the neighbourhood actually moved and
        heterogeneous shards stop pulling the workers apart between rounds.  One launch per iteration
        applies every worker's local step (momentum `momentum`, optionally Nesterov, L2 weight decay as
        SGD's), the round's mix and the buffer update mh' = mu * mh + (1 - mu) * (x_t - x_{t+1}) / lr
        (csrc/qgm_mix.hip); mu=None is mu = momentum, the paper's setting.  It moves the bytes of SGD with
        momentum and needs no extra communication.

        Allocates `grad_arena` / `grads` as attach_sgd does (adopted parameters' .grad become views of it;
        see attach_sgd on zero_grad) and `qgm_buffer_arena` / `qgm_buffer_rows` (fp32 zeros).  A step at
        lr = 0, and a parameter group of lr_scale 0, leave the buffer as it is.  One GPU only.

        master_weights=True is the bfloat16 group's form (csrc/qgm_mix_bf16.hip; a ValueError on an fp32
        group, and a bfloat16 group refuses to attach without it), as attach_sgd's: `master_arena` /
        `master_rows` hold an fp32 master of every row, the gradient arena is bfloat16, the buffer stays
        fp32, and the launch updates and mixes the MASTERS, takes the displacement from them and rewrites
        `rows` as bf16(master).

        clip_grad_norm and param_groups are attach_sgd's (the local momentum sees the clipped gradient; a
        group's "lr_scale" scales the step and the 1 / lr of the buffer update alike, its "weight_decay"
        the L2 term)."""
        checked = self._fused_family("qgm", master_weights, clip_grad_norm)
        momentum, mu, weight_decay = qgm_arguments(momentum, mu, weight_decay)
        self.qgm_buffer_arena = self._state_arena()
        self.qgm_buffer_rows = self.qgm_buffer_arena[:, :self.numel]
        self.qgm_hyper = {"momentum": momentum, "mu": mu, "weight_decay": weight_decay, "nesterov": bool(nesterov),
                          "zero_grads": bool(zero_grads)}
        self._qgm = self._attach_fused(checked, param_groups, {"m": self.qgm_buffer_arena}, None, self.qgm_hyper,
                                       (momentum, mu, weight_decay, nesterov, zero_grads))

    def qgm_step(self, it, lr, stream=None):
        """Enqueue ONE launch: every local worker's step at learning rate `lr`, round `it`'s mix of the
        updated rows and the buffer update from the rows' displacement.  Always launches -- an all-zero
        round is the local step plus the buffer update -- and returns whether the round mixed."""
        return self._fused_step(_attached(self._qgm, "qgm"), it, lr, stream)

    def qgm_device_round(self, stream=None):
        """Graph-replayable qgm_step, as sgd_device_round: the round is read from `self.iter_dev` and the
        learning rate from `self.lr_dev` when the kernel runs, then the counter is advanced.  A counter
        outside the schedule makes the launch a no-op: no step, and the buffer is not written."""
        self._fused_device_round(_attached(self._qgm, "qgm"), stream)

    def qgm_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker at the group's own
        iteration counter, as one launch; returns seconds like communicate()."""
        return self._fused_communicate(self.qgm_step, lr)

    # ------------------------------------------------------------------ gradient tracking: track + step launches
    def attach_gt(self, momentum=0.0, weight_decay=0.0, nesterov=False, zero_grads=True, master_weights=False,
                  clip_grad_norm=None, param_groups=None):
        """Give the group gradient tracking (GT-DSGD, also DIGing / DSGT: Di Lorenzo & Scutari 2016; Nedic,
        Olshevsky & Shi 2017; Pu & Nedic 2021): every worker keeps a tracker y of the network's mean gradient
        and steps along it instead of along its own gradient, which removes the stationary error
        (proportional to lr x gradient heterogeneity / spectral gap) that D-PSGD keeps at a constant learning
        rate on heterogeneous shards.  The trackers are gossiped with the round's own matrix, so an iteration
        is TWO launches on the same round: the track launch (csrc/gt_track.hip: y += g - g_prev, g_prev = g,
        the zeros over g, the round on y) and the step launch, torch.optim.SGD's update with y in the
        gradient's place and the round on the weights (for fp32 rows the fused SGD kernel itself over the
        tracker arena).  mean_i y_i equals mean_i g_i after every round of any MATCHA schedule.

        Allocates `grad_arena` / `grads` as attach_sgd does (adopted parameters' .grad become views of it; see
        attach_sgd on zero_grad), `gt_tracker_arena` / `gt_tracker_rows` and `gt_prev_grad_arena` /
        `gt_prev_grad_rows` (fp32 zeros: the first step's tracker is the gradient itself) and, with momentum,
        `mom_arena` / `momentum_rows`.  momentum, nesterov and weight_decay are attach_sgd's and act in the
        step launch: the weight decay is local (it is not part of the tracked gradient, so the track launch
        never reads the weights).  zero_grads is the track launch's.  One GPU only.

        master_weights=True is the bfloat16 group's form (csrc/gt_track_bf16.hip, csrc/gt_step_bf16.hip; a
        ValueError on an fp32 group, and a bfloat16 group refuses to attach without it), as attach_sgd's: the
        gradient arena is bfloat16, tracker, previous gradient, momentum and masters fp32, and the step launch
        rewrites `rows` as bf16(master).

        clip_grad_norm is attach_sgd's; the clip factor enters the tracked gradient (and `gt_prev_grad_rows`
        hold the clipped values), never the step.  param_groups are attach_sgd's and change only the step
        launch: a group of lr_scale 0 freezes its weights while its tracker still moves."""
        checked = self._fused_family("gt", master_weights, clip_grad_norm)
        momentum, weight_decay, nesterov = gt_arguments(momentum, weight_decay, nesterov)
        who, track_cls, clip = checked
        mixed = bool(master_weights)
        step_cls = FUSED_LAYOUTS["gt_step", mixed]
        self.gt_tracker_arena, self.gt_prev_grad_arena = self._state_arena(), self._state_arena()
        self.gt_tracker_rows = self.gt_tracker_arena[:, :self.numel]
        self.gt_prev_grad_rows = self.gt_prev_grad_arena[:, :self.numel]
        self.mom_arena = self.momentum_rows = None
        if momentum != 0.0:
            self.mom_arena = self._state_arena()
            self.momentum_rows = self.mom_arena[:, :self.numel]
        self.gt_hyper = {"momentum": momentum, "weight_decay": weight_decay, "nesterov": nesterov,
                         "zero_grads": bool(zero_grads)}
        # the track launch: _attach_fused with the tracker in the mixed row's place.  It also builds the
        # gradient arena, the masters of a mixed-precision group, the parameter runs, lr_dev and the clip state
        track = self._attach_fused(checked, param_groups, {"gp": self.gt_prev_grad_arena}, None, self.gt_hyper,
                                   (zero_grads,), mixed_row=self.gt_tracker_arena)
        if mixed:
            self.master_arena = self.arena.to(torch.float32)          # the exact widening, tails (zeros) included
            self.master_rows = self.master_arena[:, :self.numel]
        # the step launch: the SGD family's record with the tracker arena as its gradient table, no zeros over it
        arenas = {"x": self.arena, "w": self.master_arena, "g": self.gt_tracker_arena, "m": self.mom_arena,
                  "p": self.arena}
        tables = [arenas[t] for t in step_cls.family.tables]
        tables = [None if a is None else [[a[r].data_ptr()] for r in range(self.n_local)] for a in tables]
        lay = step_cls([self.numel], *tables, self.n_local)
        call = lay.call(self.engine, weight_decay, momentum, nesterov, *(() if mixed else (False,)))
        self._gt = GtState(track, FusedState(lay, call, ctypes.addressof(call), *step_cls.family))

    def gt_step(self, it, lr, stream=None):
        """Enqueue one gradient-tracking iteration at learning rate `lr` on round `it`: the norm launches of a
        clipping group, the track launch (through _scaled with the clip factors) and the step launch (through
        _grouped with parameter groups).  Always launches -- on an all-zero round the trackers take in the
        gradients' change and the weights step, unmixed -- and returns whether the round mixed."""
        gt = _attached(self._gt, "gt")
        it = self.engine.round_index(it)
        s = stream_ptr(stream)
        track, step = gt.track, gt.step
        clip = self._clip
        if clip is not None:
            clip.enqueue(s)
            rc = track.scaled(track.addr, clip.scale_ptr, it, lr, None, s)
        else:
            rc = track.run(track.addr, it, lr, None, s)
        if rc:
            check(rc, track.base)
        if self._runs is not None:
            rc = step.grouped(step.addr, self._runs.addr, None, it, lr, None, s)
        else:
            rc = step.run(step.addr, it, lr, None, s)
        if rc:
            check(rc, step.base)
        return bool(self.engine.any_active[it])

    def gt_device_round(self, stream=None):
        """Graph-replayable gt_step: both launches read the round from `self.iter_dev` (the SAME round) and the
        step launch the learning rate from `self.lr_dev` when the kernels run, then the counter is advanced
        once.  A counter outside the schedule makes both launches no-ops."""
        gt = _attached(self._gt, "gt")
        s = stream_ptr(stream)
        it = self.iter_dev.data_ptr()
        args = (it, self.engine.T, 0.0, self.lr_dev.data_ptr(), s)
        track, step = gt.track, gt.step
        clip = self._clip
        if clip is not None:
            clip.enqueue(s)
            check(track.scaled_at(track.addr, clip.scale_ptr, *args), track.base + "_scaled_at")
        else:
            check(track.run_at(track.addr, *args), track.base + "_at")
        if self._runs is not None:
            check(step.grouped_at(step.addr, self._runs.addr, None, *args), step.base + "_grouped_at")
        else:
            check(step.run_at(step.addr, *args), step.base + "_at")
        check(lib.mx_iter_advance(it, 1, s), "mx_iter_advance")

    def gt_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker under gradient tracking at the
        group's own iteration counter, as the launch pair; returns seconds like communicate()."""
        return self._fused_communicate(self.gt_step, lr)

    # ------------------------------------------------------------------ SlowMo: the outer step across iterations
    def attach_slowmo(self, beta=0.5, alpha=1.0, buffers="maintain", order=0):
        """Give the group SlowMo's outer step (Wang, Tantia, Ballas, Rabbat, ICLR 2020): every tau iterations
        of the base optimizer -- any attach_* family, or plain rounds -- slowmo_step(lr) replaces every
        worker's row by one common point in ONE launch (csrc/slowmo.hip): the exact average of the rows in
        mx_mean_rows' order `order` (0 the binomial tree, 1 rank order), then
            u' = beta * u + (a - mean) / lr;   a' = a - alpha * lr * u';   every row = a'
        with the contract's roundings (include/matcha_gossip.h).  beta = 0, alpha = 1 is the periodic exact
        average alone.  Call it AFTER the base optimizer's attach_*: the state arenas and the masters are
        resolved here, once.

        Allocates `slowmo_anchor` (a, the common point of the last outer step: a copy of local row 0, the
        master row where masters exist -- the workers are expected to be in sync, as the harness leaves them)
        and `slowmo_momentum` (u, zeros), fp32 [numel] views of ld-sized buffers, one pair per group, and
        `lr_dev` if no fused family has.  On a mixed-precision group the step averages and rewrites the fp32
        MASTERS and writes `rows` as bf16(master), so nothing has to be remembered afterwards; a bfloat16
        group without masters is refused.  Call slowmo_anchor_from_rows() after anything else that rewrites
        the rows (sync_rows, a checkpoint loaded by hand).

        buffers: what an outer step does to the base optimizer's momentum-like state -- SGD's and gradient
        tracking's momentum, AdamW's exp_avg and exp_avg_sq, Lion's exp_avg, QGM's buffer; gradient tracking's
        tracker and previous gradient are never touched.  "maintain" (default) leaves it alone; "reset" (the
        paper's choice) makes it that of a freshly attached optimizer: the arenas are zeroed on the stream and
        AdamW's step count restarts; "average" is mx_mean_rows_to in place on every fp32 arena, in the same
        order.  Anything but "maintain" needs an attached family, and "average" an fp32 state.

        For a local row count that is not a power of two (in rank order: above 2) the pinned-order mean of
        identical values can differ from the value in the last place, so a synced state is not an exact fixed
        point there.
        One GPU only: across GPUs the exact average is an all-reduce, another launch sequence."""
        who = "attach_slowmo"
        if not self._one_gpu or self.engine.max_remote:
            raise NotImplementedError(f"{who}: one GPU only (nranks = 1, no transport): the average needs every "
                                      "worker's row on this GPU")
        if self._slowmo is not None:
            raise RuntimeError(f"{who}: already attached")
        beta, alpha = float(beta), float(alpha)
        if not 0.0 <= float(np.float32(beta)) < 1.0:
            raise ValueError(f"{who}: beta={beta} outside [0, 1)")
        if not (math.isfinite(alpha) and 0.0 < float(np.float32(alpha)) < math.inf):
            raise ValueError(f"{who}: alpha={alpha} must be finite and > 0")
        if order not in (0, 1):
            raise ValueError(f"{who}: order is 0 (binomial tree) or 1 (rank order), not {order!r}")
        if buffers not in SLOWMO_BUFFERS:
            raise ValueError(f"{who}: buffers is one of {SLOWMO_BUFFERS}, not {buffers!r}")
        if self.n_local > 64:
            raise NotImplementedError(f"{who}: {self.n_local} local rows exceed the outer-step kernel's 64")
        mixed = self.dtype == torch.bfloat16
        if mixed and self.master_arena is None:
            raise ValueError(f"{who}: a bfloat16 group needs fp32 master weights for the outer step: attach an "
                             "optimizer with master_weights=True first")
        family = next((k for k in _SLOWMO_STATE if getattr(self, "_" + k) is not None), None)
        if family is None and buffers != "maintain":
            raise ValueError(f"{who}: buffers={buffers!r} acts on a fused optimizer's state and the group has "
                             "none attached: attach_sgd / attach_adamw / attach_lion / attach_qgm / attach_gt "
                             "first, or buffers='maintain'")
        arenas = [] if family is None else [getattr(self, name) for name in _SLOWMO_STATE[family]]
        arenas = [a for a in arenas if a is not None]                   # SGD without momentum has none
        if buffers == "average" and any(a.dtype != torch.float32 for a in arenas):
            raise ValueError(f"{who}: buffers='average' is mx_mean_rows_to on fp32 arenas; the bfloat16 Lion "
                             "momentum has no such mean: 'reset' or 'maintain'")
        self._slowmo_bufs = torch.zeros((2, self.ld), dtype=torch.float32, device="cuda")
        self.slowmo_anchor = self._slowmo_bufs[0, :self.numel]
        self.slowmo_momentum = self._slowmo_bufs[1, :self.numel]
        x = self.master_arena if mixed else self.arena
        call = SlowmoCall(x.data_ptr(), self._slowmo_bufs[0].data_ptr(), self._slowmo_bufs[1].data_ptr(),
                          self.arena.data_ptr() if mixed else None, self.ld, self.ld, self.numel, self.n_local,
                          int(order), alpha, beta)
        if self.lr_dev is None:
            self.lr_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
        self.slowmo_hyper = {"beta": beta, "alpha": alpha, "buffers": buffers, "order": int(order)}
        self._slowmo = SlowmoState(call, ctypes.addressof(call), buffers, arenas, family == "adamw", int(order))
        self.slowmo_anchor_from_rows()

    def _slowmo_state(self, who):
        if self._slowmo is None:
            raise MXError(f"{who}: no SlowMo state: call attach_slowmo() first")
        return self._slowmo

    def slowmo_anchor_from_rows(self):
        """Redo the anchor as a copy of local row 0 (the master row where masters exist), in the spirit of
        master_from_rows(): call it after anything but slowmo_step that rewrites the rows.  The slow momentum
        is left as it is."""
        self._slowmo_state("slowmo_anchor_from_rows")
        with torch.no_grad():
            self.slowmo_anchor.copy_((self.master_rows if self.master_rows is not None else self.rows)[0])

    def slowmo_kernel_name(self):
        """The kernel slowmo_step launches for this group (mx_slowmo_kernel_name), for reports."""
        return lib.mx_slowmo_kernel_name(self._slowmo_state("slowmo_kernel_name").addr).decode()

    def _slowmo_buffers(self, st, s, stream, host):
        """The buffer strategy's launches after the outer step, on the same stream; host: also restart
        AdamW's host step count (the eager form)."""
        if st.buffers == "maintain":
            return
        if st.buffers == "average":
            for a in st.arenas:
                check(lib.mx_mean_rows_to(a.data_ptr(), self.n_local, self.ld, self.numel, st.order, a.data_ptr(),
                                          self.n_local, self.ld, s), "mx_mean_rows_to")
            return
        with torch.no_grad(), (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            for a in st.arenas:
                a.zero_()
            if st.adam:
                self.opt_step_dev.fill_(1)
        if st.adam and host:
            self.opt_step = 0

    def slowmo_step(self, lr, stream=None):
        """Enqueue the outer step at the base optimizer's learning rate `lr` (finite and > 0): ONE launch,
        then the buffer strategy's launches (none for "maintain").  It does not advance `iter`: the next
        round is the schedule's next.  Afterwards every row equals `slowmo_anchor`."""
        st = self._slowmo_state("slowmo_step")
        lr = float(lr)
        if not (math.isfinite(lr) and 0.0 < float(np.float32(lr)) < math.inf):
            raise ValueError(f"slowmo_step: lr={lr} must be finite and > 0")
        s = stream_ptr(stream)
        rc = lib.mx_slowmo_step(st.addr, lr, None, s)
        if rc:
            check(rc, "mx_slowmo_step")
        self._slowmo_buffers(st, s, stream, True)

    def slowmo_device_step(self, stream=None):
        """Graph-replayable slowmo_step: the learning rate is read from `self.lr_dev` when the kernel runs, so
        one captured step serves every learning rate.  A learning rate of exactly 0 there makes the outer
        step's launch a complete no-op; the buffer strategy's launches run regardless.  With "reset" on an
        AdamW group `opt_step_dev` restarts and `opt_step`, the host counter, is not touched (as
        adamw_device_round leaves it)."""
        st = self._slowmo_state("slowmo_device_step")
        s = stream_ptr(stream)
        check(lib.mx_slowmo_step(st.addr, 0.0, self.lr_dev.data_ptr(), s), "mx_slowmo_step")
        self._slowmo_buffers(st, s, stream, False)

    def state_dict(self):
        """Checkpoint: the workers' rows and the iteration counter (resume on the same schedule);
        with attach_sgd(momentum != 0) the momentum rows too, with master_weights=True the fp32
        master rows, with attach_adamw the exp_avg / exp_avg_sq rows and the step count, and with
        attach_lion the lion_exp_avg rows (in the arena's dtype), with attach_qgm the qgm_buffer rows, with
        attach_gt the gt_tracker and gt_prev_grad rows (and the momentum rows), with attach_slowmo the anchor and
        the slow momentum."""
        state = {"kind": "decen", "iter": int(self.iter), "row_base": int(self.row_base),
                 "workers": list(self.workers), "rows": self.rows.detach().clone()}
        if (self._sgd is not None or self._gt is not None) and self.momentum_rows is not None:
            state["momentum_rows"] = self.momentum_rows.detach().clone()
        if self.master_rows is not None:
            state["master_rows"] = self.master_rows.detach().clone()
        if self._adamw is not None:
            state["exp_avg_rows"] = self.exp_avg_rows.detach().clone()
            state["exp_avg_sq_rows"] = self.exp_avg_sq_rows.detach().clone()
            state["opt_step"] = int(self.opt_step)
        if self._lion is not None:
            state["lion_exp_avg_rows"] = self.lion_exp_avg_rows.detach().clone()
        if self._qgm is not None:
            state["qgm_buffer_rows"] = self.qgm_buffer_rows.detach().clone()
        if self._gt is not None:
            state["gt_tracker_rows"] = self.gt_tracker_rows.detach().clone()
            state["gt_prev_grad_rows"] = self.gt_prev_grad_rows.detach().clone()
        if self._slowmo is not None:
            state["slowmo_anchor"] = self.slowmo_anchor.detach().clone()
            state["slowmo_momentum"] = self.slowmo_momentum.detach().clone()
        return state

    def load_state_dict(self, state):
        if state.get("kind") != "decen" or int(state["row_base"]) != self.row_base or \
                list(state.get("workers", self.workers)) != self.workers or \
                tuple(state["rows"].shape) != tuple(self.rows.shape):
            raise ValueError("checkpoint does not match this worker group")
        mom = state.get("momentum_rows")
        have = (self._sgd is not None or self._gt is not None) and self.momentum_rows is not None
        if mom is not None and (not have or tuple(mom.shape) != tuple(self.momentum_rows.shape)):
            raise ValueError("checkpoint carries momentum rows: attach_sgd(momentum=...) before loading it")
        master = state.get("master_rows")
        if master is not None and (self.master_rows is None or tuple(master.shape) != tuple(self.master_rows.shape)):
            raise ValueError("checkpoint carries master rows: attach_sgd(master_weights=True) before loading it "
                             "(or attach_adamw(master_weights=True))")
        adam = [state.get(k) for k in ("exp_avg_rows", "exp_avg_sq_rows")]
        if any(a is not None for a in adam) or state.get("opt_step") is not None:
            if self._adamw is None or any(a is None or tuple(a.shape) != tuple(self.rows.shape) for a in adam):
                raise ValueError("checkpoint carries Adam state (exp_avg rows): attach_adamw() before loading it")
        lion = state.get("lion_exp_avg_rows")
        if lion is not None and (self._lion is None or tuple(lion.shape) != tuple(self.lion_exp_avg_rows.shape)
                                 or lion.dtype != self.lion_exp_avg_rows.dtype):
            raise ValueError("checkpoint carries Lion state (lion_exp_avg rows): attach_lion() with the same "
                             "momentum_dtype before loading it")
        qgm = state.get("qgm_buffer_rows")
        if qgm is not None and (self._qgm is None or tuple(qgm.shape) != tuple(self.qgm_buffer_rows.shape)):
            raise ValueError("checkpoint carries quasi-global momentum state (qgm_buffer rows): attach_qgm() on a "
                             "group of the same shape before loading it")
        gt = [state.get(k) for k in ("gt_tracker_rows", "gt_prev_grad_rows")]
        if any(a is not None for a in gt):
            # the tracker is the running sum of the gradients' differences: without the gradient it last took in
            # (or the other way round) the next difference is wrong for ever
            if any(a is None for a in gt):
                raise ValueError("checkpoint carries half of the gradient-tracking state: gt_tracker_rows and "
                                 "gt_prev_grad_rows are only valid together")
            if self._gt is None or any(tuple(a.shape) != tuple(self.gt_tracker_rows.shape) for a in gt):
                raise ValueError("checkpoint carries gradient-tracking state (gt_tracker rows): attach_gt() on a "
                                 "group of the same shape before loading it")
        slow = [state.get(k) for k in ("slowmo_anchor", "slowmo_momentum")]
        if any(a is not None for a in slow):
            # the momentum is a displacement from the anchor it was taken at: either alone says nothing
            if any(a is None for a in slow):
                raise ValueError("checkpoint carries half of the SlowMo state: slowmo_anchor and slowmo_momentum "
                                 "are only valid together")
            if self._slowmo is None or any(tuple(a.shape) != tuple(self.slowmo_anchor.shape) for a in slow):
                raise ValueError("checkpoint carries SlowMo state (slowmo_anchor): attach_slowmo() on a group of "
                                 "the same shape before loading it")
        with torch.no_grad():
            self.rows.copy_(state["rows"])
            if self._gt is not None:             # a checkpoint without them: tracker and previous gradient zeros
                for rows, a in zip((self.gt_tracker_rows, self.gt_prev_grad_rows), gt):
                    rows.zero_() if a is None else rows.copy_(a)
            if self._qgm is not None:            # a checkpoint without them: the buffer starts as zeros
                self.qgm_buffer_rows.zero_() if qgm is None else self.qgm_buffer_rows.copy_(qgm)
            if self._lion is not None:           # a checkpoint without them: the buffer starts as zeros
                self.lion_exp_avg_rows.zero_() if lion is None else self.lion_exp_avg_rows.copy_(lion)
            if self._adamw is not None:          # a checkpoint without them: zero buffers, step 0
                for rows, a in zip((self.exp_avg_rows, self.exp_avg_sq_rows), adam):
                    rows.zero_() if a is None else rows.copy_(a)
                self.opt_step = int(state.get("opt_step") or 0)
                self.opt_step_dev.fill_(self.opt_step + 1)
            if have:                             # a checkpoint without them: the buffers start as zeros
                self.momentum_rows.zero_() if mom is None else self.momentum_rows.copy_(mom)
            if self.master_rows is not None:     # a checkpoint without them: the widened rows
                self.master_rows.copy_(self.rows if master is None else master)
            if self._slowmo is not None:         # a checkpoint without them: the anchor from row 0, zero momentum
                if slow[0] is None:
                    self.slowmo_anchor_from_rows()
                    self.slowmo_momentum.zero_()
                else:
                    self.slowmo_anchor.copy_(slow[0])
                    self.slowmo_momentum.copy_(slow[1])
        self.iter = int(state["iter"])

    def communicate(self):
        """One round at the group's own iteration counter; returns seconds like the reference's
        communicate() (0 for a skipped round)."""
        it = self.iter
        self.iter += 1
        if np.sum(self.topology.active_flags[it]) == 0:
            return 0
        torch.cuda.synchronize()
        tic = time.time()
        self.step(it)
        self.wait_round()
        return time.time() - tic
