"""ChocoSGD compressed gossip on the GPU (communicator.py:161-268, compressors.py:3-19).

ChocoWorkerGroup keeps, for a block of workers on this GPU, the parameter arena x and the
persistent Choco state x_hat and s (all [n_local, P] in HBM).  Per round:
    q_r = top-k(|x_r - x_hat_r|)            mx_topk_abs_diff   (prepare_comm_buffer, 175-196)
    [N > 1] RCCL exchange of the messages   mx_exchange_round  (12 k bytes per edge direction)
    s / x_hat updates + dense x update      mx_choco_apply     (averaging, 200-230; one fused pass)
With compressor="sign" the message is the scaled-sign (1-bit) quantizer Q(v) = (|v|_1 / P) sign(v) instead
(csrc/choco_sign.hip): q_r = (scale_r, one bit per column, set where x_r - x_hat_r < 0), P/8 bytes on the
wire; mx_choco_sign_compress and the elementwise mx_choco_sign_apply take the two kernels' places.  A 1-bit
message has no zero: a zero difference travels as +scale (torch.sign would give 0).
With compressor="quant" it is the bucketed stochastic quantizer at bits = 4 or 8 (csrc/choco_quant.hip: QSGD's
qsgd_s normalised per 256 columns): q_r = (one fp32 norm per bucket, one sign-and-level code per column), drawn
from a counter-based hash of (seed, round, worker, column); mx_choco_quant_compress is one launch with no
workspace, mx_choco_quant_apply the elementwise apply.  With one_launch=True (nranks = 1, at most 16 rows) both,
and the SGD step of attach_sgd(), are ONE launch that keeps the messages in LDS (csrc/choco_quant_round.hip:
mx_choco_quant_round / mx_choco_quant_sgd_round), with the same bits in x, x_hat and s.  That form alone also
serves models held in bfloat16 (dtype=torch.bfloat16, csrc/choco_quant_round_bf16.hip): x, x_hat, s and the
momentum stay fp32, the gradients come in as bfloat16 and the same launch rewrites the models as bf16_rne(x).
attach_adamw() puts torch.optim.AdamW's (or Adam's) step in front of that one launch instead of SGD's
(csrc/choco_quant_adamw_round.hip, csrc/choco_quant_adamw_round_bf16.hip: exp_avg and exp_avg_sq fp32).
With compressor="randk" the message is random sparsification (csrc/choco_randk.hip): top-k's k = topk_count(P, ratio)
columns and top-k's layout, but the columns are drawn from a counter-based hash of (seed, round, worker, column) and
never depend on the data; mx_choco_randk_compress is one launch that touches only the selected columns, with no
workspace and nothing for check_topk() to check, and every later step of the round is top-k's own.
Under PullTransport (N > 1, one process per GPU of a node) the messages are not sent: every rank
publishes the messages its peers read this round into its IPC-shared snapshot buffer
(mx_snapshot_publish_rows), the device
gate (mx_pull_gate) waits for the partners' epochs and points a device slot table at their
snapshots, mx_pull_fetch copies the round's partner messages from the owners' HBM into the receive
slots, and the apply pass runs as under RCCL (pull_read="fetch"; "direct": the apply reads them in
place, mx_choco_apply_slots) -- no host step per round, as VirtualWorkerGroup's pull round
(engine.PullTransport).
"""
import time

import numpy as np
import torch

from ._lib import MXError, check, lib, require_device, stream_ptr
from .engine import (PULL_HEADER, Consensus, GossipEngine, PullTransport, ROW_ALIGN, default_comm, owner_table,
                     partition, wait_round)


def topk_count(P, ratio):
    """compressors.py:11 -- k = max(1, int(len * (1 - ratio)))."""
    return max(1, int(P * (1 - ratio)))


COMPRESSORS = ("topk", "sign", "quant", "randk")


class ChocoWorkerGroup:
    def __init__(self, topology, models=None, numel=None, *, ratio=None, consensus_lr, rank=0, nranks=1,
                 comm=None, adopt=True, placement=None, pull_read="fetch", dtype=torch.float32,
                 compressor="topk", bits=None, seed=0, one_launch=False):
        """compressor: "topk" (compressors.get_top_k; `ratio` required), "sign" (the scaled-sign
        quantizer), "quant" (the bucketed stochastic quantizer: `bits` 4 or 8, default 8; `seed` of its
        counter-based random numbers) or "randk" (random sparsification: `ratio` required, k and the message
        layout as top-k's, the columns drawn from `seed`, the round and the worker); "sign" and "quant" take no
        `ratio` and have k = 0; only "topk" has something for check_topk() to check, and PullTransport is built
        for "topk" alone.
        one_launch (compressor="quant", nranks = 1, at most 16 rows): a round, and with attach_sgd() the SGD
        step in front of it, is ONE launch (csrc/choco_quant_round.hip) that keeps the messages on chip --
        the same bits in x, x_hat and s as the two launches; there are no message slots, so message(),
        compress() and average() raise, and `round_norms` ([n_local, ceil(P/256)] fp32) holds the last
        round's bucket norms.
        dtype=torch.bfloat16 (that one_launch form only; everything else raises NotImplementedError): the
        models are bfloat16 and adopt a bfloat16 arena, `rows` is its [:, :numel] view, every launch rewrites it as
        the rounded image of `x`; `x` (fp32, `master_rows` is its [:, :numel] view -- None on an fp32 group) starts
        as the models' exact widening and is what the round updates; attach_sgd's gradient arena is bfloat16, its
        momentum fp32; master_from_rows() re-widens after the models were written from outside.
        placement: as VirtualWorkerGroup (None / "contiguous", "auto" or a worker order);
        `workers` lists the worker id of each local row.  pull_read (PullTransport only): "fetch"
        (default) copies the round's partner messages from their owners' snapshots into the receive
        slots (mx_pull_fetch) before the apply; "direct" lets the apply read them in place
        (mx_choco_apply_slots: no copy, but a system-scope acquire per apply workgroup and a table
        load per message).  Same bits; which is faster across GPUs is measured by bench.py."""
        if pull_read not in ("fetch", "direct"):
            raise ValueError("pull_read must be 'fetch' or 'direct'")
        if compressor not in COMPRESSORS:
            raise ValueError(f"compressor must be one of {COMPRESSORS}, not {compressor!r}")
        if compressor in ("topk", "randk") and ratio is None:
            raise ValueError(f"ChocoWorkerGroup: compressor={compressor!r} needs a ratio")
        if compressor not in ("topk", "randk") and ratio is not None:
            raise ValueError(f"ChocoWorkerGroup: compressor={compressor!r} takes no ratio")
        if compressor != "topk" and isinstance(comm, PullTransport):
            raise NotImplementedError(f"ChocoWorkerGroup: compressor={compressor!r} under PullTransport -- the "
                                      "publish / gate / fetch sizing of its messages is not built")
        if bits is not None and compressor != "quant":
            raise ValueError(f"ChocoWorkerGroup: bits belongs to compressor='quant', not {compressor!r}")
        if compressor == "quant" and (8 if bits is None else bits) not in (4, 8):
            raise ValueError(f"ChocoWorkerGroup: compressor='quant' has bits 4 or 8, not {bits!r}")
        if one_launch and compressor != "quant":
            raise ValueError(f"ChocoWorkerGroup: one_launch belongs to compressor='quant', not {compressor!r} "
                             "(a top-k threshold and a sign scale are row-wide)")
        if dtype != torch.float32 and (dtype != torch.bfloat16 or compressor != "quant" or not one_launch or
                                       nranks > 1 or comm is not None):
            raise NotImplementedError(f"ChocoWorkerGroup: {dtype} rows -- the top-k, sign and two-launch quant kernels "
                                      "and every transport are fp32-only; bfloat16 models take compressor='quant', "
                                      "one_launch=True with nranks = 1 (csrc/choco_quant_round_bf16.hip)")
        if one_launch and (nranks > 1 or comm is not None):
            raise NotImplementedError("ChocoWorkerGroup: one_launch needs every worker's row on this GPU (nranks = 1, "
                                      "no transport); use the two-launch path (one_launch=False)")
        self.one_launch = bool(one_launch)
        self.compressor = compressor
        self.sign = compressor == "sign"
        self.quant = compressor == "quant"
        self.randk = compressor == "randk"
        self.bits = (8 if bits is None else int(bits)) if self.quant else None
        self.seed = int(seed)
        self.pull_read = pull_read
        self.dtype = dtype
        require_device()
        from .placement import block_workers, place
        n = int(topology.size)
        topology, self.placement = place(topology, nranks, placement)
        self.row_base, self.n_local = partition(n, nranks)[rank]
        self.workers = block_workers(self.placement, self.row_base, self.n_local)
        if one_launch and self.n_local > 16:
            raise NotImplementedError(f"ChocoWorkerGroup: one_launch holds a tile of at most 16 rows on chip, not "
                                      f"{self.n_local}; use the two-launch path (one_launch=False)")
        if nranks > 1 and comm is None:
            comm = default_comm()
        self.engine = GossipEngine(topology, self.row_base, self.n_local, comm=comm,
                                   owner=owner_table(n, nranks))
        self.topology = topology
        self.ratio = ratio
        self.consensus_lr = consensus_lr
        self.iter = 0
        if models is not None:
            if len(models) != self.n_local:
                raise ValueError(f"{len(models)} models for {self.n_local} local workers")
            self.numel = int(sum(p.numel() for p in models[0].parameters()))
        else:
            self.numel = int(numel)
        # attach_sgd: the models whose parameters are views of `x` (their .grad become views of the gradient arena)
        self._adopted = list(models) if models is not None and adopt else None
        self._copied_models = models is not None and not adopt
        self._sgd = None                     # attach_sgd's hyperparameters
        self._adamw = None                   # attach_adamw's, in the entry points' order
        self._iters = None                   # a one-launch step on an inactive round: 0 .. T on the device
        self.grad_arena = self.grads = self.mom_arena = self.momentum_rows = self.lr_dev = None
        self.exp_avg_arena = self.exp_avg_sq_arena = self.exp_avg_rows = self.exp_avg_sq_rows = None
        self.opt_step = self.opt_step_dev = None
        P = self.numel
        self.ld = (P + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
        self.x = torch.zeros((self.n_local, self.ld), dtype=torch.float32, device="cuda")
        self.x_hat = torch.zeros_like(self.x)     # communicator.py:179-182 (lazy zeros)
        self.s = torch.zeros_like(self.x)
        # bfloat16 models: their arena, the image of x that every launch rewrites; x is the fp32 master
        self.arena = self.x if dtype == torch.float32 else torch.zeros_like(self.x, dtype=dtype)
        if models is not None:
            for r, m in enumerate(models):
                off = 0
                for p in m.parameters():
                    if p.dtype != dtype or p.device.type != "cuda":
                        raise TypeError(f"worker parameters must be {dtype} CUDA tensors")
                    k = p.numel()
                    view = self.arena[r, off:off + k].view(p.shape)
                    view.copy_(p.data)
                    if adopt:
                        p.data = view
                    off += k
            self.master_from_rows()
        if self.quant:
            # header 64 | norm f32[ceil(P/256)] padded to 64 | codes uint8[32 bits ceil(P/256)]; no workspace
            self.k = self.kpad = self.work_ld = 0
            self.msg_bytes = int(lib.mx_choco_quant_msg_bytes(P, self.bits))
            self.codes_off = 64 + 64 * ((P + 4095) // 4096)
        elif self.sign:
            # scale f32 | L f64 | P int64 | zeros to 64 | bits uint8[8 ceil(P/64)] (mx_choco_sign_compress)
            self.k = self.kpad = 0
            self.msg_bytes = int(lib.mx_choco_sign_msg_bytes(P))
            self.work_ld = int(lib.mx_choco_sign_work_bytes(P, 1))
        else:
            self.k = topk_count(P, ratio)
            self.kpad = (self.k + 1) // 2 * 2
            # vals f32[kpad] | idx int64[k] | tile bounds int32[ceil(P/4096) + 1] (written by the top-k)
            self.msg_bytes = int(lib.mx_choco_msg_bytes(P, self.k))
            self.bnd_off = 4 * self.kpad + 8 * self.k
            self.work_ld = 0 if self.randk else int(lib.mx_topk_work_bytes(P))    # rand-k selects without scratch
        self.msg_ld = (self.msg_bytes + 255) // 256 * 256
        self.round_norms = None
        if self.one_launch:                  # no message slots: the norms are all of a message that reaches memory
            self.round_norms = torch.zeros((self.n_local, (P + 255) // 256), dtype=torch.float32, device="cuda")
        self.msgs = torch.empty(0 if self.one_launch else self.engine.n_slots * self.msg_ld, dtype=torch.uint8,
                                device="cuda")
        self.work = torch.zeros(self.n_local * self.work_ld, dtype=torch.uint8, device="cuda")  # zero on first use
        self.apply_work = torch.empty(0 if self.k == 0 else int(lib.mx_choco_apply_work_bytes(P, self.engine.n_slots)),
                                      dtype=torch.uint8, device="cuda")
        self.gamma32 = float(np.float32(consensus_lr))
        self.iter_dev = torch.zeros(1, dtype=torch.int64, device="cuda")   # device_round's counter
        self._pull = None
        self._consensus = None               # consensus_distance(): built on first use
        self.consensus_dists = self.consensus_stats = None
        self._one_gpu = nranks == 1 and comm is None
        if isinstance(comm, PullTransport):
            # each rank's snapshot buffer holds two generations of its rows' messages; the gate
            # points the remote entries of the slot table at the round's partners' snapshots
            # (placeholder: this rank's own snapshot 0).  "fetch": mx_pull_fetch copies them into
            # the receive slots and the apply reads local memory only; "direct": the apply reads
            # every slot through the table, acquiring at system scope first (peer-reads bit)
            self._pull = comm.bind(self, row_bytes=self.msg_ld)
            ptrs = [self.msgs.data_ptr() + r * self.msg_ld for r in range(self.n_local)]
            ptrs += [self._pull.own + PULL_HEADER] * (self.engine.n_slots - self.n_local)
            self.slot_ptrs = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
            if pull_read == "direct":
                check(lib.mx_plan_set_peer_reads(self.engine.plan.data_ptr(), self.engine.T + 1, self.n_local,
                                                 self.engine.M, 1, stream_ptr()), "mx_plan_set_peer_reads")
                self.engine.peer_reads = True

    @property
    def rows(self):
        """The models' rows: `x` itself, or on a bfloat16 group its bfloat16 image."""
        return self.arena[:, :self.numel]

    @property
    def master_rows(self):
        """The fp32 rows the round updates under bfloat16 models (`x`); None on an fp32 group."""
        return self.x[:, :self.numel] if self.dtype == torch.bfloat16 else None

    def master_from_rows(self):
        """x = f32(rows), the exact widening: after the models were written from outside.  Nothing on an fp32 group."""
        if self.arena is not self.x:
            self.x.copy_(self.arena)

    def consensus_distance(self, stream=None):
        """VirtualWorkerGroup.consensus_distance over the `x` arena: every worker's distance from the mean
        row in `consensus_dists` (returned; fp32 CUDA [n_local]) and (consensus distance, norm of the
        mean) in `consensus_stats`, enqueued without a host synchronisation.  nranks = 1 only."""
        if not self._one_gpu:
            raise NotImplementedError("consensus_distance: the mean needs every worker's rows on this GPU "
                                      "(nranks = 1, no transport); a cross-GPU consensus distance is not built")
        if self._consensus is None:
            self._consensus = Consensus([self.numel], [[self.x[r].data_ptr() for r in range(self.n_local)]], 4)
            self.consensus_dists, self.consensus_stats = self._consensus.dists, self._consensus.stats
        self._consensus.enqueue(stream_ptr(stream))
        return self.consensus_dists

    @property
    def publish_cols(self):
        """Floats of a message slot the pull round publishes (msg_bytes rounded up to 16 bytes: what
        mx_pull_fetch and mx_choco_apply_slots read)."""
        return (self.msg_bytes + 15) // 16 * 4

    def message(self, slot):
        """(values float32[k], indices int64[k]) views of message `slot` (index-sorted); with
        compressor="sign": (scale, a 0-dim float32 view, bits uint8[ceil(P/8)], column c = bit c & 7 of
        byte c >> 3); with compressor="quant": (norms float32[ceil(P/256)], codes uint8[ceil(P bits / 8)])."""
        self._needs_slots("message")
        base = slot * self.msg_ld
        if self.quant:
            return (self.msgs[base + 64:base + 64 + 4 * ((self.numel + 255) // 256)].view(torch.float32),
                    self.msgs[base + self.codes_off:base + self.codes_off + (self.numel * self.bits + 7) // 8])
        if self.sign:
            return (self.msgs[base:base + 4].view(torch.float32)[0],
                    self.msgs[base + 64:base + 64 + (self.numel + 7) // 8])
        vals = self.msgs[base:base + 4 * self.k].view(torch.float32)
        idx = self.msgs[base + 4 * self.kpad:base + 4 * self.kpad + 8 * self.k].view(torch.int64)
        return vals, idx

    def compress(self, it, stream=None):
        """prepare_comm_buffer (communicator.py:175-196): every local row's top-k message of
        x - x_hat into its message slot (compressor="sign": its scaled-sign message; "quant": its quantized
        message of round `it`; "randk": its k random columns of round `it`)."""
        self._needs_slots("compress")
        if self.quant:
            return self._quant_compress(int(it), None, stream)
        if self.randk:
            return self._randk_compress(int(it), None, stream)
        if self.sign:
            check(lib.mx_choco_sign_compress(self.x.data_ptr(), self.x_hat.data_ptr(), self.ld, self.n_local,
                                             self.numel, self.msgs.data_ptr(), self.msg_ld, self.work.data_ptr(),
                                             stream_ptr(stream)), "mx_choco_sign_compress")
            return
        check(lib.mx_topk_abs_diff_rows(self.x.data_ptr(), self.x_hat.data_ptr(), self.ld, self.n_local,
                                        self.numel, self.k, self.msgs.data_ptr(), self.msg_ld, 4 * self.kpad,
                                        self.bnd_off, self.work.data_ptr(), self.work_ld, stream_ptr(stream)),
              "mx_topk_abs_diff_rows")

    def _needs_slots(self, what):
        if self.one_launch:
            raise MXError(f"ChocoWorkerGroup.{what}: a one_launch group has no message slots -- its messages never "
                          "reach memory (round_norms holds the last round's norms)")

    def _quant_round(self, it, iter_dev, stream, sgd=None, n_iters=None, adamw=None):
        """The one-launch round at plan record `it`, or at the device counter (`iter_dev`: its address, valid below
        `n_iters`, by default the schedule's length); `sgd`: (lr, lr_dev) of the SGD step in front of it; `adamw`:
        (lr, lr_dev, step, step_dev) of the AdamW step in front of it."""
        bf = self.dtype == torch.bfloat16        # the models' image p after s, and _bf16 in the entry point's name
        head = (self.x_hat.data_ptr(), self.s.data_ptr(), *((self.arena.data_ptr(),) if bf else ()), self.ld,
                self.n_local, self.numel, self.bits, self.engine.plan.data_ptr())
        at = (iter_dev, self.engine.T if n_iters is None else n_iters) if iter_dev else (int(it),)
        tail = (self.engine.M, self.engine.alpha32, self.gamma32, self.seed, self.row_base,
                self.round_norms.data_ptr(), self.round_norms.shape[1])
        step, par = ("adamw", adamw) if adamw is not None else ("sgd", sgd) if sgd is not None else (None, None)
        stem, build = self._QUANT_STEPS[step]
        rows, hyper = build(self, par)           # the step's arrays after x, its constants after the round's
        fn = stem + ("_bf16" if bf else "") + ("_at" if iter_dev else "")
        check(getattr(lib, fn)(self.x.data_ptr(), *rows, *head, *at, *tail, *hyper, stream_ptr(stream)), fn)

    def _quant_sgd_args(self, par):
        if self._sgd is None:
            raise MXError("no SGD state: call attach_sgd() first")
        m = self.mom_arena.data_ptr() if self.mom_arena is not None else None
        return (self.grad_arena.data_ptr(), m), (float(par[0]), par[1], *self._sgd)

    def _quant_adamw_args(self, par):
        if self._adamw is None:
            raise MXError("no AdamW state: call attach_adamw() first")
        return ((self.grad_arena.data_ptr(), self.exp_avg_arena.data_ptr(), self.exp_avg_sq_arena.data_ptr()),
                (float(par[0]), par[1], *self._adamw, self._bias_dev.data_ptr(), self._bias_dev.shape[0], int(par[2]),
                 par[3]))

    # the steps of the one-launch round: the entry point's name stem and the builder of the step's arguments from
    # the caller's tuple (sgd: (lr, lr_dev); adamw: (lr, lr_dev, step, step_dev)).  A new step is one row
    _QUANT_STEPS = {None: ("mx_choco_quant_round", lambda self, par: ((), ())),
                    "sgd": ("mx_choco_quant_sgd_round", _quant_sgd_args),
                    "adamw": ("mx_choco_quant_adamw_round", _quant_adamw_args)}

    def _quant_compress(self, it, iter_dev, stream=None):
        """mx_choco_quant_compress at round `it`, or at the device counter (`iter_dev`: its address)"""
        check(lib.mx_choco_quant_compress(self.x.data_ptr(), self.x_hat.data_ptr(), self.ld, self.n_local, self.numel,
                                          self.bits, self.msgs.data_ptr(), self.msg_ld, self.seed, it, iter_dev,
                                          self.engine.T if iter_dev else 0, self.row_base, stream_ptr(stream)),
              "mx_choco_quant_compress")

    def _randk_compress(self, it, iter_dev, stream=None):
        """mx_choco_randk_compress at round `it`, or at the device counter (`iter_dev`: its address)"""
        check(lib.mx_choco_randk_compress(self.x.data_ptr(), self.x_hat.data_ptr(), self.ld, self.n_local, self.numel,
                                          self.k, self.msgs.data_ptr(), self.msg_ld, self.seed, it, iter_dev,
                                          self.engine.T if iter_dev else 0, self.row_base, stream_ptr(stream)),
              "mx_choco_randk_compress")

    def _compress_at(self, stream=None):
        """compress() of a graph-replayable round: the quantizer and rand-k read their round from the device counter"""
        if self.quant:
            return self._quant_compress(0, self.iter_dev.data_ptr(), stream)
        if self.randk:
            return self._randk_compress(0, self.iter_dev.data_ptr(), stream)
        self.compress(0, stream)

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
        """True when partner messages are read from the peers' IPC-mapped snapshots (PullTransport)."""
        return self._pull is not None

    def close(self):
        """Release the pull transport's shared buffers; COLLECTIVE under PullTransport (as
        VirtualWorkerGroup.close: a barrier after this rank's last apply, then unmap and free)."""
        if self._pull is not None:
            import torch.distributed as dist
            torch.cuda.synchronize()
            dist.barrier(group=self._pull.transport.group)
            self._pull.close()
            self._pull = None

    def check_topk(self, stream=None):
        """Synchronise and raise MXError if a top-k row barrier's bounded wait expired since the
        last check (mx_topk_check: that round's messages are undefined; never a GPU hang).  Nothing to
        check with compressor="sign", "quant" or "randk": their kernels have no barrier and no wait."""
        if self.k == 0 or self.randk:
            return
        check(lib.mx_topk_check(self.work.data_ptr(), self.work_ld, self.n_local, self.numel, stream_ptr(stream)),
              "mx_topk_check")

    def average(self, it, stream=None):
        """averaging (communicator.py:200-230): receive partner messages ([N > 1] over the
        transport into the message slots after the local ones), then the s / x_hat scatters and
        the dense x update."""
        self._needs_slots("average")
        it = self.engine.round_index(it)         # mx_choco_apply indexes the plan table by `it`
        if self._pull is not None:
            return self._average_pull(it, stream)
        mbase = self.msgs.data_ptr()
        if self.engine.comm is not None:
            self.engine.exchange(it, [mbase + r * self.msg_ld for r in range(self.n_local)],
                                 mbase + self.n_local * self.msg_ld, self.msg_ld, self.msg_bytes, stream)
        if self.quant:
            check(lib.mx_choco_quant_apply(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                           self.numel, self.bits, mbase, self.msg_ld, self.engine.n_slots,
                                           self.engine.plan.data_ptr(), int(it), self.n_local, self.engine.M,
                                           self.engine.alpha32, self.gamma32, stream_ptr(stream)),
                  "mx_choco_quant_apply")
            return
        if self.sign:
            check(lib.mx_choco_sign_apply(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                          self.numel, mbase, self.msg_ld, self.engine.n_slots,
                                          self.engine.plan.data_ptr(), int(it), self.n_local, self.engine.M,
                                          self.engine.alpha32, self.gamma32, stream_ptr(stream)),
                  "mx_choco_sign_apply")
            return
        check(lib.mx_choco_apply(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                 self.numel, self.k, mbase, self.msg_ld, self.engine.n_slots,
                                 self.engine.plan.data_ptr(), int(it), self.n_local, self.engine.M,
                                 self.engine.alpha32, self.gamma32, self.apply_work.data_ptr(),
                                 stream_ptr(stream)), "mx_choco_apply")

    def _average_pull(self, it, stream=None):
        """PullTransport averaging, four launches (three with pull_read="direct") and no host wait:
        the local messages a peer reads this round into snapshot `round % 2` (system-scope release
        per workgroup), the gate
        (this rank's epoch out, bounded waits for the partners', remote slot table -> their
        snapshots), the fetch of the round's partner messages from their owners' HBM into the
        receive slots, the apply.  A gate that expired earlier raises here."""
        st = self._pull
        msg = st.error()
        if msg:
            raise MXError(msg)
        eng = self.engine
        par = st.round & 1
        st.round += 1
        s = stream_ptr(stream)
        frow = (eng._adhoc_flags.data_ptr() if it == eng.T else eng.flags_dev.data_ptr() + it * eng.M)
        # the messages of the rows a peer reads this round (an active partner in another block)
        check(lib.mx_snapshot_publish_rows(self.msgs.data_ptr(), self.msg_ld // 4, st.own + PULL_HEADER + par * st.half,
                                           self.msg_ld // 4, self.publish_cols, self.n_local, frow, eng.M,
                                           eng.partner_dev.data_ptr(), eng.n, self.row_base, s),
              "mx_snapshot_publish_rows")
        tr = st.transport
        check(lib.mx_pull_gate(frow, st.prev_row.data_ptr(), eng.M, eng.partner_dev.data_ptr(), eng.n,
                               st.owner_dev.data_ptr(), st.ranks_dev.data_ptr(), tr.nranks, tr.rank, self.row_base,
                               self.n_local, self.msg_ld, par, st.round, self.slot_ptrs.data_ptr(), eng.n_slots,
                               tr.timeout_s, st.err_dev, s), "mx_pull_gate")
        if self.pull_read == "direct":
            check(lib.mx_choco_apply_slots(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                           self.numel, self.k, self.slot_ptrs.data_ptr(), eng.n_slots,
                                           eng.plan.data_ptr(), int(it), self.n_local, eng.M, eng.alpha32,
                                           self.gamma32, s), "mx_choco_apply_slots")
            return
        mbase = self.msgs.data_ptr()
        rec = eng.plan.data_ptr() + 4 * int(it) * eng.plan_words
        check(lib.mx_pull_fetch(self.slot_ptrs.data_ptr(), self.n_local, eng.max_remote, rec,
                                mbase + self.n_local * self.msg_ld, self.msg_ld, self.msg_bytes, s), "mx_pull_fetch")
        check(lib.mx_choco_apply(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld, self.numel,
                                 self.k, mbase, self.msg_ld, eng.n_slots, eng.plan.data_ptr(), int(it), self.n_local,
                                 eng.M, eng.alpha32, self.gamma32, self.apply_work.data_ptr(), s), "mx_choco_apply")

    def device_round(self, stream=None):
        """Graph-replayable round at the device counter `self.iter_dev` (then advanced): top-k of
        every row, then mx_choco_apply_at, which reads the round on the device and leaves the state
        untouched for a round without active matchings (the reference skips those,
        communicator.py:249-250; the messages written meanwhile are scratch).  One GPU only."""
        if self.engine.comm is not None:
            raise RuntimeError("device_round: graph-replayable rounds need all partners on this GPU (nranks = 1)")
        if self.one_launch:
            self._quant_round(0, self.iter_dev.data_ptr(), stream)
            check(lib.mx_iter_advance(self.iter_dev.data_ptr(), 1, stream_ptr(stream)), "mx_iter_advance")
            return
        self._compress_at(stream)
        self._apply_at(stream)

    def _apply_at(self, stream=None):
        """The apply launch at the device counter, then the counter's advance (device_round,
        sgd_device_round)."""
        sp = stream_ptr(stream)
        if self.quant:
            check(lib.mx_choco_quant_apply_at(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                              self.numel, self.bits, self.msgs.data_ptr(), self.msg_ld,
                                              self.engine.n_slots, self.engine.plan.data_ptr(),
                                              self.iter_dev.data_ptr(), self.engine.T, self.n_local, self.engine.M,
                                              self.engine.alpha32, self.gamma32, sp), "mx_choco_quant_apply_at")
        elif self.sign:
            check(lib.mx_choco_sign_apply_at(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                             self.numel, self.msgs.data_ptr(), self.msg_ld, self.engine.n_slots,
                                             self.engine.plan.data_ptr(), self.iter_dev.data_ptr(), self.engine.T,
                                             self.n_local, self.engine.M, self.engine.alpha32, self.gamma32, sp),
                  "mx_choco_sign_apply_at")
        else:
            check(lib.mx_choco_apply_at(self.x.data_ptr(), self.x_hat.data_ptr(), self.s.data_ptr(), self.ld,
                                        self.numel, self.k, self.msgs.data_ptr(), self.msg_ld, self.engine.n_slots,
                                        self.engine.plan.data_ptr(), self.iter_dev.data_ptr(), self.engine.T,
                                        self.n_local, self.engine.M, self.engine.alpha32, self.gamma32,
                                        self.apply_work.data_ptr(), sp), "mx_choco_apply_at")
        check(lib.mx_iter_advance(self.iter_dev.data_ptr(), 1, sp), "mx_iter_advance")

    def step(self, it, stream=None):
        """One round at iteration `it`; False (nothing done) for an all-zero flags row."""
        if not self.engine.any_active[it]:
            return False
        if self.one_launch:
            self._quant_round(self.engine.round_index(it), None, stream)
            return True
        self.compress(it, stream)
        self.average(it, stream)
        return True

    # ------------------------------------------------------------------ SGD step fused into the round
    def attach_sgd(self, momentum=0.0, weight_decay=0.0, nesterov=False, zero_grads=True):
        """Give the group torch.optim.SGD's state (dampening 0) so that every worker's optimizer.step() +
        zero_grad() (train_mpi.py:131-142) runs on the way into the compressor (csrc/choco_sgd.hip): with
        compressor="sign" inside the compress pass itself, with "topk" as one launch before the selection.

        Allocates `grad_arena` ([n_local, ld] zeros of the models' dtype; `grads` is its [:, :numel] view) and, with
        momentum, `mom_arena` / `momentum_rows`, and `lr_dev` (the device rounds' learning rate).  For
        adopted models every parameter's .grad becomes the matching view of the gradient arena (see
        VirtualWorkerGroup.attach_sgd on zero_grad(set_to_none=True), which would detach them); a group
        whose models were copied (adopt=False) is refused: their gradients never reach the arena.
        The exchange runs after the step, so any transport the unfused round has works here too."""
        momentum, weight_decay = float(momentum), float(weight_decay)
        if nesterov and momentum == 0.0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if self._adamw is not None:
            raise ValueError("ChocoWorkerGroup.attach_sgd: the group carries one optimizer, and attach_adamw() gave "
                             "it AdamW")
        self._attach_grads("attach_sgd")
        self.mom_arena = self.momentum_rows = None
        if momentum != 0.0:
            self.mom_arena = torch.zeros_like(self.x)
            self.momentum_rows = self.mom_arena[:, :self.numel]
        self.sgd_hyper = {"momentum": momentum, "weight_decay": weight_decay, "nesterov": bool(nesterov),
                          "zero_grads": bool(zero_grads)}
        self._sgd = (weight_decay, momentum, int(bool(nesterov)), int(bool(zero_grads)))

    def _attach_grads(self, who):
        """The gradient arena of a fused step (zeros of the models' dtype; adopted parameters' .grad become its
        views) and `lr_dev`, the device rounds' learning rate."""
        if self._copied_models:
            raise ValueError(f"ChocoWorkerGroup.{who}: the models were copied (adopt=False); their gradients "
                             "would never reach the group's gradient arena")
        self.grad_arena = torch.zeros_like(self.arena)
        self.grads = self.grad_arena[:, :self.numel]
        for r, m in enumerate(self._adopted or ()):
            off = 0
            for p in m.parameters():
                k = p.numel()
                p.grad = self.grad_arena[r, off:off + k].view(p.shape)
                off += k
        self.lr_dev = torch.zeros(1, dtype=torch.float32, device="cuda")

    def _sgd_launch(self, compress, lr, lr_dev, iter_dev, stream):
        """The step of every local row: fused into the sign compress pass (`compress`), or alone."""
        if self._sgd is None:
            raise MXError("no SGD state: call attach_sgd() first")
        m = self.mom_arena.data_ptr() if self.mom_arena is not None else None
        tail = (float(lr), lr_dev, *self._sgd, iter_dev, self.engine.T if iter_dev else 0, stream_ptr(stream))
        if compress:
            check(lib.mx_choco_sign_sgd_compress(self.x.data_ptr(), self.grad_arena.data_ptr(), m,
                                                 self.x_hat.data_ptr(), self.ld, self.n_local, self.numel,
                                                 self.msgs.data_ptr(), self.msg_ld, self.work.data_ptr(), *tail),
                  "mx_choco_sign_sgd_compress")
        else:
            check(lib.mx_choco_sgd_step(self.x.data_ptr(), self.grad_arena.data_ptr(), m, self.ld, self.n_local,
                                        self.numel, *tail), "mx_choco_sgd_step")

    def sgd_compress(self, lr, stream=None, it=0):
        """optimizer.step() + zero_grad() + prepare_comm_buffer of every local row: with compressor="sign"
        one fused launch (and the finish), with "topk" and "quant" the step launch, then compress(it)."""
        self._needs_slots("sgd_compress")
        self._sgd_launch(self.sign, lr, None, None, stream)
        if not self.sign:
            self.compress(it, stream)

    def sgd_step(self, it, lr, stream=None):
        """Every local worker's SGD update at learning rate `lr`, then round `it` on the updated rows.
        sign: the fused step + compress launch, then average(); topk: the step launch, compress(),
        average().  A round with no active matching is the step launch alone (False is returned): the
        reference communicates nothing there (communicator.py:249-250) but its optimizers still step."""
        if not self.engine.any_active[it]:
            if self.dtype == torch.bfloat16:
                # the step has to rewrite the image: the same launch in its _at form, whose counter is entry `it` of
                # a constant table -- it finds the record inactive and is the step alone (a host `iter` would not look)
                self._quant_round(0, self._iter_entry(it), stream, sgd=(lr, None), n_iters=self.engine.T + 1)
            else:
                self._sgd_launch(False, lr, None, None, stream)
            return False
        if self.one_launch:                  # the step, the quantizer and the round: one launch
            self._quant_round(self.engine.round_index(it), None, stream, sgd=(lr, None))
            return True
        self.sgd_compress(lr, stream, it)
        self.average(it, stream)
        return True

    def sgd_device_round(self, stream=None):
        """Graph-replayable sgd_step: the round is read from `self.iter_dev` and the learning rate from
        `self.lr_dev` when the kernels run, then the counter is advanced.  The step runs whatever the
        round (the messages of a round without active matchings are scratch, as device_round's); a
        counter outside the schedule makes every launch a no-op: no SGD step either.  One GPU only."""
        if self.engine.comm is not None:
            raise RuntimeError("sgd_device_round: graph-replayable rounds need all partners on this GPU (nranks = 1)")
        if self._sgd is None:
            raise MXError("no SGD state: call attach_sgd() first")
        if self.one_launch:                  # a round of the schedule with no active matching: the step alone
            self._quant_round(0, self.iter_dev.data_ptr(), stream, sgd=(0.0, self.lr_dev.data_ptr()))
            check(lib.mx_iter_advance(self.iter_dev.data_ptr(), 1, stream_ptr(stream)), "mx_iter_advance")
            return
        self._sgd_launch(self.sign, 0.0, self.lr_dev.data_ptr(), self.iter_dev.data_ptr(), stream)
        if not self.sign:
            self._compress_at(stream)
        self._apply_at(stream)

    def sgd_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker at the group's own iteration
        counter; returns seconds like communicate() (a round with no active matching: the step's)."""
        it = self.iter
        self.iter += 1
        torch.cuda.synchronize()
        tic = time.time()
        self.sgd_step(it, lr)
        self.wait_round()
        toc = time.time()
        self.check_topk()
        return toc - tic

    def _iter_entry(self, it):
        """The address of entry round_index(it) of a constant device table 0 .. T: a counter for the _at launches
        (valid below T + 1), through which a host-side step reaches the record of a round with no active matching"""
        if self._iters is None:
            self._iters = torch.arange(self.engine.T + 1, dtype=torch.int64, device="cuda")
        return self._iters.data_ptr() + 8 * self.engine.round_index(it)

    # ------------------------------------------------------------------ AdamW step fused into the one-launch round
    def attach_adamw(self, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True, zero_grads=True):
        """Give the group torch.optim.AdamW's state (decoupled=False: torch.optim.Adam's, the decay as an L2 term
        in the gradient; no amsgrad, no maximize) so that every worker's optimizer.step() + zero_grad()
        (train_mpi.py:131-142), the quantizer and the round are ONE launch (csrc/choco_quant_adamw_round.hip; bfloat16
        models: csrc/choco_quant_adamw_round_bf16.hip).  compressor="quant", one_launch=True groups only, and not
        together with attach_sgd.

        Allocates `grad_arena` / `grads` as attach_sgd does (the models' dtype; adopted parameters' .grad become
        views), `exp_avg_arena` / `exp_avg_rows` and `exp_avg_sq_arena` / `exp_avg_sq_rows` (fp32 zeros) and the
        bias-correction table (engine.adam_bias_table) on the device.  `opt_step` counts the optimizer steps taken
        (adamw_step runs step opt_step + 1); `opt_step_dev` (int64 CUDA, starts at 1) is the NEXT step of
        adamw_device_round and `lr_dev` its learning rate, as VirtualWorkerGroup.attach_adamw's."""
        if not (self.quant and self.one_launch):
            raise NotImplementedError("ChocoWorkerGroup.attach_adamw: AdamW runs inside the one-launch quantized round "
                                      "only (compressor='quant', one_launch=True); there is no standalone Adam step "
                                      "launch for the slot-based paths (top-k, sign, the two quant launches)")
        if self._sgd is not None:
            raise ValueError("ChocoWorkerGroup.attach_adamw: the group carries one optimizer, and attach_sgd() gave "
                             "it SGD")
        from .engine import adam_bias_table, adam_hyper
        betas = (float(betas[0]), float(betas[1]))
        eps, weight_decay = float(eps), float(weight_decay)
        if eps < 0.0 or weight_decay < 0.0:
            raise ValueError("attach_adamw: eps and weight_decay must not be negative")
        bias = adam_bias_table(*betas)                               # ValueError for betas it cannot serve
        self._attach_grads("attach_adamw")
        self.exp_avg_arena, self.exp_avg_sq_arena = torch.zeros_like(self.x), torch.zeros_like(self.x)
        self.exp_avg_rows = self.exp_avg_arena[:, :self.numel]
        self.exp_avg_sq_rows = self.exp_avg_sq_arena[:, :self.numel]
        self._bias_dev = torch.from_numpy(bias).cuda()
        self.opt_step = 0
        self.opt_step_dev = torch.ones(1, dtype=torch.int64, device="cuda")
        self.adamw_hyper = {"betas": betas, "eps": eps, "weight_decay": weight_decay, "decoupled": bool(decoupled),
                            "zero_grads": bool(zero_grads)}
        wd, omb1, beta2, omb2, eps32, dec, zg = adam_hyper(betas, eps, weight_decay, decoupled, zero_grads)
        self._adamw = (omb1, beta2, omb2, eps32, wd, dec, zg)        # the entry points' order

    def adamw_step(self, it, lr, stream=None):
        """ONE launch: every local worker's AdamW update number opt_step + 1 at learning rate `lr`, then round `it`
        on the updated rows; opt_step += 1.  A round with no active matching is the step alone (False is returned):
        the same launch in its _at form, whose counter is entry `it` of a constant table, finds the record inactive."""
        if self._adamw is None:
            raise MXError("no AdamW state: call attach_adamw() first")
        opt = (lr, None, self.opt_step + 1, None)
        active = bool(self.engine.any_active[it])
        if active:
            self._quant_round(self.engine.round_index(it), None, stream, adamw=opt)
        else:
            self._quant_round(0, self._iter_entry(it), stream, adamw=opt, n_iters=self.engine.T + 1)
        self.opt_step += 1
        return active

    def adamw_device_round(self, stream=None):
        """Graph-replayable adamw_step: the round is read from `self.iter_dev`, the optimizer step from
        `self.opt_step_dev` and the learning rate from `self.lr_dev` when the kernel runs, then both counters are
        advanced (unconditionally, as sgd_device_round advances iter_dev).  A round counter outside the schedule or
        a step below 1 makes the launch a no-op.  `self.opt_step` (adamw_step's host counter) is not touched."""
        if self._adamw is None:
            raise MXError("no AdamW state: call attach_adamw() first")
        sp = stream_ptr(stream)
        self._quant_round(0, self.iter_dev.data_ptr(), stream,
                          adamw=(0.0, self.lr_dev.data_ptr(), 0, self.opt_step_dev.data_ptr()))
        check(lib.mx_iter_advance(self.iter_dev.data_ptr(), 1, sp), "mx_iter_advance")
        check(lib.mx_iter_advance(self.opt_step_dev.data_ptr(), 1, sp), "mx_iter_advance")

    def adamw_communicate(self, lr):
        """optimizer.step() + zero_grad() + communicate() of every worker at the group's own iteration counter, as
        one launch; returns seconds like communicate()."""
        it = self.iter
        self.iter += 1
        torch.cuda.synchronize()
        tic = time.time()
        self.adamw_step(it, lr)
        self.wait_round()
        return time.time() - tic

    def state_dict(self):
        """Checkpoint: rows (the fp32 `x`: under bfloat16 models the masters, with a "dtype" tag), the persistent
        Choco state x_hat / s (communicator.py:179-182) and the iteration counter; with attach_adamw the exp_avg /
        exp_avg_sq rows and the optimizer step count."""
        P = self.numel
        state = {"kind": "choco", "iter": int(self.iter), "row_base": int(self.row_base), "k": int(self.k),
                 "workers": list(self.workers),
                 "rows": self.x[:, :P].detach().clone(), "x_hat": self.x_hat[:, :P].detach().clone(),
                 "s": self.s[:, :P].detach().clone()}
        if self.sign:                        # a top-k group's checkpoint stays key for key what it was
            state["compressor"] = "sign"
        if self.quant:
            state.update(compressor="quant", bits=self.bits, seed=self.seed)
        if self.randk:
            state.update(compressor="randk", seed=self.seed)
        if self.dtype == torch.bfloat16:     # `rows` are the fp32 masters either way: an fp32 group loads them
            state["dtype"] = "bfloat16"
        if self.momentum_rows is not None:   # attach_sgd with momentum; without it, key for key what it was
            state["momentum_rows"] = self.momentum_rows.detach().clone()
        if self._adamw is not None:          # attach_adamw; every other group's checkpoint is key for key what it was
            state["exp_avg_rows"] = self.exp_avg_rows.detach().clone()
            state["exp_avg_sq_rows"] = self.exp_avg_sq_rows.detach().clone()
            state["opt_step"] = int(self.opt_step)
        return state

    def load_state_dict(self, state):
        P = self.numel
        if state.get("kind") != "choco" or int(state["row_base"]) != self.row_base or \
                list(state.get("workers", self.workers)) != self.workers or \
                state.get("compressor", "topk") != self.compressor or state.get("bits") != self.bits or \
                int(state["k"]) != self.k or tuple(state["rows"].shape) != (self.n_local, P):
            raise ValueError("checkpoint does not match this Choco worker group")
        if ("momentum_rows" in state) != (self.momentum_rows is not None):
            raise ValueError("checkpoint does not match this Choco worker group: it was saved %s SGD momentum rows, "
                             "this group is attached %s them" % (("with", "without") if "momentum_rows" in state
                                                                 else ("without", "with")))
        adam = [state.get(k) for k in ("exp_avg_rows", "exp_avg_sq_rows")]
        if any(a is None for a in adam) != all(a is None for a in adam):
            # exp_avg without exp_avg_sq (or the other way round) would bias every later step
            raise ValueError("checkpoint carries half of the Adam state: exp_avg_rows and exp_avg_sq_rows are only "
                             "valid together")
        if (adam[0] is not None) != (self._adamw is not None):
            raise ValueError("checkpoint does not match this Choco worker group: it was saved %s AdamW state, this "
                             "group is attached %s it" % (("with", "without") if adam[0] is not None
                                                          else ("without", "with")))
        if any(a is not None and tuple(a.shape) != (self.n_local, P) for a in adam):
            raise ValueError("checkpoint does not match this Choco worker group: the shape of its Adam state")
        with torch.no_grad():
            if self._adamw is not None:
                self.exp_avg_rows.copy_(adam[0])
                self.exp_avg_sq_rows.copy_(adam[1])
                self.opt_step = int(state.get("opt_step") or 0)
                self.opt_step_dev.fill_(self.opt_step + 1)
            if self.momentum_rows is not None:
                self.momentum_rows.copy_(state["momentum_rows"])
            self.x[:, :P].copy_(state["rows"])
            self.x_hat[:, :P].copy_(state["x_hat"])
            self.s[:, :P].copy_(state["s"])
            if self.arena is not self.x:     # the image of the loaded masters
                self.arena[:, :P].copy_(self.x[:, :P].to(self.dtype))
        self.iter = int(state["iter"])
        if self.quant or self.randk:
            self.seed = int(state["seed"])       # the resumed run draws the saved run's random numbers

    def communicate(self):
        it = self.iter
        self.iter += 1
        if np.sum(self.topology.active_flags[it]) == 0:
            return 0
        torch.cuda.synchronize()
        tic = time.time()
        self.step(it)
        self.wait_round()
        toc = time.time()
        self.check_topk()
        return toc - tic
