"""Store policy A/B (mx_mix_set "store_policy": 1 nt, 2 sc1, 3 sc1 nt, 4 sc0 sc1; 0 auto) of the row
kernel's 8-slot class and of the centralized mean, in one process.

Row kernel, graph 0, full rounds (every row active): per size, every policy settled (WARM rounds), then
ROUNDS back-to-back rounds between one event pair; PASSES passes, the policies in alternating order.  Bits:
3 rounds from the same rows under every policy.  Then the mean (mx_mean_rows_to, 8 rows in place) the same
way.  SMALL sizes (rows the L2s or the Infinity Cache hold, and the launch-bound configs) run auto against
forced nt, eagerly and -- with GRAPH=1 -- as a captured graph of 20 rounds: auto must launch nt's
instantiation there, so the two columns are one kernel timed twice.  The four fused optimizer rounds
(FUSED, FUSED_SIZES; momentum SGD and AdamW steps, zero_grads off) under their own knob (mx_<family>_set
"store_policy": 1 nt, 2 sc1, 3 sc1 nt), timed the same way; bits: x / w, p, m and v after 3 steps.  One JSON
line per size.

    SIZES=25600000,36546980,14800000 SMALL=4000000,181668,666547 MEAN=25600000 \\
        FUSED=sgd,sgd_bf16,adamw,adamw_bf16 python tools/store_policy_ab.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
from conftest import Topo  # noqa: E402

L = pkg.lib
E = pkg.engine
n = 8
NAMES = {0: "auto", 1: "nt", 2: "sc1", 3: "sc1_nt", 4: "sc0_sc1"}


def ints(key, default):
    return [int(float(x)) for x in os.environ.get(key, default).split(",") if x]


sizes = ints("SIZES", "25600000,36546980,14800000")
small = ints("SMALL", "4000000,181668,666547")
mean_sizes = ints("MEAN", "25600000")
policies = ints("POLICIES", "1,2,3,4")
rounds = int(os.environ.get("ROUNDS", "300"))
warm = int(os.environ.get("WARM", "20"))
passes = int(os.environ.get("PASSES", "2"))
use_graph = os.environ.get("GRAPH", "1") != "0"
saved = E.mix_tuning()
gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, n, 4, True)
topo = Topo(gp.neighbors_info, 2 / 7, np.ones((rounds + warm + 8, len(gp.neighbors_info)), np.uint8))


def timed(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for j in range(count):
        fn(j)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / count


def report(head, res, sums, pols):
    out = dict(head)
    for p in pols:
        out[NAMES[p]] = {"ms_min": round(min(res[p]), 5), "ms_all": [round(x, 5) for x in res[p]],
                         "same_bits": sums[p] == sums[pols[0]]}
    base = min(res[pols[0]])
    out["vs_" + NAMES[pols[0]]] = {NAMES[p]: round(min(res[p]) / base, 4) for p in pols[1:]}
    print(json.dumps(out), flush=True)


def rows_ab(P, pols, graph):
    grp = pkg.VirtualWorkerGroup(topo, numel=P)
    sums, res = {}, {p: [] for p in pols}
    for p in pols:
        E.set_mix_tuning(store_policy=p)
        for r in range(n):
            pkg._lib.check(L.mx_synth_fill(grp.rows[r].data_ptr(), P, 1234 + r, None))
        for j in range(3):
            grp.engine.mix(j, grp.layout)
        torch.cuda.synchronize()
        sums[p] = int(grp.rows[:, :P].contiguous().view(torch.int32).to(torch.int64).sum())
    graphs = {}
    if graph:
        K = 20
        for p in pols:                          # the dispatch runs at capture: one graph per policy
            E.set_mix_tuning(store_policy=p)
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                grp.device_rounds(K)
                torch.cuda.synchronize()
                with torch.cuda.graph(g, stream=s):
                    grp.device_rounds(K)
            torch.cuda.current_stream().wait_stream(s)
            graphs[p] = g
    for rep in range(passes):
        for p in (pols if rep % 2 == 0 else pols[::-1]):
            E.set_mix_tuning(store_policy=p)
            if graph:
                grp.iter_dev.fill_(0)
                graphs[p].replay()
                grp.iter_dev.fill_(0)
                res[p].append(timed(lambda j: graphs[p].replay(), rounds // K) / K)
            else:
                for j in range(warm):
                    grp.engine.mix(j, grp.layout)
                res[p].append(timed(lambda j: grp.engine.mix(warm + j, grp.layout), rounds))
    report({"kernel": "mix_kernel_rows", "P": P, "graph_replayed": bool(graph), "round_bytes": 2 * n * P * 4,
            "rounds": rounds}, res, sums, pols)
    del graphs
    grp.close()
    del grp
    torch.cuda.empty_cache()


def mean_ab(P, pols):
    ld = (P + 63) // 64 * 64
    rows = torch.empty((n, ld), dtype=torch.float32, device="cuda")

    def one(_=0):
        pkg._lib.check(L.mx_mean_rows_to(rows.data_ptr(), n, ld, P, 0, rows.data_ptr(), n, ld, None))

    sums, res = {}, {p: [] for p in pols}
    for p in pols:
        E.set_mix_tuning(store_policy=p)
        for r in range(n):
            pkg._lib.check(L.mx_synth_fill(rows[r].data_ptr(), P, 1234 + r, None))
        one()
        torch.cuda.synchronize()
        sums[p] = int(rows[:, :P].contiguous().view(torch.int32).to(torch.int64).sum())
    for rep in range(passes):
        for p in (pols if rep % 2 == 0 else pols[::-1]):
            E.set_mix_tuning(store_policy=p)
            for _ in range(warm):
                one()
            res[p].append(timed(one, rounds))
    report({"kernel": "mean_tile_kernel", "P": P, "round_bytes": 2 * n * P * 4, "rounds": rounds}, res, sums, pols)


def fused_ab(kind, P, pols):
    """one fused optimizer family's step (momentum SGD / AdamW, zero_grads off) under its own store_policy"""
    adam, mixed = kind.startswith("adamw"), kind.endswith("bf16")
    T = 64
    ftopo = Topo(gp.neighbors_info, 2 / 7, np.ones((T, len(gp.neighbors_info)), np.uint8))
    grp = pkg.VirtualWorkerGroup(ftopo, numel=P, dtype=torch.bfloat16 if mixed else torch.float32)
    if adam:
        grp.attach_adamw(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, zero_grads=False, master_weights=mixed)
        step = lambda j: grp.adamw_step(j % T, 1e-3)
    else:
        grp.attach_sgd(momentum=0.9, weight_decay=5e-4, zero_grads=False, master_weights=mixed)
        step = lambda j: grp.sgd_step(j % T, 1e-2)
    fam = E.FAMILIES["adamw" if adam else "sgd", mixed]
    fsaved = int(fam.get(b"store_policy"))

    def put(store_policy):
        pkg._lib.check(fam.set(b"store_policy", int(store_policy)), fam.base + "_set")

    def fill():
        with torch.no_grad():
            (grp.master_rows if mixed else grp.rows).normal_(0.0, 1.0)
            if mixed:
                grp.rows.copy_(grp.master_rows)
            grp.grads.normal_(0.0, 0.01)
            for t in ((grp.exp_avg_rows, grp.exp_avg_sq_rows) if adam else (grp.momentum_rows,)):
                t.zero_()

    def digest():
        torch.cuda.synchronize()
        ts = [grp.master_rows if mixed else grp.rows] + ([grp.rows] if mixed else []) + \
             ([grp.exp_avg_rows, grp.exp_avg_sq_rows] if adam else [grp.momentum_rows])
        return tuple(int(t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
                         .to(torch.int64).sum()) for t in ts)

    sums, res = {}, {p: [] for p in pols}
    try:
        torch.manual_seed(7)
        fill()
        keep = [t.clone() for t in ([grp.master_rows if mixed else grp.rows] + [grp.grads])]
        for p in pols:
            put(store_policy=p)
            grp.opt_step = 0                    # AdamW's bias correction: the same three steps
            with torch.no_grad():
                (grp.master_rows if mixed else grp.rows).copy_(keep[0])
                if mixed:
                    grp.rows.copy_(keep[0])
                grp.grads.copy_(keep[1])
                for t in ((grp.exp_avg_rows, grp.exp_avg_sq_rows) if adam else (grp.momentum_rows,)):
                    t.zero_()
            for j in range(3):
                step(j)
            sums[p] = digest()
        del keep
        for rep in range(passes):
            for p in (pols if rep % 2 == 0 else pols[::-1]):
                put(store_policy=p)
                for j in range(warm):
                    step(j)
                res[p].append(timed(step, rounds))
    finally:
        put(fsaved)
    report({"kernel": "fused_round_rows", "family": kind, "P": P, "rounds": rounds}, res, sums, pols)
    grp.close()
    del grp
    torch.cuda.empty_cache()


fused = [k for k in os.environ.get("FUSED", "sgd,sgd_bf16,adamw,adamw_bf16").split(",") if k]
fused_sizes = ints("FUSED_SIZES", "25600000")

try:
    for P in sizes:
        rows_ab(P, policies, False)
    for P in mean_sizes:
        mean_ab(P, policies)
    for kind in fused:
        for P in fused_sizes:
            fused_ab(kind, P, [1, 2, 3])
    for P in small:
        rows_ab(P, [1, 0], False)
        if use_graph:
            rows_ab(P, [1, 0], True)
finally:
    E.set_mix_tuning(**saved)
