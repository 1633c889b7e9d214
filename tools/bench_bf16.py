"""fp32 against bfloat16 worker rows on the headline shape, in ONE process: graph 0, 8 workers x
25.6M parameters, every matching active.  Per dtype: a settle burst sized with bench.settle_rounds,
then K back-to-back rounds between one HIP event pair (a GPU-side time per round).  One JSON line:
ms per round, algorithmic bytes (2 * 8 * P * element size), TB/s, and the ratio of the two times.
Then 64 sampled columns of the bf16 rows are checked against the specification (tests/bf16ref.py:
the oracle's fp32 chain on the widened inputs, rounded to nearest even once); a failed check
withholds the rates, as bench.py does.

    python tools/bench_bf16.py [--params 25600000] [--rounds 200] [--settle-ms 50] [--ab]

--ab also times the bf16 kernel's optional levers (mx_mix_bf16_set: streaming hints off / on, the
workgroups-per-CU cap, the work-item width), each settled the same way, over --reps passes in
alternating order, under "ab".
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
import bench  # noqa: E402
import oracle as O  # noqa: E402
from bf16ref import same_bf16, spec_round  # noqa: E402
from conftest import Topo  # noqa: E402

L = pkg.lib
N = 8


def timed(grp, settle, K, T):
    """`settle` untimed rounds, then K rounds between one event pair: ms per round"""
    for j in range(settle):
        grp.engine.mix(j % T, grp.layout)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for j in range(K):
        grp.engine.mix(j % T, grp.layout)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=25_600_000)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    P, K, T = args.params, args.rounds, 64
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    alpha = 2 / 7
    topo = Topo(partner, alpha, np.ones((T, partner.shape[0]), np.uint8))
    g32 = pkg.VirtualWorkerGroup(topo, numel=P)
    g16 = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16)
    for r in range(N):
        pkg._lib.check(L.mx_synth_fill(g32.rows[r].data_ptr(), P, 1234 + r, None))
    g16.rows.copy_(g32.rows)                     # the same values, rounded once

    # the check first: 64 columns spread over the row (both ends and a tile edge included)
    cols_h = np.linspace(0, P - 1, 64).astype(np.int64)
    cols_h[1] = min(P - 1, 2047)
    cols = torch.from_numpy(cols_h).cuda()
    snap = g16.rows.index_select(1, cols).view(torch.int16).cpu().numpy().view(np.uint16)
    ok = True
    for it in range(3):
        g16.engine.mix(it, g16.layout)
        want = spec_round(O, snap, partner, np.ones(partner.shape[0], np.uint8), alpha)
        snap = g16.rows.index_select(1, cols).view(torch.int16).cpu().numpy().view(np.uint16)
        ok = ok and same_bf16(snap, want)
    out = {"tool": "bench_bf16", "graph": 0, "workers": N, "params": P, "rounds": K, "settle_ms": args.settle_ms,
           "device": torch.cuda.get_device_properties(0).gcnArchName, "bf16_check_64_columns": ok}
    if not ok:
        out["withheld"] = "the bf16 rows differ from the specification: no rate is reported"
        print(json.dumps(out), flush=True)
        return 1
    res = {}
    for name, grp, elem in (("fp32", g32, 4), ("bf16", g16, 2)):
        nbytes = 2 * N * P * elem
        settle = bench.settle_rounds(nbytes, args.settle_ms)
        ms = timed(grp, settle, K, T)
        res[name] = {"ms_per_round": round(ms, 5), "algorithmic_bytes": nbytes, "settle_rounds": settle,
                     "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 4)}
    out.update(res)
    out["time_ratio_bf16_over_fp32"] = round(res["bf16"]["ms_per_round"] / res["fp32"]["ms_per_round"], 4)
    out["rate_ratio_bf16_over_fp32"] = round(res["bf16"]["tb_per_s"] / res["fp32"]["tb_per_s"], 4)
    if args.ab:
        saved = {k: int(L.mx_mix_bf16_get(k.encode())) for k in ("nontemporal", "wgpc", "split")}
        variants = [("default", {}), ("nt0", {"nontemporal": 0}), ("nt1", {"nontemporal": 1})] + \
                   [(f"wgpc{w}", {"wgpc": w}) for w in (4, 5, 6, 8)] + \
                   [("split1", {"split": 1}), ("split4", {"split": 4}), ("split1_wgpc3", {"split": 1, "wgpc": 3}),
                    ("split4_wgpc8", {"split": 4, "wgpc": 8})]
        nbytes = 2 * N * P * 2
        settle = bench.settle_rounds(nbytes, args.settle_ms)
        ab = {name: [] for name, _ in variants}
        for rep in range(args.reps):
            for name, knobs in (variants if rep % 2 == 0 else variants[::-1]):
                for k, v in {**saved, **knobs}.items():
                    pkg._lib.check(L.mx_mix_bf16_set(k.encode(), v), "mx_mix_bf16_set")
                ab[name].append(round(timed(g16, settle, K, T), 5))
        for k, v in saved.items():
            pkg._lib.check(L.mx_mix_bf16_set(k.encode(), v), "mx_mix_bf16_set")
        out["ab"] = {"ms_per_round": ab, "note": "bf16 kernel, each entry settled then timed over `rounds` rounds; "
                     "passes run in alternating order"}
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
