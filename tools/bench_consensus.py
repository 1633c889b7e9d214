"""The consensus-distance launches (mx_consensus, csrc/consensus.hip) against the gradient-norm launches over
the same arena and against doing it with torch, in ONE process: the headline shape, 8 rows x 25.6M columns,
and 64 rows x 3.2M (the same bytes), each as fp32 and as bfloat16 rows.  Timed, each after a settle burst sized
with bench.settle_rounds, as K back-to-back calls between one HIP event pair:

  (a) consensus    the two launches of mx_consensus: every row's distance from the mean row, the consensus
                   distance and the norm of the mean, from one read of n * P * element size bytes
  (b) grad_norm    mx_grad_norm over the same arena (csrc/grad_norm.hip): the yardstick, which moves exactly
                   the same bytes with less arithmetic
  (c) torch        (rows.double() - rows.double().mean(0)).pow(2).sum(1): what a user writes without the kernel
                   (fp64 temporaries of 8 bytes per element; --torch-rounds calls)

First the device figures are checked against the torch fp64 expression (1 fp32 ulp: both are within half an
ulp and a few 1e-9 of the exact value on these well-spread rows); a failed check withholds the rates.  Every
figure is timed in --passes passes in alternating order; ratios use the means and "spread" is (max - min) /
mean.  --blocks-per-cu lists further values of the "blocks_per_cu" knob to time (a) under.  One JSON line,
also written to profiles/consensus_bench.json.

    python tools/bench_consensus.py [--rounds 300] [--settle-ms 50] [--modes fp32,bf16] [--shapes 8x25600000,64x3200000]
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
import bench  # noqa: E402

L = pkg.lib
E = pkg.engine


def timed(step, settle, K):
    """`settle` untimed calls, then K calls between one event pair: ms per call"""
    for _ in range(settle):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(K):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / K


def ulps(a, b):
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max().item())


def run_shape(n, P, mode, K, torch_rounds, settle_ms, passes, sweep):
    bf16 = mode == "bf16"
    esz = 2 if bf16 else 4
    ld = (P + E.ROW_ALIGN - 1) // E.ROW_ALIGN * E.ROW_ALIGN
    arena = torch.zeros((n, ld), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    rows = arena[:, :P]
    tmp = torch.empty(P, dtype=torch.float32, device="cuda") if bf16 else None
    for r in range(n):
        if bf16:
            pkg._lib.check(L.mx_synth_fill(tmp.data_ptr(), P, 1234 + r, None))
            rows[r].copy_(tmp)
        else:
            pkg._lib.check(L.mx_synth_fill(rows[r].data_ptr(), P, 1234 + r, None))
    del tmp
    ptrs = [[arena[r].data_ptr() for r in range(n)]]
    cons = E.Consensus([P], ptrs, esz)
    s = pkg._lib.stream_ptr

    def torch_expr():
        x = rows.double()
        m = x.mean(0)
        return (x - m).pow(2).sum(1), m.pow(2).sum()

    # the check: the device figures against torch's fp64 expression, within 1 fp32 ulp
    cons.enqueue(s())
    D, M = torch_expr()
    want_d, want_s = D.sqrt().float(), torch.stack([(D.sum() / n).sqrt(), M.sqrt()]).float()
    torch.cuda.synchronize()
    ud, us = ulps(cons.dists, want_d), ulps(cons.stats, want_s)
    ok = bool(torch.isfinite(cons.dists).all().item() and torch.isfinite(cons.stats).all().item()) and max(ud, us) <= 1
    out = {"rows": n, "params": P, "mode": mode, "bytes_per_element": esz, "check_max_ulp": max(ud, us), "check": ok,
           "consensus_distance": float(cons.stats[0]), "mean_norm": float(cons.stats[1])}
    del D, M, want_d, want_s
    torch.cuda.empty_cache()
    if not ok:
        out["withheld"] = "the device figures differ from torch's fp64 expression by more than 1 ulp: no rate is reported"
        return out

    table = types.SimpleNamespace(g_ptrs=cons.x_ptrs, seg_len=cons.seg_len, n_local=n)
    norm = E.GradNorm([P], table, esz, 1.0)
    nbytes = n * P * esz
    settle = bench.settle_rounds(nbytes, settle_ms)
    figures = [("a_consensus", lambda: cons.enqueue(s()), K, settle), ("b_grad_norm", lambda: norm.enqueue(s()), K, settle),
               ("c_torch", torch_expr, torch_rounds, 2)]
    ms = {name: [] for name, _, _, _ in figures}
    for rep in range(passes):
        for name, step, k, st in (figures if rep % 2 == 0 else figures[::-1]):
            ms[name].append(round(timed(step, st, k), 5))
    for name, _, _, _ in figures:
        mean = float(np.mean(ms[name]))
        out[name] = {"ms_per_call": round(mean, 5), "ms_per_call_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / mean, 4), "algorithmic_bytes": nbytes,
                     "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4)}
    out["consensus_over_grad_norm"] = round(out["a_consensus"]["ms_per_call"] / out["b_grad_norm"]["ms_per_call"], 4)
    out["torch_over_consensus"] = round(out["c_torch"]["ms_per_call"] / out["a_consensus"]["ms_per_call"], 2)
    if sweep:
        saved = E.consensus_tuning()
        out["blocks_per_cu_sweep_ms"] = {}
        try:
            for v in sweep:
                E.set_consensus_tuning(blocks_per_cu=v)
                out["blocks_per_cu_sweep_ms"][str(v)] = round(timed(lambda: cons.enqueue(s()), settle, K), 5)
        finally:
            E.set_consensus_tuning(**saved)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x25600000,64x3200000")
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--torch-rounds", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--blocks-per-cu", default="", help="further blocks_per_cu values to time the consensus launches under")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_bench.json"))
    args = ap.parse_args()
    sweep = [int(v) for v in args.blocks_per_cu.split(",") if v]
    out = {"tool": "bench_consensus", "rounds": args.rounds, "torch_rounds": args.torch_rounds, "settle_ms": args.settle_ms,
           "passes": args.passes, "device": torch.cuda.get_device_properties(0).gcnArchName,
           "knobs_consensus": E.consensus_tuning(), "knobs_grad_norm": E.grad_norm_tuning(), "results": []}
    rc = 0
    for shape in args.shapes.split(","):
        n, P = (int(v) for v in shape.split("x"))
        for mode in args.modes.split(","):
            res = run_shape(n, P, mode, args.rounds, args.torch_rounds, args.settle_ms, args.passes, sweep)
            out["results"].append(res)
            if "withheld" in res:
                rc = 1
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
