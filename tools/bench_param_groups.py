"""Per-parameter-group weight decay / lr scale in the fused AdamW rounds (the mx_adamw_mix[_bf16]_grouped
entry points) against the ungrouped step of the same library, on the headline shape, in ONE process:
graph 0, 8 workers x 25.6M parameters, every matching active, betas (0.9, 0.999), eps 1e-8, decoupled
weight decay 1e-2 -- once for the fp32 group (csrc/adamw_mix.hip) and once for the mixed-precision group
(bfloat16 gradients, csrc/adamw_mix_bf16.hip).  Timed, each after a settle burst sized with
bench.settle_rounds, as K back-to-back steps between one HIP event pair:

  (a) ungrouped    the fused step (mx_adamw_mix[_bf16])
  (b) one run      the grouped step with ONE run (wd, 1.0): every work item on the uniform path
  (c) transformer  a transformer-like table: repeating 1024 x 1024 decayed matrix, 1024 bias, 2 x 1024
                   normalisation parameters (bias and norm without decay: one 3072-column run), to the
                   end of the row -- 3 work items in 2051 hold a boundary
  (d) worst case   alternating 64-column runs (wd, 1.0) / (0, 1.0): every work item resolves the run per
                   element

The bytes moved are the same 28 per element in all four (the tables are a few KB; (d)'s are 4.8 MB, read
through the cache), so (b) / (a) and (c) / (a) measure the instruction stream alone; the yardstick is
(a)'s own two-pass spread widened by 1 %.  (d) is reported only.  Every figure is timed in --passes
passes (default 2) in alternating order; both passes are reported, ratios use their means and "spread"
is (max - min) / mean.  One JSON line, also written to profiles/param_groups_bench.json.

    python tools/bench_param_groups.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--modes fp32,bf16]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
import bench  # noqa: E402
from conftest import Topo  # noqa: E402

L = pkg.lib
N = 8
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 1e-2, 1e-3
WD32 = float(np.float32(WD))


def timed(step, settle, K):
    """`settle` untimed steps, then K steps between one event pair: ms per step"""
    for j in range(settle):
        step(j)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for j in range(K):
        step(j)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / K


def transformer_runs(P):
    """[1024 x 1024 matrix (decayed) | 1024 bias + 2 x 1024 norm parameters (no decay)] repeated over [0, P)"""
    runs, at = [], 0
    while at < P:
        for width, wd in ((1024 * 1024, WD32), (3 * 1024, 0.0)):
            if at < P:
                end = min(P, at + width)
                runs.append((at, end, wd, 1.0))
                at = end
    return runs


def alternating_runs(P, width=64):
    return [(a, min(P, a + width), WD32 if (a // width) % 2 == 0 else 0.0, 1.0) for a in range(0, P, width)]


def run_mode(mode, P, K, T, settle_ms, passes):
    mixed = mode == "bf16"
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    topo = Topo(partner, 2 / 7, np.ones((T, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16 if mixed else torch.float32)
    grp.attach_adamw(betas=(B1, B2), eps=EPS, weight_decay=WD, zero_grads=False, master_weights=mixed)
    tmp = torch.empty(P, dtype=torch.float32, device="cuda") if mixed else None
    weights = grp.master_rows if mixed else grp.rows

    def fill():
        with torch.no_grad():
            for r in range(N):
                pkg._lib.check(L.mx_synth_fill(weights[r].data_ptr(), P, 1234 + r, None))
                if mixed:
                    pkg._lib.check(L.mx_synth_fill(tmp.data_ptr(), P, 4321 + r, None))
                    grp.grads[r].copy_(tmp)
                else:
                    pkg._lib.check(L.mx_synth_fill(grp.grads[r].data_ptr(), P, 4321 + r, None))
            grp.exp_avg_arena.zero_()
            grp.exp_avg_sq_arena.zero_()

    s = pkg._lib.stream_ptr
    call = grp._adamw_state()
    plain_fn, grouped_fn = grp._adamw.run, grp._adamw.grouped
    tables = {"b_one_run": pkg.engine.ParamRuns(P, [(0, P, WD32, 1.0)]),
              "c_transformer": pkg.engine.ParamRuns(P, transformer_runs(P)),
              "d_alternating_64": pkg.engine.ParamRuns(P, alternating_runs(P))}
    step_no = [0]

    def ungrouped(j):
        step_no[0] += 1
        pkg._lib.check(plain_fn(call, j % T, step_no[0], LR, None, s()), "mx_adamw_mix")

    def grouped(name):
        addr = tables[name].addr

        def step(j):
            step_no[0] += 1
            pkg._lib.check(grouped_fn(call, addr, None, j % T, step_no[0], LR, None, s()), "mx_adamw_mix_grouped")
        return step

    figures = (("a_ungrouped", ungrouped),) + tuple((name, grouped(name)) for name in tables)
    nbytes = 28 * N * P
    ms = {name: [] for name, _ in figures}
    for rep in range(passes):
        for name, step in (figures if rep % 2 == 0 else figures[::-1]):
            fill()
            step_no[0] = 0
            ms[name].append(round(timed(step, bench.settle_rounds(nbytes, settle_ms), K), 5))
    out = {"mode": mode, "runs": {name: len(t.runs) for name, t in tables.items()}}
    for name, _ in figures:
        mean = float(np.mean(ms[name]))
        out[name] = {"ms_per_step": round(mean, 5), "ms_per_step_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / mean, 4), "algorithmic_bytes": nbytes,
                     "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4)}
    a = out["a_ungrouped"]
    margin = 1.0 + a["spread"] + 0.01
    out["margin"] = round(margin, 4)
    for name in tables:
        key = name[0] + "_over_a"
        out[key] = round(out[name]["ms_per_step"] / a["ms_per_step"], 4)
        if name[0] in "bc":
            out[key + "_within_margin"] = bool(out[key] <= margin)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=25_600_000)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups_bench.json"))
    args = ap.parse_args()
    out = {"tool": "bench_param_groups", "graph": 0, "workers": N, "params": args.params, "rounds": args.rounds,
           "settle_ms": args.settle_ms, "passes": args.passes,
           "hyper": {"lr": LR, "betas": [B1, B2], "eps": EPS, "weight_decay": WD, "decoupled": True},
           "device": torch.cuda.get_device_properties(0).gcnArchName,
           "knobs_bf16": pkg.engine.adamw_mix_bf16_tuning(), "knobs_fp32": pkg.engine.adamw_mix_tuning()}
    for mode in args.modes.split(","):
        out[mode] = run_mode(mode, args.params, args.rounds, 64, args.settle_ms, args.passes)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
