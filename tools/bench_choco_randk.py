"""ms per compress() and per ChocoSGD round with rand-k against top-k at the same ratio (0.99), on bench.py's Choco
shape (8 x 14,774,436, graph 0, every matching active) and on one row of it (a rank's share at N = 8, null
transport, stand-in partner messages).  One process: a warm-up and a settle burst, then the two compressors
alternating, each timing from device events around at least MIN_S seconds of calls; the median over the
alternations is reported.  rand-k's compress is also timed at denser messages (--ratios), beside the sign
compressor's streaming pass over the same rows: where gathering the selected columns stops paying.  One JSON
line per shape.  No GPU: fails."""
import argparse
import json
import sys

import numpy as np
import torch

from bench_choco_sign import T, build, pkg, reps_for, timed


def figure(P, one_row, min_s, alternations, ratios):
    GP = pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)     # budget 1: every matching, every round
    groups = {"randk": build(GP, P, one_row, compressor="randk", ratio=0.99),
              "topk": build(GP, P, one_row, ratio=0.99)}
    calls = {(k, what): getattr(g, what) for k, g in groups.items() for what in ("compress", "step")}
    for fn in calls.values():                            # warm-up, then a settle burst
        timed(fn, 10)
    for fn in calls.values():
        timed(fn, 50)
    reps = {kw: reps_for(fn, min_s) for kw, fn in calls.items()}
    ms = {kw: [] for kw in calls}
    for _ in range(alternations):
        for kw, fn in calls.items():
            ms[kw].append(timed(fn, reps[kw]))
    groups["topk"].check_topk()
    out = {"shape": f"{groups['randk'].n_local} x {P}", "ratio": 0.99, "k": int(groups["randk"].k)}
    for (k, what), v in ms.items():
        name = f"{k}_{'compress' if what == 'compress' else 'round'}_ms"
        out[name], out[name + "_all"] = round(float(np.median(v)), 4), [round(x, 4) for x in v]
    for what in ("compress", "round"):
        out[f"topk_over_randk_{what}"] = round(out[f"topk_{what}_ms"] / out[f"randk_{what}_ms"], 2)
    del groups, calls
    dense = {"sign": build(GP, P, one_row, compressor="sign").compress}
    dense.update({str(r): build(GP, P, one_row, compressor="randk", ratio=r).compress for r in ratios})
    for fn in dense.values():
        timed(fn, 20)
    out["compress_ms_by_ratio"] = {k: round(timed(fn, reps_for(fn, min_s)), 4) for k, fn in dense.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    ap.add_argument("--ratios", default="0.99,0.9,0.75,0.5,0.0", help="rand-k ratios of the density sweep")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_randk: no GPU -- nothing is measured without one")
    for one_row in (False, True):
        print(json.dumps(figure(a.numel, one_row, a.min_seconds, a.alternations,
                                [float(r) for r in a.ratios.split(",")])), flush=True)


if __name__ == "__main__":
    main()
