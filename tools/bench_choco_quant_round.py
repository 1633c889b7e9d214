"""ms per quantized ChocoSGD round, and per SGD iteration (step + round, momentum 0.9, zero_grads), in the two
forms of compressor="quant": the two launches (compress, apply; with SGD a step launch in front) and
one_launch=True (csrc/choco_quant_round.hip), at 8 and 4 bits; the sign round and the top-1 % round of the same
run as context.  Shapes: bench.py's Choco shape (8 x 14,774,436, graph 0, every matching active) and one row of
it as a one-worker group (nranks = 1, no partner: the row applies its own message -- the one-launch form needs
every partner on this GPU, so this is not tools/bench_choco_quant.py's one-row share with stand-in partners).
One process: a warm-up and a settle burst, then the contenders alternating, each timing from device events
around at least MIN_S seconds of work; the median over the alternations is reported.  The yardstick of a
one-launch figure is the two-launch contender of the same run.  TB/s are the bytes the algorithm needs, from
shapes, over the time: 24 + 1/64 per parameter for a one-launch round (x, x_hat, s in and out, the norms out), 44
for an iteration (g and m in, m and the zeros over g out, on top).  One JSON line per shape; --out also writes
them as one profile.  No GPU: fails."""
import argparse
import json
import sys

import numpy as np
import torch

from bench_choco_sign import T, build, pkg, reps_for, timed

LR = 0.01


class OneWorker:
    """a processor of one worker with no partner: what ChocoWorkerGroup reads of a topology"""
    size, neighbors_info, neighbor_weight = 1, [[-1]], 0.5
    active_flags = [[1]] * T


def figure(P, one_row, min_s, alternations):
    GP = OneWorker() if one_row else pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)
    groups = {f"{form}{bits}": build(GP, P, False, compressor="quant", bits=bits, one_launch=form == "one")
              for bits in (8, 4) for form in ("two", "one")}
    for g in groups.values():
        g.attach_sgd(momentum=0.9, weight_decay=5e-4)
    fns = {k + "_round": g.step for k, g in groups.items()}
    fns.update({k + "_sgd": (lambda it, g=g: g.sgd_step(it, LR)) for k, g in groups.items()})
    if not one_row:                                  # context: the other two compressors' rounds
        fns["sign_round"] = build(GP, P, False, compressor="sign").step
        topk = build(GP, P, False, ratio=0.99)
        fns["topk_round"] = topk.step
    for fn in fns.values():                          # warm-up, then a settle burst
        for it in range(10):
            fn(it)
    torch.cuda.synchronize()
    for fn in fns.values():
        timed(fn, 50)
    reps = {k: reps_for(fn, min_s) for k, fn in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(alternations):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps[k]))
    if not one_row:
        topk.check_topk()
    n = groups["one8"].n_local
    out = {"shape": f"{n} x {P}", "calls_per_timing": reps}
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
        out[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 4)
    for bits in (8, 4):
        for what, nbytes in (("round", 24 + 1 / 64), ("sgd", 44 + 1 / 64)):
            one, two = out[f"one{bits}_{what}_ms"], out[f"two{bits}_{what}_ms"]
            out[f"one{bits}_{what}_over_two"] = round(one / two, 4)
            out[f"one{bits}_{what}_TB_per_s"] = round(nbytes * n * P / (one * 1e-3) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    ap.add_argument("--out", default=None, help="also write the shapes as one JSON profile to this path")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_quant_round: no GPU -- nothing is measured without one")
    shapes = []
    for one_row in (False, True):
        shapes.append(figure(a.numel, one_row, a.min_seconds, a.alternations))
        print(json.dumps(shapes[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": f"tools/bench_choco_quant_round.py (P = {a.numel}, >= {a.min_seconds} s per timing, "
                               f"{a.alternations} alternations)", "device": torch.cuda.get_device_name(0),
                       "shapes": shapes}, f, indent=1)


if __name__ == "__main__":
    main()
