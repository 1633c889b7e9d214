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
them as one profile.  No GPU: fails.

--bf16 measures the mixed-precision SGD iteration instead (csrc/choco_quant_round_bf16.hip: bfloat16 models and
gradients over fp32 x, x_hat, s and momentum) on the 8-row shape, at 8 and 4 bits, with momentum 0.9 and with
none, three contenders alternating in one process: "mixed", that launch; "fp32", the fp32 one-launch iteration;
"wrapper", what a bfloat16 trainer would put around the fp32 launch -- widen the bfloat16 gradients into the fp32
gradient arena, the fp32 launch, cast x into the bfloat16 models, zero the bfloat16 gradients (three torch
launches more).  Bytes per parameter of the mixed launch: g 2 + 2, m 8, x 8, x_hat 8, s 8, p 2 = 38 (30 without
momentum), + 1/64 for the norms."""
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


def figure_bf16(P, bits, mom, min_s, alternations):
    GP = pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)
    kw = dict(compressor="quant", bits=bits, one_launch=True)
    fp32, wrapped = build(GP, P, False, **kw), build(GP, P, False, **kw)
    mixed = pkg.ChocoWorkerGroup(GP, numel=P, consensus_lr=0.1, dtype=torch.bfloat16, **kw)
    mixed.rows.copy_(fp32.rows)                      # build() fills fp32 rows: the models are their image
    mixed.master_from_rows()
    for g in (mixed, fp32, wrapped):
        g.attach_sgd(momentum=mom, weight_decay=5e-4)
    gb, pb = torch.zeros_like(mixed.grad_arena), torch.zeros_like(mixed.arena)   # the wrapper's bfloat16 side

    def wrapper(it):
        wrapped.grad_arena.copy_(gb)
        wrapped.sgd_step(it, LR)
        pb.copy_(wrapped.x)
        gb.zero_()

    fns = {"mixed": lambda it: mixed.sgd_step(it, LR), "fp32": lambda it: fp32.sgd_step(it, LR), "wrapper": wrapper}
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
    n, nbytes = mixed.n_local, (38 if mom else 30) + 1 / 64
    out = {"shape": f"{n} x {P}", "bits": bits, "momentum": mom, "calls_per_timing": reps}
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
        out[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 4)
    out["mixed_over_fp32"] = round(out["mixed_ms"] / out["fp32_ms"], 4)
    out["mixed_over_wrapper"] = round(out["mixed_ms"] / out["wrapper_ms"], 4)
    out["mixed_bytes_per_param"] = nbytes
    out["mixed_TB_per_s"] = round(nbytes * n * P / (out["mixed_ms"] * 1e-3) / 1e12, 3)
    out["fp32_TB_per_s"] = round((nbytes + 2) * n * P / (out["fp32_ms"] * 1e-3) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    ap.add_argument("--bf16", action="store_true", help="the mixed-precision SGD iteration against the fp32 one-launch "
                    "iteration and the unfused wrapper around it")
    ap.add_argument("--out", default=None, help="also write the shapes as one JSON profile to this path")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_quant_round: no GPU -- nothing is measured without one")
    shapes = []
    for one_row in () if a.bf16 else (False, True):
        shapes.append(figure(a.numel, one_row, a.min_seconds, a.alternations))
        print(json.dumps(shapes[-1]), flush=True)
    for bits, mom in ((8, 0.9), (4, 0.9), (8, 0.0), (4, 0.0)) if a.bf16 else ():
        shapes.append(figure_bf16(a.numel, bits, mom, a.min_seconds, a.alternations))
        print(json.dumps(shapes[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": f"tools/bench_choco_quant_round.py{' --bf16' if a.bf16 else ''} (P = {a.numel}, "
                               f">= {a.min_seconds} s per timing, "
                               f"{a.alternations} alternations)", "device": torch.cuda.get_device_name(0),
                       "shapes": shapes}, f, indent=1)


if __name__ == "__main__":
    main()
