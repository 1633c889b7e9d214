"""ms per AdamW training iteration of the one-launch quantized ChocoSGD round (csrc/choco_quant_adamw_round.hip:
step + zero_grad + quantizer + round in one launch) at bench.py's Choco shape (8 x 14,774,436, graph 0, every
matching active), at 8 and 4 bits, three contenders alternating in one process:
    "fused"    ChocoWorkerGroup.attach_adamw / adamw_step, the one launch;
    "unfused"  torch.optim.AdamW(foreach=True) over the same rows + zero_grad, then the one-launch round
               (ChocoWorkerGroup.step): the best a trainer can do without the fused step;
    "sgd"      the one-launch SGD iteration with momentum 0.9 (attach_sgd / sgd_step), 40 bytes per parameter.
A warm-up and a settle burst, then each timing from device events around at least MIN_S seconds of back-to-back
calls; the median over the alternations and the spread (max - min) / median are reported.  Bytes the algorithm
needs per parameter, from shapes: x, x_hat, s, m, v in and out and g in and zeroed = 48 (+ 1/64 for the norms).
One JSON line per bit width; --out also writes them as one profile.  No GPU: fails.

--bf16 measures the mixed-precision forms (bfloat16 models and gradients; csrc/choco_quant_adamw_round_bf16.hip, 46
bytes; the SGD iteration 38): "unfused" is then the widening of the bfloat16 gradients into an fp32 arena, foreach
AdamW on the fp32 masters, the one-launch bfloat16 round (which rewrites the models) and the zeroing of the
bfloat16 gradients."""
import argparse
import json
import sys

import numpy as np
import torch

from bench_choco_sign import T, build, pkg, reps_for, timed

LR = 1e-3


def figure(P, bits, bf16, min_s, alternations):
    GP = pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)
    kw = dict(compressor="quant", bits=bits, one_launch=True)
    src = build(GP, P, False, **kw)                  # build() fills fp32 rows

    def group():
        if not bf16:
            return build(GP, P, False, **kw)
        g = pkg.ChocoWorkerGroup(GP, numel=P, consensus_lr=0.1, dtype=torch.bfloat16, **kw)
        g.rows.copy_(src.rows)
        g.master_from_rows()
        return g

    fused, plain, sgd = group(), group(), group()
    del src
    fused.attach_adamw(weight_decay=1e-2)
    sgd.attach_sgd(momentum=0.9, weight_decay=5e-4)
    # the unfused contender: torch's AdamW on views of the group's fp32 rows, their gradients views of one arena
    g32 = torch.zeros_like(plain.x)
    gb = torch.zeros_like(plain.arena) if bf16 else None
    params = [torch.nn.Parameter(plain.x[r, :P]) for r in range(plain.n_local)]
    for r, p in enumerate(params):
        p.grad = g32[r, :P]
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=1e-2, foreach=True)

    def unfused(it):
        if bf16:
            g32.copy_(gb)
        opt.step()
        opt.zero_grad(set_to_none=False)
        plain.step(it)
        if bf16:
            gb.zero_()

    fns = {"fused": lambda it: fused.adamw_step(it, LR), "unfused": unfused, "sgd": lambda it: sgd.sgd_step(it, LR)}
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
    n, nbytes, sgd_bytes = fused.n_local, (46 if bf16 else 48) + 1 / 64, (38 if bf16 else 40) + 1 / 64
    out = {"shape": f"{n} x {P}", "bits": bits, "bf16": bool(bf16), "calls_per_timing": reps}
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
        out[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 4)
    out["fused_over_sgd"] = round(out["fused_ms"] / out["sgd_ms"], 4)
    out["bytes_fused_over_sgd"] = round(nbytes / sgd_bytes, 4)
    out["fused_over_unfused"] = round(out["fused_ms"] / out["unfused_ms"], 4)
    out["fused_TB_per_s"] = round(nbytes * n * P / (out["fused_ms"] * 1e-3) / 1e12, 3)
    out["sgd_TB_per_s"] = round(sgd_bytes * n * P / (out["sgd_ms"] * 1e-3) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    ap.add_argument("--bf16", action="store_true", help="the mixed-precision forms (bfloat16 models and gradients)")
    ap.add_argument("--out", default=None, help="also write the figures as one JSON profile to this path")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_quant_adamw_round: no GPU -- nothing is measured without one")
    shapes = []
    for bits in (8, 4):
        shapes.append(figure(a.numel, bits, a.bf16, a.min_seconds, a.alternations))
        print(json.dumps(shapes[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": f"tools/bench_choco_quant_adamw_round.py{' --bf16' if a.bf16 else ''} (P = {a.numel}, "
                               f">= {a.min_seconds} s per timing, {a.alternations} alternations)",
                       "device": torch.cuda.get_device_name(0), "shapes": shapes}, f, indent=1)


if __name__ == "__main__":
    main()
