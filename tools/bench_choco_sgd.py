"""ms per ChocoSGD ITERATION (every worker's SGD step with momentum 0.9, then the round) with the step fused
into the round and with torch's optimizer in front of it, on bench_choco_sign.py's shapes (8 x 14,774,436,
graph 0, every matching active; and one row of it) and by its method: one process, a warm-up and a settle
burst, then the contenders alternating, each timing from device events around at least MIN_S seconds; the
median over the alternations is reported, with every repeat beside it.  Contenders:
    a  sign, fused     ChocoWorkerGroup.sgd_step: the step inside the compress pass, then the apply
    b  sign, unfused   torch.optim.SGD(foreach=True).step() + zero_grad(set_to_none=False) per worker, step()
    c  topk, fused     sgd_step of a top-1 % group: the step launch, the selection, the apply
    d  topk, unfused   as b
The fused compress launch is also timed alone against the unfused compress launch, both as TB/s of the bytes
the algorithm needs, from shapes: 28 + 1/8 per parameter (x, g, m, x_hat in; x, m, g out; the bits) against
8 + 1/8.  One JSON line per shape, collected in --out.  No GPU: fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_choco_sign import ROOT, T, build, pkg, reps_for, timed  # noqa: E402

LR, MOM, WD = 0.05, 0.9, 5e-4


def torch_iteration(g):
    """contender b / d on group g: one torch optimizer per worker over a parameter that is the worker's row"""
    opts = []
    for r in range(g.n_local):
        p = torch.nn.Parameter(g.rows[r])
        p.grad = torch.zeros_like(p)
        opts.append(torch.optim.SGD([p], lr=LR, momentum=MOM, weight_decay=WD, foreach=True))

    def run(it):
        for o in opts:
            o.step()
            o.zero_grad(set_to_none=False)
        g.step(it)
    return run


def figure(P, one_row, min_s, alternations):
    GP = pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)     # budget 1: every matching, every round
    fns = {}
    groups = {}
    for name, kw in (("sign", dict(compressor="sign")), ("topk", dict(ratio=0.99))):
        fused, plain = build(GP, P, one_row, **kw), build(GP, P, one_row, **kw)
        fused.attach_sgd(MOM, WD)
        fns[name + "_fused"] = lambda it, g=fused: g.sgd_step(it, LR)
        fns[name + "_unfused"] = torch_iteration(plain)
        groups[name] = (fused, plain)
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
    for fused, plain in groups.values():
        fused.check_topk()
        plain.check_topk()
    sf, sp = groups["sign"]
    n = sf.n_local
    alone = {"fused": [], "unfused": []}
    fc, uc = (lambda it: sf.sgd_compress(LR)), sp.compress
    rf, ru = reps_for(fc, min_s), reps_for(uc, min_s)
    for _ in range(alternations):
        alone["fused"].append(timed(fc, rf))
        alone["unfused"].append(timed(uc, ru))
    out = {"shape": f"{n} x {P}", "momentum": MOM, "iterations_per_timing": reps}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k in fns:
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_ms_all"] = [round(v, 4) for v in ms[k]]
    for name in ("sign", "topk"):
        out[name + "_fused_over_unfused"] = round(med[name + "_fused"] / med[name + "_unfused"], 3)
    for k, bpp in (("fused", 28 + 1 / 8), ("unfused", 8 + 1 / 8)):
        m = float(np.median(alone[k]))
        out["compress_" + k] = {"ms": round(m, 4), "ms_all": [round(v, 4) for v in alone[k]], "bytes_per_param": bpp,
                                "TB_per_s": round(bpp * n * P / (m * 1e-3) / 1e12, 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "choco_sgd_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_sgd: no GPU -- nothing is measured without one")
    results = []
    for one_row in (False, True):
        results.append(figure(a.numel, one_row, a.min_seconds, a.alternations))
        print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_choco_sgd.py", "device": torch.cuda.get_device_name(0), "shapes": results}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
