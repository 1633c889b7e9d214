"""ms per ChocoSGD round with the bucketed stochastic quantizer at 8 and 4 bits, the scaled-sign compressor and
top-1 % (ratio 0.99), on bench.py's Choco shape (8 x 14,774,436, graph 0, every matching active) and on one row
of it (a rank's share at N = 8, null transport, stand-in partner messages).  One process: a warm-up and a
settle burst, then the four contenders alternating, each timing from device events around at least MIN_S
seconds of rounds; the median over the alternations is reported.  The compress and apply launches of the two
quantizers and of the sign compressor are also timed alone, alternating, and given as TB/s of the bytes the
algorithm needs, from shapes: per parameter 8 + b/8 + 1/64 for a compress pass (x, x_hat in, codes and norms
out; sign: 8 + 1/8) and 24 + (deg + 1)(b/8 + 1/64) for an apply pass (x, x_hat, s in and out, the messages of
deg partners and the row's own; sign: 24 + (deg + 1)/8).  The yardstick of a quantizer launch is the sign
launch of the same run.  One JSON line per shape.  No GPU: fails."""
import argparse
import json
import sys

import numpy as np
import torch

from bench_choco_sign import T, build, pkg, reps_for, timed


def figure(P, one_row, min_s, alternations):
    GP = pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)     # budget 1: every matching, every round
    groups = {"quant8": build(GP, P, one_row, compressor="quant", bits=8),
              "quant4": build(GP, P, one_row, compressor="quant", bits=4),
              "sign": build(GP, P, one_row, compressor="sign"), "topk": build(GP, P, one_row, ratio=0.99)}
    for g in groups.values():                        # warm-up, then a settle burst
        for it in range(10):
            g.step(it)
    torch.cuda.synchronize()
    for g in groups.values():
        timed(g.step, 50)
    reps = {k: reps_for(g.step, min_s) for k, g in groups.items()}
    ms = {k: [] for k in groups}
    for _ in range(alternations):
        for k, g in groups.items():
            ms[k].append(timed(g.step, reps[k]))
    groups["topk"].check_topk()
    sign = groups["sign"]
    partner = np.asarray(sign.topology.neighbors_info)           # as placed: local row r is column row_base + r
    deg = float(np.mean([(partner[:, sign.row_base + r] >= 0).sum() for r in range(sign.n_local)]))
    n = sign.n_local
    per_param = {k: (1 / 8 if k == "sign" else groups[k].bits / 8 + 1 / 64) for k in ("quant8", "quant4", "sign")}
    launches = {(k, p): getattr(groups[k], p) for k in per_param for p in ("compress", "average")}
    lreps = {kp: reps_for(fn, min_s) for kp, fn in launches.items()}
    lms = {kp: [] for kp in launches}
    for _ in range(alternations):
        for kp, fn in launches.items():
            lms[kp].append(timed(fn, lreps[kp]))
    out = {"shape": f"{n} x {P}", "mean_degree": deg, "rounds_per_timing": reps,
           "wire_bytes_per_message": {k: 12 * int(g.k) if k == "topk" else int(g.msg_bytes) for k, g in groups.items()}}
    for k in groups:
        out[k + "_round_ms"] = round(float(np.median(ms[k])), 4)
        out[k + "_round_ms_all"] = [round(v, 4) for v in ms[k]]
    for (k, p), v in lms.items():
        nbytes = 8 + per_param[k] if p == "compress" else 24 + (deg + 1) * per_param[k]
        med = float(np.median(v))
        out[f"{k}_{'compress' if p == 'compress' else 'apply'}"] = {
            "ms": round(med, 4), "ms_all": [round(x, 4) for x in v], "bytes_per_param": round(nbytes, 4),
            "TB_per_s": round(nbytes * n * P / (med * 1e-3) / 1e12, 3),
            "TB_per_s_all": [round(nbytes * n * P / (x * 1e-3) / 1e12, 3) for x in v]}
    for k in ("quant8", "quant4"):
        for p in ("compress", "apply"):
            out[f"{k}_{p}_over_sign_rate"] = round(out[f"{k}_{p}"]["TB_per_s"] / out[f"sign_{p}"]["TB_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_quant: no GPU -- nothing is measured without one")
    for one_row in (False, True):
        print(json.dumps(figure(a.numel, one_row, a.min_seconds, a.alternations)), flush=True)


if __name__ == "__main__":
    main()
