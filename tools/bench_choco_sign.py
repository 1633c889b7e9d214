"""ms per ChocoSGD round with the scaled-sign compressor and with top-1 % (ratio 0.99), on bench.py's Choco
shape (8 x 14,774,436, graph 0, every matching active) and on one row of it (a rank's share at N = 8, null
transport, stand-in partner messages).  One process: a warm-up and a settle burst, then the two compressors
alternating, each timing from device events around at least MIN_S seconds of rounds; the median over the
alternations is reported.  The sign round's two passes are also timed alone and given as TB/s of the bytes
the algorithm needs, from shapes: 8 + 1/8 per parameter for the compress pass (x, x_hat in, bits out),
24 + (deg + 1) / 8 for the apply pass (x, x_hat, s in and out, the bits of deg partners and the row's own).
One JSON line per shape.  No GPU: fails."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
from nullcomm import NullComm  # noqa: E402

T = 64                     # schedule rows (every matching active in each)


def build(GP, P, one_row, **kw):
    if not one_row:
        g = pkg.ChocoWorkerGroup(GP, numel=P, consensus_lr=0.1, **kw)
        for i in range(g.n_local):
            pkg._lib.check(pkg.lib.mx_synth_fill(g.rows[i].data_ptr(), P, 1234 + i, None))
        return g
    g = pkg.ChocoWorkerGroup(GP, numel=P, consensus_lr=0.1, rank=0, nranks=8, comm=NullComm(0, 8), placement="auto",
                             **kw)
    for s in range(g.n_local, g.engine.n_slots):      # partner stand-ins: messages of other synthetic rows
        pkg._lib.check(pkg.lib.mx_synth_fill(g.rows[0].data_ptr(), P, 7000 + s, None))
        g.compress(0)
        torch.cuda.synchronize()
        g.msgs[s * g.msg_ld:(s + 1) * g.msg_ld].copy_(g.msgs[:g.msg_ld])
    pkg._lib.check(pkg.lib.mx_synth_fill(g.rows[0].data_ptr(), P, 1234 + g.workers[0], None))
    if not g.sign:
        g.work.zero_()
    return g


def timed(fn, reps):
    """ms per call of fn(it) over `reps` calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for it in range(reps):
        fn(it % T)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def reps_for(fn, min_s):
    """calls of fn that fill min_s seconds, from a 20-call probe"""
    ms = timed(fn, 20)
    return max(20, int(np.ceil(1e3 * min_s / ms)))


def figure(P, one_row, min_s, alternations):
    GP = pkg.MatchaProcessor(pkg.select_graph(0), 1.0, 0, 8, T, True)     # budget 1: every matching, every round
    sign = build(GP, P, one_row, compressor="sign")
    topk = build(GP, P, one_row, ratio=0.99)
    for g in (sign, topk):                           # warm-up, then a settle burst
        for it in range(10):
            g.step(it)
    torch.cuda.synchronize()
    for g in (sign, topk):
        timed(g.step, 50)
    rs, rt = reps_for(sign.step, min_s), reps_for(topk.step, min_s)
    ms = {"sign": [], "topk": []}
    for _ in range(alternations):
        ms["sign"].append(timed(sign.step, rs))
        ms["topk"].append(timed(topk.step, rt))
    topk.check_topk()
    comp = timed(sign.compress, reps_for(sign.compress, min_s))
    app = timed(sign.average, reps_for(sign.average, min_s))
    partner = np.asarray(sign.topology.neighbors_info)           # as placed: local row r is column row_base + r
    deg = float(np.mean([(partner[:, sign.row_base + r] >= 0).sum() for r in range(sign.n_local)]))
    n = sign.n_local
    comp_bytes, app_bytes = 8 + 1 / 8, 24 + (deg + 1) / 8
    s_ms, t_ms = float(np.median(ms["sign"])), float(np.median(ms["topk"]))
    return {"shape": f"{n} x {P}", "rounds_per_timing": {"sign": rs, "topk": rt},
            "sign_round_ms": round(s_ms, 4), "sign_round_ms_all": [round(v, 4) for v in ms["sign"]],
            "topk_round_ms": round(t_ms, 4), "topk_round_ms_all": [round(v, 4) for v in ms["topk"]],
            "sign_over_topk": round(s_ms / t_ms, 3),
            "wire_bytes_per_message": {"sign": int(sign.msg_bytes), "topk": 12 * int(topk.k)},
            "mean_degree": deg,
            "compress": {"ms": round(comp, 4), "bytes_per_param": comp_bytes,
                         "TB_per_s": round(comp_bytes * n * P / (comp * 1e-3) / 1e12, 3)},
            "apply": {"ms": round(app, 4), "bytes_per_param": round(app_bytes, 4),
                      "TB_per_s": round(app_bytes * n * P / (app * 1e-3) / 1e12, 3)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--numel", default=14_774_436, type=int)
    ap.add_argument("--min-seconds", default=0.5, type=float, help="device time each timing covers at least")
    ap.add_argument("--alternations", default=3, type=int)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_choco_sign: no GPU -- nothing is measured without one")
    for one_row in (False, True):
        print(json.dumps(figure(a.numel, one_row, a.min_seconds, a.alternations)), flush=True)


if __name__ == "__main__":
    main()
