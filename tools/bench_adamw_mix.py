"""The AdamW update fused into the gossip round against the unfused best case and against the fused SGD
step, on the headline shape, in ONE process: graph 0, 8 workers x 25.6M fp32 parameters, every matching
active, betas (0.9, 0.999), eps 1e-8, decoupled weight decay 1e-2.  Each figure is taken after a settle
burst sized with bench.settle_rounds, as K back-to-back steps between one HIP event pair, in two passes
whose order alternates:

  (a) fused       VirtualWorkerGroup.adamw_step: one launch (a_zero: the same with zero_grads)
  (b) unfused     torch.optim.AdamW's op sequence applied ONCE to the whole [8, ld] arenas (p.mul_,
                  exp_avg.lerp_, exp_avg_sq.mul_, .addcmul_, sqrt, / bc2_sqrt, + eps, p.addcdiv_: 8
                  launches), then group.step
  (c) fused SGD   VirtualWorkerGroup.sgd_step (momentum 0.9, weight decay 5e-4) on a second group
  (d) mix         group.step alone

One JSON line (also written to profiles/adamw_mix_bench.json): ms per step (the mean of the passes, and
each pass), the TB/s that implies on the algorithmic bytes (28 / 32 per element for a / a_zero, 88 for b,
20 for c, 8 for d -- all 8 rows are active), the (b)/(a) time ratio next to the 88/28 = 3.14 the byte
count predicts, and rate(a)/rate(c).  First, 64 sampled columns of three fused steps are checked against
the specification (tests/adamref.py); a failed check withholds the rates, as bench.py does.

    python tools/bench_adamw_mix.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--ab]

--ab also times the kernel's knobs (mx_adamw_mix_set: streaming hints, workgroups-per-CU cap, persistent
grid), each settled the same way, over --reps passes in alternating order, under "ab".
"""
import argparse
import ctypes
import importlib
import json
import math
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
from adamref import bias_table, spec_round  # noqa: E402
from conftest import Topo  # noqa: E402

L = pkg.lib
N = 8
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 1e-2, 1e-3
HYPER = (B1, B2, EPS, WD, True)
SGD_WD, SGD_MOM = 5e-4, 0.9


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=25_600_000)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_mix_bench.json"))
    args = ap.parse_args()
    P, K, T = args.params, args.rounds, 64
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    alpha = 2 / 7
    ones = np.ones(partner.shape[0], np.uint8)
    topo = Topo(partner, alpha, np.ones((T, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=P)
    grp.attach_adamw(betas=(B1, B2), eps=EPS, weight_decay=WD, zero_grads=False)

    def fill_grads(g):
        for r in range(N):
            pkg._lib.check(L.mx_synth_fill(g.grads[r].data_ptr(), P, 4321 + r, None))

    for r in range(N):
        pkg._lib.check(L.mx_synth_fill(grp.rows[r].data_ptr(), P, 1234 + r, None))
    fill_grads(grp)
    lay = grp._adamw[0]
    call_zero = lay.call(grp.engine, (B1, B2), EPS, WD, True, True)
    table = bias_table(B1, B2)

    # the check first: 64 columns spread over the row (both ends and a tile edge included)
    cols_h = np.linspace(0, P - 1, 64).astype(np.int64)
    cols_h[1] = min(P - 1, lay.tile - 1)
    cols = torch.from_numpy(cols_h).cuda()

    def sample():
        return [t.index_select(1, cols).cpu().numpy()
                for t in (grp.rows, grp.grads, grp.exp_avg_rows, grp.exp_avg_sq_rows)]

    ok = True
    for it in range(3):
        X, G, Mo, V = sample()
        grp.adamw_step(it, LR)
        wx, wm, wv, _ = spec_round(O, X, G, Mo, V, it + 1, partner, ones, alpha, LR, HYPER, table)
        gx, gg, gm, gv = sample()
        ok = ok and all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                        for a, b in ((gx, wx), (gm, wm), (gv, wv), (gg, G)))
    out = {"tool": "bench_adamw_mix", "graph": 0, "workers": N, "params": P, "rounds": K, "settle_ms": args.settle_ms,
           "passes": args.passes,
           "hyper": {"lr": LR, "betas": [B1, B2], "eps": EPS, "weight_decay": WD, "decoupled": True},
           "sgd_hyper": {"weight_decay": SGD_WD, "momentum": SGD_MOM},
           "device": torch.cuda.get_device_properties(0).gcnArchName, "fused_check_64_columns": ok,
           "knobs": pkg.engine.adamw_mix_tuning()}
    if not ok:
        out["withheld"] = "the fused step differs from the specification: no rate is reported"
        print(json.dumps(out), flush=True)
        return 1

    sgd = pkg.VirtualWorkerGroup(topo, numel=P)
    sgd.attach_sgd(momentum=SGD_MOM, weight_decay=SGD_WD, zero_grads=False)
    for r in range(N):
        pkg._lib.check(L.mx_synth_fill(sgd.rows[r].data_ptr(), P, 1234 + r, None))
    fill_grads(sgd)

    x, g, m, v = grp.arena, grp.grad_arena, grp.exp_avg_arena, grp.exp_avg_sq_arena
    s = pkg._lib.stream_ptr
    zstep = [0]

    def fused(j):
        grp.adamw_step(j % T, LR)

    def fused_zero(j):
        zstep[0] += 1
        pkg._lib.check(L.mx_adamw_mix(ctypes.addressof(call_zero), j % T, zstep[0], LR, None, s()), "mx_adamw_mix")

    def unfused(j):
        t = j + 1
        x.mul_(1 - LR * WD)
        m.lerp_(g, 1 - B1)
        v.mul_(B2).addcmul_(g, g, value=1 - B2)
        denom = (v.sqrt() / math.sqrt(1 - B2 ** t)).add_(EPS)
        x.addcdiv_(m, denom, value=-LR / (1 - B1 ** t))
        grp.step(j % T)

    def fused_sgd(j):
        sgd.sgd_step(j % T, LR)

    def mix(j):
        grp.step(j % T)

    elems = N * P
    entries = [("a_fused", fused, 28), ("b_unfused", unfused, 88), ("c_fused_sgd", fused_sgd, 20), ("d_mix", mix, 8),
               ("a_zero_fused_zero_grads", fused_zero, 32)]
    ms = {name: [] for name, _, _ in entries}
    for rep in range(args.passes):
        for name, step, per_elem in (entries if rep % 2 == 0 else entries[::-1]):
            settle = bench.settle_rounds(per_elem * elems, args.settle_ms)
            ms[name].append(round(timed(step, settle, K), 5))
            if name == "a_zero_fused_zero_grads":    # the gradients back, for the entries that follow
                fill_grads(grp)
    res = {}
    for name, _, per_elem in entries:
        nbytes = per_elem * elems
        mean = sum(ms[name]) / len(ms[name])
        res[name] = {"ms_per_step": round(mean, 5), "ms_per_step_passes": ms[name], "algorithmic_bytes": nbytes,
                     "bytes_per_element": per_elem, "settle_rounds": bench.settle_rounds(nbytes, args.settle_ms),
                     "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4)}
    out.update(res)
    out["speedup_b_over_a"] = round(res["b_unfused"]["ms_per_step"] / res["a_fused"]["ms_per_step"], 4)
    out["speedup_b_over_a_predicted_by_bytes"] = round(88 / 28, 4)
    out["rate_ratio_a_over_c"] = round(res["a_fused"]["tb_per_s"] / res["c_fused_sgd"]["tb_per_s"], 4)
    out["rate_ratio_a_over_d"] = round(res["a_fused"]["tb_per_s"] / res["d_mix"]["tb_per_s"], 4)
    if args.ab:
        saved = pkg.engine.adamw_mix_tuning()
        variants = [("default", {}), ("nt0", {"nontemporal": 0}), ("nt1", {"nontemporal": 1})] + \
                   [(f"wgpc{w}", {"wgpc": w}) for w in (3, 4, 5, 6, 8)] + \
                   [(f"persistent_bpc{b}", {"flat_small": 0, "blocks_per_cu": b}) for b in (2, 4, 8)]
        settle = bench.settle_rounds(28 * elems, args.settle_ms)
        ab = {name: [] for name, _ in variants}
        for rep in range(args.reps):
            for name, knobs in (variants if rep % 2 == 0 else variants[::-1]):
                pkg.engine.set_adamw_mix_tuning(**{**saved, **knobs})
                ab[name].append(round(timed(fused, settle, K), 5))
        pkg.engine.set_adamw_mix_tuning(**saved)
        out["ab"] = {"ms_per_step": ab, "note": "fused step (28 B/element), each entry settled then timed over "
                     "`rounds` steps; passes run in alternating order"}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
