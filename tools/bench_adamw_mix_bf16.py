"""Mixed-precision AdamW fused into the bf16 gossip round against the unfused sequence, against the fp32
fused AdamW step and against the mixed-precision fused SGD step, on the headline shape, in ONE process:
graph 0, 8 workers x 25.6M parameters, every matching active, betas (0.9, 0.999), eps 1e-8, decoupled
weight decay 1e-2.  Timed, each after a settle burst sized with bench.settle_rounds, as K back-to-back
steps between one HIP event pair:

  (a) fused       VirtualWorkerGroup(dtype=bfloat16).attach_adamw(master_weights=True).adamw_step: one
                  launch (a_zero: the same with zero_grads)
  (b) unfused     the op sequence the launch replaces, run ONCE over whole [8, ld] arenas: g32 = g.float();
                  torch.optim.AdamW's eight single-tensor ops on fp32 masters (p.mul_, exp_avg.lerp_,
                  exp_avg_sq.mul_, .addcmul_, sqrt, / bc2_sqrt, + eps, p.addcdiv_); the fp32 group.step of
                  the masters; p.copy_(w) (fp32 read, bf16 write)
  (c) fused fp32  the fp32 group's adamw_step (csrc/adamw_mix.hip)
  (d) fused SGD   the bfloat16 group's mixed-precision sgd_step (csrc/sgd_mix_bf16.hip; momentum 0.9,
                  weight decay 5e-4)

Every figure is timed in --passes passes (default 2) in alternating order; both passes are reported,
the headline ratios use their means and "spread" is (max - min) / mean over the passes.  One JSON line
(also written to profiles/adamw_mix_bf16_bench.json): ms per step, the TB/s that implies on the
algorithmic bytes (28 / 30 per element for a / a_zero, 100 for b, 28 for c, 20 for d), the (b)/(a) time
ratio next to the 100/28 = 3.57 the byte count predicts, rate(a)/rate(c) and rate(a)/rate(d).  First, 64
sampled columns of three fused mixed-precision steps are checked against the specification
(tests/adambf16ref.py); a failed check withholds the rates, as bench.py does.

    python tools/bench_adamw_mix_bf16.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--ab]

--ab also times the kernel's knobs (mx_adamw_mix_bf16_set: streaming hints, workgroups-per-CU cap,
persistent grid), each settled the same way, over --reps passes in alternating order, under "ab".
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
import bf16ref  # noqa: E402
import oracle as O  # noqa: E402
from adambf16ref import spec_round  # noqa: E402
from adamref import bias_table  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_mix_bf16_bench.json"))
    args = ap.parse_args()
    P, K, T = args.params, args.rounds, 64
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    alpha = 2 / 7
    ones = np.ones(partner.shape[0], np.uint8)
    topo = Topo(partner, alpha, np.ones((T, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16)
    grp.attach_adamw(betas=(B1, B2), eps=EPS, weight_decay=WD, zero_grads=False, master_weights=True)
    f32 = pkg.VirtualWorkerGroup(topo, numel=P)
    f32.attach_adamw(betas=(B1, B2), eps=EPS, weight_decay=WD, zero_grads=False)
    sgd = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16)
    sgd.attach_sgd(momentum=SGD_MOM, weight_decay=SGD_WD, zero_grads=False, master_weights=True)
    m_u, v_u = torch.zeros_like(f32.arena), torch.zeros_like(f32.arena)    # the unfused sequence's Adam state

    def fill():
        """masters, gradients and optimizer state of all the groups: the same synthetic values (the bf16
        gradients are the fp32 group's, rounded), zero Adam / momentum state, step 0"""
        for r in range(N):
            pkg._lib.check(L.mx_synth_fill(f32.rows[r].data_ptr(), P, 1234 + r, None))
            pkg._lib.check(L.mx_synth_fill(f32.grads[r].data_ptr(), P, 4321 + r, None))
        with torch.no_grad():
            for g in (grp, sgd):
                g.master_rows.copy_(f32.rows)
                g.grads.copy_(f32.grads)
            for t in (grp.exp_avg_arena, grp.exp_avg_sq_arena, f32.exp_avg_arena, f32.exp_avg_sq_arena,
                      sgd.mom_arena, m_u, v_u):
                t.zero_()
        grp.opt_step = f32.opt_step = 0

    fill()
    lay = grp._adamw[0]
    call_zero = lay.call(grp.engine, (B1, B2), EPS, WD, True, True)
    table = bias_table(B1, B2)

    # the check first: 64 columns spread over the row (both ends and a tile edge included)
    cols_h = np.linspace(0, P - 1, 64).astype(np.int64)
    cols_h[1] = min(P - 1, lay.tile - 1)
    cols = torch.from_numpy(cols_h).cuda()

    def sample():
        w, m, v = (t.index_select(1, cols).cpu().numpy() for t in (grp.master_rows, grp.exp_avg_rows,
                                                                   grp.exp_avg_sq_rows))
        g, p = (t.view(torch.int16).index_select(1, cols).cpu().numpy().view(np.uint16) for t in (grp.grads, grp.rows))
        return w, g, m, v, p

    ok = True
    for it in range(3):
        W, G, Mo, V, _ = sample()
        grp.adamw_step(it, LR)
        ww, wm, wv, wp, _ = spec_round(O, W, G, Mo, V, it + 1, partner, ones, alpha, LR, HYPER, table)
        gw, gg, gm, gv, gpb = sample()
        ok = ok and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in ((gw, ww), (gm, wm), (gv, wv))) \
            and np.array_equal(gg, G) and bf16ref.same_bf16(gpb, wp)
    out = {"tool": "bench_adamw_mix_bf16", "graph": 0, "workers": N, "params": P, "rounds": K,
           "settle_ms": args.settle_ms, "passes": args.passes,
           "hyper": {"lr": LR, "betas": [B1, B2], "eps": EPS, "weight_decay": WD, "decoupled": True},
           "sgd_hyper": {"weight_decay": SGD_WD, "momentum": SGD_MOM},
           "device": torch.cuda.get_device_properties(0).gcnArchName, "fused_check_64_columns": bool(ok),
           "knobs": pkg.engine.adamw_mix_bf16_tuning(), "knobs_fp32": pkg.engine.adamw_mix_tuning(),
           "knobs_sgd_bf16": pkg.engine.sgd_mix_bf16_tuning()}
    if not ok:
        out["withheld"] = "the fused step differs from the specification: no rate is reported"
        print(json.dumps(out), flush=True)
        return 1

    w, g, p = f32.arena, grp.grad_arena, grp.arena   # the unfused sequence's fp32 masters, bf16 gradients and models
    s = pkg._lib.stream_ptr
    zstep = [0]

    def fused(j):
        grp.adamw_step(j % T, LR)

    def fused_zero(j):
        zstep[0] += 1
        pkg._lib.check(L.mx_adamw_mix_bf16(ctypes.addressof(call_zero), j % T, zstep[0], LR, None, s()),
                       "mx_adamw_mix_bf16")

    def unfused(j):
        t = j + 1
        g32 = g.float()
        w.mul_(1 - LR * WD)
        m_u.lerp_(g32, 1 - B1)
        v_u.mul_(B2).addcmul_(g32, g32, value=1 - B2)
        denom = (v_u.sqrt() / math.sqrt(1 - B2 ** t)).add_(EPS)
        w.addcdiv_(m_u, denom, value=-LR / (1 - B1 ** t))
        f32.step(j % T)
        p.copy_(w)

    def fused_fp32(j):
        f32.adamw_step(j % T, LR)

    def fused_sgd(j):
        sgd.sgd_step(j % T, LR)

    elems = N * P
    figures = (("a_fused", fused, 28), ("b_unfused", unfused, 100), ("c_fused_fp32", fused_fp32, 28),
               ("d_fused_sgd_bf16", fused_sgd, 20), ("a_zero_fused_zero_grads", fused_zero, 30))
    ms = {name: [] for name, _, _ in figures}
    for rep in range(args.passes):
        for name, step, per_elem in (figures if rep % 2 == 0 else figures[::-1]):
            fill()                                   # every figure from the same finite values
            zstep[0] = 0
            settle = bench.settle_rounds(per_elem * elems, args.settle_ms)
            ms[name].append(round(timed(step, settle, K), 5))
    res = {}
    for name, _, per_elem in figures:
        nbytes = per_elem * elems
        mean = float(np.mean(ms[name]))
        res[name] = {"ms_per_step": round(mean, 5), "ms_per_step_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / mean, 4), "algorithmic_bytes": nbytes,
                     "bytes_per_element": per_elem, "settle_rounds": bench.settle_rounds(nbytes, args.settle_ms),
                     "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4)}
    out.update(res)
    out["speedup_b_over_a"] = round(res["b_unfused"]["ms_per_step"] / res["a_fused"]["ms_per_step"], 4)
    out["speedup_b_over_a_predicted_by_bytes"] = round(100 / 28, 4)
    out["rate_ratio_a_over_c"] = round(res["a_fused"]["tb_per_s"] / res["c_fused_fp32"]["tb_per_s"], 4)
    out["rate_ratio_a_over_d"] = round(res["a_fused"]["tb_per_s"] / res["d_fused_sgd_bf16"]["tb_per_s"], 4)
    if args.ab:
        saved = pkg.engine.adamw_mix_bf16_tuning()
        variants = [("default", {}), ("nt0", {"nontemporal": 0}), ("nt1", {"nontemporal": 1})] + \
                   [(f"wgpc{c}", {"wgpc": c}) for c in (3, 4, 5, 6, 8)] + \
                   [(f"persistent_bpc{b}", {"flat_small": 0, "blocks_per_cu": b}) for b in (2, 4, 8)]
        settle = bench.settle_rounds(28 * elems, args.settle_ms)
        ab = {name: [] for name, _ in variants}
        fill()
        for rep in range(args.reps):
            for name, knobs in (variants if rep % 2 == 0 else variants[::-1]):
                pkg.engine.set_adamw_mix_bf16_tuning(**{**saved, **knobs})
                ab[name].append(round(timed(fused, settle, K), 5))
        pkg.engine.set_adamw_mix_bf16_tuning(**saved)
        out["ab"] = {"ms_per_step": ab, "note": "fused mixed-precision step (28 B/element), each entry settled then "
                     "timed over `rounds` steps; passes run in alternating order"}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
