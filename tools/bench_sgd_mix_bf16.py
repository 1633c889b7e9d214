"""Mixed-precision SGD fused into the bf16 gossip round against the unfused sequence and against the
fp32 fused step, on the headline shape, in ONE process: graph 0, 8 workers x 25.6M parameters, every
matching active, weight decay 5e-4 and momentum 0.9.  Timed, each after a settle burst sized with
bench.settle_rounds, as K back-to-back steps between one HIP event pair:

  (a) fused       VirtualWorkerGroup(dtype=bfloat16).attach_sgd(master_weights=True).sgd_step: one launch
                  (a_zero: the same with zero_grads)
  (b) unfused     the op sequence the launch replaces, run ONCE over whole [8, ld] arenas:
                  g32 = g.float(); d = g32 + wd*w; buf *= mom; buf += d; w -= lr*buf (fp32 masters);
                  the fp32 group.step of the masters; p.copy_(w) (fp32 read, bf16 write)
  (c) fused fp32  the fp32 group's sgd_step (csrc/sgd_mix.hip)

Every figure is timed in --passes passes (default 2) in alternating order; both passes are reported,
the headline ratios use their means and "spread" is (max - min) / mean over the passes.  One JSON line
(also written to profiles/sgd_mix_bf16_bench.json): ms per step, the TB/s that implies on the
algorithmic bytes (20 / 22 per element for a / a_zero, 64 for b, 20 for c), speedup (b)/(a) and
rate(a)/rate(c).  First, 64 sampled columns of three fused mixed-precision steps are checked against the
specification (tests/sgdbf16ref.py); a failed check withholds the rates, as bench.py does.

    python tools/bench_sgd_mix_bf16.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--ab]

--ab also times the kernel's knobs (mx_sgd_mix_bf16_set: streaming hints, workgroups-per-CU cap,
persistent grid), each settled the same way, over --reps passes in alternating order, under "ab".
"""
import argparse
import ctypes
import importlib
import json
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
from conftest import Topo  # noqa: E402
from sgdbf16ref import spec_round  # noqa: E402

L = pkg.lib
N = 8
WD, MOM, LR = 5e-4, 0.9, 1e-3


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_mix_bf16_bench.json"))
    args = ap.parse_args()
    P, K, T = args.params, args.rounds, 64
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    alpha = 2 / 7
    ones = np.ones(partner.shape[0], np.uint8)
    topo = Topo(partner, alpha, np.ones((T, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16)
    grp.attach_sgd(momentum=MOM, weight_decay=WD, zero_grads=False, master_weights=True)
    f32 = pkg.VirtualWorkerGroup(topo, numel=P)
    f32.attach_sgd(momentum=MOM, weight_decay=WD, zero_grads=False)

    def fill():
        """masters, momentum and gradients of both groups: the same synthetic values (the bf16
        gradients are the fp32 group's, rounded)"""
        for r in range(N):
            pkg._lib.check(L.mx_synth_fill(f32.rows[r].data_ptr(), P, 1234 + r, None))
            pkg._lib.check(L.mx_synth_fill(f32.grads[r].data_ptr(), P, 4321 + r, None))
            pkg._lib.check(L.mx_synth_fill(f32.momentum_rows[r].data_ptr(), P, 999 + r, None))
        with torch.no_grad():
            grp.master_rows.copy_(f32.rows)
            grp.momentum_rows.copy_(f32.momentum_rows)
            grp.grads.copy_(f32.grads)

    fill()
    lay = grp._sgd[0]
    call_zero = lay.call(grp.engine, WD, MOM, False, True)

    # the check first: 64 columns spread over the row (both ends and a tile edge included)
    cols_h = np.linspace(0, P - 1, 64).astype(np.int64)
    cols_h[1] = min(P - 1, lay.tile - 1)
    cols = torch.from_numpy(cols_h).cuda()

    def sample():
        w, m = (t.index_select(1, cols).cpu().numpy() for t in (grp.master_rows, grp.momentum_rows))
        g, p = (t.view(torch.int16).index_select(1, cols).cpu().numpy().view(np.uint16) for t in (grp.grads, grp.rows))
        return w, g, m, p

    ok = True
    for it in range(3):
        W, G, Mo, _ = sample()
        grp.sgd_step(it, LR)
        ww, wm, wp, _ = spec_round(O, W, G, Mo, partner, ones, alpha, (LR, WD, MOM, False))
        gw, gg, gm, gpb = sample()
        ok = ok and np.array_equal(gw.view(np.uint32), ww.view(np.uint32)) and \
            np.array_equal(gm.view(np.uint32), wm.view(np.uint32)) and np.array_equal(gg, G) and \
            bf16ref.same_bf16(gpb, wp)
    out = {"tool": "bench_sgd_mix_bf16", "graph": 0, "workers": N, "params": P, "rounds": K,
           "settle_ms": args.settle_ms, "passes": args.passes,
           "hyper": {"lr": LR, "weight_decay": WD, "momentum": MOM, "nesterov": False},
           "device": torch.cuda.get_device_properties(0).gcnArchName, "fused_check_64_columns": bool(ok),
           "knobs": pkg.engine.sgd_mix_bf16_tuning(), "knobs_fp32": pkg.engine.sgd_mix_tuning()}
    if not ok:
        out["withheld"] = "the fused step differs from the specification: no rate is reported"
        print(json.dumps(out), flush=True)
        return 1

    w, buf = f32.arena, f32.mom_arena                # the unfused sequence's fp32 masters and momentum
    g, p = grp.grad_arena, grp.arena
    s = pkg._lib.stream_ptr

    def fused(j):
        grp.sgd_step(j % T, LR)

    def fused_zero(j):
        pkg._lib.check(L.mx_sgd_mix_bf16(ctypes.addressof(call_zero), j % T, LR, None, s()), "mx_sgd_mix_bf16")

    def unfused(j):
        g32 = g.float()
        d = g32.add(w, alpha=WD)
        buf.mul_(MOM)
        buf.add_(d)
        w.add_(buf, alpha=-LR)
        f32.step(j % T)
        p.copy_(w)

    def fused_fp32(j):
        f32.sgd_step(j % T, LR)

    elems = N * P
    figures = (("a_fused", fused, 20), ("b_unfused", unfused, 64), ("c_fused_fp32", fused_fp32, 20),
               ("a_zero_fused_zero_grads", fused_zero, 22))
    ms = {name: [] for name, _, _ in figures}
    for rep in range(args.passes):
        for name, step, per_elem in (figures if rep % 2 == 0 else figures[::-1]):
            fill()                                   # every pass from the same finite values
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
    out["rate_ratio_a_over_c"] = round(res["a_fused"]["tb_per_s"] / res["c_fused_fp32"]["tb_per_s"], 4)
    if args.ab:
        saved = pkg.engine.sgd_mix_bf16_tuning()
        variants = [("default", {}), ("nt0", {"nontemporal": 0}), ("nt1", {"nontemporal": 1})] + \
                   [(f"wgpc{c}", {"wgpc": c}) for c in (3, 4, 5, 6, 8)] + \
                   [(f"persistent_bpc{b}", {"flat_small": 0, "blocks_per_cu": b}) for b in (2, 4, 8)]
        settle = bench.settle_rounds(20 * elems, args.settle_ms)
        ab = {name: [] for name, _ in variants}
        fill()
        for rep in range(args.reps):
            for name, knobs in (variants if rep % 2 == 0 else variants[::-1]):
                pkg.engine.set_sgd_mix_bf16_tuning(**{**saved, **knobs})
                ab[name].append(round(timed(fused, settle, K), 5))
        pkg.engine.set_sgd_mix_bf16_tuning(**saved)
        out["ab"] = {"ms_per_step": ab, "note": "fused mixed-precision step (20 B/element), each entry settled then "
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
