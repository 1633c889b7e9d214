"""The fused Lion rounds against the fused SGD-momentum and AdamW rounds of the same precision and
against the unfused sequence, on the headline shape, in ONE process: graph 0, 8 workers x 25.6M
parameters, every matching active, betas (0.9, 0.99), decoupled weight decay 1e-2, zero_grads on in every
fused figure.  Timed, each after a settle burst sized with bench.settle_rounds, as K back-to-back steps
between one HIP event pair:

  lion_fp32       VirtualWorkerGroup.attach_lion().lion_step (csrc/lion_mix.hip)                    24 B/element
  sgd_fp32        the fp32 group's sgd_step, momentum 0.9 (csrc/sgd_mix.hip): the yardstick         24
  adamw_fp32      the fp32 group's adamw_step (csrc/adamw_mix.hip)                                  36
  lion_mp32       bfloat16 group, attach_lion(master_weights=True), fp32 momentum                   22
  lion_mp16       the same with momentum_dtype=torch.bfloat16 (csrc/lion_mix_bf16.hip)              18
  sgd_mp          the bfloat16 group's mixed-precision sgd_step: the yardstick                      22
  adamw_mp        the bfloat16 group's mixed-precision adamw_step                                   30
  lion_unfused    the op sequence the mixed-precision launch replaces, run ONCE over whole [8, ld]
                  arenas: g32 = g.float() (2 + 4 bytes), w.mul_(1 - lr wd) (8), c = m.lerp(g32, 1 - b1)
                  (12), s = c.sign() (8), w.add_(s, alpha=-lr) (12), m.lerp_(g32, 1 - b2) (12), the fp32
                  group.step of the masters (8), p.copy_(w) (4 + 2): 72 bytes per element, the gradients
                  not zeroed

Every figure is timed in --passes passes (default 2) in alternating order; all passes are reported, the
ratios use their means and "spread" is (max - min) / mean over the passes.  One JSON line (also written
to profiles/lion_mix_bench.json): ms per step, the TB/s that implies on the algorithmic bytes, and each
Lion figure's time over its yardstick's next to the yardstick's own spread.  First, 64 sampled columns of
three steps of each Lion group are checked against the specification (tests/lionref.py); a failed check
withholds the rates, as bench.py does.

    python tools/bench_lion_mix.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--passes 2]
"""
import argparse
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
import lionref  # noqa: E402
import oracle as O  # noqa: E402
from conftest import Topo  # noqa: E402

L = pkg.lib
N = 8
B1, B2, WD, LR = 0.9, 0.99, 1e-2, 1e-4
SGD_WD, SGD_MOM = 5e-4, 0.9
ADAM = {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": WD}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lion_mix_bench.json"))
    args = ap.parse_args()
    P, K, T = args.params, args.rounds, 64
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    alpha = 2 / 7
    ones = np.ones(partner.shape[0], np.uint8)
    topo = Topo(partner, alpha, np.ones((T, partner.shape[0]), np.uint8))
    BF = torch.bfloat16

    def make(attach, dtype=torch.float32, **kw):
        g = pkg.VirtualWorkerGroup(topo, numel=P, dtype=dtype)
        getattr(g, attach)(zero_grads=True, master_weights=dtype == BF, **kw)
        return g

    lion = {"lion_fp32": make("attach_lion", betas=(B1, B2), weight_decay=WD),
            "lion_mp32": make("attach_lion", BF, betas=(B1, B2), weight_decay=WD),
            "lion_mp16": make("attach_lion", BF, betas=(B1, B2), weight_decay=WD, momentum_dtype=BF)}
    sgd = {"sgd_fp32": make("attach_sgd", momentum=SGD_MOM, weight_decay=SGD_WD),
           "sgd_mp": make("attach_sgd", BF, momentum=SGD_MOM, weight_decay=SGD_WD)}
    adamw = {"adamw_fp32": make("attach_adamw", **ADAM), "adamw_mp": make("attach_adamw", BF, **ADAM)}
    groups = {**lion, **sgd, **adamw}
    f32 = lion["lion_fp32"]
    src_x, src_g = torch.empty_like(f32.rows), torch.empty_like(f32.rows)
    for r in range(N):
        pkg._lib.check(L.mx_synth_fill(src_x[r].data_ptr(), P, 1234 + r, None))
        pkg._lib.check(L.mx_synth_fill(src_g[r].data_ptr(), P, 4321 + r, None))
    m_u = torch.zeros_like(f32.arena)                # the unfused sequence's momentum
    mix_u = pkg.VirtualWorkerGroup(topo, numel=P)    # ... and its fp32 masters, mixed by group.step

    def fill(g):
        """masters, gradients and optimizer state of group g from the same synthetic values (bf16
        gradients are the fp32 ones, rounded), zero state, step 0"""
        with torch.no_grad():
            (g.master_rows if g.master_rows is not None else g.rows).copy_(src_x)
            g.grads.copy_(src_g)
            for name in ("lion_exp_avg_arena", "mom_arena", "exp_avg_arena", "exp_avg_sq_arena"):
                t = getattr(g, name, None)
                if t is not None:
                    t.zero_()
        if getattr(g, "_adamw", None) is not None:
            g.opt_step = 0

    # the check first: 64 columns spread over the row (both ends and a tile edge included)
    cols_h = np.linspace(0, P - 1, 64).astype(np.int64)
    cols_h[1] = min(P - 1, f32._lion.layout.tile - 1)
    cols = torch.from_numpy(cols_h).cuda()

    def bits(t):
        return t.view(torch.int16).index_select(1, cols).cpu().numpy().view(np.uint16)

    def vals(t):
        return t.index_select(1, cols).cpu().numpy()

    ok = True
    for name, g in lion.items():
        fill(g)
        mixed, m16 = name != "lion_fp32", name == "lion_mp16"
        for it in range(3):
            with torch.no_grad():
                g.grads.copy_(src_g)                 # zero_grads consumed them
            x = vals(g.master_rows if mixed else g.rows)
            gr = bits(g.grads) if mixed else vals(g.grads)
            m = bits(g.lion_exp_avg_rows) if m16 else vals(g.lion_exp_avg_rows)
            g.lion_step(it, LR)
            if mixed:
                wx, wm, wp, _ = lionref.spec_round_bf16(O, x, gr, m, partner, ones, alpha, LR, (B1, B2, WD), m_bf16=m16)
                ok = ok and bf16ref.same_bf16(bits(g.rows), wp)
            else:
                wx, wm, _ = lionref.spec_round(O, x, gr, m, partner, ones, alpha, LR, (B1, B2, WD))
            ok = ok and lionref.eq32(vals(g.master_rows if mixed else g.rows), wx)
            ok = ok and (np.array_equal(bits(g.lion_exp_avg_rows), wm) if m16 else
                         lionref.eq32(vals(g.lion_exp_avg_rows), wm))
            ok = ok and not bits(g.grads).any() if mixed else ok and not vals(g.grads).any()
    E = pkg.engine
    out = {"tool": "bench_lion_mix", "graph": 0, "workers": N, "params": P, "rounds": K, "settle_ms": args.settle_ms,
           "passes": args.passes, "zero_grads": True,
           "hyper": {"lr": LR, "betas": [B1, B2], "weight_decay": WD},
           "sgd_hyper": {"weight_decay": SGD_WD, "momentum": SGD_MOM},
           "adamw_hyper": {"betas": list(ADAM["betas"]), "eps": ADAM["eps"], "weight_decay": WD},
           "device": torch.cuda.get_device_properties(0).gcnArchName, "fused_check_64_columns": bool(ok),
           "knobs": {"lion_mix": E.lion_mix_tuning(), "lion_mix_bf16": E.lion_mix_bf16_tuning(),
                     "sgd_mix": E.sgd_mix_tuning(), "sgd_mix_bf16": E.sgd_mix_bf16_tuning()}}
    if not ok:
        out["withheld"] = "a fused Lion step differs from the specification: no rate is reported"
        print(json.dumps(out), flush=True)
        return 1

    mp = lion["lion_mp32"]
    w, g16, p16 = mix_u.arena, mp.grad_arena, mp.arena   # the unfused sequence's masters, bf16 gradients and models

    def unfused(j):
        g32 = g16.float()
        w.mul_(1 - LR * WD)
        c = m_u.lerp(g32, 1 - B1)
        s = c.sign()
        w.add_(s, alpha=-LR)
        m_u.lerp_(g32, 1 - B2)
        mix_u.step(j % T)
        p16.copy_(w)

    def stepper(name):
        g = groups[name]
        fn = g.lion_step if name in lion else g.sgd_step if name in sgd else g.adamw_step
        return lambda j: fn(j % T, LR)

    per_elem = {"lion_fp32": 24, "sgd_fp32": 24, "adamw_fp32": 36, "lion_mp32": 22, "lion_mp16": 18, "sgd_mp": 22,
                "adamw_mp": 30, "lion_unfused": 72}
    figures = [(name, stepper(name)) for name in groups] + [("lion_unfused", unfused)]
    elems = N * P
    ms = {name: [] for name, _ in figures}
    for rep in range(args.passes):
        for name, step in (figures if rep % 2 == 0 else figures[::-1]):
            if name == "lion_unfused":
                fill(mp)
                with torch.no_grad():
                    mix_u.rows.copy_(src_x)
                    m_u.zero_()
            else:
                fill(groups[name])                   # every figure from the same finite values
            settle = bench.settle_rounds(per_elem[name] * elems, args.settle_ms)
            ms[name].append(round(timed(step, settle, K), 5))
    res = {}
    for name, _ in figures:
        nbytes = per_elem[name] * elems
        mean = float(np.mean(ms[name]))
        res[name] = {"ms_per_step": round(mean, 5), "ms_per_step_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / mean, 4), "algorithmic_bytes": nbytes,
                     "bytes_per_element": per_elem[name], "settle_rounds": bench.settle_rounds(nbytes, args.settle_ms),
                     "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4)}
    out.update(res)

    def ratio(a, b):
        return round(res[a]["ms_per_step"] / res[b]["ms_per_step"], 4)

    out["time_lion_fp32_over_sgd_fp32"] = ratio("lion_fp32", "sgd_fp32")
    out["time_lion_mp32_over_sgd_mp"] = ratio("lion_mp32", "sgd_mp")
    out["yardstick_spread"] = {"sgd_fp32": res["sgd_fp32"]["spread"], "sgd_mp": res["sgd_mp"]["spread"]}
    out["time_lion_mp16_over_lion_mp32"] = ratio("lion_mp16", "lion_mp32")
    out["time_lion_mp16_over_lion_mp32_predicted_by_bytes"] = round(18 / 22, 4)
    out["time_lion_mp16_over_adamw_mp"] = ratio("lion_mp16", "adamw_mp")
    out["speedup_unfused_over_lion_mp32"] = ratio("lion_unfused", "lion_mp32")
    out["speedup_unfused_over_lion_mp32_predicted_by_bytes"] = round(72 / 22, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
