"""The fused quasi-global-momentum rounds against the fused SGD-momentum rounds of the same precision (which
move the same bytes) and against the unfused torch sequence, on the headline shape, in ONE process: graph 0,
8 workers x 25.6M parameters, every matching active, momentum = mu = 0.9, weight decay 5e-4, zero_grads on in
every fused figure.  Timed, each after a settle burst sized with bench.settle_rounds, as K back-to-back steps
between one HIP event pair:

  qgm_fp32          VirtualWorkerGroup.attach_qgm().qgm_step (csrc/qgm_mix.hip), default knobs           24 B/element
  qgm_fp32_plain    the same with the other setting of the knob stage_plain (x and mh staged with plain
  / qgm_fp32_nt     loads, or with nt loads like g): whichever is not the default                        24
  sgd_fp32          the fp32 group's sgd_step, momentum 0.9 (csrc/sgd_mix.hip): the yardstick            24
  qgm_mp32          bfloat16 group, attach_qgm(master_weights=True) (csrc/qgm_mix_bf16.hip)              22
  qgm_mp32_plain    the same with the other setting of stage_plain                                       22
  / qgm_mp32_nt
  sgd_mp            the bfloat16 group's mixed-precision sgd_step: the yardstick                         22
  qgm_unfused_fp32  the torch op sequence, ONCE over whole [8, ld] arenas: x_old = x.clone() (8 bytes),
                    d = g.add(x, alpha=wd) (12), m = d.add(mh, alpha=beta) (12), x.add_(m, alpha=-lr) (12),
                    group.step (8), x_old.sub_(x) (12), mh.mul_(mu) (8), mh.add_(x_old, alpha=(1 - mu) / lr)
                    (12): 84 bytes per element, the gradients not zeroed
  qgm_unfused_mp    the same on fp32 masters with g32 = g.float() (2 + 4) in front and p.copy_(w) (4 + 2)
                    behind: 96 bytes per element
  --wgpc C ...      adds qgm_fp32_wgpcC / qgm_mp32_wgpcC: the default knobs under a cap of C workgroups per CU
  --combo k=v,k=v   adds qgm_fp32_<k><v>_... / qgm_mp32_<k><v>_...: both QGM steps under that set of knobs

Every figure is timed in --passes passes (default 2) in alternating order; all passes are reported, the
ratios use their means and "spread" is (max - min) / mean over the passes.  One JSON line (also written to
profiles/qgm_mix_bench.json): ms per step, the TB/s that implies on the algorithmic bytes, and each QGM
figure's time over its yardstick's next to the yardstick's own spread.  First, 64 sampled columns of three
steps of each QGM group are checked against the specification (tests/qgmref.py); a failed check withholds
the rates, as bench.py does.

    python tools/bench_qgm_mix.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--passes 2] [--wgpc 4 6]
                                  [--combo stage_plain=0,wgpc=4 nontemporal=0]
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
import oracle as O  # noqa: E402
import qgmref  # noqa: E402
from conftest import Topo  # noqa: E402

L = pkg.lib
N = 8
BETA, MU, WD, LR = 0.9, 0.9, 5e-4, 0.01
HYPER = (BETA, MU, WD, False)


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
    ap.add_argument("--wgpc", type=int, nargs="*", default=[])
    ap.add_argument("--combo", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qgm_mix_bench.json"))
    args = ap.parse_args()
    P, K, T = args.params, args.rounds, 64
    E = pkg.engine
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    alpha = 2 / 7
    ones = np.ones(partner.shape[0], np.uint8)
    topo = Topo(partner, alpha, np.ones((T, partner.shape[0]), np.uint8))
    BF = torch.bfloat16

    def make(attach, dtype=torch.float32, **kw):
        g = pkg.VirtualWorkerGroup(topo, numel=P, dtype=dtype)
        getattr(g, attach)(zero_grads=True, master_weights=dtype == BF, weight_decay=WD, **kw)
        return g

    qgm = {"qgm_fp32": make("attach_qgm", momentum=BETA, mu=MU), "qgm_mp32": make("attach_qgm", BF, momentum=BETA, mu=MU)}
    sgd = {"sgd_fp32": make("attach_sgd", momentum=BETA), "sgd_mp": make("attach_sgd", BF, momentum=BETA)}
    groups = {**qgm, **sgd}
    setters = {"qgm_fp32": E.set_qgm_mix_tuning, "qgm_mp32": E.set_qgm_mix_bf16_tuning}
    defaults = {"qgm_fp32": E.qgm_mix_tuning(), "qgm_mp32": E.qgm_mix_bf16_tuning()}
    other = 1 - defaults["qgm_fp32"]["stage_plain"]         # the staging that is not the default
    combos = [{"wgpc": c} for c in args.wgpc] + [{k: int(v) for k, v in (kv.split("=") for kv in c.split(","))}
                                                 for c in args.combo]
    f32, mp = qgm["qgm_fp32"], qgm["qgm_mp32"]
    src_x, src_g = torch.empty_like(f32.rows), torch.empty_like(f32.rows)
    for r in range(N):
        pkg._lib.check(L.mx_synth_fill(src_x[r].data_ptr(), P, 1234 + r, None))
        pkg._lib.check(L.mx_synth_fill(src_g[r].data_ptr(), P, 4321 + r, None))
    mix_u = pkg.VirtualWorkerGroup(topo, numel=P)    # the unfused sequences' fp32 rows / masters, mixed by group.step
    mh_u = torch.zeros_like(f32.arena)               # ... and their buffer

    def fill(g):
        """rows / masters and gradients of group g from the same synthetic values (bf16 gradients are the fp32
        ones, rounded), zero state"""
        with torch.no_grad():
            (g.master_rows if g.master_rows is not None else g.rows).copy_(src_x)
            g.grads.copy_(src_g)
            for name in ("qgm_buffer_arena", "mom_arena"):
                t = getattr(g, name, None)
                if t is not None:
                    t.zero_()

    # the check first: 64 columns spread over the row (both ends and a tile edge included), under both stagings
    cols_h = np.linspace(0, P - 1, 64).astype(np.int64)
    cols_h[1] = min(P - 1, f32._qgm.layout.tile - 1)
    cols = torch.from_numpy(cols_h).cuda()

    def bits(t):
        return t.view(torch.int16).index_select(1, cols).cpu().numpy().view(np.uint16)

    def vals(t):
        return t.index_select(1, cols).cpu().numpy()

    ok = True
    for plain in (0, 1):
        for name, g in qgm.items():
            setters[name](stage_plain=plain)
            fill(g)
            mixed = name == "qgm_mp32"
            for it in range(3):
                with torch.no_grad():
                    g.grads.copy_(src_g)                 # zero_grads consumed them
                x = vals(g.master_rows if mixed else g.rows)
                gr = bits(g.grads) if mixed else vals(g.grads)
                m = vals(g.qgm_buffer_rows)
                g.qgm_step(it, LR)
                if mixed:
                    wx, wm, wp, _ = qgmref.spec_round_bf16(O, x, gr, m, partner, ones, alpha, LR, HYPER)
                    ok = ok and bf16ref.same_bf16(bits(g.rows), wp) and not bits(g.grads).any()
                else:
                    wx, wm, _ = qgmref.spec_round(O, x, gr, m, partner, ones, alpha, LR, HYPER)
                    ok = ok and not vals(g.grads).any()
                ok = ok and qgmref.eq32(vals(g.master_rows if mixed else g.rows), wx)
                ok = ok and qgmref.eq32(vals(g.qgm_buffer_rows), wm)
            setters[name](stage_plain=defaults[name]["stage_plain"])
    out = {"tool": "bench_qgm_mix", "graph": 0, "workers": N, "params": P, "rounds": K, "settle_ms": args.settle_ms,
           "passes": args.passes, "zero_grads": True,
           "hyper": {"lr": LR, "momentum": BETA, "mu": MU, "weight_decay": WD, "nesterov": False},
           "device": torch.cuda.get_device_properties(0).gcnArchName, "fused_check_64_columns": bool(ok),
           "knobs": {"qgm_mix": E.qgm_mix_tuning(), "qgm_mix_bf16": E.qgm_mix_bf16_tuning(),
                     "sgd_mix": E.sgd_mix_tuning(), "sgd_mix_bf16": E.sgd_mix_bf16_tuning()}}
    if not ok:
        out["withheld"] = "a fused QGM step differs from the specification: no rate is reported"
        print(json.dumps(out), flush=True)
        return 1

    x_u, g32_u, g16, p16 = mix_u.arena, f32.grad_arena, mp.grad_arena, mp.arena

    def unfused_tail(d, j):
        x_old = x_u.clone()
        m = d.add(mh_u, alpha=BETA)
        x_u.add_(m, alpha=-LR)
        mix_u.step(j % T)
        x_old.sub_(x_u)
        mh_u.mul_(MU)
        mh_u.add_(x_old, alpha=(1 - MU) / LR)

    def unfused_fp32(j):
        unfused_tail(g32_u.add(x_u, alpha=WD), j)

    def unfused_mp(j):
        unfused_tail(g16.float().add_(x_u, alpha=WD), j)
        p16.copy_(x_u)

    def stepper(name):
        g = groups[name]
        fn = g.qgm_step if name in qgm else g.sgd_step
        return lambda j: fn(j % T, LR)

    # figure -> (the group it runs on, its step, its bytes per element, the knobs it runs under)
    figures = []
    for base, yard, per in (("qgm_fp32", "sgd_fp32", 24), ("qgm_mp32", "sgd_mp", 22)):
        figures.append((base, base, stepper(base), per, {}))
        figures.append((base + ("_plain" if other else "_nt"), base, stepper(base), per, {"stage_plain": other}))
        for knobs in combos:
            figures.append((base + "_" + "_".join(f"{k}{v}" for k, v in knobs.items()), base, stepper(base), per, knobs))
        figures.append((yard, yard, stepper(yard), per, {}))
    figures.append(("qgm_unfused_fp32", "qgm_fp32", unfused_fp32, 84, {}))
    figures.append(("qgm_unfused_mp", "qgm_mp32", unfused_mp, 96, {}))
    elems = N * P
    ms = {f[0]: [] for f in figures}
    for rep in range(args.passes):
        for name, gname, step, per, knobs in (figures if rep % 2 == 0 else figures[::-1]):
            fill(groups[gname])                      # every figure from the same finite values
            if "unfused" in name:
                with torch.no_grad():
                    mix_u.rows.copy_(src_x)
                    mh_u.zero_()
            settle = bench.settle_rounds(per * elems, args.settle_ms)
            if knobs:
                setters[gname](**knobs)
            try:
                ms[name].append(round(timed(step, settle, K), 5))
            finally:
                if knobs:
                    setters[gname](**{k: defaults[gname][k] for k in knobs})
    res = {}
    for name, _, _, per, knobs in figures:
        nbytes = per * elems
        mean = float(np.mean(ms[name]))
        res[name] = {"ms_per_step": round(mean, 5), "ms_per_step_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / mean, 4), "algorithmic_bytes": nbytes,
                     "bytes_per_element": per, "settle_rounds": bench.settle_rounds(nbytes, args.settle_ms),
                     "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4), "knobs": knobs}
    out.update(res)

    def ratio(a, b):
        return round(res[a]["ms_per_step"] / res[b]["ms_per_step"], 4)

    for name, gname, _, _, _ in figures:
        if name.startswith("qgm_fp32"):
            out[f"time_{name}_over_sgd_fp32"] = ratio(name, "sgd_fp32")
        elif name.startswith("qgm_mp32"):
            out[f"time_{name}_over_sgd_mp"] = ratio(name, "sgd_mp")
    out["yardstick_spread"] = {"sgd_fp32": res["sgd_fp32"]["spread"], "sgd_mp": res["sgd_mp"]["spread"]}
    out["speedup_unfused_over_qgm_fp32"] = ratio("qgm_unfused_fp32", "qgm_fp32")
    out["speedup_unfused_over_qgm_fp32_predicted_by_bytes"] = round(84 / 24, 4)
    out["speedup_unfused_over_qgm_mp32"] = ratio("qgm_unfused_mp", "qgm_mp32")
    out["speedup_unfused_over_qgm_mp32_predicted_by_bytes"] = round(96 / 22, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
