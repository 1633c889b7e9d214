"""Global-norm gradient clipping in the fused AdamW rounds against doing it with torch before the fused
step, on the headline shape, in ONE process: graph 0, 8 workers x 25.6M parameters, every matching
active, betas (0.9, 0.999), eps 1e-8, decoupled weight decay 1e-2 -- once for the mixed-precision group
(bfloat16 gradients, csrc/adamw_mix_bf16.hip) and once for the fp32 group (csrc/adamw_mix.hip).  Timed,
each after a settle burst sized with bench.settle_rounds, as K back-to-back steps between one HIP event
pair:

  (a) fused        the fused step without clipping (mx_adamw_mix[_bf16])
  (b) norm         the norm launches alone (mx_grad_norm, csrc/grad_norm.hip), with their read rate on
                   n * P * element size bytes; (b_torch) torch.linalg.vector_norm(grad_arena, dim=1) over
                   the same arena, the yardstick for that rate; (b_flat) torch.linalg.vector_norm(grad_arena),
                   ONE norm of the whole arena -- not what clipping per worker needs, but the rate torch's
                   reduction reaches when it is not held to 8 output rows
  (c) clipped      norm launches + the scaled fused step: adamw_step of a clip_grad_norm group
  (d) unfused      the best torch can do before the fused step: vector_norm(grad_arena, dim=1), the
                   factor, grad_arena.mul_(factor), then (a)
  (e) scaled x1    the scaled fused step alone (mx_adamw_mix[_bf16]_scaled), every factor 1.0

max_norm is 1e30, so every factor is exactly 1.0 and the values stay what fill() wrote through every
figure ((d)'s mul_ still makes its full pass); the kernels' time does not depend on the factor.  Every
figure is timed in --passes passes (default 2) in alternating order; both passes are reported, ratios
use their means and "spread" is (max - min) / mean.  First the device norms are checked against
torch's fp64 vector_norm (1 fp32 ulp); a failed check withholds the rates.  One JSON line, also written
to profiles/clip_bench.json.

    python tools/bench_clip.py [--params 25600000] [--rounds 300] [--settle-ms 50] [--modes bf16,fp32]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
import bench  # noqa: E402
from conftest import Topo  # noqa: E402

L = pkg.lib
N = 8
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 1e-2, 1e-3
MAX_NORM = 1e30


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


def run_mode(mode, P, K, T, settle_ms, passes):
    mixed = mode == "bf16"
    gp = pkg.GraphProcessor(pkg.select_graph(0), 1.0, 0, N, 4, True)
    partner = np.asarray(gp.neighbors_info, np.int32)
    topo = Topo(partner, 2 / 7, np.ones((T, partner.shape[0]), np.uint8))
    grp = pkg.VirtualWorkerGroup(topo, numel=P, dtype=torch.bfloat16 if mixed else torch.float32)
    grp.attach_adamw(betas=(B1, B2), eps=EPS, weight_decay=WD, zero_grads=False, master_weights=mixed,
                     clip_grad_norm=MAX_NORM)
    esz = grp.grad_arena.element_size()
    tmp = torch.empty(P, dtype=torch.float32, device="cuda") if mixed else None
    weights = grp.master_rows if mixed else grp.rows

    def fill():
        with torch.no_grad():
            for r in range(N):
                pkg._lib.check(L.mx_synth_fill(weights[r].data_ptr(), P, 1234 + r, None))
                if mixed:
                    pkg._lib.check(L.mx_synth_fill(tmp.data_ptr(), P, 4321 + r, None))
                    grp.grads[r].copy_(tmp)
                else:
                    pkg._lib.check(L.mx_synth_fill(grp.grads[r].data_ptr(), P, 4321 + r, None))
            grp.exp_avg_arena.zero_()
            grp.exp_avg_sq_arena.zero_()
        grp.opt_step = 0

    fill()
    # the check: the device norms against torch's fp64 norm of the same arena, within 1 fp32 ulp
    norms = grp.grad_norm().clone()
    want = torch.linalg.vector_norm(grp.grads.double(), dim=1).float()
    torch.cuda.synchronize()
    ulp = (norms.view(torch.int32).long() - want.view(torch.int32).long()).abs().max().item()
    ok = bool(torch.isfinite(norms).all().item()) and ulp <= 1 and bool((grp.grad_scales == 1.0).all().item())
    out = {"mode": mode, "grad_bytes_per_element": esz, "norm_check_max_ulp": int(ulp), "norm_check": ok,
           "grad_norms": [float(x) for x in norms.cpu()]}
    if not ok:
        out["withheld"] = "the device norms differ from torch's fp64 norm by more than 1 ulp: no rate is reported"
        return out

    s = pkg._lib.stream_ptr
    call = grp._adamw_state()
    plain_fn, scaled_fn = grp._adamw.run, grp._adamw.scaled
    ones = torch.ones(N, dtype=torch.float32, device="cuda")
    step_no = [0]
    ga = grp.grad_arena

    def fused(j):
        step_no[0] += 1
        pkg._lib.check(plain_fn(call, j % T, step_no[0], LR, None, s()), "mx_adamw_mix")

    def norm_only(j):
        grp._clip.enqueue(s())

    def norm_torch(j):
        torch.linalg.vector_norm(ga, dim=1)

    def norm_torch_flat(j):
        torch.linalg.vector_norm(ga)

    def clipped(j):
        grp.adamw_step(j % T, LR)

    def unfused(j):
        total = torch.linalg.vector_norm(ga, dim=1)
        coef = torch.clamp(MAX_NORM / (total + 1e-6), max=1.0)
        ga.mul_(coef.to(ga.dtype)[:, None])
        fused(j)

    def scaled_ones(j):
        step_no[0] += 1
        pkg._lib.check(scaled_fn(call, ones.data_ptr(), j % T, step_no[0], LR, None, s()), "mx_adamw_mix_scaled")

    elems = N * P
    step_b = 28                                           # the fused step's bytes per element, either mode
    figures = (("a_fused", fused, step_b), ("b_norm", norm_only, esz), ("b_torch_vector_norm", norm_torch, esz),
               ("b_flat_torch_vector_norm", norm_torch_flat, esz),
               ("c_clipped", clipped, step_b + esz), ("d_unfused", unfused, step_b + 3 * esz),
               ("e_scaled_ones", scaled_ones, step_b))
    ms = {name: [] for name, _, _ in figures}
    for rep in range(passes):
        for name, step, per_elem in (figures if rep % 2 == 0 else figures[::-1]):
            fill()
            step_no[0] = 0
            settle = bench.settle_rounds(per_elem * elems, settle_ms)
            ms[name].append(round(timed(step, settle, K), 5))
    for name, _, per_elem in figures:
        nbytes = per_elem * elems
        mean = float(np.mean(ms[name]))
        out[name] = {"ms_per_step": round(mean, 5), "ms_per_step_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / mean, 4), "algorithmic_bytes": nbytes,
                     "bytes_per_element": per_elem, "tb_per_s": round(nbytes / (mean * 1e-3) / 1e12, 4)}
    m = {k: out[k]["ms_per_step"] for k, _, _ in figures}
    out["norm_rate_over_torch"] = round(m["b_torch_vector_norm"] / m["b_norm"], 4)
    out["norm_rate_over_torch_flat"] = round(m["b_flat_torch_vector_norm"] / m["b_norm"], 4)
    out["e_over_a"] = round(m["e_scaled_ones"] / m["a_fused"], 4)
    out["c_over_a"] = round(m["c_clipped"] / m["a_fused"], 4)
    out["d_over_c"] = round(m["d_unfused"] / m["c_clipped"], 4)
    out["c_minus_a_minus_b_ms"] = round(m["c_clipped"] - m["a_fused"] - m["b_norm"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=25_600_000)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--modes", default="bf16,fp32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    out = {"tool": "bench_clip", "graph": 0, "workers": N, "params": args.params, "rounds": args.rounds,
           "settle_ms": args.settle_ms, "passes": args.passes, "max_norm": MAX_NORM,
           "hyper": {"lr": LR, "betas": [B1, B2], "eps": EPS, "weight_decay": WD, "decoupled": True},
           "device": torch.cuda.get_device_properties(0).gcnArchName,
           "knobs_grad_norm": pkg.engine.grad_norm_tuning(), "knobs_bf16": pkg.engine.adamw_mix_bf16_tuning(),
           "knobs_fp32": pkg.engine.adamw_mix_tuning()}
    rc = 0
    for mode in args.modes.split(","):
        out[mode] = run_mode(mode, args.params, args.rounds, 64, args.settle_ms, args.passes)
        if "withheld" in out[mode]:
            rc = 1
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
