"""The SlowMo outer step (mx_slowmo_step, csrc/slowmo.hip) against the same step spelled out with the existing
pieces and against the in-place mean, in ONE process, on the headline shape 8 rows x 25.6M columns, as an fp32
group and as a mixed-precision one (fp32 masters + their bfloat16 image).  Timed, each after a settle burst
sized with bench.settle_rounds, as K back-to-back calls between one HIP event pair:

  (a) fused      one mx_slowmo_step launch: reads every row, a and u once, writes them once (and the image):
                 80 bytes per column at 8 rows, 96 mixed
  (b) unfused    mx_mean_rows to a scratch row, four torch element-wise ops (tmp = a - mean; u *= beta;
                 u += tmp / lr; a -= alpha lr u), the broadcast rows.copy_(a) and, mixed, p.copy_(rows), each
                 once over whole arrays: 116 bytes per column, 164 mixed
  (c) mean       mx_mean_rows_to in place on the same rows: 64 bytes per column -- the yardstick: the same
                 access pattern with two arrays and a few flops less

First (a) is checked against (b) on the same inputs (relative 1e-5: the torch ops round differently, so not bit
for bit -- the bits are the tests' business); a failed check withholds the rates.  Every figure is timed in
--passes passes in alternating order; ratios use the means and "spread" is (max - min) / mean.  One JSON line,
also written to profiles/slowmo_bench.json.

    python tools/bench_slowmo.py [--rounds 300] [--settle-ms 50] [--modes fp32,mixed] [--shape 8x25600000]
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
sys.path.insert(0, ROOT)
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
import bench  # noqa: E402

L = pkg.lib
E = pkg.engine
check = pkg._lib.check
LR, ALPHA, BETA = 0.1, 1.0, 0.5


def timed(step, settle, K):
    """`settle` untimed calls, then K calls between one event pair: ms per call"""
    for _ in range(settle):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(K):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / K


def run_mode(n, P, mode, K, settle_ms, passes, order):
    mixed = mode == "mixed"
    ld = (P + E.ROW_ALIGN - 1) // E.ROW_ALIGN * E.ROW_ALIGN
    arena = torch.zeros((n, ld), dtype=torch.float32, device="cuda")
    rows = arena[:, :P]
    image = torch.zeros((n, ld), dtype=torch.bfloat16, device="cuda") if mixed else None
    state = torch.zeros((3, ld), dtype=torch.float32, device="cuda")          # a, u, scratch
    a, u, tmp = state[0, :P], state[1, :P], state[2, :P]
    mean = torch.empty(ld, dtype=torch.float32, device="cuda")
    s = pkg._lib.stream_ptr

    def fill():
        for r in range(n):
            check(L.mx_synth_fill(arena[r].data_ptr(), P, 1234 + r, None))
        check(L.mx_synth_fill(state[0].data_ptr(), P, 99, None))
        check(L.mx_synth_fill(state[1].data_ptr(), P, 98, None))

    call = E.SlowmoCall(arena.data_ptr(), state[0].data_ptr(), state[1].data_ptr(),
                        image.data_ptr() if mixed else None, ld, ld, P, n, order, ALPHA, BETA)
    addr = ctypes.addressof(call)
    rl, al = float(np.float32(1) / np.float32(LR)), float(np.float32(ALPHA) * np.float32(LR))

    def fused():
        rc = L.mx_slowmo_step(addr, LR, None, s())
        if rc:
            check(rc, "mx_slowmo_step")

    def unfused():
        check(L.mx_mean_rows(arena.data_ptr(), n, ld, P, order, mean.data_ptr(), s()))
        torch.sub(a, mean[:P], out=tmp)
        u.mul_(BETA)
        u.add_(tmp, alpha=rl)
        a.add_(u, alpha=-al)
        rows.copy_(a)                                                         # the broadcast
        if mixed:
            image[:, :P].copy_(rows)

    def mean_in_place():
        check(L.mx_mean_rows_to(arena.data_ptr(), n, ld, P, order, arena.data_ptr(), n, ld, s()))

    # the check: one fused step against the unfused sequence on the same inputs
    fill()
    fused()
    got = [t.clone() for t in (rows[0], rows[n - 1], a, u)] + ([image[n - 1, :P].clone()] if mixed else [])
    fill()
    unfused()
    want = [rows[0], rows[n - 1], a, u] + ([image[n - 1, :P]] if mixed else [])
    torch.cuda.synchronize()
    err = max(float(((g.float() - w.float()).abs() / (w.float().abs() + 1)).max().item()) for g, w in zip(got, want))
    ok = err <= (1e-2 if mixed else 1e-5)                                     # the image: one bf16 ulp at most
    ok_main = max(float(((g - w).abs() / (w.abs() + 1)).max().item()) for g, w in zip(got[:4], want[:4])) <= 1e-5
    out = {"rows": n, "params": P, "mode": mode, "order": order, "check_max_rel_err": err, "check": bool(ok and ok_main),
           "kernel": L.mx_slowmo_kernel_name(addr).decode()}
    del got, want
    torch.cuda.empty_cache()
    if not out["check"]:
        out["withheld"] = "the fused step differs from the unfused sequence: no rate is reported"
        return out

    per_col = {"a_fused": 4 * (2 * n + 4) + (2 * n if mixed else 0),
               "b_unfused": 4 * (n + 1) + 12 + 8 + 12 + 12 + 4 * (n + 1) + (6 * n if mixed else 0),
               "c_mean": 8 * n}
    figures = [("a_fused", fused), ("b_unfused", unfused), ("c_mean", mean_in_place)]
    settle = {name: bench.settle_rounds(per_col[name] * P, settle_ms) for name, _ in figures}
    ms = {name: [] for name, _ in figures}
    fill()
    for rep in range(passes):
        for name, step in (figures if rep % 2 == 0 else figures[::-1]):
            ms[name].append(round(timed(step, settle[name], K), 5))
    for name, _ in figures:
        m = float(np.mean(ms[name]))
        out[name] = {"ms_per_call": round(m, 5), "ms_per_call_passes": ms[name],
                     "spread": round((max(ms[name]) - min(ms[name])) / m, 4), "bytes_per_column": per_col[name],
                     "algorithmic_bytes": per_col[name] * P, "tb_per_s": round(per_col[name] * P / (m * 1e-3) / 1e12, 4)}
    out["unfused_over_fused"] = round(out["b_unfused"]["ms_per_call"] / out["a_fused"]["ms_per_call"], 4)
    out["unfused_over_fused_predicted_by_bytes"] = round(per_col["b_unfused"] / per_col["a_fused"], 4)
    out["fused_rate_over_mean_rate"] = round(out["a_fused"]["tb_per_s"] / out["c_mean"]["tb_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="8x25600000")
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--modes", default="fp32,mixed")
    ap.add_argument("--order", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slowmo_bench.json"))
    args = ap.parse_args()
    n, P = (int(v) for v in args.shape.split("x"))
    out = {"tool": "bench_slowmo", "rounds": args.rounds, "settle_ms": args.settle_ms, "passes": args.passes,
           "device": torch.cuda.get_device_properties(0).gcnArchName, "knobs_slowmo": E.slowmo_tuning(),
           "knobs_mix": {k: v for k, v in E.mix_tuning().items() if k in ("mean_wgpc", "store_policy")}, "results": []}
    rc = 0
    for mode in args.modes.split(","):
        res = run_mode(n, P, mode, args.rounds, args.settle_ms, args.passes, args.order)
        out["results"].append(res)
        if "withheld" in res:
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
