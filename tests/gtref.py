"""Gradient tracking's specification (GT-DSGD; csrc/gt_track.hip, csrc/gt_track_bf16.hip, csrc/gt_step_bf16.hip and
the fused SGD kernel over the trackers), restated in numpy for the tests and never the code under test.  One
iteration is two launches on the same round; every line is one fp32 rounding.

track   gs = f32(g)                       bf16 g widened exactly (bf16ref.upcast); multiplied by the row's clip
                                          factor where there is one (clipref.scale_grad)
        t  = f32(gs - gp)
        y' = f32(y + t)
        gp = gs
        y  = the round on the y' values   groupref.mix: y' itself on an all-zero round and, with
                                          idle_rows="skip", for rows of degree 0

step    torch.optim.SGD's update with the tracker in the gradient's place (groupref.sgd_update: sgdref.sgd_ref per
        parameter run at lr_r = groupref.run_lr(lr, s_r) and decay wd_r), then the round on the x' values; the
        mixed-precision form rounds the stored master to bfloat16 once (p).

hyper = (wd, mom, nesterov).  The clip factor enters the track launch only, the runs the step launch only."""
import numpy as np

import bf16ref
import clipref
import groupref

F32 = np.float32


def track(O, y, g, gp, partner, flags, alpha, idle_rows="skip", scale=None):
    """the track launch on fp32 arrays (g already widened): (y, gp', y')"""
    y, gp = np.asarray(y, F32), np.asarray(gp, F32)
    gs = np.asarray(g, F32).copy() if scale is None else clipref.scale_grad(g, scale)
    with np.errstate(all="ignore"):
        t = (gs - gp).astype(F32)
        yp = (y + t).astype(F32)
    return groupref.mix(O, yp, partner, flags, alpha, idle_rows), gs, yp


def track_bf16(O, y, g_bits, gp, partner, flags, alpha, idle_rows="skip", scale=None):
    """the track launch over bfloat16 gradient bit patterns (uint16)"""
    return track(O, y, bf16ref.upcast(g_bits), gp, partner, flags, alpha, idle_rows, scale)


def _runs(runs, wd, P):
    return [(0, P, float(F32(wd)), 1.0)] if runs is None else runs


def step(O, x, y, m, partner, flags, alpha, lr, hyper, idle_rows="skip", runs=None):
    """the step launch: (x, m', x'); m is None without momentum"""
    wd, mom, nesterov = hyper
    x = np.asarray(x, F32)
    xp, m2 = groupref.sgd_update(x, y, m, _runs(runs, wd, x.shape[1]), lr, mom, nesterov)
    return groupref.mix(O, xp, partner, flags, alpha, idle_rows), m2, xp


def step_bf16(O, w, y, m, partner, flags, alpha, lr, hyper, idle_rows="skip", runs=None):
    """the mixed-precision step launch: (w, m', p_bits, w')"""
    w2, m2, wp = step(O, w, y, m, partner, flags, alpha, lr, hyper, idle_rows, runs)
    return w2, m2, bf16ref.rne_bf16(w2), wp


def spec_round(O, s, g, partner, flags, alpha, lr, hyper, idle_rows="skip", scale=None, runs=None, mixed=False):
    """One iteration from the state s = {x, y, gp, m}: {x, y, gp, m, p, yp, xp, y_track}.  g: fp32 values, or
    bfloat16 bit patterns when mixed; x: the rows, or the masters when mixed.  y_track is the tracker after the
    track launch -- what the step launch reads -- and equals y."""
    g32 = bf16ref.upcast(g) if mixed else np.asarray(g, F32)
    y, gp, yp = track(O, s["y"], g32, s["gp"], partner, flags, alpha, idle_rows, scale)
    x, m, xp = step(O, s["x"], y, s["m"], partner, flags, alpha, lr, hyper, idle_rows, runs)
    return {"x": x, "y": y, "gp": gp, "m": m, "p": bf16ref.rne_bf16(x) if mixed else None, "yp": yp, "xp": xp}


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def eq32(got, want):
    return bool(np.array_equal(u32(got), u32(want)))
