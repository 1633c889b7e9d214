"""The mixed-precision fused SGD + mixing round's specification (csrc/sgd_mix_bf16.hip), composed of the
existing helpers and never the code under test:

    g32 = f32(g)                                  exact widening, bits << 16          bf16ref.upcast
    d   = fmaf(wd, w, g32) if wd != 0 else g32
    m   = f32(f32(mom * m) + d);  d = fmaf(mom, m, d) if nesterov else m      [mom != 0]
    w'  = fmaf(-lr, d, w)
    w   = the fp32 fused round on w' (sgdref.spec_round: the oracle's chain, ascending matchings, self
          term last; rows the record leaves alone, and every row of an all-zero round, keep w')
    p   = bf16_rne(w)                             one rounding to nearest even        bf16ref.rne_bf16

w and m compare uint32 for uint32, p with bf16ref.same_bf16 (a NaN of any payload where a NaN is
expected: neither torch's cast nor v_cvt_pk_bf16_f32 pins the payload)."""
import numpy as np

import bf16ref
import sgdref


def spec_round(O, w, g_bits, m, partner, flags, alpha, hyper, idle_rows="skip"):
    """One mixed-precision round of every worker: (w_out, m', p_bits, w').  w / m float32 (m None
    without momentum), g_bits bfloat16 bit patterns (uint16), hyper = (lr, wd, mom, nesterov)."""
    w_out, m2, wp = sgdref.spec_round(O, np.asarray(w, np.float32), bf16ref.upcast(g_bits), m, partner, flags, alpha,
                                      hyper, idle_rows)
    return w_out, m2, bf16ref.rne_bf16(w_out), wp


def sgd_only(w, g_bits, m, hyper):
    """The SGD step alone (an all-zero round), without an oracle: (w', m', p_bits)."""
    lr, wd, mom, nesterov = hyper
    wp, m2 = sgdref.sgd_ref(np.asarray(w, np.float32), bf16ref.upcast(g_bits), m, lr, wd, mom, nesterov)
    return wp, m2, bf16ref.rne_bf16(wp)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def eq32(got, want):
    return bool(np.array_equal(u32(got), u32(want)))
