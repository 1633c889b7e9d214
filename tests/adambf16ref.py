"""The mixed-precision fused AdamW / Adam + mixing round's specification (csrc/adamw_mix_bf16.hip),
composed of the existing helpers and never the code under test:

    g32 = f32(g)                                  exact widening, bits << 16          bf16ref.upcast
    w', m', v' = adamref.adam_ref(w, g32, m, v, t, ...)       torch's lines, one fp32 rounding each
    w   = the fp32 fused round on w' (adamref.spec_round: the oracle's chain, ascending matchings, self
          term last; rows the record leaves alone, and every row of an all-zero round, keep w')
    p   = bf16_rne(w)                             one rounding to nearest even        bf16ref.rne_bf16

w, m and v compare uint32 for uint32, p with bf16ref.same_bf16 (a NaN of any payload where a NaN is
expected: neither torch's cast nor v_cvt_pk_bf16_f32 pins the payload)."""
import numpy as np

import adamref
import bf16ref


def spec_round(O, w, g_bits, m, v, t, partner, flags, alpha, lr, hyper, table, idle_rows="skip"):
    """One mixed-precision round of every worker at optimizer step t: (w_out, m', v', p_bits, w').
    w / m / v float32, g_bits bfloat16 bit patterns (uint16), hyper = (beta1, beta2, eps, wd, decoupled)."""
    w_out, m2, v2, wp = adamref.spec_round(O, np.asarray(w, np.float32), bf16ref.upcast(g_bits), m, v, t, partner,
                                           flags, alpha, lr, hyper, table, idle_rows)
    return w_out, m2, v2, bf16ref.rne_bf16(w_out), wp


def adam_only(w, g_bits, m, v, t, lr, hyper, table):
    """The optimizer step alone (an all-zero round), without an oracle: (w', m', v', p_bits)."""
    wp, m2, v2 = adamref.adam_ref(np.asarray(w, np.float32), bf16ref.upcast(g_bits), m, v, t, lr, hyper, table)
    return wp, m2, v2, bf16ref.rne_bf16(wp)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def eq32(got, want):
    return bool(np.array_equal(u32(got), u32(want)))
