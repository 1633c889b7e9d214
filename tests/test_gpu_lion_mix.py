"""Lion fused into the fp32 gossip round (csrc/lion_mix.hip, VirtualWorkerGroup.attach_lion): x, g and m
fp32.

Every comparison is against the specification restated in tests/lionref.py, never the code under test,
uint32 for uint32 (a NaN of any payload where the specification is a NaN, in the special-values test
only).  The test bodies are tests/lionkit.py's, shared with the mixed-precision file.

Shapes are the smallest at which each path can go wrong: 1-9 columns (the element path, one and two
4-element chunks), 63-65 (a wave's seam), 255-257 (a 256-column pass seam) and per row class one layout
tile - 1, one tile, one tile + 9 and three tiles + 5 (the vector path, the tail, the tile seam, several
work items); ER(64) at the three largest only."""
import pytest

import lionkit as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = K.KINDS["f32"]


@pytest.mark.parametrize("hyper", ["H0", "H1", "H2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "ring32", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows, hyper):
    K.run_rounds(pkg, O, F32, name, idle_rows, hyper)


def test_signed_zero_survives_a_zero_direction(pkg, O):
    K.run_signed_zero(pkg, O, F32)


@pytest.mark.parametrize("where", ["x", "g", "m"])
def test_special_values(pkg, O, where):
    K.run_special_values(pkg, O, F32, where)


def test_abi_offsets_segments_and_guards(pkg, O):
    K.run_abi(pkg, O, F32)


@pytest.mark.parametrize("mode", ["clip", "groups", "both"])
def test_scaled_and_grouped(pkg, O, mode):
    K.run_scaled_grouped(pkg, O, F32, mode)


def test_graph_replay_equals_eager_steps(pkg, O):
    K.run_graph_replay(pkg, O, F32)


@pytest.mark.parametrize("knobs", [{"grid": 2}, {"nontemporal": 0}, {"nontemporal": 1}, {"wgpc": 4},
                                   {"blocks_per_cu": 1}, {"flat_small": 0}])
def test_knobs_change_no_bits(pkg, knobs):
    K.run_knobs(pkg, F32, knobs)


def test_checkpoints(pkg, O):
    K.run_checkpoints(pkg, O, F32)


def test_attach_errors(pkg):
    K.run_attach_errors(pkg, F32)


def test_virtual_trainer_fused_lion(pkg, O):
    K.run_trainer(pkg, O, F32)


def test_refusals_write_nothing(pkg):
    """the host-side refusals of the raw entry points, and a peer-reads plan record: nothing is written"""
    import ctypes
    import numpy as np
    from conftest import Topo
    L, INVALID = pkg.lib, pkg._lib.MX_ERR_INVALID
    partner, alpha = K.topology(pkg, "g0")
    grp = K.group(pkg, F32, Topo(partner, alpha, np.ones((2, partner.shape[0]), np.uint8)), 300, "H1", True)
    rng = np.random.default_rng(51)
    X = rng.standard_normal((8, 300)).astype(np.float32)
    K.put(grp, F32, x=X, m=X * 0.5, g=K.rand_g(F32, rng, (8, 300)))
    before = K.state(grp, F32)
    lay = grp._lion.layout

    def refused(**fields):
        call = lay.call(grp.engine, (0.9, 0.99), 1e-2, True)
        for k, v in fields.items():
            setattr(call, k, v)
        s = pkg._lib.stream_ptr()
        return L.mx_lion_mix(ctypes.addressof(call), 0, K.LR, None, s) == INVALID and \
            L.mx_lion_mix_at(ctypes.addressof(call), grp.iter_dev.data_ptr(), 2, K.LR, None, s) == INVALID

    assert refused(n_slots=9) and refused(n_local=65, n_slots=65) and refused(M=33)
    assert refused(m_ptrs_dev=None) and b"momentum" in L.mx_last_error()
    assert refused(x_ptrs_dev=None) and refused(g_ptrs_dev=None)
    call = lay.call(grp.engine, (0.9, 0.99), 1e-2, True)
    assert L.mx_lion_mix_at(ctypes.addressof(call), None, 2, K.LR, None, pkg._lib.stream_ptr()) == INVALID
    assert K.same_state(F32, K.state(grp, F32), before)
    args = (grp.engine.plan.data_ptr(), grp.engine.T + 1, grp.n_local, grp.engine.M)
    pkg._lib.check(L.mx_plan_set_peer_reads(*args, 1, pkg._lib.stream_ptr()))
    grp.lion_step(0, K.LR)
    grp.iter_dev.fill_(0)
    grp.lion_device_round()
    assert K.same_state(F32, K.state(grp, F32), before)
    pkg._lib.check(L.mx_plan_set_peer_reads(*args, 0, pkg._lib.stream_ptr()))
    assert grp.lion_step(0, K.LR)                                    # the bit cleared: the same launch now writes
    after = K.state(grp, F32)
    assert not K.same(F32, after, before, "x") and not after["g"].any()
