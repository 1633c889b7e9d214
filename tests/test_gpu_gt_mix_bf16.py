"""Gradient tracking (GT-DSGD) on bfloat16 rows over fp32 masters (csrc/gt_track_bf16.hip and csrc/gt_step_bf16.hip,
VirtualWorkerGroup.attach_gt(master_weights=True)): fp32 masters w, bfloat16 gradients g and model rows p, the
tracker y, the previous gradient gp and the momentum m fp32.

Every comparison is against the specification restated in tests/gtref.py, never the code under test: w, y, gp and
m uint32 for uint32 and p uint16 for uint16 (a NaN of any payload where the specification is a NaN, in the
special-values test only), after each of the two launches and after the pair.  The test bodies are
tests/gtkit.py's, shared with the fp32 file, whose shapes these are."""
import pytest

import gtkit as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MP32 = K.KINDS["mp32"]


@pytest.mark.parametrize("hyper", ["H0", "H1", "H2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "ring32", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows, hyper):
    K.run_rounds(pkg, O, MP32, name, idle_rows, hyper)


def test_lr_scale_zero_freezes_w_while_the_tracker_moves(pkg, O):
    K.run_lr_scale_zero(pkg, O, MP32)


def test_past_the_schedule_and_peer_reads_write_nothing(pkg):
    K.run_noops(pkg, MP32)


def test_refusals_write_nothing(pkg):
    K.run_refusals(pkg, MP32)


@pytest.mark.parametrize("where", ["g", "gp", "y", "x"])
def test_special_values(pkg, O, where):
    K.run_special_values(pkg, O, MP32, where)


def test_abi_offsets_segments_and_guards(pkg, O):
    K.run_abi(pkg, O, MP32)


@pytest.mark.parametrize("mode", ["clip", "groups", "both"])
def test_scaled_and_grouped(pkg, O, mode):
    K.run_scaled_grouped(pkg, O, MP32, mode)


def test_graph_replay_equals_eager_steps(pkg, O):
    K.run_graph_replay(pkg, O, MP32)


@pytest.mark.parametrize("knobs", [{"grid": 2}, {"nontemporal": 0}, {"nontemporal": 1}, {"wgpc": 4},
                                   {"blocks_per_cu": 1}, {"flat_small": 0}, {"nontemporal": 1, "grid": 2}])
def test_knobs_change_no_bits(pkg, knobs):
    K.run_knobs(pkg, MP32, knobs)


def test_checkpoints(pkg, O):
    K.run_checkpoints(pkg, O, MP32)


def test_attach_errors(pkg):
    K.run_attach_errors(pkg, MP32)


def test_virtual_trainer_fused_gt(pkg, O):
    K.run_trainer(pkg, O, MP32)
