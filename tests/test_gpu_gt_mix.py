"""Gradient tracking (GT-DSGD) on fp32 rows (csrc/gt_track.hip and the fused SGD kernel over the trackers,
VirtualWorkerGroup.attach_gt): x, g, the tracker y, the previous gradient gp and the momentum m fp32.

Every comparison is against the specification restated in tests/gtref.py, never the code under test: x, y, gp and
m uint32 for uint32 (a NaN of any payload where the specification is a NaN, in the special-values test only),
after each of the two launches and after the pair.  The test bodies are tests/gtkit.py's, shared with the
mixed-precision file.

Shapes: the five topologies of lionkit.topology (3 workers by hand, graph 0, a 16-worker graph, a ring of 32,
ER(64)), both idle modes, three hyper sets (no momentum and no decay; momentum 0.9 with decay; Nesterov), the
widths 1..9, 63..65, 255..257, T - 1, T, T + 9, 3T + 5 (ER(64): the last three), three consecutive rounds of each
flag kind with the state carried, both zero_grads settings."""
import pytest

import gtkit as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = K.KINDS["f32"]


@pytest.mark.parametrize("hyper", ["H0", "H1", "H2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "ring32", "er64", "hand3"])
def test_rounds_match_spec(pkg, O, name, idle_rows, hyper):
    K.run_rounds(pkg, O, F32, name, idle_rows, hyper)


def test_lr_scale_zero_freezes_x_while_the_tracker_moves(pkg, O):
    K.run_lr_scale_zero(pkg, O, F32)


def test_past_the_schedule_and_peer_reads_write_nothing(pkg):
    K.run_noops(pkg, F32)


def test_refusals_write_nothing(pkg):
    K.run_refusals(pkg, F32)


@pytest.mark.parametrize("where", ["g", "gp", "y", "x"])
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
                                   {"blocks_per_cu": 1}, {"flat_small": 0}, {"nontemporal": 1, "grid": 2}])
def test_knobs_change_no_bits(pkg, knobs):
    K.run_knobs(pkg, F32, knobs)


def test_checkpoints(pkg, O):
    K.run_checkpoints(pkg, O, F32)


def test_attach_errors(pkg):
    K.run_attach_errors(pkg, F32)


def test_virtual_trainer_fused_gt(pkg, O):
    K.run_trainer(pkg, O, F32)


def test_fp32_step_is_the_fused_sgd_kernel(pkg, O):
    K.run_fp32_step_is_sgd(pkg, O)


def test_end_to_end_removes_the_heterogeneity_error(pkg, O):
    K.run_end_to_end(pkg, O)
