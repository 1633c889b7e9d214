"""Mixed-precision Lion fused into the bf16 gossip round (csrc/lion_mix_bf16.hip,
VirtualWorkerGroup.attach_lion(master_weights=True)): fp32 master rows w, bfloat16 gradients g, bfloat16
model rows p = bf16(w), and the momentum m in fp32 ("mp32") or in bfloat16 ("mp16":
momentum_dtype=torch.bfloat16).

Every comparison is against the specification restated in tests/lionref.py, never the code under test: w
and an fp32 m uint32 for uint32, p and a bfloat16 m uint16 for uint16 (a NaN of any payload where the
specification is a NaN, in the special-values test only).  The test bodies are tests/lionkit.py's, shared
with the fp32 file; the shapes are described there and in tests/test_gpu_lion_mix.py."""
import numpy as np
import pytest

import lionkit as K
import lionref
from conftest import Topo

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS = ["mp32", "mp16"]


@pytest.mark.parametrize("hyper", ["H0", "H1", "H2"])
@pytest.mark.parametrize("idle_rows", ["skip", "canonical"])
@pytest.mark.parametrize("name", ["g0", "g16", "ring32", "er64", "hand3"])
@pytest.mark.parametrize("kind", KINDS)
def test_rounds_match_spec(pkg, O, kind, name, idle_rows, hyper):
    K.run_rounds(pkg, O, K.KINDS[kind], name, idle_rows, hyper)


@pytest.mark.parametrize("kind", KINDS)
def test_signed_zero_survives_a_zero_direction(pkg, O, kind):
    K.run_signed_zero(pkg, O, K.KINDS[kind])


@pytest.mark.parametrize("where", ["x", "g", "m"])
@pytest.mark.parametrize("kind", KINDS)
def test_special_values(pkg, O, kind, where):
    K.run_special_values(pkg, O, K.KINDS[kind], where)


@pytest.mark.parametrize("kind", KINDS)
def test_abi_offsets_segments_and_guards(pkg, O, kind):
    """for a bfloat16 momentum the offsets include 8-byte-aligned ones that are not 16-byte aligned (row 1:
    the vector path) and ones that are not 8-byte aligned (the element path)"""
    K.run_abi(pkg, O, K.KINDS[kind])


@pytest.mark.parametrize("mode", ["clip", "groups", "both"])
@pytest.mark.parametrize("kind", KINDS)
def test_scaled_and_grouped(pkg, O, kind, mode):
    K.run_scaled_grouped(pkg, O, K.KINDS[kind], mode)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_equals_eager_steps(pkg, O, kind):
    K.run_graph_replay(pkg, O, K.KINDS[kind])


@pytest.mark.parametrize("knobs", [{"grid": 2}, {"nontemporal": 0}, {"nontemporal": 1}, {"wgpc": 4},
                                   {"blocks_per_cu": 1}, {"flat_small": 0}])
@pytest.mark.parametrize("kind", KINDS)
def test_knobs_change_no_bits(pkg, kind, knobs):
    K.run_knobs(pkg, K.KINDS[kind], knobs)


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoints(pkg, O, kind):
    ckpt, topo, P = K.run_checkpoints(pkg, O, K.KINDS[kind])
    other = K.KINDS["mp32" if kind == "mp16" else "mp16"]            # the other momentum dtype refuses it
    with pytest.raises(ValueError, match="momentum_dtype"):
        K.group(pkg, other, topo, P, "H1", True).load_state_dict(ckpt)


@pytest.mark.parametrize("kind", KINDS)
def test_attach_errors(pkg, kind):
    K.run_attach_errors(pkg, K.KINDS[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_virtual_trainer_fused_lion(pkg, O, kind):
    K.run_trainer(pkg, O, K.KINDS[kind])


def test_bf16_momentum_against_fp32_momentum(pkg, O):
    """20 steps of the bf16-momentum group and 20 of the fp32-momentum group from the same start and the
    same gradients: each equals its own specification bit for bit.  The two are different optimizers by
    design; the share of p elements on which they differ after 20 steps is printed, a recorded
    observation with no threshold."""
    partner, alpha = K.topology(pkg, "g0")
    steps = 20
    rng = np.random.default_rng(91)
    flags = (rng.random((steps, partner.shape[0])) < 0.5).astype(np.uint8)
    n, P = 8, 4101
    X0 = rng.standard_normal((n, P)).astype(np.float32)
    Gs = [K.rand_g(K.KINDS["mp32"], rng, (n, P)) for _ in range(steps)]
    final = {}
    for kind in KINDS:
        kd = K.KINDS[kind]
        grp = K.group(pkg, kd, Topo(partner, alpha, flags), P, "H1", True)
        K.put(grp, kd, x=X0)
        s = {"x": X0, "m": K.zero_m(kd, (n, P))}
        for it in range(steps):
            K.put(grp, kd, g=Gs[it])
            grp.lion_step(it, 1e-3)
            s = K.spec(O, kd, s, Gs[it], partner, flags[it], alpha, 1e-3, "H1")
        got = K.state(grp, kd)
        assert K.same(kd, got, s), kind
        final[kind] = got
    dp = float((final["mp16"]["p"] != final["mp32"]["p"]).mean())
    dw = float((lionref.u32(final["mp16"]["x"]) != lionref.u32(final["mp32"]["x"])).mean())
    far = float(np.abs(final["mp16"]["x"].astype(np.float64) - final["mp32"]["x"].astype(np.float64)).max())
    print(f"bf16 vs fp32 momentum after {steps} steps at lr 1e-3: p differs on {100 * dp:.2f} % of {n * P} elements, "
          f"the masters on {100 * dw:.2f} %, max |w16 - w32| = {far:.3e}")
