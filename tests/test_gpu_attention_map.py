"""The standalone attention-map op (gnca_attention_f32, GraphAugmentation.attention_map) on the GPU:
against the reference's recorded maps (golden fixtures), the float64 oracle, the step's own
``return_attention`` path, and itself (bitwise run to run).

Tolerance: |map - ref| <= 2e-5 on the min-max normalised map (values in [0, 1]), the bound
test_gpu_parity.py sets for this map.  Normalising divides by the raw map's range, so the oracle
cases use seeded inputs whose float64 raw range is at least 1e-2 per sample, asserted on the oracle.
"""
import random

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests.golden_io import Case

pytestmark = pytest.mark.gpu

ATOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ["graph_torus_latest_attn_b2_40", "graph_zeropad_ep380_attn_b1_40"])
def test_matches_reference_fixture(dev, name):
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import desc_for, weights_on
    c = Case(name)
    B, C, H, W = c.x_in.shape
    desc = desc_for(c, B, H, W, c.chosen(0), 0, attention=False)
    w, keep = S.make_weights(weights_on(c, dev))
    got = S.attention_map(desc, w, torch.from_numpy(c.x_in).to(dev)).cpu().numpy()
    err = float(np.abs(got - c.attn).max())
    print(f"[attention_map] {name}: max |hip - reference| = {err:.3e}")
    np.testing.assert_allclose(got, c.attn, rtol=0, atol=ATOL)


# (B, C, H, W, r, K)
SHAPES = {
    "ragged_2x16x17x29_r4_k8": (2, 16, 17, 29, 4, 8),      # wrap and pad on every side
    "tiny_1x4x5x7_r2_k40": (1, 4, 5, 7, 2, 40),            # k clamped to the 16 offsets, halo > canvas
    "c32_3x32x24x24_r5_k16": (3, 32, 24, 24, 5, 16),
    "tiles_2x12x72x72_r4_k8": (2, 12, 72, 72, 4, 8),       # several workgroups per sample
}


def _graph_and_state(shape, zp, a2a, dev, K=None):
    """A default-initialised GraphAugmentation and a uniform state with a dead region (alpha = 0 on
    the upper half of the canvas, so the sender mask matters), both seeded."""
    from graph_neural_cellular_automata_amd import GraphAugmentation
    B, C, H, W, r, k = shape
    torch.manual_seed(1000 + 7 * H + W + C)
    g = GraphAugmentation(C, d_model=16, attention_radius=r, num_neighbors=k if K is None else K,
                          alive_to_alive=a2a, zero_padded_shift=zp, alpha_thr=0.1).to(dev)
    x = torch.rand(B, C, H, W)
    x[:, 3, : (H + 1) // 2] = 0.0
    x[:, 3, :, : max(1, W // 4)] *= 0.05
    return g, x


def _oracle_map(g, x, chosen):
    """(normalised map, per-sample raw range) in float64, from the oracle's own building blocks."""
    p = {"graph." + k: v.detach().cpu().numpy().astype(np.float64) for k, v in g.state_dict().items()}
    x64 = x.numpy().astype(np.float64)
    _, attn = O.graph_message(x64, p, chosen, zero_padded_shift=g.zero_padded_shift,
                              alive_to_alive=g.alive_to_alive, alpha_thr=g.alpha_thr, return_attention=True)
    if not chosen:
        return attn, None
    shift = O.shift_pad if g.zero_padded_shift else O.shift_roll
    M = O.conv1x1(x64, p["graph.msg_proj.weight"], p["graph.msg_proj.bias"])
    Wt = O.offset_weights(x64, p, chosen, zero_padded_shift=g.zero_padded_shift)
    A = O.alive_mask(x64, g.alpha_thr) if g.alive_to_alive else np.ones_like(x64[:, :1])
    raw = sum(np.abs(Wt[o][:, None, None, None] * shift(M * A, dy, dx)).mean(axis=1)
              for o, (dy, dx) in enumerate(chosen))
    rng = raw.max(axis=(1, 2)) - raw.min(axis=(1, 2))
    # the restated raw map normalises to the oracle's map: the range asserted is the oracle's
    norm = (raw - raw.min(axis=(1, 2), keepdims=True)) / (rng[:, None, None] + 1e-8)
    np.testing.assert_allclose(norm, attn, rtol=0, atol=1e-12)
    return attn, rng


@pytest.mark.parametrize("a2a", [True, False], ids=["a2a", "all"])
@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_matches_f64_oracle(dev, shape, zp, a2a):
    g, x = _graph_and_state(SHAPES[shape], zp, a2a, dev)
    random.seed(5)
    chosen = g.sample_offsets()
    assert len(chosen) == min(SHAPES[shape][5], len(g.offsets))
    ref, rng = _oracle_map(g, x, chosen)
    assert (rng >= 1e-2).all(), f"oracle raw range {rng} too small for a normalised comparison"
    got = g.attention_map(x.to(dev), offsets=chosen)
    assert got.shape == ref.shape and not got.requires_grad
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"[attention_map] {shape} {'zeropad' if zp else 'torus'} a2a={a2a}: raw range >= {rng.min():.3f}, "
          f"max |hip - f64| = {err:.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=ATOL)


@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
def test_no_offsets_gives_zeros(dev, zp):
    """k = 0 (num_neighbors = 0, or an empty offset list): zeros, as graph_augmentation.py:141-147."""
    g, x = _graph_and_state(SHAPES["ragged_2x16x17x29_r4_k8"], zp, True, dev, K=0)
    assert g.sample_offsets() == []
    got = g.attention_map(x.to(dev))
    assert got.shape == (2, 17, 29) and torch.count_nonzero(got).item() == 0
    assert torch.count_nonzero(g.attention_map(x.to(dev), offsets=[])).item() == 0
    ref, _ = _oracle_map(g, x, [])
    assert not ref.any()


@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
def test_matches_step_attention_path(dev, zp):
    """The map ``model(x, return_attention=True)`` returns (K1's GNCA_ATTENTION path) on the same
    offsets; also ``offsets=None`` draws exactly the one ``random.sample`` forward draws."""
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    torch.manual_seed(3)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=0.25,
                          graph_zero_padded_shift=zp).to(dev).eval()
    x = torch.rand(2, 16, 40, 40)
    x[:, 3, :13] = 0.0
    x = x.to(dev)
    random.seed(8)
    with torch.no_grad():
        _, ref = model(x, return_attention=True)
    after = random.random()
    random.seed(8)
    chosen = model.graph.sample_offsets()
    got = model.graph.attention_map(x, offsets=chosen)
    err = float((got - ref).abs().max())
    print(f"[attention_map] vs the step's return_attention ({'zeropad' if zp else 'torus'}): {err:.3e}")
    assert err <= ATOL, err
    random.seed(8)
    drawn = model.graph.attention_map(x)
    assert random.random() == after
    assert torch.equal(drawn, got)


@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
def test_bitwise_reproducible(dev, zp):
    g, x = _graph_and_state(SHAPES["tiles_2x12x72x72_r4_k8"], zp, True, dev)
    random.seed(6)
    chosen = g.sample_offsets()
    xd = x.to(dev)
    a = g.attention_map(xd, offsets=chosen)
    b = g.attention_map(xd, offsets=chosen)
    assert torch.equal(a, b)
    assert float(a.min()) == 0.0 and 0.999 < float(a.max()) <= 1.0   # min-max normalised per sample
