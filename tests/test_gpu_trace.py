"""``trace()`` on the GPU (gnca_rollout_trace_f32): the recorded frames are bitwise the prefixes of
``rollout()``, the recorded maps bitwise ``attention_map`` on the prefix states, on every rollout
plan (the small-batch fold, the one-stream compact fold, the two-sub-batch pipeline), in both graph
modes and on the classic model; two calls joined with ``first_step`` equal one; and a 64-step trace
stays within the project's drift bound of the float64 oracle (state 1e-4 with identical alive masks,
maps 2e-5).  All with ``fire_rate=0.5``, a fixed ``seed`` and fixed ``offsets``."""
import random

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests.golden_io import Case

pytestmark = pytest.mark.gpu

GAIN, THR, MSG, FIRE, SEED = 0.05, 0.12, 0.25, 0.5, 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _graph_model(dev, zp=False):
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=GAIN, alpha_thr=THR, message_gain=MSG,
                          graph_zero_padded_shift=zp).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    return model


def _state(B, H, dev, seed=31):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(B, 16, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, 12, H, H, device=dev, generator=g)
    return x


def _offsets(model, T, seed=17):
    rr = random.Random(seed)
    return [rr.sample(model.graph.offsets, 8) for _ in range(T)]


def _plan(model, B, H):
    """(compact field, fold, sub-batches) the rollout pipeline plans for this model and shape."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    d = S.make_desc(B=B, C=16, H=H, W=H, hidden=128, d_model=16, offsets=model.graph.offsets[:8],
                    flags=L.USE_GROUPNORM | L.HIDDEN_ONLY | model.graph.flags(False), update_gain=GAIN,
                    alpha_thr=THR, message_gain=MSG, fire_rate=FIRE, fire_mode=L.FIRE_HASH, rng_seed=SEED)
    return S.rollout_compact(d), S.rollout_fold(d), S.rollout_subs(d)


def _check_prefixes(model, x, T, record, offs, attention):
    kw = dict(fire_rate=FIRE, seed=SEED)
    tr = model.trace(x, T, record=record, channels=16, return_attention=attention, offsets=offs, **kw)
    assert tr.steps == record and tr.frames.shape == (len(record), *x.shape)
    assert not tr.frames.requires_grad and not tr.x_final.requires_grad
    with torch.no_grad():
        assert torch.equal(tr.x_final, model.rollout(x, T, offsets=offs, **kw)), "x_final"
        for r, t in enumerate(record):
            assert torch.equal(tr.frames[r], model.rollout(x, t, offsets=offs[:t], **kw)), f"frame after step {t}"
            if attention:
                prev = x if t == 1 else model.rollout(x, t - 1, offsets=offs[:t - 1], **kw)
                want = model.graph.attention_map(prev, offsets=offs[t - 1])
                assert torch.equal(tr.attention[r], want), f"map of step {t}"
    if not attention:
        assert tr.attention is None
    return tr


def test_prefixes_small_batch_fold(dev):
    """B=2 x 24^2, T=7, record=[1,4,7]: the dense-field fold, a record point at the first step."""
    model = _graph_model(dev)
    assert _plan(model, 2, 24) == (False, True, 1)
    _check_prefixes(model, _state(2, 24, dev), 7, [1, 4, 7], _offsets(model, 7), attention=False)


def test_prefixes_one_stream_compact_fold(dev):
    """B=128 x 72^2: the compact field folded on one stream."""
    model = _graph_model(dev)
    assert _plan(model, 128, 72) == (True, True, 1)
    _check_prefixes(model, _state(128, 72, dev), 6, [2, 5, 6], _offsets(model, 6), attention=False)


def test_prefixes_two_sub_batches(dev):
    """B=192 x 72^2: the two-stream sub-batch pipeline; with maps, which run on the caller's stream
    after each piece's sub-batch streams have joined."""
    model = _graph_model(dev)
    assert _plan(model, 192, 72) == (True, False, 2)
    _check_prefixes(model, _state(192, 72, dev), 6, [1, 3, 6], _offsets(model, 6), attention=True)


@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
def test_graph_modes_maps_and_channel_slice(dev, zp):
    """Both shift modes at B=2 x 24^2 with maps (pieces also end one step before a record point), and
    ``channels=4`` (the default) is the slice of ``channels=C``."""
    model = _graph_model(dev, zp)
    x, offs = _state(2, 24, dev), _offsets(model, 7)
    full = _check_prefixes(model, x, 7, [1, 4, 7], offs, attention=True)
    rgba = model.trace(x, 7, record=[1, 4, 7], return_attention=True, fire_rate=FIRE, seed=SEED, offsets=offs)
    assert rgba.frames.shape == (3, 2, 4, 24, 24)
    assert torch.equal(rgba.frames, full.frames[:, :, :4])
    assert torch.equal(rgba.attention, full.attention) and torch.equal(rgba.x_final, full.x_final)
    # an odd channel count and a canvas whose plane is no multiple of 4 floats: the scalar frame copy
    odd = model.trace(x[:, :, :23, :23].contiguous(), 3, every=2, channels=3, fire_rate=FIRE, seed=SEED,
                      offsets=offs[:3])
    ref = model.trace(x[:, :, :23, :23].contiguous(), 3, every=2, channels=16, fire_rate=FIRE, seed=SEED,
                      offsets=offs[:3])
    assert odd.steps == [2, 3] and torch.equal(odd.frames, ref.frames[:, :, :3])


def test_every_draws_offsets_like_rollout(dev):
    """``offsets=None``: one ``random.sample`` per step in step order, so a trace and a rollout started
    from the same ``random`` state run the same steps; ``every`` records n, 2n, ... and T."""
    model = _graph_model(dev)
    x = _state(2, 24, dev)
    random.seed(12)
    tr = model.trace(x, 7, every=3, channels=16, fire_rate=FIRE, seed=SEED)
    after = random.random()
    random.seed(12)
    with torch.no_grad():
        ref = model.rollout(x, 7, fire_rate=FIRE, seed=SEED)
    assert random.random() == after
    assert tr.steps == [3, 6, 7] and torch.equal(tr.x_final, ref) and torch.equal(tr.frames[2], ref)
    # grad mode does not matter: always no_grad, detached
    xg = x.clone().requires_grad_(True)
    random.seed(12)
    tg = model.trace(xg, 7, every=3, channels=16, fire_rate=FIRE, seed=SEED)
    assert not tg.x_final.requires_grad and tg.x_final.grad_fn is None and torch.equal(tg.frames, tr.frames)


def test_split_calls_continue_one_fire_stream(dev):
    """trace(x, 4) then trace(x_final, 3, first_step=4) with the same seed and the matching offsets is
    the 7-step trace, bitwise: "grow, damage, regrow" as two calls."""
    model = _graph_model(dev)
    x, offs = _state(2, 24, dev), _offsets(model, 7)
    kw = dict(channels=16, return_attention=True, fire_rate=FIRE, seed=SEED)
    one = model.trace(x, 7, offsets=offs, **kw)
    a = model.trace(x, 4, offsets=offs[:4], **kw)
    b = model.trace(a.x_final, 3, offsets=offs[4:], first_step=4, **kw)
    assert a.steps == [1, 2, 3, 4] and b.steps == [1, 2, 3]
    assert torch.equal(torch.cat([a.frames, b.frames]), one.frames)
    assert torch.equal(torch.cat([a.attention, b.attention]), one.attention)
    assert torch.equal(b.x_final, one.x_final)
    # without first_step the second call restarts the fire stream: a different state
    c = model.trace(a.x_final, 3, offsets=offs[4:], **kw)
    assert not torch.equal(c.x_final, one.x_final)


def test_classic_model_matches_rollout_prefixes(dev):
    from graph_neural_cellular_automata_amd import NeuralCA
    torch.manual_seed(0)
    model = NeuralCA(16, 128, update_gain=GAIN, alpha_thr=THR).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    x = _state(2, 24, dev)
    tr = model.trace(x, 7, record=[1, 4, 7], channels=16, fire_rate=FIRE, seed=SEED)
    assert tr.attention is None and tr.steps == [1, 4, 7]
    with torch.no_grad():
        for r, t in enumerate(tr.steps):
            assert torch.equal(tr.frames[r], model.rollout(x, t, fire_rate=FIRE, seed=SEED)), t
        assert torch.equal(tr.x_final, model.rollout(x, 7, fire_rate=FIRE, seed=SEED))
    with pytest.raises(ValueError):
        model.trace(x, 7, return_attention=True)


def test_drift_vs_f64_oracle(dev):
    """64 steps, every=16, B=2 x 16 x 40^2, torus, the trained nca_latest.pt weights carried by the
    golden fixtures: frames against the float64 oracle rollout <= 1e-4 with identical alive masks
    (the project's drift bound), maps against the oracle's <= 2e-5."""
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    c = Case("graph_torus_latest_grown_b1_72")
    m = c.meta
    model = NeuralCAGraph(16, 128, update_gain=m["update_gain"], alpha_thr=m["alpha_thr"],
                          message_gain=m["message_gain"], hidden_only=m["hidden_only"],
                          graph_alive_to_alive=m["alive_to_alive"], graph_zero_padded_shift=False)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.weights.items()})
    model = model.to(dev).eval()
    p64 = {k: v.astype(np.float64) for k, v in c.weights.items()}
    B, H, T = 2, 40, 64
    x = _state(B, H, dev, seed=7)
    offs = _offsets(model, T, seed=29)
    tr = model.trace(x, T, every=16, channels=16, return_attention=True, fire_rate=FIRE, seed=SEED, offsets=offs)
    assert tr.steps == [16, 32, 48, 64]
    cfg = c.cfg()
    ref = x.cpu().numpy().astype(np.float64)
    frames, maps = {}, {}
    for t in range(1, T + 1):
        fm = O.hash_fire_mask(SEED, t - 1, 0, B, H, H, FIRE)
        ref, attn = O.nca_step(ref, p64, cfg, chosen=offs[t - 1], fire_mask=fm, return_attention=True)
        if t in tr.steps:
            frames[t], maps[t] = ref, attn
    got_f, got_a = tr.frames.cpu().numpy(), tr.attention.cpu().numpy()
    errs = [float(np.abs(got_f[r] - frames[t]).max()) for r, t in enumerate(tr.steps)]
    aerrs = [float(np.abs(got_a[r] - maps[t]).max()) for r, t in enumerate(tr.steps)]
    flips = [int((O.alive_mask(got_f[r], m["alpha_thr"]) != O.alive_mask(frames[t], m["alpha_thr"])).sum())
             for r, t in enumerate(tr.steps)]
    print(f"[trace drift] steps {tr.steps}: frames max |hip - f64| = {['%.3e' % e for e in errs]}, "
          f"maps {['%.3e' % e for e in aerrs]}, alive flips {flips}")
    assert max(errs) <= 1e-4, errs
    assert sum(flips) == 0, flips
    assert max(aerrs) <= 2e-5, aerrs
    assert np.abs(tr.x_final.cpu().numpy() - frames[T]).max() <= 1e-4
