"""The image metrics on the GPU (gnca_image_metrics_f32 / gnca_rollout_trace_metrics_f32) against the
float64 oracle of tests/metrics_ref.py.

Parity tolerance ``|got - ref| <= 1e-6 + 1e-6 |ref|`` for mse, psnr and ssim: the kernel's internals
are fp64, so only the fp32 premultiply (shared with the oracle) and the final rounding to fp32
(<= 1.9e-6 at 30 dB, <= 6e-8 at values <= 1) differ.  The pixel-perfect count is exact on data whose
``|P - T|`` keeps a 1e-6 margin from 0.05 (asserted on the oracle side)."""
import random

import numpy as np
import pytest
import torch

from tests import metrics_ref as MR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _target(rng, N, H, W):
    t = rng.random((N, 4, H, W), dtype=np.float32)
    t[:, :3] *= t[:, 3:4]          # premultiplied
    return t


def _noisy_pred(rng, target, C, sigma=0.035):
    """A state whose premultiplied rgba is the target plus noise: alpha = target alpha + noise (kept >= 0.02), rgb = (t + n) / alpha."""
    N, _, H, W = target.shape
    pred = rng.standard_normal((N, C, H, W)).astype(np.float32)
    a = np.clip(target[:, 3:4] + sigma * rng.standard_normal((N, 1, H, W)).astype(np.float32), 0.02, None)
    pred[:, 3:4] = a
    pred[:, :3] = (target[:, :3] + sigma * rng.standard_normal((N, 3, H, W)).astype(np.float32)) / a
    return pred


def _assert_close(got, ref, what):
    for k, name in ((0, "mse"), (2, "psnr"), (3, "ssim")):
        g, r = got[:, k].astype(np.float64), ref[:, k]
        err = np.abs(g - r)
        print(f"{what} {name}: max |got - ref| = {err.max():.3e} (ref {r})")
        assert (err <= 1e-6 + 1e-6 * np.abs(r)).all(), (what, name, g, r)


# (H, W, C, per-sample target): one window; non-square, nothing divides; wider than any tile;
# a C=16 state slice with a per-sample target; the headline canvas (3 bands of rows) with a broadcast target
PARITY = [(7, 7, 4, True), (9, 13, 4, True), (8, 131, 4, False), (40, 40, 16, True), (72, 72, 16, False)]


@pytest.mark.parametrize("H,W,C,per_sample", PARITY, ids=[f"{h}x{w}c{c}" for h, w, c, _ in PARITY])
def test_parity_with_the_oracle(dev, H, W, C, per_sample):
    from graph_neural_cellular_automata_amd.loss import loss_premult_rgba
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    rng = np.random.default_rng(H * 1000 + W)
    N = 3
    target = _target(rng, N if per_sample else 1, H, W)
    pred = rng.random((N, C, H, W), dtype=np.float32) * 1.2 - 0.1
    if C > 4:
        pred[:, 4:] = rng.standard_normal((N, C - 4, H, W)).astype(np.float32)
    ref = MR.image_metrics(pred, target)
    x, t = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
    m = image_metrics(x, t if per_sample else t[0])
    assert m.stacked.shape == (N, 4) and m.ssim.shape == (N,) and not m.stacked.requires_grad
    got = m.stacked.cpu().numpy()
    _assert_close(got, ref, f"{H}x{W}")
    assert np.abs(got[:, 1] - ref[:, 1]).max() <= 1e-6       # (the exact count: test_pixel_perfect_count)
    # the channel slice state[:, :4] is read in place through its strides: the same result, bitwise
    assert torch.equal(image_metrics(x[:, :4], t).stacked, m.stacked)
    loss = loss_premult_rgba(x[:, :4], t)
    torch.testing.assert_close(m.mse, loss, rtol=1e-6, atol=1e-7)


def test_pixel_perfect_count(dev):
    """pred = target + noise at 3 x 4 x 72 x 72: pixel_perfect * H * W is the oracle's count exactly."""
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    H = W = 72
    seed = 1     # (random data keeps the margin for about one seed in three: this one does, as asserted)
    rng = np.random.default_rng(seed)
    target = _target(rng, 3, H, W)
    pred = _noisy_pred(rng, target, 4)
    P = MR.premultiply(pred)
    d = np.abs(P.astype(np.float64) - target.astype(np.float64))
    # the conditions, on the oracle side: no |P - T| within 1e-6 of the threshold (beyond any fp32 or
    # FMA-contraction error, <= 1.2e-7), and a fraction that is neither 0 nor 1
    assert np.abs(d - 0.05).min() > 1e-6, "this seed does not keep the margin"
    counts = np.array([MR.pixel_perfect_count(P[n], target[n]) for n in range(3)])
    frac = counts / float(H * W)
    assert ((frac >= 0.2) & (frac <= 0.8)).all(), frac
    m = image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev))
    got = m.pixel_perfect.cpu().numpy().astype(np.float64) * (H * W)
    print(f"seed {seed}: counts {counts}, got {got}")
    assert np.array_equal(np.rint(got), counts) and np.abs(got - counts).max() < 1e-2
    # (a near-target image: ssim ~0.9 and psnr ~29 dB, where the relative part of the bound matters)
    _assert_close(m.stacked.cpu().numpy(), MR.image_metrics(pred, target), "noisy target")


def test_edges(dev):
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    rng = np.random.default_rng(5)
    # pred == target (alpha 1, so P == pred): ssim exactly 1, psnr +inf, mse 0, every cell perfect
    t = _target(rng, 2, 40, 29)
    t[:, 3] = 1
    x = torch.from_numpy(t).to(dev)
    m = image_metrics(x, x)
    assert torch.equal(m.ssim, torch.ones(2, device=dev)), m.ssim
    assert torch.isinf(m.psnr).all() and (m.psnr > 0).all()
    assert torch.equal(m.mse, torch.zeros(2, device=dev)) and torch.equal(m.pixel_perfect, torch.ones(2, device=dev))
    # constant images: every window has zero variance; S = (2ab + C1) / (a^2 + b^2 + C1)
    pc = np.ones((1, 4, 9, 13), np.float32)
    pc[:, :3] = 0.5
    tc = np.ones((1, 4, 9, 13), np.float32)
    tc[:, :3] = 0.25
    got = image_metrics(torch.from_numpy(pc).to(dev), torch.from_numpy(tc).to(dev)).stacked.cpu().numpy()
    ref = MR.image_metrics(pc, tc)
    _assert_close(got, ref, "constant")
    assert abs(got[0, 3] - (2 * 0.5 * 0.25 + 1e-4) / (0.25 + 0.0625 + 1e-4)) <= 2e-6
    assert got[0, 1] == 0.0
    # values outside [0, 1] are clipped for psnr and ssim only: pred 1.5 against target 1.0
    po = np.ones((1, 4, 8, 8), np.float32)
    po[:, :3] = 1.5
    to = np.ones((1, 4, 8, 8), np.float32)
    got = image_metrics(torch.from_numpy(po).to(dev), torch.from_numpy(to).to(dev)).stacked.cpu().numpy()
    assert abs(got[0, 0] - 3 * 0.25 / 4) <= 1e-7 and got[0, 1] == 0.0      # unclipped
    assert np.isinf(got[0, 2]) and got[0, 3] == 1.0                         # clipped: equal images
    ref = MR.image_metrics(po, to)
    assert np.isinf(ref[0, 2]) and abs(ref[0, 3] - 1) <= 1e-15 and abs(ref[0, 0] - got[0, 0]) <= 1e-7
    # too small for a window: NaN ssim, the other columns finite and right
    ps, ts = rng.random((2, 4, 6, 9), dtype=np.float32), _target(rng, 2, 6, 9)
    got = image_metrics(torch.from_numpy(ps).to(dev), torch.from_numpy(ts).to(dev)).stacked.cpu().numpy()
    ref = MR.image_metrics(ps, ts)
    assert np.isnan(got[:, 3]).all() and np.isnan(ref[:, 3]).all() and np.isfinite(got[:, :3]).all()
    assert (np.abs(got[:, :3] - ref[:, :3]) <= 1e-6 + 1e-6 * np.abs(ref[:, :3])).all()


@pytest.mark.parametrize("H,W", [(72, 72), (9, 131)], ids=["72x72", "9x131"])
def test_invariance(dev, H, W):
    """Image n of a batch of 5 is bitwise the same image alone and at another batch position; two runs
    are bitwise equal."""
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.random((5, 16, H, W), dtype=np.float32)).to(dev)
    t = torch.from_numpy(_target(rng, 5, H, W)).to(dev)
    full = image_metrics(x, t).stacked
    assert torch.equal(full, image_metrics(x, t).stacked)
    for n in range(5):
        assert torch.equal(image_metrics(x[n:n + 1], t[n:n + 1]).stacked[0], full[n]), n
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(image_metrics(x[perm], t[perm]).stacked, full[perm])
    # a broadcast target is the per-sample target repeated
    assert torch.equal(image_metrics(x, t[2]).stacked, image_metrics(x, t[2:3].expand(5, -1, -1, -1).contiguous()).stacked)


# ---- trace(target=...) ----
GAIN, THR, MSG, FIRE, SEED = 0.05, 0.12, 0.25, 0.5, 5
B, HH, T, EVERY = 3, 24, 7, 3


def _models(dev):
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    torch.manual_seed(0)
    g = NeuralCAGraph(16, 128, update_gain=GAIN, alpha_thr=THR, message_gain=MSG,
                      graph_zero_padded_shift=False).to(dev).eval()
    c = NeuralCA(16, 128, update_gain=GAIN, alpha_thr=THR).to(dev).eval()
    with torch.no_grad():
        g.update_net[2].weight.normal_(0, 0.05)
        c.update_net[2].weight.normal_(0, 0.05)
    return g, c


def _state(dev):
    gen = torch.Generator(device=dev).manual_seed(31)
    x = torch.rand(B, 16, HH, HH, device=dev, generator=gen)
    x[:, 4:] = torch.randn(B, 12, HH, HH, device=dev, generator=gen)
    return x


@pytest.mark.parametrize("per_sample", [False, True], ids=["broadcast", "per_sample"])
def test_trace_metrics_graph(dev, per_sample):
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    model, _ = _models(dev)
    x = _state(dev)
    rr = random.Random(17)
    offs = [rr.sample(model.graph.offsets, 8) for _ in range(T)]
    t = torch.from_numpy(_target(np.random.default_rng(2), B if per_sample else 1, HH, HH)).to(dev)
    t = t if per_sample else t[0]
    kw = dict(every=EVERY, fire_rate=FIRE, seed=SEED, offsets=offs)
    base = model.trace(x, T, **kw)
    assert base.metrics is None and base.steps == [3, 6, 7]
    tr = model.trace(x, T, target=t, **kw)
    assert tr.metrics.stacked.shape == (3, B, 4) and tr.metrics.ssim.shape == (3, B)
    assert torch.equal(tr.frames, base.frames) and torch.equal(tr.x_final, base.x_final)
    assert torch.equal(tr.metrics.stacked, image_metrics(tr.frames, t).stacked)
    assert torch.isfinite(tr.metrics.stacked).all()
    # against the oracle too, on the recorded frames
    ref = MR.image_metrics(tr.frames[1].cpu().numpy(), t.cpu().numpy())
    _assert_close(tr.metrics.stacked[1].cpu().numpy(), ref, "trace frame 1")
    # frames=False: the same metrics and x_final, no frames
    nf = model.trace(x, T, target=t, frames=False, **kw)
    assert nf.frames is None and torch.equal(nf.metrics.stacked, tr.metrics.stacked)
    assert torch.equal(nf.x_final, base.x_final) and nf.steps == base.steps
    # with maps: unchanged
    am = model.trace(x, T, return_attention=True, **kw)
    at = model.trace(x, T, return_attention=True, target=t, frames=False, **kw)
    assert torch.equal(at.attention, am.attention) and torch.equal(at.metrics.stacked, tr.metrics.stacked)
    assert torch.equal(at.x_final, base.x_final) and at.frames is None
    # frames=False without a target: x_final (and maps) only
    bare = model.trace(x, T, return_attention=True, frames=False, **kw)
    assert bare.frames is None and bare.metrics is None and torch.equal(bare.attention, am.attention)
    assert torch.equal(bare.x_final, base.x_final)


def test_trace_metrics_classic(dev):
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    _, model = _models(dev)
    x = _state(dev)
    t = torch.from_numpy(_target(np.random.default_rng(3), B, HH, HH)).to(dev)
    kw = dict(every=EVERY, fire_rate=FIRE, seed=SEED)
    base = model.trace(x, T, **kw)
    tr = model.trace(x, T, target=t, channels=16, **kw)
    assert torch.equal(tr.frames[:, :, :4], base.frames) and torch.equal(tr.x_final, base.x_final)
    assert torch.equal(tr.metrics.stacked, image_metrics(tr.frames, t).stacked)
    nf = model.trace(x, T, target=t, frames=False, **kw)
    assert nf.frames is None and torch.equal(nf.metrics.stacked, tr.metrics.stacked)
    assert torch.equal(nf.x_final, base.x_final)


def test_trace_without_target_is_todays_call(dev):
    """``trace()`` without ``target`` is bitwise gnca_rollout_trace_f32 through ``step.trace``."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    model, _ = _models(dev)
    x = _state(dev)
    rr = random.Random(17)
    offs = [rr.sample(model.graph.offsets, 8) for _ in range(T)]
    tr = model.trace(x, T, every=EVERY, return_attention=True, fire_rate=FIRE, seed=SEED, offsets=offs)
    w, keep = S.make_weights(dict(perception=model.perception.conv.weight, w1=model.update_net[0].weight,
                                  b1=model.update_net[0].bias, w2=model.update_net[2].weight,
                                  gn_weight=model.norm.weight, gn_bias=model.norm.bias,
                                  **model.graph.weight_tensors()))
    d = S.make_desc(B=B, C=16, H=HH, W=HH, hidden=128, d_model=model.graph.d_model, offsets=offs[0],
                    flags=L.USE_GROUPNORM | L.HIDDEN_ONLY | model.graph.flags(False), update_gain=GAIN,
                    alpha_thr=THR, message_gain=MSG, fire_rate=FIRE, fire_mode=L.FIRE_HASH, rng_seed=SEED)
    out, frames, attn = S.trace(d, w, x, T, offs, [3, 6, 7], 4, want_attention=True)
    assert torch.equal(tr.x_final, out) and torch.equal(tr.frames, frames) and torch.equal(tr.attention, attn)
