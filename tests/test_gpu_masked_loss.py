"""The classic objective on the GPU (``masked_loss`` / ``stability_loss``: gnca_loss_masked_f32,
gnca_loss_stability_f32 and their backwards) against the float64 oracle of tests/loss_ref.py and the
reference trainers' own results (tests/golden/loss/loss_*.npz).

Tolerances (derived, not tuned):

* value: ``|got - ref64| <= 1e-6 (|primary| + |bg_alpha| + |bg_rgb| + |area|)``.  The primary's terms are
  non-negative and carry 3 fp32 roundings each (the difference, its square, the cast: <= 1.8e-7
  relative), the penalties are exact products summed in fp64, the knobs are rounded to fp32 once
  (<= 6e-8) and the result once more.
* gradient, per sample: ``|got - ref64| <= 2e-6 max|ref64 gradient of that sample|``: at most about 5 fp32
  roundings (6e-7) on terms whose absolute sum is within 2x of that maximum for knobs <= 1.
* stability: value 1e-6 relative, gradient ``2e-6 max|ref64|``.
"""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_ref as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "loss_*.npz")))
KNOBS = (0.2, 0.3, 0.7, 0.4)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _data(B, H, W, C, per_sample, seed):
    """pred in [-0.2, 1.2] with some exact zeros, inside a C-channel state; a target about half alive."""
    rng = np.random.default_rng(seed)
    state = rng.standard_normal((B, C, H, W)).astype(np.float32)
    state[:, :4] = rng.random((B, 4, H, W), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
    state[:, :3][rng.random((B, 3, H, W)) < 0.05] = 0
    target = rng.random((B if per_sample else 1, 4, H, W), dtype=np.float32)
    target[:, 3] = np.where(target[:, 3] > 0.5, target[:, 3], np.float32(0.4) * target[:, 3])
    return state, target


def _check_value(got, m, what):
    scale = np.abs(m.primary) + np.abs(m.bg_alpha) + np.abs(m.bg_rgb) + np.abs(m.area)
    err = np.abs(got.astype(np.float64) - m.value)
    print(f"{what}: value err / scale = {(err / np.maximum(scale, 1e-300)).max():.3e} (bound 1e-6)")
    assert (err <= 1e-6 * scale).all(), (what, got, m.value)


def _check_grad(got, ref, what, bound=2e-6):
    B = ref.shape[0]
    err = np.abs(got.astype(np.float64) - ref).reshape(B, -1).max(1)
    top = np.abs(ref).reshape(B, -1).max(1)
    print(f"{what}: grad err / max|ref| per sample = {err / np.maximum(top, 1e-300)} (bound {bound})")
    assert (err <= bound * top).all(), (what, err, top)


def _run_masked(dev, state, target, knobs, g, C, **kw):
    """-> (per_sample, extra outputs, d/d state of sum(g * per_sample)), through the slice state[:, :4]."""
    from graph_neural_cellular_automata_amd.loss import masked_loss
    x = torch.from_numpy(state).to(dev).requires_grad_(True)
    t = torch.from_numpy(target).to(dev)
    out = masked_loss(x[:, :4] if C > 4 else x, t, *knobs, **kw)
    per = out[0] if isinstance(out, tuple) else out
    (per * torch.from_numpy(np.asarray(g, np.float32)).to(dev)).sum().backward()
    return per.detach(), out, x.grad


# (B, H, W, channels of the state pred is a slice of, per-sample target, target given as [4,H,W])
PARITY = [(1, 7, 7, 4, True, True), (5, 9, 13, 16, True, False), (3, 24, 30, 16, False, False),
          (2, 40, 40, 4, True, False), (2, 72, 72, 16, False, True)]


@pytest.mark.parametrize("B,H,W,C,per_sample,squeeze", PARITY, ids=[f"b{p[0]}_{p[1]}x{p[2]}c{p[3]}" for p in PARITY])
def test_random_parity_with_the_oracle(dev, B, H, W, C, per_sample, squeeze):
    from graph_neural_cellular_automata_amd.loss import stability_loss
    state, target = _data(B, H, W, C, per_sample, 100 * H + W)
    g = np.arange(1, B + 1, dtype=np.float32)
    tgt = target[0] if squeeze and target.shape[0] == 1 else target
    m = LR.masked_loss(state[:, :4], target, *KNOBS, g=g)
    per, _, grad = _run_masked(dev, state, tgt, KNOBS, g, C)
    assert per.shape == (B,) and per.dtype == torch.float32
    _check_value(per.cpu().numpy(), m, f"masked {B}x{H}x{W}")
    _check_grad(grad[:, :4].cpu().numpy(), m.grad, f"masked {B}x{H}x{W}")
    assert not grad[:, 4:].any()
    # stability with about half the batch close (B = 1: the one sample)
    close = np.arange(B) % 2 == 0
    sv, sg = LR.stability_loss(state[:, :4], target, close, g=0.5)
    x = torch.from_numpy(state).to(dev).requires_grad_(True)
    loss = stability_loss(x[:, :4] if C > 4 else x, torch.from_numpy(tgt).to(dev), torch.from_numpy(close).to(dev))
    assert loss.shape == () and loss.dtype == torch.float32
    (0.5 * loss).backward()
    print(f"stability {B}x{H}x{W}: value rel err {abs(float(loss.detach()) - sv) / sv:.3e}")
    assert abs(float(loss.detach()) - sv) <= 1e-6 * abs(sv)
    gs = x.grad[:, :4].cpu().numpy()
    err, top = np.abs(gs - sg).max(), np.abs(sg).max()
    print(f"stability {B}x{H}x{W}: grad err / max|ref| = {err / top:.3e}")
    assert err <= 2e-6 * top
    assert not gs[~close].any() and not x.grad[:, 4:].any()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity(dev, name):
    from graph_neural_cellular_automata_amd.loss import stability_loss
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    knobs = (meta["alpha_thr"], meta["lam_area"], meta["lam_bg_alpha"], meta["lam_bg_rgb"])
    m = LR.masked_loss(z["pred"], z["target"], *knobs, g=z["g"])     # (= the fixture's f64: test_loss_api_cpu)
    per, _, grad = _run_masked(dev, z["pred"], z["target"], knobs, z["g"], 4)
    got = per.cpu().numpy()
    scale = np.abs(m.primary) + np.abs(m.bg_alpha) + np.abs(m.bg_rgb) + np.abs(m.area)
    err = np.abs(got.astype(np.float64) - z["value_f64"])
    print(f"{name}: value {got} err {err} scale {scale}")
    assert (err <= 1e-6 * scale).all()
    _check_grad(grad.cpu().numpy(), z["grad_f64"], name)
    x = torch.from_numpy(z["pred"]).to(dev).requires_grad_(True)
    loss = stability_loss(x, torch.from_numpy(z["target"]).to(dev), torch.from_numpy(z["close"]).to(dev))
    (meta["stability_g"] * loss).backward()
    assert abs(float(loss.detach()) - float(z["stab_f64"])) <= 1e-6 * abs(float(z["stab_f64"]))
    assert np.abs(x.grad.cpu().numpy() - z["stab_grad_f64"]).max() <= 2e-6 * np.abs(z["stab_grad_f64"]).max()


def test_defaults_are_the_classic_trainers(dev):
    """``masked_loss(pred, target)`` is the classic function's default call (0.2, 5e-5, no background terms)."""
    from graph_neural_cellular_automata_amd.loss import masked_loss
    z = np.load(os.path.join(GOLDEN, "loss_classic_b3_9x13.npz"))
    x, t = torch.from_numpy(z["pred"]).to(dev), torch.from_numpy(z["target"]).to(dev)
    got = masked_loss(x, t)
    assert torch.equal(got, masked_loss(x, t, 0.2, 5e-5, 0.0, 0.0)) and not got.requires_grad
    assert (np.abs(got.cpu().numpy() - z["value_f64"]) <= 1e-6 * np.abs(z["value_f64"])).all()


def test_exactness(dev):
    """Two calls are bitwise equal; a sample's value is bitwise the same alone and at another batch
    position, from a state slice or a contiguous tensor, with a broadcast or a repeated target; the alive
    counts are the oracle's; nsteps is (per_sample < thr) * K with the strict comparison pinned."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd.loss import masked_loss
    from graph_neural_cellular_automata_amd.step import stream_ptr
    import ctypes
    B, H, W = 5, 24, 30
    state, target = _data(B, H, W, 16, True, 7)
    x, t = torch.from_numpy(state).to(dev), torch.from_numpy(target).to(dev)
    full = masked_loss(x[:, :4], t, *KNOBS)
    assert torch.equal(full, masked_loss(x[:, :4], t, *KNOBS))
    assert torch.equal(full, masked_loss(x[:, :4].contiguous(), t, *KNOBS))
    for n in range(B):
        assert torch.equal(masked_loss(x[n:n + 1, :4], t[n:n + 1], *KNOBS)[0], full[n]), n
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(masked_loss(x[perm][:, :4], t[perm], *KNOBS), full[perm])
    assert torch.equal(masked_loss(x[:, :4], t[2], *KNOBS), masked_loss(x[:, :4], t[2:3].expand(B, -1, -1, -1).contiguous(), *KNOBS))
    # the alive count, through the C ABI (the wrapper keeps it for the backward)
    d = L.MaskedLossDesc()
    d.B, d.H, d.W = B, H, W
    d.alpha_thr, d.lam_area, d.lam_bg_alpha, d.lam_bg_rgb = KNOBS
    out = torch.empty(B, dtype=torch.float32, device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    L.check(L.load().gnca_loss_masked_f32(ctypes.byref(d), x.data_ptr(), x.stride(0), t.data_ptr(), t.stride(0),
                                          out.data_ptr(), cnt.data_ptr(), None, stream_ptr(dev)), "gnca_loss_masked_f32")
    ref = LR.masked_loss(state[:, :4], target, *KNOBS)
    assert np.array_equal(cnt.cpu().numpy(), ref.alive_count) and torch.equal(out, full)
    # nsteps: thr is sample 1's own fp32 value, so sample 1 is NOT close (strict <)
    K = 24
    thr = float(full[1])
    per, k = masked_loss(x[:, :4], t, *KNOBS, stability=(thr, K))
    assert torch.equal(per, full) and k.dtype == torch.int32 and k.shape == (B,) and not k.requires_grad
    want = (full < thr).int() * K
    print(f"per_sample {full.tolist()} thr {thr!r} nsteps {k.tolist()}")
    assert torch.equal(k, want) and int(k[1]) == 0 and 0 < int((k > 0).sum()) < B
    # one ulp above: sample 1 is close too; K = 0 is allowed
    up = float(np.nextafter(np.float32(thr), np.float32(np.inf)))
    assert int(masked_loss(x[:, :4], t, *KNOBS, stability=(up, K))[1][1]) == K
    assert not masked_loss(x[:, :4], t, *KNOBS, stability=(1e9, 0))[1].any()
    # nsteps is not differentiable and does not disturb the gradient
    xg = x.clone().requires_grad_(True)
    per, k = masked_loss(xg[:, :4], t, *KNOBS, stability=(thr, K))
    assert per.requires_grad and not k.requires_grad
    per.sum().backward()
    xh = x.clone().requires_grad_(True)
    masked_loss(xh[:, :4], t, *KNOBS).sum().backward()
    assert torch.equal(xg.grad, xh.grad)


def test_edges(dev):
    from graph_neural_cellular_automata_amd.loss import masked_loss, stability_loss
    B, H, W = 3, 9, 13
    state, target = _data(B, H, W, 4, True, 3)
    target[0, 3] = 0                                    # nothing alive in sample 0
    target[1, 3] = 1                                    # everything alive in sample 1
    state[0, 0, 0, 0], state[0, 1, 0, 1] = 0, -0.0
    g = np.array([2.0, 1.0, 0.5], np.float32)
    m = LR.masked_loss(state, target, *KNOBS, g=g)
    per, _, grad = _run_masked(dev, state, target, KNOBS, g, 4)
    assert torch.isfinite(per).all() and torch.isfinite(grad).all()
    _check_value(per.cpu().numpy(), m, "edges")
    _check_grad(grad.cpu().numpy(), m.grad, "edges")
    # n_b = 0: the penalty terms only
    hw = float(H * W)
    g0 = grad[0].cpu().numpy().astype(np.float64)
    assert np.abs(g0[3] - 2.0 * (KNOBS[2] + KNOBS[1]) / hw).max() <= 2e-6 * 2.0 / hw
    assert np.abs(g0[:3] - 2.0 * KNOBS[3] * np.sign(state[0, :3].astype(np.float64)) / (3 * hw)).max() <= 2e-6 * 2.0 / hw
    assert g0[0, 0, 0] == 0.0 and g0[1, 0, 1] == 0.0    # sign(0) = 0
    # everything alive: no background term in rgb
    assert np.array_equal(m.alive_count, [0, H * W, m.alive_count[2]])
    # stability: nothing close -> exactly 0, a zero gradient, no NaN
    x = torch.from_numpy(state).to(dev).requires_grad_(True)
    t = torch.from_numpy(target).to(dev)
    none = torch.zeros(B, dtype=torch.bool, device=dev)
    loss = stability_loss(x, t, none)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not x.grad.any() and torch.isfinite(x.grad).all()
    # NaNs in samples that are not close are never read
    poisoned = torch.from_numpy(state).to(dev)
    poisoned[1] = float("nan")
    poisoned.requires_grad_(True)
    close = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    lp = stability_loss(poisoned, t, close)
    lp.backward()
    sv, sg = LR.stability_loss(state, target, [True, False, True])
    assert abs(float(lp.detach()) - sv) <= 1e-6 * sv and not poisoned.grad[1].any()
    assert np.abs(poisoned.grad.cpu().numpy() - sg).max() <= 2e-6 * np.abs(sg).max()
    assert torch.equal(lp, stability_loss(poisoned.detach(), t, close.bool()))
    # everything close: F.mse_loss on the whole batch
    x.grad = None
    every = stability_loss(x, t, ~none)
    every.backward()
    ref = F.mse_loss(torch.from_numpy(state).double(), torch.from_numpy(target).double())
    assert abs(float(every.detach()) - float(ref)) <= 1e-6 * float(ref)
    assert torch.equal(every, stability_loss(x.detach(), t, ~none))
    # B = 1, both ways
    one = stability_loss(x[2:3].detach(), t[2:3], torch.ones(1, dtype=torch.bool, device=dev))
    assert abs(float(one) - float(F.mse_loss(torch.from_numpy(state[2]).double(), torch.from_numpy(target[2]).double()))) <= 1e-6 * float(one)
    assert float(stability_loss(x[2:3].detach(), t[2:3], torch.zeros(1, dtype=torch.bool, device=dev))) == 0.0
    assert torch.equal(masked_loss(x[2:3].detach(), t[2:3], *KNOBS)[0], per[2])


# ---- the classic iteration, fused against the torch formulas on the same device tensors ----
def _torch_masked(pred, target, alpha_thr, lam_area, lam_bg_alpha=0.0, lam_bg_rgb=0.0):
    alive = (target[:, 3:4] > alpha_thr).float()
    dead = 1.0 - alive
    primary = (((pred - target) ** 2) * alive).sum(dim=(1, 2, 3)) / (alive.sum(dim=(1, 2, 3)) + 1e-8)
    return (primary + lam_bg_alpha * (pred[:, 3:4] * dead).mean(dim=(1, 2, 3))
            + lam_bg_rgb * (pred[:, :3] * dead).abs().mean(dim=(1, 2, 3)) + lam_area * pred[:, 3:4].mean(dim=(1, 2, 3)))


def test_classic_iteration_composes(dev):
    """NeuralCA(16), B=4, 16x16: 6 steps with nsteps, masked_loss with stability=(thr, 3), 3 more steps on the
    close samples, stability_loss; against the same iteration with the torch formulas (and their host
    wait) on the same seeds: identical nsteps, parameter gradients within the BPTT bound."""
    from graph_neural_cellular_automata_amd import NeuralCA
    from graph_neural_cellular_automata_amd.loss import masked_loss, stability_loss
    torch.manual_seed(0)
    model = NeuralCA(16, 128, update_gain=0.05, alpha_thr=0.12).to(dev)
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    B, H, T, K = 4, 16, 6, 3
    gen = torch.Generator(device=dev).manual_seed(5)
    x0 = torch.rand(B, 16, H, H, device=dev, generator=gen)
    x0[:, 4:] = torch.randn(B, 12, H, H, device=dev, generator=gen) * 0.3
    target = torch.rand(B, 4, H, H, device=dev, generator=gen)
    target[:, 3] = (target[:, 3] > 0.4).float()
    target[:, :3] *= target[:, 3:4]
    nca_steps = torch.tensor([6, 4, 6, 5], dtype=torch.int32, device=dev)
    kw1, kw2 = dict(fire_rate=0.5, seed=11), dict(fire_rate=0.6, seed=12)
    with torch.no_grad():
        pre = masked_loss(model.rollout(x0, T, nsteps=nca_steps, **kw1)[:, :4], target, 0.2, 5e-5)
    s = torch.sort(pre).values
    thr = float((s[1] + s[2]) / 2)          # two of the four samples are close
    assert float(s[1]) < thr < float(s[2])

    def grads():
        g = [p.grad.clone() for p in model.parameters() if p.grad is not None]
        model.zero_grad(set_to_none=True)
        return g

    state = model.rollout(x0, T, nsteps=nca_steps, **kw1)
    per_sample, k = masked_loss(state[:, :4], target, 0.2, 5e-5, stability=(thr, K))
    stab = model.rollout(state, K, nsteps=k, **kw2)
    loss = per_sample.mean() + 0.5 * stability_loss(stab[:, :4], target, k > 0)
    loss.backward()
    fused = grads()

    state = model.rollout(x0, T, nsteps=nca_steps, **kw1)
    per_t = _torch_masked(state[:, :4], target, 0.2, 5e-5)
    close = per_t.detach() < thr
    k_t = close.int() * K
    stab = model.rollout(state, K, nsteps=k_t, **kw2)
    assert close.any()
    loss_t = per_t.mean() + 0.5 * F.mse_loss(stab[close, :4], target[close])
    loss_t.backward()
    twin = grads()

    assert torch.equal(k, k_t) and int((k > 0).sum()) == 2
    print(f"loss fused {float(loss.detach()):.8f} torch {float(loss_t.detach()):.8f}")
    assert abs(float(loss.detach()) - float(loss_t.detach())) <= 1e-6 * abs(float(loss_t.detach())) + 1e-7
    assert len(fused) == len(twin) > 0
    for a, b in zip(fused, twin):
        err, top = float((a - b).abs().max()), float(b.abs().max())
        print(f"param grad {tuple(b.shape)}: err {err:.3e} max|ref| {top:.3e}")
        assert err <= 5e-5 * top + 1e-6
