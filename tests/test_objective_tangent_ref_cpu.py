"""The forward-mode objective's reference (tests/objective_tangent_ref.py) pinned without a GPU: its dlosses
against the float64 BPTT with the tap gradients injected (the loop of ``grad_helpers.bptt_oracle`` with losses at
the tapped steps, as tests/test_gpu_rollout_objective.py's ``tapped_oracle`` runs it), against a central difference
of the loss on a case where no mask can flip (the margins are asserted), and the forward-gradient assembly
against the projection of the BPTT gradient onto the directions' span.
"""
import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests import objective_tangent_ref as OR
from tests import shape_class_cases as SC
from tests import tangent_ref as TR

KNOBS = (0.2, 5e-5, 1e-3, 2e-4)
T, TAPS = 3, [1, 3]


def _setup(name, K=2):
    c = SC.CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    g = torch.Generator().manual_seed(321 + SC.seed(name))
    x = SC.state(name).numpy().astype(np.float64)
    fire = (torch.rand(T, B, 1, H, W, generator=g) <= 0.5).numpy().astype(np.float64)
    target = torch.rand(B, 4, H, W, generator=g)
    target[:, 3, :, : W // 2] *= 0.15                      # dead target cells on the left half
    target = target.numpy()
    active = np.ones((T, B), bool)
    active[2, 0] = False                                   # sample 0 is frozen before the tap at T
    offs = SC.offsets(name, T) if c["graph"] else [None] * T
    steps = [dict(chosen=offs[t], fire_mask=fire[t] if t != 1 else None, active=active[t],
                  message_gain=(c["msg"] if c["graph"] and t != 1 else 0.0)) for t in range(T)]
    V = torch.randn(K, *x.shape, generator=g).numpy().astype(np.float64)
    p = SC.params64(name)
    dps = [{k: torch.randn(p[k].shape, generator=g).numpy().astype(np.float64) for k in
            ("update_net.0.weight", "update_net.0.bias", "update_net.2.weight", "norm.weight", "norm.bias",
             "graph.msg_proj.weight", "graph.msg_proj.bias") if k in p} for _ in range(K)]
    w = torch.rand(len(TAPS), B, generator=g).numpy().astype(np.float64)
    return c, x, p, SC.oracle_cfg(name), steps, target, V, dps, w


@pytest.mark.parametrize("kind", ("premult", "masked"))
@pytest.mark.parametrize("name", ("p5", "p13", "q4h64"))
def test_dlosses_against_bptt_with_injected_tap_gradients(name, kind):
    """sum_{r,b} w[r,b] dlosses[r,k,b] == <gx, v_k> + sum_theta <g_theta, dtheta_k> to 1e-10 relative."""
    c, x, p, cfg, steps, target, V, dps, w = _setup(name)
    knobs = KNOBS if kind == "masked" else None
    tgt = target.astype(np.float64) if kind == "premult" else target
    x_T, _, losses, dl = OR.rollout_objective_jvp(x, p, cfg, V, dps, steps, TAPS, kind, tgt, knobs)
    gx, grads = OR.bptt_with_taps(x, p, cfg, steps, TAPS, kind, tgt, w, knobs)
    assert losses.shape == (len(TAPS), c["B"]) and dl.shape == (len(TAPS), len(dps), c["B"])
    for k in range(len(dps)):
        lhs = float((w * dl[:, k]).sum())
        rhs = float((gx * V[k]).sum()) + sum(float((grads[n] * d).sum()) for n, d in dps[k].items() if n in grads)
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (name, kind, k, lhs, rhs)
        assert lhs != 0.0


def test_parts_alone_and_linearity():
    """V alone plus dparams alone is the pair, and doubling both doubles dlosses."""
    c, x, p, cfg, steps, target, V, dps, w = _setup("p13")
    tgt = target.astype(np.float64)
    run = lambda VV, dd: OR.rollout_objective_jvp(x, p, cfg, VV, dd, steps, TAPS, "premult", tgt)[3]   # noqa: E731
    both, v_only, d_only = run(V, dps), run(V, [{} for _ in dps]), run(None, dps)
    np.testing.assert_allclose(v_only + d_only, both, rtol=1e-12, atol=1e-14)
    twice = run(2 * V, [{k: 2 * t for k, t in d.items()} for d in dps])
    np.testing.assert_array_equal(twice, 2 * both)


def test_central_difference_of_the_loss_with_asserted_margins():
    """(loss(step(x + e v)) - loss(step(x - e v))) / 2e against dlosses on tests/test_tangent_ref_cpu.py's state,
    whose pooled alpha and hidden pre-activations stay further from their thresholds than the segment can move
    them (asserted), both kinds; the masked kind's alive mask reads the target alone."""
    name = "p6"
    c = SC.CASES[name]
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0]
    x = SC.state(name).numpy().astype(np.float64)
    thr = float(np.float32(c["thr"]))
    x[:, 3] = np.where(x[:, 3] > 0, 0.5 + 0.4 * x[:, 3], 0.0)
    g = torch.Generator().manual_seed(77)
    v = torch.randn(x.shape, generator=g).numpy().astype(np.float64)
    target = torch.rand(c["B"], 4, c["H"], c["W"], generator=g).numpy().astype(np.float64)
    eps = 1e-8
    _, v_out, det = TR.nca_step_jvp(x, p, cfg, v, chosen=chosen, return_details=True)
    vmax = float(np.abs(v).max())
    reach_h = eps * vmax * 8 * float(np.abs(p["update_net.0.weight"].reshape(c["hidden"], -1)).sum(1).max())
    assert float(np.abs(det["hpre"]).min()) > 2 * reach_h
    assert float(np.abs(det["pooled_pre"] - thr).min()) > 2 * eps * vmax
    ap = np.full((x.shape[0], 1, x.shape[2] + 2, x.shape[3] + 2), -np.inf)
    ap[:, :, 1:-1, 1:-1] = det["xt"][:, 3:4]
    pooled = np.max([ap[:, :, i:i + x.shape[2], j:j + x.shape[3]] for i in range(3) for j in range(3)], axis=0)
    assert float(np.abs(pooled - thr).min()) > 4 * eps * max(vmax, float(np.abs(v_out).max()))
    _, _, losses, dl = OR.rollout_objective_jvp(x, p, cfg, v[None], [{}], [dict(chosen=chosen)], [1], "premult",
                                                target)
    hi = OR.premult_loss(O.nca_step(x + eps * v, p, cfg, chosen=chosen)[:, :4], target)[0]
    lo = OR.premult_loss(O.nca_step(x - eps * v, p, cfg, chosen=chosen)[:, :4], target)[0]
    err = float(np.abs((hi - lo) / (2 * eps) - dl[0, 0]).max())
    # float64 cancellation of two losses of size |L|: 2^-52 |L| / eps, a few of them
    assert err <= 2.0 ** -52 * max(1.0, float(losses.max())) * 8 / eps, err
    assert float(np.abs(dl).min()) > 1e3 * err


def test_assembly_is_the_projection_of_the_bptt_gradient():
    """K orthonormal directions inside a small coordinate subspace of update_net.2.weight, scale = 1: the assembled
    vector is Q Q^T (the BPTT gradient of sum_r w_r sum_b losses[r,b])."""
    name = "p5"
    c, x, p, cfg, steps, target, _, _, _ = _setup(name)
    tgt = target.astype(np.float64)
    key = "update_net.2.weight"
    n = p[key].size
    K, D = 4, 7
    rng = np.random.default_rng(5)
    coords = rng.choice(n, D, replace=False)
    Q, _ = np.linalg.qr(rng.standard_normal((D, K)))
    dirs = np.zeros((K, n))
    dirs[:, coords] = Q.T
    np.testing.assert_allclose(dirs @ dirs.T, np.eye(K), atol=1e-14)
    dps = [{key: dirs[k].reshape(p[key].shape)} for k in range(K)]
    wr = np.array([0.25, 1.5])
    _, _, _, dl = OR.rollout_objective_jvp(x, p, cfg, None, dps, steps, TAPS, "premult", tgt)
    coef, g = OR.forward_gradient(dl, dirs, tap_weights=wr, scale=1.0)
    _, grads = OR.bptt_with_taps(x, p, cfg, steps, TAPS, "premult", tgt, np.repeat(wr[:, None], c["B"], 1))
    full = grads[key].reshape(-1)
    proj = dirs.T @ (dirs @ full)
    np.testing.assert_allclose(coef, dirs @ full, rtol=1e-10, atol=1e-14 * float(np.abs(full).max()))
    np.testing.assert_allclose(g, proj, rtol=0, atol=1e-10 * float(np.abs(proj).max()))
    assert float(np.abs(proj).max()) > 0 and not g[np.setdiff1d(np.arange(n), coords)].any()
