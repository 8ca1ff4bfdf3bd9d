"""The weight-direction tangent reference (tests/param_tangent_ref.py) pinned without a GPU: by duality against
the float64 VJP oracle INCLUDING its weight gradients (<gy, v'> == <gx, v> + sum <g_theta, dtheta>), one step and
three chained steps through ``grad_helpers.bptt_oracle``, by a central difference of ``nca_oracle.nca_step`` in
the weights on states whose masks and ReLUs stay clear of their thresholds (the margins are asserted), and
against ``tangent_ref.nca_step_jvp``, which a zero direction reproduces exactly.
"""
import types

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from oracle import nca_oracle_vjp as V
from tests import grad_helpers as GH
from tests import param_tangent_ref as PR
from tests import shape_class_cases as SC
from tests import tangent_ref as TR

DUAL_IDS = ("p5", "p6", "p10", "p13")     # fire masks on p5 / p13, GroupNorm off on p10


def _tangent(name, seed=0):
    c = SC.CASES[name]
    g = torch.Generator().manual_seed(555 + SC.seed(name) + seed)
    return torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g).numpy().astype(np.float64)


def _direction(name, p, seed=0):
    """A dense N(0,1) direction for every parameter of the case that a direction may perturb."""
    g = torch.Generator().manual_seed(909 + SC.seed(name) + seed)
    return {k: torch.randn(tuple(np.shape(p[k])), generator=g).numpy().astype(np.float64)
            for k in PR.DIRECTION_KEYS if k in p}


def _fire64(name):
    f = SC.fire_mask(name)
    return None if f is None else f.numpy().astype(np.float64)


def _pool(a):
    B, _, H, W = a.shape
    ap = np.full((B, 1, H + 2, W + 2), -np.inf)
    ap[:, :, 1:-1, 1:-1] = a
    return np.max([ap[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)


def test_directions_cover_every_parameter_of_the_cases():
    have = set()
    for n in DUAL_IDS:
        have |= set(_direction(n, SC.params64(n)))
    assert have == set(PR.DIRECTION_KEYS)
    assert any(SC.CASES[n]["fire_rate"] < 1 for n in DUAL_IDS) and any(not SC.CASES[n]["gn"] for n in DUAL_IDS)
    assert not any(SC.CASES[n]["zp"] for n in DUAL_IDS)


@pytest.mark.parametrize("name", DUAL_IDS)
def test_duality_against_the_vjp_oracle(name):
    """<gy, v'> == <gx, v> + sum_theta <g_theta, dtheta> with (gx, g_theta) from nca_step_vjp, to 1e-10 relative."""
    c = SC.CASES[name]
    x = SC.state(name).numpy().astype(np.float64)
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0] if c["graph"] else None
    fire = _fire64(name)
    v, gy, dp = _tangent(name), SC.cotangent(name).numpy().astype(np.float64), _direction(name, p)
    x_out, v_out = PR.nca_step_param_jvp(x, p, cfg, v, dp, chosen=chosen, fire_mask=fire)
    np.testing.assert_allclose(x_out, O.nca_step(x, p, cfg, chosen=chosen, fire_mask=fire), rtol=0, atol=1e-13)
    gx, grads = V.nca_step_vjp(x, p, cfg, gy, chosen=chosen, fire_mask=fire)
    assert set(dp) <= set(grads), (name, set(dp) - set(grads))
    lhs = float((gy * v_out).sum())
    terms = [float((gx * v).sum())] + [float((grads[k] * dp[k]).sum()) for k in dp]
    rhs = float(sum(terms))
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (name, lhs, rhs)
    # each tensor's term on its own (v = 0, one tensor's direction): no term hides behind another
    for k in dp:
        _, vk = PR.nca_step_param_jvp(x, p, cfg, 0 * v, {k: dp[k]}, chosen=chosen, fire_mask=fire)
        a, b = float((gy * vk).sum()), float((grads[k] * dp[k]).sum())
        assert abs(a - b) <= 1e-10 * max(abs(a), abs(b)), (name, k, a, b)
    # linear in the pair
    _, v2 = PR.nca_step_param_jvp(x, p, cfg, 2 * v, {k: 2 * t for k, t in dp.items()}, chosen=chosen, fire_mask=fire)
    np.testing.assert_array_equal(v2, 2 * v_out)


@pytest.mark.parametrize("name", DUAL_IDS)
def test_zero_direction_is_the_state_tangent(name):
    c = SC.CASES[name]
    x = SC.state(name).numpy().astype(np.float64)
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0] if c["graph"] else None
    fire, v = _fire64(name), _tangent(name)
    x_ref, v_ref = TR.nca_step_jvp(x, p, cfg, v, chosen=chosen, fire_mask=fire)
    for dp in ({}, {k: 0 * t for k, t in _direction(name, p).items()}):
        x_out, v_out = PR.nca_step_param_jvp(x, p, cfg, v, dp, chosen=chosen, fire_mask=fire)
        np.testing.assert_array_equal(x_out, x_ref)
        np.testing.assert_array_equal(v_out, v_ref)


def test_three_chained_steps_against_bptt_oracle():
    """<dL/dx_T, v_T> == <dL/dx_0, v> + sum_theta <dL/dtheta, dtheta> with both gradients from
    grad_helpers.bptt_oracle on a three-step rollout with per-step offsets, a message-off step, a fire mask and a
    masked sample."""
    name = "p13"
    c = SC.CASES[name]
    B, T = c["B"], 3
    x = SC.state(name).numpy().astype(np.float64)
    p, base = SC.params64(name), SC.oracle_cfg(name)
    offs = SC.offsets(name, T)
    g = torch.Generator().manual_seed(31)
    fire = (torch.rand(T, B, 1, c["H"], c["W"], generator=g) <= 0.5).numpy().astype(np.float64)
    active = np.ones((T, B), bool)
    active[2, 0] = False
    use_graph, rates = [True, False, True], [0.5, 1.0, 0.5]
    case = types.SimpleNamespace(
        x_in=x, meta={"rollout": T}, cfg=lambda: dict(base), active=active, use_graph=use_graph,
        fire_mask=fire, fire_rates=rates, offsets=offs,
        target=torch.rand(4, c["H"], c["W"], generator=g).numpy().astype(np.float64))
    step_fn = lambda s, cfg, ch, f: O.nca_step(s, p, cfg, chosen=ch, fire_mask=f)                 # noqa: E731
    vjp_fn = lambda s, cfg, gy, ch, f: V.nca_step_vjp(s, p, cfg, gy, chosen=ch, fire_mask=f)      # noqa: E731
    x_T, _, g0, gw = GH.bptt_oracle(case, step_fn, vjp_fn)
    _, gT = GH.premult_loss_and_grad(x_T, case.target)
    v, dp = _tangent(name), _direction(name, p)
    steps_kw = [dict(chosen=offs[t], active=active[t], message_gain=base["message_gain"] if use_graph[t] else 0.0,
                     fire_mask=fire[t] if rates[t] < 1.0 else None) for t in range(T)]
    xs, vs = PR.rollout_param_jvp(x, p, base, v, dp, steps_kw)
    np.testing.assert_allclose(xs, x_T, rtol=0, atol=1e-12)
    lhs = float((gT * vs).sum())
    terms = [float((g0 * v).sum())] + [float((gw[k] * dp[k]).sum()) for k in dp]
    rhs = float(sum(terms))
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    # the weights alone (v = 0): the identity that checks BPTT weight gradients
    _, v0 = PR.rollout_param_jvp(x, p, base, 0 * v, dp, steps_kw)
    lhs0, rhs0 = float((gT * v0).sum()), float(sum(terms[1:]))
    assert abs(lhs0 - rhs0) <= 1e-10 * max(abs(lhs0), abs(rhs0)), (lhs0, rhs0)


@pytest.mark.parametrize("name", DUAL_IDS)
def test_central_difference_in_the_weights(name):
    """(step(x; theta + e dtheta) - step(x; theta - e dtheta)) / 2e in float64, v = 0, on a state whose post-update
    pooled alpha and hidden pre-activations stay further from their thresholds than the segment theta +- e dtheta
    can move them, so that no mask and no ReLU flips along it; the margins are asserted.  (The pre-update and
    sender masks read x alone, which does not move.)"""
    c = SC.CASES[name]
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0] if c["graph"] else None
    fire = _fire64(name)
    x = SC.state(name).numpy().astype(np.float64)
    thr = float(np.float32(c["thr"]))
    x[:, 3] = np.where(x[:, 3] > 0, 0.5 + 0.4 * x[:, 3], 0.0)   # alpha: 0 on the upper third, >= 0.5 below
    dp = _direction(name, p)
    eps = 1e-8
    _, v_out, det = PR.nca_step_param_jvp(x, p, cfg, 0 * x, dp, chosen=chosen, fire_mask=fire, return_details=True)
    # |d hpre| <= eps (max|dW1| * max_cell |y|_1 + max|db1|)
    reach_h = eps * (float(np.abs(dp["update_net.0.weight"]).max()) * det["y_l1"] +
                     float(np.abs(dp["update_net.0.bias"]).max()))
    margin_h = float(np.abs(det["hpre"]).min())
    margin_post = float(np.abs(_pool(det["xt"][:, 3:4]) - thr).min())
    assert margin_h > 2 * reach_h, (name, margin_h, reach_h)
    # the updated alpha moves by eps |v'_alpha| to first order (v_out is that derivative where the gate is open, and
    # update_gain (1 - t^2) xn' is bounded by it wherever the gate is shut on a channel other than alpha)
    assert margin_post > 4 * eps * max(1.0, float(np.abs(v_out).max())), (name, margin_post)
    pp = {k: (t + eps * dp[k] if k in dp else t) for k, t in p.items()}
    pm = {k: (t - eps * dp[k] if k in dp else t) for k, t in p.items()}
    fd = (O.nca_step(x, pp, cfg, chosen=chosen, fire_mask=fire) - O.nca_step(x, pm, cfg, chosen=chosen, fire_mask=fire)) / (2 * eps)
    # float64 cancellation: 2^-52 |x'| / eps ~ 1e-7 for |x'| of a few units; second order: eps^2 |dtheta|^2, negligible
    err = float(np.abs(fd - v_out).max())
    assert err <= 2.0 ** -52 * max(1.0, float(np.abs(x).max())) * 8 / eps, (name, err)


def test_zero_padded_shift_is_refused():
    name = "p7"
    x = SC.state(name).numpy().astype(np.float64)
    with pytest.raises(ValueError):
        PR.nca_step_param_jvp(x, SC.params64(name), SC.oracle_cfg(name), x, {}, chosen=SC.offsets(name)[0])
