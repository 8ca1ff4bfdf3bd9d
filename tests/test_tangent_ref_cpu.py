"""The tangent reference (tests/tangent_ref.py) pinned twice without a GPU: by duality against the
float64 VJP oracle (<gy, J v> == <J^T gy, v>), one step and three chained steps through
``grad_helpers.bptt_oracle``, and by a central difference of ``nca_oracle.nca_step`` on a state whose
pooled alpha and hidden pre-activations stay clear of their thresholds (the test asserts that margin).
"""
import types

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from oracle import nca_oracle_vjp as V
from tests import grad_helpers as GH
from tests import shape_class_cases as SC
from tests import tangent_ref as TR

DUAL_IDS = ("p5", "p6", "p10", "p13")     # fire masks on p5 / p13, GroupNorm off on p10


def _tangent(name, B=None, seed=0):
    c = SC.CASES[name]
    g = torch.Generator().manual_seed(555 + SC.seed(name) + seed)
    return torch.randn(c["B"] if B is None else B, c["C"], c["H"], c["W"], generator=g).numpy().astype(np.float64)


def _fire64(name):
    f = SC.fire_mask(name)
    return None if f is None else f.numpy().astype(np.float64)


def test_case_choice_covers_fire_and_no_groupnorm():
    assert any(SC.CASES[n]["fire_rate"] < 1 for n in DUAL_IDS)
    assert any(not SC.CASES[n]["gn"] for n in DUAL_IDS)
    assert any(SC.CASES[n]["graph"] and SC.CASES[n]["gn"] for n in DUAL_IDS)
    assert not any(SC.CASES[n]["zp"] for n in DUAL_IDS)


@pytest.mark.parametrize("name", DUAL_IDS)
def test_duality_against_the_vjp_oracle(name):
    """<gy, J v> from tangent_ref equals <J^T gy, v> from nca_step_vjp to 1e-10 relative (float64)."""
    c = SC.CASES[name]
    x = SC.state(name).numpy().astype(np.float64)
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0] if c["graph"] else None
    fire = _fire64(name)
    v, gy = _tangent(name), SC.cotangent(name).numpy().astype(np.float64)
    x_out, v_out = TR.nca_step_jvp(x, p, cfg, v, chosen=chosen, fire_mask=fire)
    # (the reference normalises by rstd as the VJP oracle does, the step oracle divides: last-bit differences)
    np.testing.assert_allclose(x_out, O.nca_step(x, p, cfg, chosen=chosen, fire_mask=fire), rtol=0, atol=1e-13)
    gx, _ = V.nca_step_vjp(x, p, cfg, gy, chosen=chosen, fire_mask=fire)
    lhs, rhs = float((gy * v_out).sum()), float((gx * v).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (name, lhs, rhs)
    # linear in v
    _, v2 = TR.nca_step_jvp(x, p, cfg, 2 * v, chosen=chosen, fire_mask=fire)
    np.testing.assert_array_equal(v2, 2 * v_out)


def test_post_alive_replaces_the_gate():
    name = "p6"
    x = SC.state(name).numpy().astype(np.float64)
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0]
    v = _tangent(name)
    none = np.zeros((x.shape[0], 1) + x.shape[2:])
    x_out, v_out = TR.nca_step_jvp(x, p, cfg, v, chosen=chosen, post_alive=none)
    assert not x_out[:, 3].any() and not v_out[:, 3].any()
    _, v_all = TR.nca_step_jvp(x, p, cfg, v, chosen=chosen, post_alive=np.ones_like(none))
    np.testing.assert_array_equal(v_all[:, [0, 1, 2, 4, 5]], v_out[:, [0, 1, 2, 4, 5]])


def test_three_chained_steps_against_bptt_oracle():
    """<dL/dx_T, J_3 J_2 J_1 v> == <dL/dx_0, v> with dL/dx_0 from grad_helpers.bptt_oracle on a
    three-step rollout with per-step offsets, a message-off step, a fire mask and a masked sample."""
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
    case = types.SimpleNamespace(
        x_in=x, meta={"rollout": T}, cfg=lambda: dict(base), active=active, use_graph=[True, False, True],
        fire_mask=fire, fire_rates=[0.5, 1.0, 0.5], offsets=offs,
        target=torch.rand(4, c["H"], c["W"], generator=g).numpy().astype(np.float64))
    step_fn = lambda s, cfg, ch, f: O.nca_step(s, p, cfg, chosen=ch, fire_mask=f)                 # noqa: E731
    vjp_fn = lambda s, cfg, gy, ch, f: V.nca_step_vjp(s, p, cfg, gy, chosen=ch, fire_mask=f)      # noqa: E731
    x_T, _, g0, _ = GH.bptt_oracle(case, step_fn, vjp_fn)
    _, gT = GH.premult_loss_and_grad(x_T, case.target)
    v = _tangent(name)
    xs, vs = x, v
    for t in range(T):
        m = active[t]
        cfg = dict(base, message_gain=base["message_gain"] if case.use_graph[t] else 0.0)
        f = fire[t][m] if case.fire_rates[t] < 1.0 else None
        xo, vo = TR.nca_step_jvp(xs[m], p, cfg, vs[m], chosen=offs[t], fire_mask=f)
        xs, vs = xs.copy(), vs.copy()
        xs[m], vs[m] = xo, vo
    np.testing.assert_allclose(xs, x_T, rtol=0, atol=1e-12)
    lhs, rhs = float((gT * vs).sum()), float((g0 * v).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_central_difference_with_asserted_margins():
    """A second, independent pin: (step(x + e v) - step(x - e v)) / 2e in float64 on a state whose
    pooled alpha (pre- and post-update) and hidden pre-activations stay further from their thresholds
    than the segment x +- e v can move them, so that no mask and no ReLU flips along it; the test
    asserts those margins."""
    name = "p6"
    c = SC.CASES[name]
    p, cfg = SC.params64(name), SC.oracle_cfg(name)
    chosen = SC.offsets(name)[0]
    x = SC.state(name).numpy().astype(np.float64)
    thr = float(np.float32(c["thr"]))
    x[:, 3] = np.where(x[:, 3] > 0, 0.5 + 0.4 * x[:, 3], 0.0)   # alpha: 0 on the upper third, >= 0.5 below
    v = _tangent(name)
    eps = 1e-8
    _, v_out, det = TR.nca_step_jvp(x, p, cfg, v, chosen=chosen, return_details=True)
    vmax = float(np.abs(v).max())
    # |d hpre| <= eps max|v| * (largest L1 norm of a perception filter: Sobel, 8) * max_row |W1|_1
    reach_h = eps * vmax * 8 * float(np.abs(p["update_net.0.weight"].reshape(c["hidden"], -1)).sum(1).max())
    margin_h = float(np.abs(det["hpre"]).min())
    margin_pre = float(np.abs(det["pooled_pre"] - thr).min())
    margin_post = float(np.abs(_pool(det["xt"][:, 3:4]) - thr).min())
    assert margin_h > 2 * reach_h, (margin_h, reach_h)
    assert margin_pre > 2 * eps * vmax, margin_pre
    # the updated alpha moves by eps |v'_alpha| to first order (v_out is that derivative where the gate is open)
    assert margin_post > 4 * eps * max(vmax, float(np.abs(v_out).max())), margin_post
    fd = (O.nca_step(x + eps * v, p, cfg, chosen=chosen) - O.nca_step(x - eps * v, p, cfg, chosen=chosen)) / (2 * eps)
    # float64 cancellation: 2^-52 |x'| / eps ~ 1e-7 for |x'| of a few units; second order: eps^2, negligible
    err = float(np.abs(fd - v_out).max())
    assert err <= 2.0 ** -52 * max(1.0, float(np.abs(x).max())) * 8 / eps, err


def _pool(a):
    B, _, H, W = a.shape
    ap = np.full((B, 1, H + 2, W + 2), -np.inf)
    ap[:, :, 1:-1, 1:-1] = a
    return np.max([ap[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)


def test_zero_padded_shift_is_refused():
    name = "p7"
    x = SC.state(name).numpy().astype(np.float64)
    with pytest.raises(ValueError):
        TR.nca_step_jvp(x, SC.params64(name), SC.oracle_cfg(name), x, chosen=SC.offsets(name)[0])
