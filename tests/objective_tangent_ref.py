"""CPU reference of the forward-mode objective -- TEST INFRASTRUCTURE ONLY.

Numpy float64 on ``tests/param_tangent_ref.py`` (the chained tangents with weight directions) and
``tests/loss_ref.py`` (the masked loss and its gradient); the premultiplied loss and its gradient per sample are
written out here as ``tests/grad_helpers.premult_loss_and_grad`` writes the batch mean's.

``rollout_objective_jvp`` carries K pairs ``(v_k, dtheta_k)`` beside one primal through a step list and, after
every tapped step, forms ``losses[r, b]`` and ``dlosses[r, k, b] = <d losses[r, b] / d S, v_k[b]>``.
``bptt_with_taps`` is the reverse-mode counterpart (``oracle/nca_oracle_vjp.py`` with the tap gradients added
between two steps), and ``forward_gradient`` the assembly ``g = scale sum_k (sum_r w_r sum_b dl[r,k,b]) dir_k``.
"""
from __future__ import annotations

import numpy as np

from tests import loss_ref as LR
from tests import param_tangent_ref as PR


def premult_loss(pred: np.ndarray, target: np.ndarray):
    """(value [B], grad [B,4,H,W]) of the per-sample premultiplied-RGBA MSE and d value[b] / d pred[b]."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    if target.ndim == 3:
        target = target[None]
    B, _, H, W = pred.shape
    a = pred[:, 3:4]
    r_rgb = pred[:, :3] * a - target[:, :3]
    r_a = a - target[:, 3:4]
    n = 4 * H * W
    value = ((r_rgb ** 2).sum(axis=(1, 2, 3)) + (r_a ** 2).sum(axis=(1, 2, 3))) / n
    g = np.empty((B, 4, H, W), np.float64)
    g[:, :3] = (2.0 / n) * r_rgb * a
    g[:, 3:4] = (2.0 / n) * ((r_rgb * pred[:, :3]).sum(1, keepdims=True) + r_a)
    return value, g


def tap_loss(kind: str, state: np.ndarray, target: np.ndarray, knobs=None):
    """(value [B], grad [B,4,H,W] float64) of one tap: the loss of ``state[:, :4]`` per sample with g = 1.  The
    masked kind takes the float32 state and target (its alive mask is a float32 comparison)."""
    if kind == "premult":
        return premult_loss(state[:, :4], target)
    m = LR.masked_loss(np.asarray(state[:, :4], np.float32), np.asarray(target, np.float32), *knobs)
    return m.value, m.grad


def dlosses_of(grad: np.ndarray, V: np.ndarray) -> np.ndarray:
    """[K,B]: the dot of the tap's gradient [B,4,H,W] with channels 0..3 of each tangent of V [K,B,C,H,W]."""
    return np.einsum("bchw,kbchw->kb", grad, np.asarray(V, np.float64)[:, :, :4])


def rollout_objective_jvp(x, p, cfg, V, dps, steps_kw: list, taps: list, kind: str, target, knobs=None):
    """(x_final, v_final [K,...], losses [R,B], dlosses [R,K,B]) of the step list ``steps_kw`` (one dict per step,
    as ``param_tangent_ref.rollout_param_jvp`` takes them) with taps after the steps ``taps`` (from 1)."""
    x = np.asarray(x, np.float64)
    K = len(dps)
    vs = [np.zeros_like(x) if V is None else np.asarray(V[k], np.float64) for k in range(K)]
    losses, dl = [], []
    for t, kw in enumerate(steps_kw):
        outs = [PR.rollout_param_jvp(x, p, cfg, vs[k], dps[k], [kw]) for k in range(K)]
        x, vs = outs[0][0], [o[1] for o in outs]
        if t + 1 in taps:
            value, grad = tap_loss(kind, x, target, knobs)
            losses.append(value)
            dl.append(dlosses_of(grad, np.stack(vs)))
    return x, np.stack(vs), np.stack(losses), np.stack(dl)


def bptt_with_taps(x, p, cfg, steps_kw: list, taps: list, kind: str, target, weights, knobs=None):
    """(gx, {name: grad}) of ``sum_{r,b} weights[r,b] losses[r,b]`` in float64: the steps forward, then
    ``nca_step_vjp`` backward with each tap's gradient added before the step that produced the tapped state: the
    loop of ``grad_helpers.bptt_oracle`` with losses at the tapped steps.  Pure float64, the steps' own masks (a
    ``post_alive`` in ``steps_kw`` is not supported)."""
    from oracle import nca_oracle as O
    from oracle import nca_oracle_vjp as VJ
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    tape, states = [], [x]
    for kw in steps_kw:
        kw = dict(kw)
        m = np.ones(B, bool) if kw.get("active") is None else np.asarray(kw["active"], bool)
        scfg = dict(cfg, message_gain=kw["message_gain"]) if "message_gain" in kw else cfg
        fire = None if kw.get("fire_mask") is None else np.asarray(kw["fire_mask"], np.float64)[m]
        tape.append((x[m], m, scfg, kw.get("chosen"), fire))
        x = x.copy()
        if m.any():
            x[m] = O.nca_step(x[m], p, scfg, chosen=kw.get("chosen"), fire_mask=fire)
        states.append(x)
    g = np.zeros_like(x)
    total = {}
    for t in range(len(steps_kw), 0, -1):
        if t in taps:
            _, grad = tap_loss(kind, states[t], target, knobs)
            g = g.copy()
            g[:, :4] += np.asarray(weights, np.float64)[taps.index(t)][:, None, None, None] * grad
        sub, m, scfg, chosen, fire = tape[t - 1]
        if not m.any():
            continue
        gx, grads = VJ.nca_step_vjp(sub, p, scfg, g[m], chosen=chosen, fire_mask=fire)
        g = g.copy()
        g[m] = gx
        for k, v in grads.items():
            total[k] = total.get(k, 0) + v
    return g, total


def forward_gradient(dlosses: np.ndarray, dirs: np.ndarray, tap_weights=None, scale=None):
    """(coef [K], g [P]) of dlosses [R,K,B] and the directions dirs [K,P], in float64."""
    R, K, B = dlosses.shape
    w = np.ones(R) if tap_weights is None else np.asarray(tap_weights, np.float64)
    scale = 1.0 / (K * B) if scale is None else scale
    coef = scale * np.einsum("r,rk->k", w, dlosses.sum(axis=2))
    return coef, coef @ np.asarray(dirs, np.float64)
