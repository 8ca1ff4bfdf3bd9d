"""CPU reference of the Gauss-Newton product -- TEST INFRASTRUCTURE ONLY.

Numpy float64 on ``tests/param_tangent_ref.py`` (the chained tangent with a weight direction), ``tests/loss_ref.py``
(the masked loss's alive mask) and the loop of ``tests/objective_tangent_ref.py::bptt_with_taps`` with the injected
loss gradients replaced by the taps' curvature fields.

``gauss_newton`` carries ONE pair ``(v, dtheta)`` beside the primal through a step list, forms after every tapped
step ``field_r = P^T H P v_r`` (the loss's Gauss-Newton curvature at the tapped state applied to its tangent) and
``quad_r = v_r^T P^T H P v_r``, then runs ``nca_step_vjp`` backward with ``scale[r] * field_r`` added before the
step that produced the tapped state: ``product = G_tt dtheta + G_tx v``, ``gx = G_xt dtheta + G_xx v``.
"""
from __future__ import annotations

import numpy as np

from tests import loss_ref as LR
from tests import objective_tangent_ref as OR
from tests import param_tangent_ref as PR


def premult_curvature(state4, v4):
    """(field [B,4,H,W], quad [B]) of the premultiplied loss: p = (rgb * a, a), H = (2/N) I, the residual term
    (p - target) d2p/dS2 dropped.  The expressions and their order are the kernel's."""
    S, v = np.asarray(state4, np.float64), np.asarray(v4, np.float64)
    B, _, H, W = S.shape
    s = 2.0 / (4.0 * float(H * W))
    a, v3 = S[:, 3], v[:, 3]
    field = np.empty_like(S)
    fa, e = v3.copy(), v3 * v3
    for c in range(3):
        pd = a * v[:, c] + S[:, c] * v3
        field[:, c] = s * a * pd
        fa = fa + S[:, c] * pd
        e = e + pd * pd
    field[:, 3] = s * fa
    return field, s * e.sum(axis=(1, 2))


def premult_jacobian(state4):
    """[B,H,W,4,4]: d p_i / d S_j per pixel of p = (S_0 S_3, S_1 S_3, S_2 S_3, S_3)."""
    S = np.asarray(state4, np.float64)
    B, _, H, W = S.shape
    J = np.zeros((B, H, W, 4, 4))
    for c in range(3):
        J[..., c, c] = S[:, 3]
        J[..., c, 3] = S[:, c]
    J[..., 3, 3] = 1.0
    return J


def masked_curvature(target32, v4, alpha_thr):
    """(field [B,4,H,W], quad [B]) of the masked loss: 2 alive v / D with D = n + 1e-8 and n the target's alive
    cell count (the float32 comparison); the penalties carry no curvature."""
    v = np.asarray(v4, np.float64)
    B, _, H, W = v.shape
    alive = np.broadcast_to(LR.alive_mask(np.asarray(target32, np.float32), alpha_thr), (B, 1, H, W)).astype(np.float64)
    D = alive.sum(axis=(1, 2, 3)) + 1e-8
    field = 2.0 * (alive * v) / D[:, None, None, None]
    return field, 2.0 * (alive * v * v).sum(axis=(1, 2, 3)) / D


def tap_curvature(kind: str, state, v, target, knobs=None):
    """(field [B,4,H,W], quad [B]) of one tap at ``state`` along the tangent ``v`` (channels 0..3 are read)."""
    if kind == "premult":
        return premult_curvature(np.asarray(state)[:, :4], np.asarray(v)[:, :4])
    return masked_curvature(target, np.asarray(v)[:, :4], knobs[0])


def gauss_newton(x, p, cfg, v, dp, steps_kw: list, taps: list, kind: str, target, scale, knobs=None, states=None):
    """One Gauss-Newton product in float64.  ``steps_kw``: one dict per step as ``param_tangent_ref.rollout_param_jvp``
    takes them; ``taps``: tapped steps (from 1); ``scale``: one number per tap; ``v``: a tangent of ``x`` or None;
    ``dp``: a weight direction (may be empty).  ``states``: None, or the T + 1 states S_0 .. S_T a float32 run
    produced: every step then starts from the float64 copy of that run's own input state (teacher forcing, with
    the run's post mask in ``steps_kw[t]["post_alive"]``) and the loss terms are taken at its tapped states.

    Returns a dict: ``x_final``, ``losses`` [R,B], ``dlosses`` [R,B], ``quad`` [R,B], ``fields`` [R,B,4,H,W],
    ``gx``, ``product`` {name: array} and ``energy`` = sum_r scale_r sum_b quad[r,b]."""
    from oracle import nca_oracle_vjp as VJ
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    vv = np.zeros_like(x) if v is None else np.asarray(v, np.float64)
    dp = dict(dp or {})
    ins, losses, dl, quad, fields = [], [], [], [], []
    for t, kw in enumerate(steps_kw):
        xin = x if states is None else np.asarray(states[t], np.float64)
        ins.append(xin)
        x, vv = PR.rollout_param_jvp(xin, p, cfg, vv, dp, [kw])
        if t + 1 in taps:
            st = x if states is None else np.asarray(states[t + 1])
            st_l = st if kind == "premult" else np.asarray(st, np.float32)
            tg = np.asarray(target, np.float64) if kind == "premult" else np.asarray(target, np.float32)
            value, grad = OR.tap_loss(kind, st_l, tg, knobs)
            f, q = tap_curvature(kind, np.asarray(st, np.float64), vv, target, knobs)
            losses.append(value)
            dl.append(OR.dlosses_of(grad, vv[None])[0])
            fields.append(f)
            quad.append(q)
    g = np.zeros_like(x)
    total = {}
    for t in range(len(steps_kw), 0, -1):
        if t in taps:
            r = taps.index(t)
            g = g.copy()
            g[:, :4] += float(scale[r]) * fields[r]
        kw = dict(steps_kw[t - 1])
        m = np.ones(B, bool) if kw.get("active") is None else np.asarray(kw["active"], bool)
        if not m.any():
            continue
        scfg = dict(cfg, message_gain=kw["message_gain"]) if "message_gain" in kw else cfg
        fire = None if kw.get("fire_mask") is None else np.asarray(kw["fire_mask"], np.float64)[m]
        post = None if kw.get("post_alive") is None else np.asarray(kw["post_alive"], np.float64)[m]
        gx, grads = VJ.nca_step_vjp(ins[t - 1][m], p, scfg, g[m], chosen=kw.get("chosen"), fire_mask=fire,
                                    post_alive=post)
        g = g.copy()
        g[m] = gx
        for k, val in grads.items():
            total[k] = total.get(k, 0) + val
    quad = np.stack(quad)
    energy = float(sum(float(scale[r]) * quad[r].sum() for r in range(len(taps))))
    return dict(x_final=x if states is None else np.asarray(states[-1], np.float64), losses=np.stack(losses),
                dlosses=np.stack(dl), quad=quad, fields=np.stack(fields), gx=g,
                product={k: val for k, val in total.items() if k in PR.DIRECTION_KEYS}, energy=energy)


def inner(res: dict, v, dp) -> float:
    """<dp, product> + <v, gx> of a ``gauss_newton`` result with the direction ``(v, dp)``."""
    s = 0.0 if v is None else float((res["gx"] * np.asarray(v, np.float64)).sum())
    for k, d in (dp or {}).items():
        if k in res["product"]:
            s += float((res["product"][k] * np.asarray(d, np.float64).reshape(res["product"][k].shape)).sum())
    return s
