"""CPU reference of the weight-direction tangent of the NCA step -- TEST INFRASTRUCTURE ONLY.

``tests/tangent_ref.py`` with a direction of the weights carried beside the state tangent, written out in
numpy on ``oracle/nca_oracle.py``'s functions with the same conventions: the alive, sender and fire masks are
constants, the perception bank is frozen, and in torus mode the offset weights are the constant 1/k, so the
query, key and scaling directions have exactly zero effect and are not read.  Torus mode only.  Every
function takes the dtype of its input.

With ``y = perceive(x)``, ``hpre``, ``h = relu(hpre)``, ``s_z = 1/k sum_o shift_o(A_send z)``, ``cnt`` = live
senders / k, ``m``, ``xhat``, ``rstd`` and ``t = tanh(xn)`` the primal step's intermediates at ``x``, the pair
``(v, dtheta)`` with ``dtheta = (dW1, db1, dW2, dgamma, dbeta, dWm, dbm)`` is carried to ``v'``::

    h'  = [hpre > 0] (W1 perceive(v) + dW1 y + db1)
    u'  = (W2 h' + dW2 h
           + message_gain (1 - tanh^2(m)) hidden_only(Wm s_v + dWm s_x + dbm cnt)) fire A_pre
    xn' = gamma rstd (u' - mean(u') - xhat mean(xhat u')) + dgamma xhat + dbeta     (without GroupNorm xn' = u')
    v'  = v + update_gain (1 - t^2) xn';   v'[:, 3] *= post_alive(x')

The ``dgamma xhat + dbeta`` term applies at every cell, dead and unfired ones included.  A direction is a dict
keyed by state_dict names; a missing key is a zero direction.
"""
from __future__ import annotations

import numpy as np

from oracle.nca_oracle import alive_mask, conv1x1, perceive, shift_roll

DIRECTION_KEYS = ("update_net.0.weight", "update_net.0.bias", "update_net.2.weight", "norm.weight", "norm.bias",
                  "graph.msg_proj.weight", "graph.msg_proj.bias")


def nca_step_param_jvp(x: np.ndarray, p: dict, cfg: dict, v: np.ndarray, dp: dict, *, chosen=None, fire_mask=None,
                       post_alive=None, return_details=False):
    """``(x_out, v_out)``: the step at ``x`` and its tangent applied to the pair ``(v, dp)``.

    ``post_alive`` and ``return_details`` as ``tangent_ref.nca_step_jvp``'s (the details gain ``y_l1``, the
    largest L1 norm of a cell's perception vector, which bounds how far a weight nudge moves ``hpre``)."""
    if cfg.get("zero_padded_shift", False) and cfg.get("graph", True) and chosen:
        raise ValueError("the tangent reference covers torus mode only")
    dt = x.dtype
    v = v.astype(dt)
    B, C, H, W = x.shape
    f = lambda k: np.asarray(p[k], dt)  # noqa: E731
    d = lambda k: np.asarray(dp[k], dt).reshape(np.shape(p[k])) if k in dp else np.zeros(np.shape(p[k]), dt)  # noqa: E731
    W1 = f("update_net.0.weight").reshape(-1, 3 * C)
    b1 = f("update_net.0.bias")
    W2 = f("update_net.2.weight").reshape(C, -1)
    dW1 = d("update_net.0.weight").reshape(-1, 3 * C)
    db1 = d("update_net.0.bias")
    dW2 = d("update_net.2.weight").reshape(C, -1)
    pw = p["perception.conv.weight"]
    graph = cfg.get("graph", True)
    chosen = list(chosen or [])
    # primal
    y = perceive(x, pw)
    hpre = conv1x1(y, W1, b1)
    h = np.maximum(hpre, 0)
    u = conv1x1(h, W2, None)
    ud = conv1x1((hpre > 0) * (conv1x1(perceive(v, pw), W1, None) + conv1x1(y, dW1, db1)), W2, None) \
        + conv1x1(h, dW2, None)
    if graph and chosen:
        Wm, bm = f("graph.msg_proj.weight").reshape(C, C), f("graph.msg_proj.bias")
        dWm, dbm = d("graph.msg_proj.weight").reshape(C, C), d("graph.msg_proj.bias")
        a2a = cfg["alive_to_alive"]
        A_send = alive_mask(x, cfg.get("graph_alpha_thr", cfg["alpha_thr"])) if a2a else np.ones((B, 1, H, W), dt)
        M = conv1x1(x, Wm, bm) * A_send
        Md = (conv1x1(v, Wm, None) + conv1x1(x, dWm, dbm)) * A_send
        wo = dt.type(1.0) / dt.type(len(chosen))
        m = sum(shift_roll(M, dy, dx) for dy, dx in chosen) * wo
        md = sum(shift_roll(Md, dy, dx) for dy, dx in chosen) * wo
        if cfg["hidden_only"] and C >= 4:
            m[:, :4] = 0
            md[:, :4] = 0
        tm = np.tanh(m)
        g = dt.type(cfg["message_gain"])
        u = u + tm * g
        ud = ud + g * (1 - tm * tm) * md
    fire = np.ones((B, 1, H, W), dt) if fire_mask is None else fire_mask.astype(dt)
    A_pre = alive_mask(x, cfg["alpha_thr"])
    u = u * fire * A_pre
    ud = ud * fire * A_pre
    if cfg.get("use_groupnorm", True):
        mean = lambda z: z.reshape(B, -1).mean(1)[:, None, None, None]  # noqa: E731
        mu = mean(u)
        rstd = 1.0 / np.sqrt(u.reshape(B, -1).var(1) + dt.type(cfg.get("gn_eps", 1e-3)))[:, None, None, None]
        xhat = (u - mu) * rstd
        gam = f("norm.weight")[None, :, None, None]
        xn = xhat * gam + f("norm.bias")[None, :, None, None]
        xnd = gam * rstd * (ud - mean(ud) - xhat * mean(xhat * ud)) \
            + d("norm.weight")[None, :, None, None] * xhat + d("norm.bias")[None, :, None, None]
    else:
        xn, xnd = u, ud
    t = np.tanh(xn)
    gain = dt.type(cfg["update_gain"])
    xt = x + t * gain
    vt = v + gain * (1 - t * t) * xnd
    post = alive_mask(xt, cfg["alpha_thr"])
    gate = post if post_alive is None else np.asarray(post_alive, dt).reshape(post.shape)
    x_out, v_out = xt.copy(), vt.copy()
    x_out[:, 3:4] *= gate
    v_out[:, 3:4] *= gate
    if return_details:
        a = x[:, 3:4]
        ap = np.full((B, 1, H + 2, W + 2), -np.inf, dt)
        ap[:, :, 1:-1, 1:-1] = a
        pooled = np.max([ap[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)
        return x_out, v_out, dict(hpre=hpre, pooled_pre=pooled, xt=xt, post=gate,
                                  y_l1=float(np.abs(y).sum(1).max()))
    return x_out, v_out


def rollout_param_jvp(x, p, cfg, v, dp, steps_kw: list):
    """Chain ``nca_step_param_jvp`` with the one direction ``dp`` over ``steps_kw``: one dict of keyword arguments
    per step, which may hold ``active`` (a [B] bool array: the other samples pass ``x`` and ``v`` through and
    receive no parameter term) and ``message_gain`` (this step's gain; 0 ignores ``dWm`` / ``dbm``)."""
    for kw in steps_kw:
        kw = dict(kw)
        active = kw.pop("active", None)
        scfg = dict(cfg, message_gain=kw.pop("message_gain")) if "message_gain" in kw else cfg
        m = np.ones(x.shape[0], bool) if active is None else np.asarray(active, bool)
        if not m.any():
            continue
        for k in ("fire_mask", "post_alive"):
            if kw.get(k) is not None:
                kw[k] = np.asarray(kw[k])[m]
        xo, vo = nca_step_param_jvp(x[m], p, scfg, v[m], dp, **kw)
        x, v = x.copy(), v.copy()
        x[m], v[m] = xo, vo
    return x, v
