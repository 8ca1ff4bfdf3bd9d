"""CPU reference of the forward-mode tangent of the NCA step -- TEST INFRASTRUCTURE ONLY.

The Jacobian-vector product of one step, written out in numpy on ``oracle/nca_oracle.py``'s functions
with the conventions of ``oracle/nca_oracle_vjp.py``: the pre- and post-update alive masks, the sender
mask and the fire mask are constants, the perception bank is frozen, and in torus mode the offset
weights are the constant 1/k.  Torus mode only (the zero-padded shift's offset weights depend on the
state; the library refuses it).  Every function takes the dtype of its input.

With ``hpre``, ``m`` (the message before tanh, after the hidden-only zeroing), ``xhat``, ``rstd`` and
``t = tanh(xn)`` the primal step's intermediates at ``x``, one step ``x -> x'`` carries ``v -> v'``::

    y'  = perceive(v)
    h'  = [hpre > 0] (W1 y')
    u'  = W2 h' + message_gain (1 - tanh^2(m)) hidden_only(sum_o w_o shift_o(A_send (Wm v)))
    u'  = u' fire A_pre
    xn' = gamma rstd (u' - mean(u') - xhat mean(xhat u'))       (without GroupNorm xn' = u')
    v'  = v + update_gain (1 - t^2) xn';   v'[:, 3] *= post_alive(x')
"""
from __future__ import annotations

import numpy as np

from oracle.nca_oracle import alive_mask, conv1x1, perceive, shift_roll


def nca_step_jvp(x: np.ndarray, p: dict, cfg: dict, v: np.ndarray, *, chosen=None, fire_mask=None,
                 post_alive=None, return_details=False):
    """``(x_out, v_out)``: the step at ``x`` and its tangent applied to ``v``.

    ``post_alive``: a [B,1,H,W] {0,1} array that replaces the post-update alive mask computed here, in
    the gate of ``x_out`` and of ``v_out`` alike (``nca_step_vjp``'s argument).
    ``return_details``: also a dict with ``hpre``, ``pooled_pre`` (the 3x3-pooled alpha of ``x``),
    ``xt`` (the updated state before the gate) and ``post`` (the mask used)."""
    if cfg.get("zero_padded_shift", False) and cfg.get("graph", True) and chosen:
        raise ValueError("the tangent reference covers torus mode only")
    dt = x.dtype
    v = v.astype(dt)
    B, C, H, W = x.shape
    f = lambda k: np.asarray(p[k], dt)  # noqa: E731
    W1 = f("update_net.0.weight").reshape(-1, 3 * C)
    b1 = f("update_net.0.bias")
    W2 = f("update_net.2.weight").reshape(C, -1)
    pw = p["perception.conv.weight"]
    graph = cfg.get("graph", True)
    chosen = list(chosen or [])
    # primal
    hpre = conv1x1(perceive(x, pw), W1, b1)
    u = conv1x1(np.maximum(hpre, 0), W2, None)
    ud = conv1x1((hpre > 0) * conv1x1(perceive(v, pw), W1, None), W2, None)
    if graph and chosen:
        Wm, bm = f("graph.msg_proj.weight").reshape(C, C), f("graph.msg_proj.bias")
        a2a = cfg["alive_to_alive"]
        A_send = alive_mask(x, cfg.get("graph_alpha_thr", cfg["alpha_thr"])) if a2a else np.ones((B, 1, H, W), dt)
        M, Md = conv1x1(x, Wm, bm) * A_send, conv1x1(v, Wm, None) * A_send
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
        xnd = gam * rstd * (ud - mean(ud) - xhat * mean(xhat * ud))
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
        return x_out, v_out, dict(hpre=hpre, pooled_pre=pooled, xt=xt, post=gate)
    return x_out, v_out


def rollout_jvp(x, p, cfg, v, steps_kw: list):
    """Chain ``nca_step_jvp`` over ``steps_kw`` (one dict of keyword arguments per step)."""
    for kw in steps_kw:
        x, v = nca_step_jvp(x, p, cfg, v, **kw)
    return x, v
