"""Float64 oracle of the classic trainer's objective: the target-masked loss with its three penalties
and the stability phase's loss, each with its gradient by torch autograd, on the CPU.

Everything is float64 except the one decision the float32 code makes on float32 data: a cell is alive
where the float32 target alpha is greater than ``np.float32(alpha_thr)`` (in float64 a target alpha
equal to ``float32(0.2)`` would count as alive, since ``float32(0.2) > 0.2``), and the denominator
``n + 1e-8`` is the float32 sum the trainer forms (``n`` itself from ``n = 1`` on; the float64 sum differs
from it by at most 1e-8 relative, far inside any bound used here).  ``masked_loss`` returns the four
components separately so that a test can scale its tolerance by them.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch


class Masked(NamedTuple):
    value: np.ndarray       # [B] float64: primary + bg_alpha + bg_rgb + area
    primary: np.ndarray     # [B] sum over alive cells and 4 channels of (pred - target)^2 / float32(n + 1e-8)
    bg_alpha: np.ndarray    # [B] lam_bg_alpha * mean(pred_alpha * dead)
    bg_rgb: np.ndarray      # [B] lam_bg_rgb * mean(|pred_rgb * dead|)
    area: np.ndarray        # [B] lam_area * mean(pred_alpha)
    alive_count: np.ndarray  # [B] int64
    grad: np.ndarray        # [B,4,H,W] float64: d (sum_b g[b] value[b]) / d pred


def alive_mask(target: np.ndarray, alpha_thr: float) -> np.ndarray:
    """[B or 1,1,H,W] bool: the float32 comparison."""
    target = np.asarray(target)
    assert target.dtype == np.float32
    if target.ndim == 3:
        target = target[None]
    return target[:, 3:4] > np.float32(alpha_thr)


def masked_loss(pred, target, alpha_thr=0.2, lam_area=5e-5, lam_bg_alpha=0.0, lam_bg_rgb=0.0, g=None) -> Masked:
    """pred [B,4,H,W], target [4,H,W] / [1,4,H,W] / [B,4,H,W], both float32 arrays; ``g`` [B] weights the
    samples in the gradient (default: ones)."""
    pred, target = np.asarray(pred), np.asarray(target)
    assert pred.dtype == np.float32 and target.dtype == np.float32
    if target.ndim == 3:
        target = target[None]
    B, _, H, W = pred.shape
    alive = torch.from_numpy(np.broadcast_to(alive_mask(target, alpha_thr), (B, 1, H, W)).copy()).double()
    dead = 1.0 - alive
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy(target.astype(np.float64))
    n = alive.sum(dim=(1, 2, 3))
    denom = (n.float() + 1e-8).double()   # the float32 code's denominator: n itself from n = 1 on, 1e-8 at n = 0
    primary = (((p - t) ** 2) * alive).sum(dim=(1, 2, 3)) / denom
    bg_alpha = lam_bg_alpha * (p[:, 3:4] * dead).mean(dim=(1, 2, 3))
    bg_rgb = lam_bg_rgb * (p[:, :3] * dead).abs().mean(dim=(1, 2, 3))
    area = lam_area * p[:, 3:4].mean(dim=(1, 2, 3))
    value = primary + bg_alpha + bg_rgb + area
    w = torch.ones(B, dtype=torch.float64) if g is None else torch.as_tensor(np.asarray(g, np.float64))
    (value * w).sum().backward()
    f = lambda x: x.detach().numpy().copy()
    return Masked(f(value), f(primary), f(bg_alpha), f(bg_rgb), f(area), f(n).astype(np.int64), f(p.grad))


def stability_loss(pred, target, close, g=1.0):
    """(value, grad [B,4,H,W]) of ``g * mse(pred[close], target[close])`` in float64; no close sample:
    (0, zeros), the term the trainer skips."""
    pred, target = np.asarray(pred), np.asarray(target)
    assert pred.dtype == np.float32 and target.dtype == np.float32
    if target.ndim == 3:
        target = target[None]
    close = np.asarray(close).astype(bool)
    B = pred.shape[0]
    assert close.shape == (B,)
    if not close.any():
        return 0.0, np.zeros(pred.shape, np.float64)
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.broadcast_to(target, pred.shape).astype(np.float64))
    idx = torch.from_numpy(close)
    value = ((p[idx] - t[idx]) ** 2).mean()
    (value * g).backward()
    return float(value.detach()), p.grad.numpy().copy()
