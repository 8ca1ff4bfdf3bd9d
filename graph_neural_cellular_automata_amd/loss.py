"""The graph trainer's loss on the device, fused.

``loss_premult_rgba(pred, target)`` has the reference's signature and result
(``src/training/train_graph_augmented_nca.py:52-61``: full-canvas MSE on premultiplied RGBA,
per-sample [B]); forward and backward are one HIP launch each (``gnca_loss_premult_f32`` /
``gnca_loss_premult_bwd_f32``) instead of the reference's chain of elementwise ops.  ``pred`` may
be the channel slice ``state[:, :4]`` of a contiguous state (read in place through its stride).

``masked_loss(pred, target, ...)`` and ``stability_loss(pred, target, close)`` are the classic
trainer's objective (``src/training/train_intermediate_loss.py:37-51`` and ``:256-267``; the graph
trainer's ``masked_loss`` with its two background penalties, ``train_graph_augmented_nca.py:30-49``,
is the same function with two more knobs): MSE where the *target* is alive plus the penalties, per
sample, and the stability phase's MSE over the close samples.  One launch each way for the first
(``gnca_loss_masked_f32`` / ``gnca_loss_masked_bwd_f32``), two forward and one backward for the second
(``gnca_loss_stability_f32`` / ``gnca_loss_stability_bwd_f32``).  ``masked_loss(..., stability=(thr, K))``
also returns the stability phase's per-sample step counts, so neither the close mask nor its count
reaches the host between the rollout and ``backward()``::

    state = model.rollout(state, T, nsteps=nca_steps, fire_rate=rates)
    per_sample, k = masked_loss(state[:, :4], target, 0.2, 5e-5, stability=(0.01, 24))
    stab = model.rollout(state, 24, nsteps=k, fire_rate=rates2)
    loss = per_sample.mean() + 0.5 * stability_loss(stab[:, :4], target, k > 0)
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .step import stream_ptr


def _strided_ok(t: torch.Tensor) -> bool:
    B, C, H, W = t.shape
    return t.stride(1) == H * W and t.stride(2) == W and t.stride(3) == 1


class _PremultLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        B, _, H, W = pred.shape
        out = torch.empty(B, dtype=torch.float32, device=pred.device)
        tbs = 0 if target.shape[0] == 1 or target.stride(0) == 0 else target.stride(0)
        L.check(L.load().gnca_loss_premult_f32(B, H, W, pred.data_ptr(), pred.stride(0), target.data_ptr(),
                                               tbs, out.data_ptr(), stream_ptr(pred.device)),
                "gnca_loss_premult_f32")
        ctx.save_for_backward(pred, target)
        ctx.tbs = tbs
        return out

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        B, _, H, W = pred.shape
        gp = torch.empty(B, 4, H, W, dtype=torch.float32, device=pred.device)
        g = g.contiguous().float()
        L.check(L.load().gnca_loss_premult_bwd_f32(B, H, W, pred.data_ptr(), pred.stride(0), target.data_ptr(),
                                                   ctx.tbs, g.data_ptr(), gp.data_ptr(), gp.stride(0),
                                                   stream_ptr(pred.device)),
                "gnca_loss_premult_bwd_f32")
        return gp, None


def _prepare(pred: torch.Tensor, target: torch.Tensor):
    """``ValueError`` unless pred is [B,4,H,W] and target [4,H,W], [1,4,H,W] or [B,4,H,W]; the target comes
    back with its batch dimension."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[1] != 4:
        raise ValueError("pred must be [B,4,H,W]")
    B, _, H, W = pred.shape
    if not isinstance(target, torch.Tensor):
        raise ValueError("target must be a tensor")
    if target.dim() == 3:
        target = target.unsqueeze(0)
    # the kernels index the target with pred's geometry: reject what F.mse_loss could not
    # broadcast (the reference raises there) instead of reading out of bounds on the device
    if target.dim() != 4 or tuple(target.shape[1:]) != (4, H, W) or target.shape[0] not in (1, B):
        raise ValueError(f"target of shape {tuple(target.shape)} does not match pred [{B},4,{H},{W}] "
                         f"(expected [4,{H},{W}], [1,4,{H},{W}] or [{B},4,{H},{W}])")
    if B == 0 or H == 0 or W == 0:
        raise ValueError(f"pred of shape {tuple(pred.shape)} is empty")
    return pred, target


def _on_device(pred: torch.Tensor, target: torch.Tensor, name: str):
    if pred.device.type != "cuda" or pred.dtype != torch.float32:
        raise RuntimeError(f"{name} runs on a float32 ROCm tensor (no CPU path)")
    if not _strided_ok(pred):
        pred = pred.contiguous()
    target = target.to(pred.device, torch.float32)
    if target.shape[0] != 1 and target.stride(0) != 0:
        target = target.contiguous()
    else:
        target = target[:1].contiguous()
    return pred, target


def _tbs(target: torch.Tensor) -> int:
    return 0 if target.shape[0] == 1 or target.stride(0) == 0 else target.stride(0)


def _entry(name: str):
    fn = getattr(L.load(), name, None)
    if fn is None:
        raise L.GncaError(f"libgnca.so at {L.LIB_PATH} has no {name}; rebuild it")
    return fn


class _MaskedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, knobs, stability):
        B, _, H, W = pred.shape
        d = L.MaskedLossDesc()
        d.B, d.H, d.W = B, H, W
        d.alpha_thr, d.lam_area, d.lam_bg_alpha, d.lam_bg_rgb = knobs
        if stability is not None:
            d.close_thresh, d.close_steps = stability
        out = torch.empty(B, dtype=torch.float32, device=pred.device)
        alive = torch.empty(B, dtype=torch.int32, device=pred.device)
        nsteps = torch.empty(B, dtype=torch.int32, device=pred.device) if stability is not None else None
        tbs = _tbs(target)
        L.check(_entry("gnca_loss_masked_f32")(ctypes.byref(d), pred.data_ptr(), pred.stride(0), target.data_ptr(),
                                               tbs, out.data_ptr(), alive.data_ptr(),
                                               None if nsteps is None else nsteps.data_ptr(),
                                               stream_ptr(pred.device)),
                "gnca_loss_masked_f32")
        ctx.save_for_backward(pred, target, alive)
        ctx.desc, ctx.tbs = d, tbs
        if nsteps is None:
            return out
        ctx.mark_non_differentiable(nsteps)
        return out, nsteps

    @staticmethod
    def backward(ctx, g, *unused):
        pred, target, alive = ctx.saved_tensors
        B, _, H, W = pred.shape
        gp = torch.empty(B, 4, H, W, dtype=torch.float32, device=pred.device)
        g = g.contiguous().float()
        L.check(_entry("gnca_loss_masked_bwd_f32")(ctypes.byref(ctx.desc), pred.data_ptr(), pred.stride(0),
                                                   target.data_ptr(), ctx.tbs, alive.data_ptr(), g.data_ptr(),
                                                   gp.data_ptr(), gp.stride(0), stream_ptr(pred.device)),
                "gnca_loss_masked_bwd_f32")
        return gp, None, None, None


class _StabilityLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, close):
        B, _, H, W = pred.shape
        size = _entry("gnca_loss_stability_workspace_bytes")(B)
        ws = torch.empty((size + 7) // 8, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        scale = torch.empty(1, dtype=torch.float32, device=pred.device)
        tbs = _tbs(target)
        L.check(_entry("gnca_loss_stability_f32")(B, H, W, pred.data_ptr(), pred.stride(0), target.data_ptr(), tbs,
                                                  close.data_ptr(), loss.data_ptr(), scale.data_ptr(),
                                                  ws.data_ptr(), ws.numel() * 8, stream_ptr(pred.device)),
                "gnca_loss_stability_f32")
        ctx.save_for_backward(pred, target, close, scale)
        ctx.tbs = tbs
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target, close, scale = ctx.saved_tensors
        B, _, H, W = pred.shape
        gp = torch.empty(B, 4, H, W, dtype=torch.float32, device=pred.device)
        g = g.reshape(1).contiguous().float()
        L.check(_entry("gnca_loss_stability_bwd_f32")(B, H, W, pred.data_ptr(), pred.stride(0), target.data_ptr(),
                                                      ctx.tbs, close.data_ptr(), scale.data_ptr(), g.data_ptr(),
                                                      gp.data_ptr(), gp.stride(0), stream_ptr(pred.device)),
                "gnca_loss_stability_bwd_f32")
        return gp, None, None


def loss_premult_rgba(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per-sample [B] MSE between (pred_rgb * pred_alpha, pred_alpha) and target ([B or 1,4,H,W])."""
    if pred.dim() != 4 or pred.shape[1] != 4:
        raise ValueError("pred must be [B,4,H,W]")
    B, _, H, W = pred.shape
    if target.dim() == 3:
        target = target.unsqueeze(0)
    # the kernels index the target with pred's geometry: reject what F.mse_loss could not
    # broadcast (the reference raises there) instead of reading out of bounds on the device
    if target.dim() != 4 or tuple(target.shape[1:]) != (4, H, W) or target.shape[0] not in (1, B):
        raise ValueError(f"target of shape {tuple(target.shape)} does not match pred [{B},4,{H},{W}] "
                         f"(expected [4,{H},{W}], [1,4,{H},{W}] or [{B},4,{H},{W}])")
    pred, target = _on_device(pred, target, "loss_premult_rgba")
    return _PremultLoss.apply(pred, target)


def _number(v, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def masked_loss(pred: torch.Tensor, target: torch.Tensor, alpha_thr: float = 0.2, lam_area: float = 5e-5,
                lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0, *, stability=None):
    """Per-sample [B] MSE over the cells where the TARGET is alive (``target_alpha > alpha_thr``), divided
    by the alive count, plus ``lam_area * mean(pred_alpha)``, ``lam_bg_alpha * mean(pred_alpha * dead)`` and
    ``lam_bg_rgb * mean(|pred_rgb * dead|)``.  ``pred`` is the raw ``state[:, :4]`` (nothing is premultiplied).

    The positional signature and defaults are the classic trainer's ``masked_loss``
    (``train_intermediate_loss.py:37``), which has no background penalties; the graph trainer's own
    defaults for them are ``lam_bg_alpha=1e-3, lam_bg_rgb=2e-4``, and its call site passes all four knobs
    explicitly, so either trainer's call gives its reference value.

    ``stability=(threshold, K)``: also returns ``nsteps`` (int32 [B], not differentiable), ``K`` where
    ``per_sample < threshold`` and 0 elsewhere: the ``nsteps`` of the stability phase's ``rollout`` and,
    as ``nsteps > 0``, the ``close`` of ``stability_loss``."""
    pred, target = _prepare(pred, target)
    knobs = (_number(alpha_thr, "alpha_thr"), _number(lam_area, "lam_area"),
             _number(lam_bg_alpha, "lam_bg_alpha"), _number(lam_bg_rgb, "lam_bg_rgb"))
    if stability is not None:
        if not isinstance(stability, (tuple, list)) or len(stability) != 2:
            raise ValueError(f"stability must be a (threshold, K) pair, got {stability!r}")
        thr, K = _number(stability[0], "stability threshold"), stability[1]
        if isinstance(K, bool) or not isinstance(K, int) or K < 0 or K > 0x7fffffff:
            raise ValueError(f"stability K must be a non-negative int, got {K!r}")
        stability = (thr, K)
    pred, target = _on_device(pred, target, "masked_loss")
    return _MaskedLoss.apply(pred, target, knobs, stability)


def stability_loss(pred: torch.Tensor, target: torch.Tensor, close: torch.Tensor) -> torch.Tensor:
    """``F.mse_loss(pred[close], target[close])`` as a 0-dim tensor, without the host wait of the boolean
    index: ``close`` is a bool / uint8 [B] device tensor.  No close sample: exactly 0 with a zero gradient
    (the reference skips the term there)."""
    pred, target = _prepare(pred, target)
    B = pred.shape[0]
    if not isinstance(close, torch.Tensor) or tuple(close.shape) != (B,) or close.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"close must be a bool / uint8 tensor of shape ({B},)")
    if close.device != pred.device:
        raise ValueError(f"close is on {close.device}, pred on {pred.device}")
    pred, target = _on_device(pred, target, "stability_loss")
    close = close.contiguous()
    return _StabilityLoss.apply(pred, target, close.view(torch.uint8) if close.dtype == torch.bool else close)


def loss_curvature(pred: torch.Tensor, v: torch.Tensor, target: torch.Tensor, loss: str = "premult",
                   alpha_thr: float = 0.2, lam_area: float = 5e-5, lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0):
    """``(field, quad, losses, dlosses)`` of one tangent ``v`` [B,4,H,W] of ``pred`` [B,4,H,W]: ``field`` float32
    [B,4,H,W], the loss's Gauss-Newton curvature applied to ``v`` and pulled back to ``pred`` (for the
    premultiplied loss the residual term of the bilinear ``rgb * alpha`` is dropped, which keeps the curvature
    positive semidefinite; the masked loss's penalties carry none); ``quad`` float64 [B], the quadratic form
    ``v^T (P^T H P) v``; ``losses`` float32 [B], bitwise ``loss_premult_rgba`` / ``masked_loss``; ``dlosses``
    float64 [B], bitwise ``loss_tangent``'s with one direction.  One launch (``gnca_loss_curvature``), no autograd.
    ``pred`` may be the channel slice ``state[:, :4]``."""
    from .step import TAP_KINDS
    if loss not in TAP_KINDS:
        raise ValueError(f"loss must be one of {sorted(TAP_KINDS)}, got {loss!r}")
    pred, target = _prepare(pred, target)
    B, _, H, W = pred.shape
    if not isinstance(v, torch.Tensor) or tuple(v.shape) != (B, 4, H, W):
        raise ValueError(f"v must be [{B},4,{H},{W}], got {tuple(getattr(v, 'shape', ()))}")
    if v.device != pred.device or v.dtype != pred.dtype:
        raise ValueError(f"v is {v.dtype} on {v.device}, pred {pred.dtype} on {pred.device}")
    d = L.MaskedLossDesc()
    d.B, d.H, d.W = B, H, W
    if loss == "masked":
        d.alpha_thr, d.lam_area = _number(alpha_thr, "alpha_thr"), _number(lam_area, "lam_area")
        d.lam_bg_alpha, d.lam_bg_rgb = _number(lam_bg_alpha, "lam_bg_alpha"), _number(lam_bg_rgb, "lam_bg_rgb")
    with torch.no_grad():
        pred, target = _on_device(pred.detach(), target.detach(), "loss_curvature")
        v = v.detach()
        if not _strided_ok(v):
            v = v.contiguous()
        dev = pred.device
        field = torch.empty(B, 4, H, W, dtype=torch.float32, device=dev)
        quad = torch.empty(B, dtype=torch.float64, device=dev)
        losses = torch.empty(B, dtype=torch.float32, device=dev)
        dlosses = torch.empty(B, dtype=torch.float64, device=dev)
        rc = _entry("gnca_loss_curvature")(TAP_KINDS[loss], ctypes.byref(d), pred.data_ptr(), pred.stride(0),
                                           v.data_ptr(), v.stride(0), target.data_ptr(), _tbs(target),
                                           losses.data_ptr(), dlosses.data_ptr(), quad.data_ptr(), field.data_ptr(),
                                           field.stride(0), stream_ptr(dev))
        L.check(rc, "gnca_loss_curvature")
    return field, quad, losses, dlosses
