"""Forward gradients: a training step with no backward and O(1) memory in the rollout length.

``model.rollout_objective_tangent(x, T, target, dparams=dirs.dicts())`` carries K weight directions through
a rollout and returns, per tapped step, the losses and their directional derivatives ``dlosses`` [R,K,B].
``forward_gradient_`` turns those and the directions into ``.grad``::

    dirs = ParamDirections(model, K=8, seed=0)
    opt = FusedAdam(model.parameters(), lr=2e-4)
    ...
    dirs.normal_()
    out = model.rollout_objective_tangent(x, T, target, dparams=dirs.dicts(), every=8, fire_rate=0.5)
    forward_gradient_(model, out.dlosses, dirs)       # g = 1/(K B) sum_k <dL, dtheta_k> dtheta_k
    opt.step()

With directions drawn from N(0, I) that is the unbiased forward-gradient estimate of the batch mean of the
summed tap losses.  Nothing waits for the GPU: the inner products are reduced and the gradient assembled on
the device (``gnca_forward_grad``, two launches).  ``loss_tangent`` is the loss kernel alone
(``gnca_loss_tangent``): the forward-mode counterpart of the two losses' backward.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from . import loss as LS
from .step import DIRECTION_FIELDS, TAP_KINDS, stream_ptr


def _entry(name: str):
    fn = getattr(L.load(), name, None)
    if fn is None:
        raise L.GncaError(f"libgnca.so at {L.LIB_PATH} has no {name}; rebuild it")
    return fn


def loss_tangent(pred: torch.Tensor, V: torch.Tensor, target: torch.Tensor, loss: str = "premult",
                 alpha_thr: float = 0.2, lam_area: float = 5e-5, lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0):
    """``(losses, dlosses)``: ``losses`` float32 [B], bitwise ``loss_premult_rgba(pred, target)`` /
    ``masked_loss(pred, target, ...)``; ``dlosses`` float64 [K,B], the derivative of each sample's loss along
    each of the K tangents ``V`` [K,B,4,H,W] of ``pred`` [B,4,H,W]: the fp64 dot of the loss's fp32 gradient
    with ``V[k]``, in a fixed order.  ``pred`` may be the channel slice ``state[:, :4]``.  No autograd."""
    if loss not in TAP_KINDS:
        raise ValueError(f"loss must be one of {sorted(TAP_KINDS)}, got {loss!r}")
    pred, target = LS._prepare(pred, target)
    B, _, H, W = pred.shape
    if not isinstance(V, torch.Tensor) or V.dim() != 5 or tuple(V.shape[1:]) != (B, 4, H, W) or V.shape[0] < 1:
        raise ValueError(f"V must be [K,{B},4,{H},{W}] with K >= 1, got {tuple(getattr(V, 'shape', ()))}")
    if V.device != pred.device or V.dtype != pred.dtype:
        raise ValueError(f"V is {V.dtype} on {V.device}, pred {pred.dtype} on {pred.device}")
    d = L.MaskedLossDesc()
    d.B, d.H, d.W = B, H, W
    if loss == "masked":
        d.alpha_thr, d.lam_area = LS._number(alpha_thr, "alpha_thr"), LS._number(lam_area, "lam_area")
        d.lam_bg_alpha, d.lam_bg_rgb = LS._number(lam_bg_alpha, "lam_bg_alpha"), LS._number(lam_bg_rgb, "lam_bg_rgb")
    with torch.no_grad():
        pred, target = LS._on_device(pred.detach(), target.detach(), "loss_tangent")
        V = V.detach().contiguous()
        K = V.shape[0]
        losses = torch.empty(B, dtype=torch.float32, device=pred.device)
        dlosses = torch.empty(K, B, dtype=torch.float64, device=pred.device)
        rc = _entry("gnca_loss_tangent")(TAP_KINDS[loss], ctypes.byref(d), K, pred.data_ptr(), pred.stride(0),
                                         V.data_ptr(), V.stride(0), V.stride(1), target.data_ptr(), LS._tbs(target),
                                         losses.data_ptr(), dlosses.data_ptr(), stream_ptr(pred.device))
        L.check(rc, "gnca_loss_tangent")
    return losses, dlosses


class ParamDirections:
    """K directions of the model's perturbable weights in ONE flat float32 buffer ``flat`` [K,P] on the model's
    device, P the element count of the parameters named in ``DIRECTION_FIELDS``, in that order (a model without
    GroupNorm or without the graph term has fewer).  ``dicts()`` returns K dicts of views into ``flat``, each
    accepted as ``dparams``; ``normal_()`` / ``fill_()`` write the whole buffer in one launch.  ``seed``: the
    seed of the buffer's own generator (``None``: torch's default generator of the device)."""

    def __init__(self, model: torch.nn.Module, K: int, seed=None):
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= L.TANGENT_MAX_DIRS:
            raise ValueError(f"K must be an int in 1..{L.TANGENT_MAX_DIRS}, got {K!r}")
        params = dict(model.named_parameters())
        self.names = [n for n in DIRECTION_FIELDS if n in params]
        if not self.names:
            raise ValueError("the model has none of the parameters a direction may perturb")
        self.params = [params[n] for n in self.names]
        dev = self.params[0].device
        for n, p in zip(self.names, self.params):
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError(f"{n} is {p.dtype} on {p.device}; the directions are float32 on {dev}")
        self.K = K
        self.offsets, o = [], 0
        for p in self.params:
            self.offsets.append(o)
            o += p.numel()
        self.P = o
        self.flat = torch.zeros(K, self.P, dtype=torch.float32, device=dev)
        self.generator = None
        if seed is not None:
            self.generator = torch.Generator(device=dev)
            self.generator.manual_seed(int(seed))
        self._dicts = [{n: self.flat[k, o:o + p.numel()].view(p.shape)
                        for n, p, o in zip(self.names, self.params, self.offsets)} for k in range(K)]

    def normal_(self, mean: float = 0.0, std: float = 1.0):
        self.flat.normal_(mean, std, generator=self.generator)
        return self

    def fill_(self, value: float):
        self.flat.fill_(value)
        return self

    def dicts(self) -> list:
        """K dicts {parameter name: view of ``flat``}: a ``dparams`` list."""
        return [dict(d) for d in self._dicts]


def forward_gradient_(model: torch.nn.Module, dlosses: torch.Tensor, directions: ParamDirections, *,
                      tap_weights=None, scale=None, accumulate: bool = False) -> torch.Tensor:
    """Write (``accumulate=True``: add to) the ``.grad`` of every perturbable parameter:

        coef[k] = scale * sum_r tap_weights[r] * sum_b dlosses[r,k,b]
        grad    = sum_k coef[k] * directions[k]          (fp64, rounded to float32 once)

    ``dlosses``: float64 [R,K,B] (``rollout_objective_tangent(...).dlosses``) or [K,B]; ``tap_weights``: R
    numbers or a float32 [R] device tensor (``None``: ones); ``scale=None``: ``1 / (K B)``.  A ``.grad`` that is
    ``None`` is allocated.  Returns ``coef``, float64 [K] on the device; a non-finite entry says that a
    ``dlosses`` entry was non-finite.  Two launches, no host wait."""
    if not isinstance(directions, ParamDirections):
        raise ValueError("directions must be a ParamDirections")
    if not isinstance(dlosses, torch.Tensor) or dlosses.dim() not in (2, 3) or dlosses.dtype != torch.float64:
        raise ValueError("dlosses must be a float64 [R,K,B] (or [K,B]) tensor")
    if dlosses.dim() == 2:
        dlosses = dlosses.unsqueeze(0)
    R, K, B = dlosses.shape
    if K != directions.K or R < 1 or B < 1:
        raise ValueError(f"dlosses {tuple(dlosses.shape)} does not match {directions.K} directions")
    dev = directions.flat.device
    if dlosses.device != dev:
        raise ValueError(f"dlosses is on {dlosses.device}, the directions on {dev}")
    if not isinstance(accumulate, bool):
        raise ValueError(f"accumulate must be a bool, got {accumulate!r}")
    params = dict(model.named_parameters())
    for n, p in zip(directions.names, directions.params):
        if params.get(n) is not p:
            raise ValueError(f"the directions were built for another model ({n})")
    if len(directions.params) > L.OPTIM_MAX_TENSORS:
        raise ValueError(f"at most {L.OPTIM_MAX_TENSORS} tensors per call")
    tw = None
    if isinstance(tap_weights, torch.Tensor):
        if tuple(tap_weights.shape) != (R,) or tap_weights.device != dev:
            raise ValueError(f"tap_weights must be [{R}] on {dev}")
        tw = tap_weights.detach().to(torch.float32).contiguous()
    elif tap_weights is not None:
        tw = [LS._number(v, "tap weight") for v in tap_weights]
        if len(tw) != R:
            raise ValueError(f"{len(tw)} tap weights for {R} taps")
    scale = 1.0 / (K * B) if scale is None else LS._number(scale, "scale")
    if dev.type != "cuda":
        raise RuntimeError("forward_gradient_ runs on a ROCm device (no CPU path)")
    if isinstance(tw, list):   # (an upload: under capture pass a device tensor instead)
        tw = torch.tensor(tw, dtype=torch.float32).to(dev, non_blocking=True)
    fn = _entry("gnca_forward_grad")
    with torch.no_grad():
        dlosses = dlosses.detach().contiguous()
        coef = torch.empty(K, dtype=torch.float64, device=dev)
        d = L.ForwardGradDesc()
        d.K, d.R, d.B = K, R, B
        d.dlosses, d.tap_weight, d.scale, d.coef = dlosses.data_ptr(), None if tw is None else tw.data_ptr(), scale, \
            coef.data_ptr()
        d.num_tensors = len(directions.params)
        fresh = []
        for i, (p, o) in enumerate(zip(directions.params, directions.offsets)):
            if p.grad is None or not (p.grad.is_contiguous() and p.grad.dtype == torch.float32 and
                                      p.grad.device == dev):
                if p.grad is not None:
                    raise ValueError("an existing .grad must be a contiguous float32 tensor on the model's device")
                p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
                fresh.append(i)
            e = d.t[i]
            e.g, e.dir = p.grad.data_ptr(), directions.flat.data_ptr() + 4 * o
            e.dir_stride, e.numel = directions.P, p.numel()
        if accumulate and fresh:
            # a fresh .grad has nothing to add to: written in a call of its own
            for sel, flags in ((fresh, 0), ([i for i in range(d.num_tensors) if i not in fresh],
                                            L.FGRAD_ACCUMULATE)):
                if not sel:
                    continue
                sub = L.ForwardGradDesc()
                ctypes.memmove(ctypes.byref(sub), ctypes.byref(d), ctypes.sizeof(d))
                sub.num_tensors, sub.flags = len(sel), flags
                for j, i in enumerate(sel):
                    sub.t[j] = d.t[i]
                L.check(fn(ctypes.byref(sub), stream_ptr(dev)), "gnca_forward_grad")
        else:
            d.flags = L.FGRAD_ACCUMULATE if accumulate else 0
            L.check(fn(ctypes.byref(d), stream_ptr(dev)), "gnca_forward_grad")
    return coef
