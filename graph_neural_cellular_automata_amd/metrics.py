"""The trainers' quality figures on the device: MSE, pixel-perfect fraction, PSNR and SSIM.

Every iteration of the reference trainer (``src/training/train_graph_augmented_nca.py:405-422``) pulls
sample 0 to the host, re-premultiplies it and calls skimage's ``structural_similarity`` and
``peak_signal_noise_ratio`` on the CPU.  ``image_metrics(pred, target)`` computes the same four
figures for every image of the batch in one HIP launch (``gnca_image_metrics_f32``), with no host
synchronisation and no skimage; ``trace(..., target=t)`` records them per step.  ``pred`` may be the
channel slice ``state[:, :4]`` of a contiguous state, or a whole state (channels 0..3 are read in
place through its strides).

Definitions (skimage's defaults: uniform 7x7 windows, sample covariance, data range 1), with
``P = (pred_rgb * pred_alpha, pred_alpha)``, ``T = target``, ``X, Y = clip(P_rgb, T_rgb; 0, 1)``:

- ``mse``: mean of ``(P - T)^2`` over 4 channels and all cells (``loss_premult_rgba``'s value);
- ``pixel_perfect``: fraction of cells with ``|P_c - T_c| < 0.05`` in all four channels;
- ``psnr``: ``10 log10(1 / mean((X - Y)^2))`` over the colour channels, ``+inf`` for equal images;
- ``ssim``: mean structural similarity of ``X`` and ``Y`` over the colour channels and all full
  windows, ``NaN`` when ``H < 7`` or ``W < 7``.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib as L
from .step import stream_ptr

FIELDS = ("mse", "pixel_perfect", "psnr", "ssim")


class ImageMetrics(namedtuple("ImageMetrics", FIELDS)):
    """``(mse, pixel_perfect, psnr, ssim)``: views of one ``[..., 4]`` tensor, ``.stacked``."""

    def __new__(cls, stacked: torch.Tensor):
        self = super().__new__(cls, *stacked.unbind(-1))
        self.stacked = stacked
        return self


def check_target(target, B: int, H: int, W: int) -> torch.Tensor:
    """``target`` as ``[1 or B,4,H,W]``, or ``ValueError`` (shapes only: nothing is launched)."""
    if not isinstance(target, torch.Tensor):
        raise ValueError(f"target must be a tensor, got {type(target).__name__}")
    if target.dim() == 3:
        target = target.unsqueeze(0)
    # the kernel indexes the target with pred's geometry: reject a mismatch instead of reading out
    # of bounds on the device
    if target.dim() != 4 or tuple(target.shape[1:]) != (4, H, W) or target.shape[0] not in (1, B):
        raise ValueError(f"target of shape {tuple(target.shape)} does not match pred [{B},>=4,{H},{W}] "
                         f"(expected [4,{H},{W}], [1,4,{H},{W}] or [{B},4,{H},{W}])")
    return target


def device_target(target: torch.Tensor, device) -> tuple:
    """(contiguous float32 target on ``device``, its sample stride: 0 = broadcast)."""
    target = target.detach().to(device, torch.float32)
    if target.shape[0] != 1 and target.stride(0) != 0:
        target = target.contiguous()
        return target, target.stride(0)
    return target[:1].contiguous(), 0


def _inner_ok(t: torch.Tensor) -> bool:
    H, W = t.shape[-2:]
    return t.stride(-3) == H * W and t.stride(-2) == W and t.stride(-1) == 1 and t.stride(-4) >= 0


def image_metrics(pred: torch.Tensor, target: torch.Tensor) -> ImageMetrics:
    """The four figures of every image of ``pred`` ([B,C>=4,H,W] or [R,B,C>=4,H,W], channels 0..3)
    against the premultiplied RGBA ``target`` ([4,H,W], [1,4,H,W] or [B,4,H,W]).  Each field has
    ``pred``'s leading shape ([B] or [R,B]).  No gradients: runs under ``no_grad``, returns detached
    tensors.  An image's result is bitwise independent of the batch around it."""
    if not isinstance(pred, torch.Tensor) or pred.dim() not in (4, 5) or pred.shape[-3] < 4:
        raise ValueError("pred must be [B,C,H,W] or [R,B,C,H,W] with C >= 4")
    B, _, H, W = pred.shape[-4:]
    if min(pred.shape) < 1:
        raise ValueError(f"pred of shape {tuple(pred.shape)} has an empty dimension")
    target = check_target(target, B, H, W)
    if pred.device.type != "cuda" or pred.dtype != torch.float32:
        raise RuntimeError("image_metrics runs on a float32 ROCm tensor (no CPU path)")
    with torch.no_grad():
        pred = pred.detach()
        if not _inner_ok(pred):
            pred = pred.contiguous()
        target, tbs = device_target(target, pred.device)
        lib = L.load()
        lead = tuple(pred.shape[:-3])
        out = torch.empty(*lead, 4, dtype=torch.float32, device=pred.device)
        n = lib.gnca_image_metrics_workspace_bytes(B, H, W)
        ws = torch.empty(n, dtype=torch.uint8, device=pred.device) if n else None
        batches = [(pred, out)] if pred.dim() == 4 else [(pred[r], out[r]) for r in range(pred.shape[0])]
        for p, o in batches:   # one launch per recorded batch: a per-sample target follows b, not r*B+b
            L.check(lib.gnca_image_metrics_f32(B, H, W, p.data_ptr(), p.stride(0), target.data_ptr(), tbs,
                                               o.data_ptr(), None if ws is None else ws.data_ptr(), n,
                                               stream_ptr(pred.device)),
                    "gnca_image_metrics_f32")
    return ImageMetrics(out)
