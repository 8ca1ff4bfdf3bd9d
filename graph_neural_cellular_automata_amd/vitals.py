"""A view of the state itself, on the device: how much of the canvas is alive, where the pattern
lies and whether the numbers are still sane.

``state_vitals(x)`` computes 13 float64 numbers for every sample of a state in one pass over it
(``gnca_state_vitals``: one launch over the batch and a small one that combines its partial sums), with
no host synchronisation; ``trace(..., vitals=True)`` records them per step, also with ``frames=False``.

With ``a`` the alpha plane (channel 3), every comparison in float32 against ``alpha_thr``, ``i`` the row
and ``j`` the column of a cell:

- ``alive``: cells with ``max_pool3x3(a) > alpha_thr`` (neighbours outside the image do not count): the
  model's alive mask, and the cells the step's first kernel works on;
- ``mature``: cells with ``a > alpha_thr``;
- ``alpha_sum``: the sum of ``a``; ``mass``: the sum of ``clip(a, 0, 1)``;
- ``cy``, ``cx``: the centroid ``sum(clip(a,0,1) * i) / mass``, ``sum(clip(a,0,1) * j) / mass`` (NaN when
  ``mass`` is 0);
- ``y0``, ``y1``, ``x0``, ``x1``: the inclusive bounding box of the mature cells (all -1 when there is none);
- ``max_abs``: the largest ``|v|`` over all channels among finite values (0 when there is none);
- ``nonfinite``: the number of NaN and infinite values over all channels;
- ``hidden_rms``: ``sqrt(sum(v^2) / ((C-4) H W))`` over the channels from 4 on, finite values only (0 when
  ``C`` is 4).

The first ten are specified for a finite alpha plane; ``max_abs`` and ``nonfinite`` always.  Every sum is
float64 in a fixed order, so a sample's numbers are bitwise the same in any batch.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import _lib as L
from .step import stream_ptr

FIELDS = L.VITALS_FIELDS


class StateVitals(namedtuple("StateVitals", FIELDS)):
    """The 13 fields: views of one float64 ``[..., 13]`` tensor, ``.stacked``."""

    def __new__(cls, stacked: torch.Tensor):
        self = super().__new__(cls, *stacked.unbind(-1))
        self.stacked = stacked
        return self


def check_alpha_thr(alpha_thr, what: str = "alpha_thr") -> float:
    """``alpha_thr`` as a float, or ``ValueError`` unless it is a finite real number (not a bool)."""
    if isinstance(alpha_thr, bool) or not isinstance(alpha_thr, (int, float)) or not math.isfinite(alpha_thr):
        raise ValueError(f"{what} must be a finite number, got {alpha_thr!r}")
    return float(alpha_thr)


def _inner_ok(t: torch.Tensor) -> bool:
    H, W = t.shape[-2:]
    return t.stride(-3) == H * W and t.stride(-2) == W and t.stride(-1) == 1 and t.stride(-4) >= 0


def state_vitals(x: torch.Tensor, alpha_thr: float = 0.1) -> StateVitals:
    """The vitals of every sample of ``x`` ([B,C>=4,H,W] or [R,B,C>=4,H,W]); each field has ``x``'s
    leading shape ([B] or [R,B]), float64.  A channel slice or a batch slice of a contiguous state is
    read in place.  No gradients: runs under ``no_grad``, returns detached tensors."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5) or x.shape[-3] < 4:
        raise ValueError("x must be [B,C,H,W] or [R,B,C,H,W] with C >= 4")
    if min(x.shape) < 1:
        raise ValueError(f"x of shape {tuple(x.shape)} has an empty dimension")
    alpha_thr = check_alpha_thr(alpha_thr)
    if x.device.type != "cuda" or x.dtype != torch.float32:
        raise RuntimeError("state_vitals runs on a float32 ROCm tensor (no CPU path)")
    B, C, H, W = x.shape[-4:]
    with torch.no_grad():
        x = x.detach()
        if not _inner_ok(x):
            x = x.contiguous()
        lib = L.load()
        out = torch.empty(*x.shape[:-3], len(FIELDS), dtype=torch.float64, device=x.device)
        n = lib.gnca_state_vitals_workspace_bytes(B, C, H, W)
        if n == 0:
            raise L.GncaError(f"unsupported vitals shape: B={B} C={C} H={H} W={W}")
        ws = torch.empty(n, dtype=torch.uint8, device=x.device)
        batches = [(x, out)] if x.dim() == 4 else [(x[r], out[r]) for r in range(x.shape[0])]
        for s, o in batches:
            L.check(lib.gnca_state_vitals(B, C, H, W, s.data_ptr(), s.stride(0), alpha_thr, o.data_ptr(),
                                          ws.data_ptr(), n, stream_ptr(x.device)), "gnca_state_vitals")
    return StateVitals(out)
