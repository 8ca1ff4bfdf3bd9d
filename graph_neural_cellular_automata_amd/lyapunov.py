"""Blocks of tangents: the device thin QR that ``rollout_tangent_block()`` re-orthonormalises with
(Benettin's method for Lyapunov spectra).  The arithmetic is in libgnca.so
(``gnca_tangent_qr``): fp64 Gram matrix of the fp32 block, Cholesky with a pivot rule that drops
dependent columns, Q = V R^-1 in fp64 rounded once; bitwise reproducible, per sample independent,
and the host never waits.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import step as S


class TangentQR:
    """What ``orthonormalize_tangents()`` returns: ``q`` [K,B,...] float32, orthonormal columns per sample
    (all zeros for a dropped column); ``r`` float64 [B,K,K], upper triangular with a non-negative diagonal
    (row j zero for a dropped column j); ``log_diag`` float64 [B,K], ``log r[b,j,j]`` (``-inf`` for a dropped
    column).  All detached."""

    __slots__ = ("q", "r", "log_diag")

    def __init__(self, q, r, log_diag):
        self.q, self.r, self.log_diag = q, r, log_diag

    def __repr__(self):
        return f"TangentQR(q={tuple(self.q.shape)}, r={tuple(self.r.shape)})"


def check_block(V, name: str = "V") -> None:
    """ValueError unless ``V`` is a float32 tensor [K,B,...] with 1 <= K <= 16, B >= 1 and at least one
    element per sample (pure Python: nothing is drawn or launched)."""
    if not isinstance(V, torch.Tensor) or V.dim() < 3:
        raise ValueError(f"{name} must be a tensor [K,B,...], got {tuple(getattr(V, 'shape', ()))}")
    if not 1 <= V.shape[0] <= L.TANGENT_MAX_DIRS:
        raise ValueError(f"{name} holds {V.shape[0]} directions; 1 <= K <= {L.TANGENT_MAX_DIRS}")
    if V.shape[1] < 1 or V[0, 0].numel() < 1:
        raise ValueError(f"{name} has an empty batch or empty samples: {tuple(V.shape)}")
    if V.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {V.dtype}")


def orthonormalize_tangents(V: torch.Tensor, *, inplace: bool = False) -> TangentQR:
    """The thin QR of a block of tangents, per sample: ``V`` [K,B,...] (direction-major, as
    ``rollout_tangent_block`` takes it), columns ``V[:, b]`` flattened, ``V_b = Q_b R_b``.

    A column that is zero, non-finite, or in the span of the earlier ones up to its fp32 rounding
    (``d_j <= 2^-44 G_jj``) is dropped: its ``q`` is all zeros, its ``log_diag`` ``-inf``, and it does not
    touch the other columns.  ``inplace=True`` overwrites ``V`` (contiguous) with ``q``."""
    check_block(V)
    if not isinstance(inplace, bool):
        raise ValueError(f"inplace must be a bool, got {inplace!r}")
    with torch.no_grad():
        v = S._dev_f32(V.detach(), "the tangent block")
        if inplace:
            if not V.is_contiguous():
                raise ValueError("inplace=True needs a contiguous block")
            q = v
        else:
            q = torch.empty_like(v)
            q.copy_(v)
        r, log_diag, _ = S.tangent_qr(q)
    return TangentQR(q, r, log_diag)
