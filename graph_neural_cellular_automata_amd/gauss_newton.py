"""Gauss-Newton steps on a rollout objective: curvature-vector products and a conjugate-gradient solve.

``model.rollout_gauss_newton(x, T, target, dparams=d)`` returns ``G d``, the Gauss-Newton curvature of the tap
objective applied to one weight direction (a tangent forward that leaves a tape, then one BPTT with the taps'
curvature fields injected; ``DESIGN.md`` section 25).  ``cg_solve`` runs plain conjugate gradients on such an
operator, so a damped Gauss-Newton (Hessian-free, Levenberg-Marquardt) step is::

    dirs = ParamDirections(model, K=1)
    def matvec(s):
        dirs.flat[0].copy_(s)
        return model.rollout_gauss_newton(x, T, target, dparams=dirs.dicts()[0], every=8, seed=seed).product_flat()
    step, m = cg_solve(matvec, -grad_flat, iters=10, damping=1e-3)

with ``grad_flat`` the BPTT gradient in ``ParamDirections`` order and one ``seed`` (and one offset list), so that
every product sees the same rollout.  Nothing here waits for the GPU.
"""
from __future__ import annotations

import torch


def cg_solve(matvec, b: torch.Tensor, iters: int, damping: float = 0.0):
    """Conjugate gradients for ``(G + damping I) s = b`` from ``s = 0``: ``matvec(p)`` returns ``G p`` for a flat
    vector ``p`` of ``b``'s shape, dtype and device; ``G`` symmetric positive semidefinite.

    Exactly ``iters`` iterations, no ``.item()`` and no host wait: the step sizes are float64 tensors on ``b``'s
    device, and an iteration whose denominator is zero (or not finite) leaves the iterate where it is
    (``torch.where``), so a converged or singular solve stays put.  Returns ``(s, m)``: the iterate after the
    last iteration, in ``b``'s dtype, and the model values ``m[k] = 1/2 s_k^T (G + damping I) s_k - b^T s_k``
    after iteration k + 1 as a float64 [iters] tensor, non-increasing for an exact operator.  Pure torch, so it
    runs on CPU tensors too."""
    if not isinstance(b, torch.Tensor) or b.dim() != 1 or not b.is_floating_point():
        raise ValueError("b must be a flat floating-point tensor")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"iters must be a positive int, got {iters!r}")
    if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not damping >= 0.0:
        raise ValueError(f"damping must be a non-negative number, got {damping!r}")
    if not callable(matvec):
        raise ValueError("matvec must be callable")
    f64 = torch.float64
    with torch.no_grad():
        b = b.detach()
        s = torch.zeros_like(b)
        r = b.clone()                 # b - A s
        p = r.clone()
        rr = torch.dot(r.to(f64), r.to(f64))
        zero = torch.zeros((), dtype=f64, device=b.device)
        m = torch.empty(iters, dtype=f64, device=b.device)
        for k in range(iters):
            Ap = matvec(p)
            if not isinstance(Ap, torch.Tensor) or Ap.shape != b.shape:
                raise ValueError(f"matvec returned {tuple(getattr(Ap, 'shape', ()))}, expected {tuple(b.shape)}")
            Ap = Ap.detach().to(b.dtype)
            if damping:
                Ap = Ap + damping * p
            pAp = torch.dot(p.to(f64), Ap.to(f64))
            ok = torch.isfinite(pAp) & (pAp > 0) & torch.isfinite(rr)
            alpha = torch.where(ok, rr / torch.where(ok, pAp, torch.ones_like(pAp)), zero)
            s = s + (alpha * p.to(f64)).to(b.dtype)
            r = r - (alpha * Ap.to(f64)).to(b.dtype)
            rr_new = torch.dot(r.to(f64), r.to(f64))
            good = ok & (rr > 0)
            beta = torch.where(good, rr_new / torch.where(good, rr, torch.ones_like(rr)), zero)
            p = r + (beta * p.to(f64)).to(b.dtype)
            rr = rr_new
            # with r = b - A s:  1/2 s^T A s - b^T s = -1/2 s^T (b + r)
            m[k] = -0.5 * torch.dot(s.to(f64), (b + r).to(f64))
    return s, m
