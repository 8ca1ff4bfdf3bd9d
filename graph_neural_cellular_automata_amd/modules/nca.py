"""NeuralCA — mirror of src/modules/nca.py:7-105 (classic NCA: the step without the graph term)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._stepper import (GaussNewtonProduct, ObjectiveTangent, param_direction, RolloutObjective,
                       TangentBlockResult, TangentResult, TraceResult, run_gauss_newton_memory, run_rollout,
                       run_rollout_gauss_newton, run_rollout_memory, run_rollout_objective,
                       run_rollout_objective_tangent, run_rollout_tangent, run_rollout_tangent_block, run_step,
                       run_tangent_step, run_trace)
from .perception import FixedSobelPerception


class NeuralCA(nn.Module):
    def __init__(self, n_channels: int, update_hidden: int = 128, img_size: int = 40,
                 update_gain: float = 0.1, alpha_thr: float = 0.1, use_groupnorm: bool = True,
                 device: str = "cpu"):
        super().__init__()
        self.n_channels = n_channels
        self.img_size = img_size          # stored, unused (as in the reference)
        self.update_gain = update_gain
        self.alpha_thr = alpha_thr
        self.device = device              # stored, unused (as in the reference)
        self.perception = FixedSobelPerception(n_channels)
        self.update_net = nn.Sequential(
            nn.Conv2d(n_channels * 3, update_hidden, kernel_size=1, bias=True),
            nn.ReLU(inplace=False),
            nn.Conv2d(update_hidden, n_channels, kernel_size=1, bias=False))
        nn.init.zeros_(self.update_net[-1].weight)
        self.norm = nn.GroupNorm(1, n_channels, eps=1e-3, affine=True) if use_groupnorm else nn.Identity()

    @torch.no_grad()
    def _alive_mask(self, x: torch.Tensor) -> torch.Tensor:
        """max_pool2d(alpha, 3, 1, 1) > alpha_thr (nca.py:55-62); a helper, not the step."""
        return (F.max_pool2d(x[:, 3:4], kernel_size=3, stride=1, padding=1) > self.alpha_thr).float()

    def forward(self, x: torch.Tensor, fire_rate: float = 1.0, *,
                active: torch.Tensor | None = None) -> torch.Tensor:
        """One CA step on the HIP path (nca.py:64-105).  ``active``: see NeuralCAGraph.forward."""
        out, _ = run_step(self, x, fire_rate, None, None, 0.0, False, False, active=active)
        return out

    def param_direction(self, fill: float = 0.0) -> dict:
        """A correctly shaped ``dparams`` dict filled with ``fill``: see ``NeuralCAGraph.param_direction``."""
        return param_direction(self, fill)

    def tangent_step(self, x: torch.Tensor, v: torch.Tensor, fire_rate: float = 1.0, *, active=None, fire=None,
                     dparams=None):
        """One CA step and its forward-mode tangent, ``(x_out, J(x) v)``: see
        ``NeuralCAGraph.tangent_step`` (no ``offsets`` here)."""
        return run_tangent_step(self, x, v, fire_rate, None, 0.0, False, active=active, fire=fire, dparams=dparams)

    def rollout_tangent(self, x: torch.Tensor, v: torch.Tensor, steps: int, *, every=None, record=None,
                        renormalize: bool = False, fire_rate=1.0, nsteps=None, min_steps: int = 0, fire=None,
                        seed=None, sample_base: int = 0, dparams=None) -> TangentResult:
        """The tangent of a whole rollout with no tape and its per-sample log-norm curve: see
        ``NeuralCAGraph.rollout_tangent`` (no ``message_gain`` / ``offsets`` here)."""
        return run_rollout_tangent(self, x, v, steps, None, False, every=every, record=record,
                                   renormalize=renormalize, fire_rate=fire_rate, nsteps=nsteps,
                                   min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base,
                                   dparams=dparams)

    def rollout_tangent_block(self, x: torch.Tensor, V: torch.Tensor, steps: int, *, every=None, record=None,
                              orthonormalize: bool = True, fire_rate=1.0, nsteps=None, min_steps: int = 0,
                              fire=None, seed=None, sample_base: int = 0, dparams=None) -> TangentBlockResult:
        """A block of K tangents ``V`` [K,B,C,H,W] through a whole rollout, re-orthonormalised on the
        device at every recorded step: see ``NeuralCAGraph.rollout_tangent_block`` (no ``message_gain`` /
        ``offsets`` here)."""
        return run_rollout_tangent_block(self, x, V, steps, None, False, every=every, record=record,
                                         orthonormalize=orthonormalize, fire_rate=fire_rate, nsteps=nsteps,
                                         min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base,
                                         dparams=dparams)

    def rollout(self, x: torch.Tensor, steps: int, *, fire_rate=1.0, nsteps=None, min_steps: int = 0,
                fire=None, seed=None, sample_base: int = 0, recompute: bool = False,
                checkpoint_every=None) -> torch.Tensor:
        """``steps`` CA steps in one native call, one autograd node with grad enabled: see
        ``NeuralCAGraph.rollout`` (no ``message_gain`` / ``offsets`` here)."""
        return run_rollout(self, x, steps, None, False, fire_rate=fire_rate, nsteps=nsteps, min_steps=min_steps,
                           fire=fire, seed=seed, sample_base=sample_base, recompute=recompute,
                           checkpoint_every=checkpoint_every)

    def rollout_memory(self, x_or_shape, steps: int, *, fire_rate=1.0, nsteps=None, min_steps: int = 0,
                       fire=None, seed=None, sample_base: int = 0, recompute: bool = False,
                       checkpoint_every=None) -> dict:
        """Bytes ``rollout()`` with these arguments needs on the device: see
        ``NeuralCAGraph.rollout_memory``."""
        return run_rollout_memory(self, x_or_shape, steps, None, False, fire_rate=fire_rate, nsteps=nsteps,
                                  min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base,
                                  recompute=recompute, checkpoint_every=checkpoint_every)

    def rollout_objective(self, x: torch.Tensor, steps: int, target: torch.Tensor, *, every: int = 1, record=None,
                          loss: str = "premult", alpha_thr: float = 0.2, lam_area: float = 5e-5,
                          lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0, fire_rate=1.0, nsteps=None,
                          min_steps: int = 0, fire=None, seed=None, sample_base: int = 0,
                          recompute: bool = False, checkpoint_every=None) -> RolloutObjective:
        """``rollout()`` that also returns per-sample losses at intermediate steps, as one autograd node:
        see ``NeuralCAGraph.rollout_objective`` (no ``message_gain`` / ``offsets`` here).  Under
        ``no_grad`` it still returns ``x_final`` and ``losses`` (a states-only tape, freed at once); the
        tuned no-grad path stays ``trace(..., target=)``."""
        return run_rollout_objective(self, x, steps, target, None, False, every=every, record=record, loss=loss,
                                     alpha_thr=alpha_thr, lam_area=lam_area, lam_bg_alpha=lam_bg_alpha,
                                     lam_bg_rgb=lam_bg_rgb, fire_rate=fire_rate, nsteps=nsteps,
                                     min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base,
                                     recompute=recompute, checkpoint_every=checkpoint_every)

    def rollout_objective_tangent(self, x: torch.Tensor, steps: int, target: torch.Tensor, *, V=None, dparams=None,
                                  every: int = 1, record=None, loss: str = "premult", alpha_thr: float = 0.2,
                                  lam_area: float = 5e-5, lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0,
                                  fire_rate=1.0, nsteps=None, min_steps: int = 0, fire=None, seed=None,
                                  sample_base: int = 0, return_tangents: bool = False) -> ObjectiveTangent:
        """The tap losses of ``rollout_objective`` and their derivatives along K directions, forward mode, no
        tape: see ``NeuralCAGraph.rollout_objective_tangent`` (no ``message_gain`` / ``offsets`` here)."""
        return run_rollout_objective_tangent(self, x, steps, target, None, False, V=V, dparams=dparams, every=every,
                                             record=record, loss=loss, alpha_thr=alpha_thr, lam_area=lam_area,
                                             lam_bg_alpha=lam_bg_alpha, lam_bg_rgb=lam_bg_rgb, fire_rate=fire_rate,
                                             nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                             sample_base=sample_base, return_tangents=return_tangents)

    def rollout_gauss_newton(self, x: torch.Tensor, steps: int, target: torch.Tensor, *, dparams=None, v=None,
                             every: int = 1, record=None, loss: str = "premult", tap_weights=None,
                             checkpoint_every=None, alpha_thr: float = 0.2, lam_area: float = 5e-5,
                             lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0, fire_rate=1.0, nsteps=None,
                             min_steps: int = 0, fire=None, seed=None, sample_base: int = 0,
                             return_fields: bool = False) -> GaussNewtonProduct:
        """One Gauss-Newton curvature-vector product of the tap objective, a tangent forward that leaves a tape
        and one BPTT: see ``NeuralCAGraph.rollout_gauss_newton`` (no ``message_gain`` / ``offsets`` here)."""
        return run_rollout_gauss_newton(self, x, steps, target, None, False, dparams=dparams, v=v, every=every,
                                        record=record, loss=loss, alpha_thr=alpha_thr, lam_area=lam_area,
                                        lam_bg_alpha=lam_bg_alpha, lam_bg_rgb=lam_bg_rgb, tap_weights=tap_weights,
                                        checkpoint_every=checkpoint_every, fire_rate=fire_rate, nsteps=nsteps,
                                        min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base,
                                        return_fields=return_fields)

    def gauss_newton_memory(self, x_or_shape, steps: int, *, every: int = 1, record=None, checkpoint_every=None,
                            fire_rate=1.0, nsteps=None, min_steps: int = 0, fire=None, seed=None,
                            sample_base: int = 0) -> dict:
        """Bytes ``rollout_gauss_newton()`` with these arguments needs on the device: see
        ``NeuralCAGraph.gauss_newton_memory``."""
        return run_gauss_newton_memory(self, x_or_shape, steps, None, False, every=every, record=record,
                                       checkpoint_every=checkpoint_every, fire_rate=fire_rate, nsteps=nsteps,
                                       min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base)

    def trace(self, x: torch.Tensor, steps: int, *, every: int = 1, record=None, channels: int = 4,
              return_attention: bool = False, fire_rate=1.0, message_gain=None, seed=None,
              sample_base: int = 0, first_step: int = 0, offsets=None, target=None,
              frames: bool = True, diagnostics: bool = False, per_offset: bool = False,
              render=None, vitals=False) -> TraceResult:
        """``steps`` CA steps in one native call that also records frames: see ``NeuralCAGraph.trace``
        (same arguments and result; always under ``no_grad``, detached tensors).  The classic model
        has no graph term: ``return_attention=True``, ``diagnostics=True``, a ``message_gain`` or
        ``offsets`` raise ``ValueError``."""
        if return_attention:
            raise ValueError("return_attention: NeuralCA has no graph term, so no attention map")
        if diagnostics or per_offset:
            raise ValueError("diagnostics: NeuralCA has no graph term, so no graph diagnostics")
        if message_gain is not None:
            raise ValueError("message_gain given for a model without the graph term")
        return run_trace(self, x, steps, None, False, every=every, record=record, channels=channels,
                         fire_rate=fire_rate, seed=seed, sample_base=sample_base, first_step=first_step,
                         offsets=offsets, target=target, frames=frames, render=render, vitals=vitals)
