"""NeuralCAGraph — mirror of src/modules/ncagraph.py:10-168.

Same constructor signature, attributes (message_gain is read per call, alpha_thr, hidden_only,
update_gain), submodules (perception, update_net, norm, graph) and state_dict keys, so the
reference's trainer, test scripts and checkpoints use it unchanged.  forward() keeps the
reference's RNG contract: one ``random.sample`` (inside the graph step) and, only when
fire_rate < 1, one ``torch.rand(B,1,H,W)`` on x.device.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._stepper import (GaussNewtonProduct, ObjectiveTangent, param_direction, RolloutObjective,
                       TangentBlockResult, TangentResult, TraceResult, run_gauss_newton_memory, run_rollout,
                       run_rollout_gauss_newton, run_rollout_memory, run_rollout_objective,
                       run_rollout_objective_tangent, run_rollout_tangent, run_rollout_tangent_block, run_step,
                       run_tangent_step, run_trace)
from .graph_augmentation import GraphAugmentation
from .perception import FixedSobelPerception


class NeuralCAGraph(nn.Module):
    def __init__(self, n_channels: int, update_hidden: int = 128, img_size: int = 40,
                 update_gain: float = 0.1, alpha_thr: float = 0.1, use_groupnorm: bool = True, *,
                 message_gain: float = 0.5, hidden_only: bool = True, graph_d_model: int = 16,
                 graph_attention_radius: int = 4, graph_num_neighbors: int = 8,
                 graph_gating_hidden: int = 32, graph_alive_to_alive: bool = True,
                 graph_zero_padded_shift: bool = True, device: str = "cpu"):
        super().__init__()
        self.n_channels = n_channels
        self.img_size = img_size          # stored, unused (as in the reference)
        self.update_gain = float(update_gain)
        self.alpha_thr = float(alpha_thr)
        self.device = device              # stored, unused (as in the reference)
        self.perception = FixedSobelPerception(n_channels)
        self.update_net = nn.Sequential(
            nn.Conv2d(n_channels * 3, update_hidden, kernel_size=1, bias=True),
            nn.ReLU(inplace=False),
            nn.Conv2d(update_hidden, n_channels, kernel_size=1, bias=False))
        nn.init.zeros_(self.update_net[-1].weight)
        self.norm = nn.GroupNorm(1, n_channels, eps=1e-3, affine=True) if use_groupnorm else nn.Identity()
        self.graph = GraphAugmentation(
            n_channels=n_channels, d_model=graph_d_model, attention_radius=graph_attention_radius,
            num_neighbors=graph_num_neighbors, gating_hidden=graph_gating_hidden,
            alive_to_alive=graph_alive_to_alive, zero_padded_shift=graph_zero_padded_shift,
            alpha_thr=self.alpha_thr)
        self.message_gain = float(message_gain)
        self.hidden_only = bool(hidden_only)

    @torch.no_grad()
    def _alive_mask(self, x: torch.Tensor) -> torch.Tensor:
        """max_pool2d(alpha, 3, 1, 1) > alpha_thr (ncagraph.py:85-92); a helper, not the step."""
        return (F.max_pool2d(x[:, 3:4], kernel_size=3, stride=1, padding=1) > self.alpha_thr).float()

    def _apply_message_policy(self, m: torch.Tensor) -> torch.Tensor:
        """hidden_only zeroing + tanh * message_gain (ncagraph.py:94-104); a helper — inside the
        step this is fused into K1's epilogue."""
        if self.hidden_only and m.shape[1] >= 4:
            m = torch.cat([torch.zeros_like(m[:, :4]), m[:, 4:]], dim=1)
        return torch.tanh(m) * self.message_gain

    def forward(self, x: torch.Tensor, fire_rate: float = 1.0, *, return_attention: bool = False,
                active: torch.Tensor | None = None):
        """One CA step with the mid-range graph message, on the HIP path (ncagraph.py:106-168).

        ``active`` (extension, not in the reference): a [B] bool mask; ``model(x, fr, active=m)``
        equals the trainers' ``x[m] = model(x[m], fr)`` (train_graph_augmented_nca.py:305-321)
        without the sub-batch gather/scatter, except that the fire uniforms are drawn for the
        whole batch (``torch.rand(B,1,H,W)``) rather than for the active rows only."""
        chosen = self.graph.sample_offsets()
        out, attn = run_step(self, x, fire_rate, self.graph, chosen, self.message_gain,
                             self.hidden_only, return_attention, active=active)
        return (out, attn) if return_attention else out

    def param_direction(self, fill: float = 0.0) -> dict:
        """A correctly shaped ``dparams`` dict for ``tangent_step`` / ``rollout_tangent`` /
        ``rollout_tangent_block``: one tensor filled with ``fill`` per parameter a direction may perturb
        (``update_net.*``, ``norm.*``, ``graph.msg_proj.*``), keyed by its ``named_parameters()`` name."""
        return param_direction(self, fill)

    def tangent_step(self, x: torch.Tensor, v: torch.Tensor, fire_rate: float = 1.0, *, active=None, offsets=None,
                     fire=None, dparams=None):
        """One CA step and its forward-mode tangent (extension, not in the reference): ``(x_out, v_out)``
        with ``x_out`` bitwise ``forward``'s result and ``v_out = J(x) v``, the Jacobian-vector product of
        the step at ``x``, by one native call (``gnca_step_tangent``) that keeps no tape.

        The conventions are the backward's: the pre- and post-update alive masks, the sender mask and
        the fire mask are constants, the perception bank is frozen, the torus offset weights are 1/k.
        ``offsets=None`` draws ``self.graph.sample_offsets()`` and ``fire=None`` with a rate below 1
        draws ``torch.rand(B,1,H,W)`` on ``x.device``: Python's ``random`` and torch's generator are
        consumed exactly as ``forward`` consumes them.  ``offsets``: a list of (dy, dx) pairs; ``fire``:
        a [B,1,H,W] tensor of float32 uniforms or a uint8 / bool mask; ``active``: as ``forward``'s (an
        inactive sample passes ``x`` and ``v`` through).  Always runs under ``no_grad`` and returns
        detached tensors.  Torus mode only: a model built with ``graph_zero_padded_shift=True`` raises
        ``ValueError`` (its offset weights depend on the state).

        ``dparams``: a direction of the WEIGHTS carried beside ``v`` (``gnca_step_tangent_params``), so that
        ``v_out = J_x v + J_theta dparams``: a dict keyed by ``named_parameters()`` names, each tensor
        shaped like its parameter; a missing key is a zero direction, and ``v=None`` then means a zero
        state tangent.  ``graph.query_proj.*``, ``graph.key_proj.*``, ``graph.scaling`` and
        ``graph.gate_mlp.*`` are accepted and ignored (their effect is exactly zero in torus mode);
        ``perception.conv.weight`` (frozen), an unknown key, ``norm.*`` on a model without GroupNorm and a
        wrong shape, dtype or device raise ``ValueError`` before anything is drawn.  With
        ``dparams=None`` the call is the state tangent, bit for bit."""
        return run_tangent_step(self, x, v, fire_rate, self.graph, self.message_gain, self.hidden_only,
                                active=active, offsets=offsets, fire=fire, dparams=dparams)

    def rollout_tangent(self, x: torch.Tensor, v: torch.Tensor, steps: int, *, every=None, record=None,
                        renormalize: bool = False, fire_rate=1.0, message_gain=None, nsteps=None,
                        min_steps: int = 0, fire=None, seed=None, sample_base: int = 0,
                        offsets=None, dparams=None) -> TangentResult:
        """The tangent of a whole rollout (extension, not in the reference): where the nudge ``v`` of the
        state ``x`` is after ``steps`` steps, carried forward beside the state in one native call
        (``gnca_rollout_tangent``) with no tape, O(1) memory in ``steps``.

        Returns a ``TangentResult``: ``x_final``, bitwise the no-grad ``rollout()``'s result on the same
        schedule; ``v_final``, bitwise the chain of ``tangent_step`` calls; ``steps``, the recorded step
        indices; ``log_norm`` float64 [R,B], the log of the tangent's 2-norm per sample after each
        recorded step.  The schedule keywords mean what they mean in ``rollout()``; the taps follow
        ``trace()``'s rules (``every=n`` or ``record=[...]``; neither: nothing is recorded).
        ``renormalize=True`` rescales each sample's tangent to norm 1 on the device after every recorded
        step and carries the logs, so ``log_norm`` stays the un-renormalised curve while ``v`` cannot
        overflow: ``log_norm[-1] / steps`` is a finite-time Lyapunov exponent, with no host wait.
        Always runs under ``no_grad`` and returns detached tensors.  Bad arguments raise ``ValueError``
        before anything is drawn or launched.  Torus mode only (see ``tangent_step``).

        ``dparams`` (see ``tangent_step``): the same weight direction at every step
        (``gnca_rollout_tangent_params``), so that ``v_final = dx_T/dx v + dx_T/dtheta dparams``; ``v=None``
        is then a zero state tangent.  ``renormalize=True`` with a direction is a ``ValueError``: rescaling
        ``v`` alone breaks linearity in the pair.  ``log_norm`` is still recorded."""
        return run_rollout_tangent(self, x, v, steps, self.graph, self.hidden_only, every=every, record=record,
                                   renormalize=renormalize, fire_rate=fire_rate,
                                   message_gain=self.message_gain if message_gain is None else message_gain,
                                   nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                   sample_base=sample_base, offsets=offsets, dparams=dparams)

    def rollout_tangent_block(self, x: torch.Tensor, V: torch.Tensor, steps: int, *, every=None, record=None,
                              orthonormalize: bool = True, fire_rate=1.0, message_gain=None, nsteps=None,
                              min_steps: int = 0, fire=None, seed=None, sample_base: int = 0,
                              offsets=None, dparams=None) -> TangentBlockResult:
        """``rollout_tangent`` for a block of K directions ``V`` [K,B,C,H,W], 1 <= K <= 16, beside ONE
        primal state, in one native call (``gnca_rollout_tangent_block``): per step the primal step runs
        once and the two tangent kernels once per direction.

        ``orthonormalize=True`` (Benettin's method): at every recorded step the block is replaced on the
        device by Q of its thin QR per sample (``orthonormalize_tangents``' kernels, fp64, fixed order, no
        host wait) and ``log_r`` [R,B,K] carries the running sums of ``log R_jj``, so
        ``result.exponents()`` is the finite-time Lyapunov spectrum.  A direction that becomes zero,
        non-finite or dependent on the earlier ones is dropped: ``-inf`` from that record on, zeros in
        ``v_final``.  ``orthonormalize=False``: nothing is rescaled, column j is bitwise
        ``rollout_tangent(x, V[j])`` and ``log_r[:, :, j]`` its ``log_norm``.
        A sample that ``nsteps`` has finished keeps its block; later records re-factor an orthonormal
        block, so their contribution to ``log_r`` is 0 within rounding.  The schedule keywords, the taps
        and the refusals are ``rollout_tangent``'s.

        ``dparams``: a list of K dicts (see ``tangent_step``), direction j carrying the pair
        ``(V[j], dparams[j])`` (``gnca_rollout_tangent_block_params``); it needs ``orthonormalize=False``
        (mixing the tangents alone breaks linearity in the pairs), and ``V=None`` is then K zero tangents."""
        return run_rollout_tangent_block(self, x, V, steps, self.graph, self.hidden_only, every=every,
                                         record=record, orthonormalize=orthonormalize, fire_rate=fire_rate,
                                         message_gain=self.message_gain if message_gain is None else message_gain,
                                         nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                         sample_base=sample_base, offsets=offsets, dparams=dparams)

    def rollout(self, x: torch.Tensor, steps: int, *, fire_rate=1.0, message_gain=None, nsteps=None,
                min_steps: int = 0, fire=None, seed=None, sample_base: int = 0, offsets=None,
                recompute: bool = False, checkpoint_every=None) -> torch.Tensor:
        """``steps`` CA steps in one native call (extension, not in the reference); with grad enabled
        the whole rollout is ONE autograd node whose backward walks a device-side tape and reduces
        the weight gradients once per rollout.

        ``fire_rate`` / ``message_gain``: a number or ``steps`` numbers (``message_gain=None``:
        ``self.message_gain``).  ``offsets=None`` draws ``self.graph.sample_offsets()`` once per step
        in step order, consuming Python's ``random`` exactly as ``steps`` ``forward`` calls do
        (message-off steps included); else ``steps`` lists of (dy, dx) pairs.  ``nsteps``: int32 [B]
        device tensor, sample b takes step t iff ``t < nsteps[b]`` (the trainers' variable-length
        rollouts, never read on the host); steps ``t < min_steps`` run every sample.  ``fire``: a
        [steps,B,1,H,W] tensor of float32 uniforms or uint8 / bool masks; ``fire=None`` with a rate
        below 1 uses the counter-based hash masks of ``seed`` (``seed=None`` draws one integer from
        torch's default CPU generator) -- NOT the ``torch.rand`` stream ``forward`` draws from.
        ``recompute=True`` halves the tape (the backward recomputes each step's update field).
        ``checkpoint_every=k`` (an int >= 1, or ``"auto"`` = ``ceil(sqrt(steps))``) bounds it: the tape
        keeps every k-th state only and the backward re-runs the forward one segment of k steps at a
        time, so a 400-step rollout keeps 20 + 19 states instead of 400 at the price of one more
        forward.  ``x.grad`` and every parameter gradient are bitwise those of the plain tape; it
        composes with every other keyword (``rollout_memory`` gives the sizes).  Ignored under
        ``no_grad``, which records no tape.
        Under ``no_grad`` a uniform schedule (one rate, one gain, no ``nsteps``, hash or no fire)
        runs the large-batch rollout pipeline (``gnca_rollout_ex_f32``).  ``return_attention`` is
        not supported here: ``trace()`` records frames and attention maps."""
        return run_rollout(self, x, steps, self.graph, self.hidden_only, fire_rate=fire_rate,
                           message_gain=self.message_gain if message_gain is None else message_gain,
                           nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base,
                           offsets=offsets, recompute=recompute, checkpoint_every=checkpoint_every)

    def rollout_memory(self, x_or_shape, steps: int, *, fire_rate=1.0, message_gain=None, nsteps=None,
                       min_steps: int = 0, fire=None, seed=None, sample_base: int = 0, offsets=None,
                       recompute: bool = False, checkpoint_every=None) -> dict:
        """Bytes ``rollout()`` with these arguments needs on the device, as ``{"tape",
        "forward_workspace", "backward_workspace"}``, from the library's host-only size queries: no
        GPU is touched, so it also runs on a machine without one.  ``x_or_shape``: the state or its
        (B, C, H, W).  The schedule is built as ``rollout()`` builds it (``offsets=None`` draws them,
        which can move the workspaces by the offsets' reach), and Python's ``random`` and torch's CPU
        generator are left as they were found.  The tape and the backward workspace live from the
        forward to the end of the backward, the forward workspace during the forward only."""
        return run_rollout_memory(self, x_or_shape, steps, self.graph, self.hidden_only, fire_rate=fire_rate,
                                  message_gain=self.message_gain if message_gain is None else message_gain,
                                  nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                  sample_base=sample_base, offsets=offsets, recompute=recompute,
                                  checkpoint_every=checkpoint_every)

    def rollout_objective(self, x: torch.Tensor, steps: int, target: torch.Tensor, *, every: int = 1, record=None,
                          loss: str = "premult", alpha_thr: float = 0.2, lam_area: float = 5e-5,
                          lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0, fire_rate=1.0, message_gain=None,
                          nsteps=None, min_steps: int = 0, fire=None, seed=None, sample_base: int = 0,
                          offsets=None, recompute: bool = False, checkpoint_every=None) -> RolloutObjective:
        """``rollout()`` that also returns per-sample losses at intermediate steps, as ONE autograd node
        (extension, not in the reference): the trainers' supervision of several steps of one rollout
        without a chain of ``rollout()`` + loss nodes.

        Returns a ``RolloutObjective``: ``x_final`` [B,C,H,W], exactly ``rollout()``'s result;
        ``losses`` float32 [R,B], the loss of the state after each tapped step; ``steps``, the R tapped
        step indices.  The taps follow ``trace()``'s rules: ``every=n`` taps steps ``n, 2n, ...`` and
        also ``steps`` when it is not a multiple, ``record`` lists them instead (strictly increasing, in
        ``1..steps``).  ``loss="premult"`` is ``loss_premult_rgba(state[:, :4], target)``,
        ``loss="masked"`` is ``masked_loss(state[:, :4], target, alpha_thr, lam_area, lam_bg_alpha,
        lam_bg_rgb)``, bitwise; ``target`` is [4,H,W], [1,4,H,W] or [B,4,H,W].  Every other keyword is
        ``rollout()``'s.  Bad arguments raise ``ValueError`` before anything is drawn or launched.

        The losses are read from the rollout's tape in place and their gradients join the backward's
        running cotangent between two steps; build any scalar from ``losses`` (a mean, per-tap
        weights) and, if wanted, from ``x_final``, and call ``backward()`` once: ``x.grad`` is bitwise
        that of the chain of ``rollout()`` segments with a loss on each segment's end.  A sample with
        ``nsteps[b]`` below a tapped step contributes the loss of its frozen state.  A second backward
        raises, as for ``rollout()``.

        ``checkpoint_every`` is ``rollout()``'s: the forward then writes each tap's loss as its state is
        produced (``gnca_rollout_fwd_taps``), since a checkpointed tape holds few of the tapped states;
        losses and gradients are bitwise those of the plain tape.

        Under ``no_grad``, or when nothing requires grad, ``x_final`` and ``losses`` are still returned
        (a states-only tape is recorded and freed; with ``checkpoint_every`` no tape at all); that is
        not the tuned no-grad path, which stays ``trace(..., target=)``."""
        return run_rollout_objective(self, x, steps, target, self.graph, self.hidden_only, every=every,
                                     record=record, loss=loss, alpha_thr=alpha_thr, lam_area=lam_area,
                                     lam_bg_alpha=lam_bg_alpha, lam_bg_rgb=lam_bg_rgb, fire_rate=fire_rate,
                                     message_gain=self.message_gain if message_gain is None else message_gain,
                                     nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                     sample_base=sample_base, offsets=offsets, recompute=recompute,
                                     checkpoint_every=checkpoint_every)

    def rollout_objective_tangent(self, x: torch.Tensor, steps: int, target: torch.Tensor, *, V=None, dparams=None,
                                  every: int = 1, record=None, loss: str = "premult", alpha_thr: float = 0.2,
                                  lam_area: float = 5e-5, lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0,
                                  fire_rate=1.0, message_gain=None, nsteps=None, min_steps: int = 0, fire=None,
                                  seed=None, sample_base: int = 0, offsets=None,
                                  return_tangents: bool = False) -> ObjectiveTangent:
        """The forward-mode twin of ``rollout_objective`` (extension, not in the reference): the per-sample
        losses of the tapped steps AND their derivatives along K directions, in one native call
        (``gnca_rollout_objective_tangent``) with no tape, O(1) memory in ``steps`` and no backward.

        ``V`` [K,B,C,H,W] are K state tangents, ``dparams`` one dict (K = 1) or a list of K dicts of weight
        directions (see ``tangent_step``); direction k carries the pair ``(V[k], dparams[k])``, a missing
        one is zero, and at least one of the two must be given.  Returns an ``ObjectiveTangent``:
        ``x_final``, bitwise the no-grad ``rollout()``'s; ``losses`` float32 [R,B], bitwise
        ``rollout_objective``'s; ``dlosses`` float64 [R,K,B], the derivative of ``losses[r,b]`` along
        direction k, computed on the device right after the tapped step wrote its state and tangents (they
        are never recorded); ``steps``; ``v_final`` [K,B,C,H,W] with ``return_tangents=True`` (bitwise
        ``rollout_tangent_block(..., orthonormalize=False)``'s), else None.

        The loss keywords, tap rules and target shapes are ``rollout_objective``'s; the schedule keywords
        and the RNG consumption are ``rollout_tangent_block``'s.  Always under ``no_grad``; bad arguments
        raise ``ValueError`` before anything is drawn or launched.  Torus mode only (see ``tangent_step``).
        With ``forward_grad.ParamDirections`` and ``forward_grad.forward_gradient_`` this is a training step
        without a backward: ``dlosses`` and the directions become ``.grad`` with no host wait."""
        return run_rollout_objective_tangent(self, x, steps, target, self.graph, self.hidden_only, V=V,
                                             dparams=dparams, every=every, record=record, loss=loss,
                                             alpha_thr=alpha_thr, lam_area=lam_area, lam_bg_alpha=lam_bg_alpha,
                                             lam_bg_rgb=lam_bg_rgb, fire_rate=fire_rate,
                                             message_gain=self.message_gain if message_gain is None else message_gain,
                                             nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                             sample_base=sample_base, offsets=offsets,
                                             return_tangents=return_tangents)

    def rollout_gauss_newton(self, x: torch.Tensor, steps: int, target: torch.Tensor, *, dparams=None, v=None,
                             every: int = 1, record=None, loss: str = "premult", tap_weights=None,
                             checkpoint_every=None, alpha_thr: float = 0.2, lam_area: float = 5e-5,
                             lam_bg_alpha: float = 0.0, lam_bg_rgb: float = 0.0, fire_rate=1.0, message_gain=None,
                             nsteps=None, min_steps: int = 0, fire=None, seed=None, sample_base: int = 0,
                             offsets=None,
                             return_fields: bool = False) -> GaussNewtonProduct:
        """One Gauss-Newton curvature-vector product of the tap objective (extension, not in the reference):
        ``G (dparams, v) = sum_r scale_r J_r^T H_r J_r (dparams, v)`` for ``L = sum_r scale_r sum_b losses[r,b]``,
        ``scale_r = tap_weights[r] / B`` (weights default to 1; R host numbers).  ``J_r`` is the Jacobian of the
        state after tapped step r with respect to the weights and ``x``; ``H_r`` the loss's Gauss-Newton
        curvature there (``loss.loss_curvature``), so ``G`` is symmetric positive semidefinite.

        Two native calls: a tangent forward for the ONE direction ``(dparams, v)`` (a dict as ``tangent_step``
        takes it, a [B,C,H,W] tangent of ``x``; a missing one is zero, at least one must be given) that writes
        the states-only tape of ``rollout(recompute=True)`` as it goes and, after every tapped step, that
        tap's curvature field (``gnca_rollout_gn_fwd``); then the BPTT of that tape with the scaled fields
        injected where ``rollout_objective``'s backward injects the loss gradients
        (``gnca_rollout_gn_bwd``).  The primal runs once; no [R,B,C,H,W] tangents are recorded.

        Returns a ``GaussNewtonProduct``: ``product`` (a dict keyed like ``param_direction()``), ``gx``,
        ``x_final`` / ``losses`` (bitwise ``rollout_objective``'s), ``dlosses`` (bitwise
        ``rollout_objective_tangent``'s), ``quad`` and the device scalar ``energy`` =
        ``<dparams, product> + <v, gx>`` in exact arithmetic, never negative.  ``checkpoint_every`` is
        ``rollout()``'s and changes no number.  The loss keywords, tap rules and target shapes are
        ``rollout_objective``'s; the schedule keywords and the RNG consumption are ``rollout_tangent``'s.
        Always under ``no_grad``; bad arguments raise ``ValueError`` before anything is drawn or launched.
        Torus mode only (see ``tangent_step``).  ``gauss_newton.cg_solve`` turns this into a damped
        Gauss-Newton step."""
        return run_rollout_gauss_newton(self, x, steps, target, self.graph, self.hidden_only, dparams=dparams, v=v,
                                        every=every, record=record, loss=loss, alpha_thr=alpha_thr,
                                        lam_area=lam_area, lam_bg_alpha=lam_bg_alpha, lam_bg_rgb=lam_bg_rgb,
                                        tap_weights=tap_weights, checkpoint_every=checkpoint_every,
                                        fire_rate=fire_rate,
                                        message_gain=self.message_gain if message_gain is None else message_gain,
                                        nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                        sample_base=sample_base, offsets=offsets,
                                        return_fields=return_fields)

    def gauss_newton_memory(self, x_or_shape, steps: int, *, every: int = 1, record=None, checkpoint_every=None,
                            fire_rate=1.0, message_gain=None, nsteps=None, min_steps: int = 0, fire=None, seed=None,
                            sample_base: int = 0, offsets=None) -> dict:
        """Bytes ``rollout_gauss_newton()`` with these arguments needs on the device: ``tape``,
        ``forward_workspace``, ``backward_workspace`` and ``fields``.  Host-only, as ``rollout_memory``."""
        return run_gauss_newton_memory(self, x_or_shape, steps, self.graph, self.hidden_only, every=every,
                                       record=record, checkpoint_every=checkpoint_every, fire_rate=fire_rate,
                                       message_gain=self.message_gain if message_gain is None else message_gain,
                                       nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                                       sample_base=sample_base, offsets=offsets)

    def trace(self, x: torch.Tensor, steps: int, *, every: int = 1, record=None, channels: int = 4,
              return_attention: bool = False, fire_rate=1.0, message_gain=None, seed=None,
              sample_base: int = 0, first_step: int = 0, offsets=None, target=None,
              frames: bool = True, diagnostics: bool = False, per_offset: bool = False,
              render=None, vitals=False) -> TraceResult:
        """``steps`` CA steps in one native call that also records (extension, not in the reference):
        the per-step Python loop of the regeneration diagnostic and the video generators, on the
        rollout pipeline.  Always runs under ``no_grad`` and returns detached tensors, whatever the
        caller's grad mode: for gradients use ``rollout()``.

        Returns a ``TraceResult``: ``x_final``; ``frames`` [R,B,channels,H,W], channels
        ``0..channels-1`` of the state after each recorded step; ``steps``, the recorded step indices
        (from 1, within this call); ``attention`` [R,B,H,W] with ``return_attention=True``, the
        normalised map of each recorded step (computed from that step's input state and offsets, as
        ``forward(..., return_attention=True)`` does), else None.

        ``every=n`` records steps ``n, 2n, ...`` and also ``steps`` when it is not a multiple;
        ``record`` lists the indices instead (strictly increasing, in ``1..steps``).  The schedule is
        the uniform one of the no-grad ``rollout()``: one ``fire_rate`` and one ``message_gain``
        (``None``: ``self.message_gain``), hash fire masks of ``seed`` when the rate is below 1.
        ``first_step`` is the hash RNG's step base: ``trace(x, 4, seed=s)`` followed by
        ``trace(x_final, 3, seed=s, first_step=4)`` (and the matching offsets) continues one fire
        stream, so "grow, damage, regrow" is two calls.  ``offsets=None`` draws
        ``self.graph.sample_offsets()`` once per step in step order, as ``rollout()`` does.  Bad
        arguments raise ``ValueError`` before anything is drawn or launched.

        ``target`` (premultiplied RGBA, [4,H,W], [1,4,H,W] or [B,4,H,W]) also measures: the result's
        ``metrics`` is an ``ImageMetrics`` (mse, pixel_perfect, psnr, ssim; ``metrics.py``) of shape
        [R,B], the state after each recorded step against the target, bitwise
        ``image_metrics(frames, target)``.  ``frames=False`` allocates and records no frames
        (``result.frames`` is None): a regeneration curve is then [R,B,4] floats and nothing else.

        ``diagnostics=True`` also records, for every recorded step, ``self.graph.diagnostics`` of that
        step's input state with that step's offsets (the convention of ``attention``): the result's
        ``diagnostics`` is a ``GraphDiagnostics`` whose fields lead with the R axis, bitwise the
        standalone call's; ``per_offset=True`` includes the [R,B,k,H,W] stack.  The other results are
        bitwise those of the trace without it.

        ``render=True`` or ``render=dict(upscale=4, mode="rgb", alpha_thr=None, cmap="viridis")`` also turns
        the recorded frames into uint8 images on the device, one launch over all of them: the result's
        ``rgb_u8`` [R,B,H*upscale,W*upscale,3|4] is bitwise ``render.render_rgb(frames, ...)``
        (``alpha_thr=None``: ``self.alpha_thr``), and with ``return_attention`` its ``attention_u8``
        [R,B,H,W,3] is bitwise ``render.colorize(attention, cmap)``.  Needs ``frames=True`` and
        ``channels >= 4``.

        ``vitals=True`` (``alpha_thr = self.alpha_thr``) or ``vitals=<threshold>`` also takes
        ``vitals.state_vitals`` of the whole state after each recorded step: the result's ``vitals`` is a
        ``StateVitals`` of shape [R,B] (live and mature counts, alpha sums, centroid, bounding box, largest
        magnitude, non-finite count, hidden rms), bitwise the standalone call on those states.  It works
        with ``frames=False``: ``trace(x, T, every=1, frames=False, vitals=True).vitals.alive`` is a growth
        curve.  The other results are bitwise those of the trace without it."""
        return run_trace(self, x, steps, self.graph, self.hidden_only, every=every, record=record,
                         channels=channels, return_attention=return_attention, fire_rate=fire_rate,
                         message_gain=self.message_gain if message_gain is None else message_gain, seed=seed,
                         sample_base=sample_base, first_step=first_step, offsets=offsets, target=target,
                         frames=frames, diagnostics=diagnostics, per_offset=per_offset, render=render,
                         vitals=vitals)
