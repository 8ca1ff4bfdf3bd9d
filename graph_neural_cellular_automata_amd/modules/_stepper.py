"""Shared forward of NeuralCA / NeuralCAGraph: descriptor + weights -> one HIP step."""
from __future__ import annotations

import contextlib
import ctypes
import random
import weakref

import torch
import torch.nn as nn

from .. import _lib as L
from .. import metrics as M
from .. import render as R
from .. import step as S
from .. import vitals as V


class _ParamPack(torch.autograd.Function):
    """Routes ONE flat gradient to a group of parameters.

    Every step of a rollout hands its parameter gradients to the rollout's shared pack token as
    one flat tensor, so autograd sums them with one add per step and the parameters'
    AccumulateGrad runs once per backward instead of once per parameter per step (12 small
    launches per step at the trainer's size).  The token's value is never read."""

    @staticmethod
    def forward(ctx, sizes, *params):
        ctx.set_materialize_grads(False)
        ctx.sizes = sizes
        ctx.shapes = [p.shape for p in params]
        return params[0].new_empty(sum(sizes))

    @staticmethod
    def backward(ctx, flat):
        if flat is None:
            return (None,) * (1 + len(ctx.shapes))
        return (None, *[g.view(s) for g, s in zip(flat.split(ctx.sizes), ctx.shapes)])


class _Pack:
    """A group of parameters (state_dict names) behind one _ParamPack token."""

    def __init__(self, named):
        self.names = tuple(n for n, _ in named)
        self.params = [p for _, p in named]
        self.sizes = tuple(p.numel() for p in self.params)
        self.token = _ParamPack.apply(self.sizes, *self.params)

    def views(self, flat):
        return {n: g.view(p.shape) for n, g, p in zip(self.names, flat.split(self.sizes), self.params)}


_PACKS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
# fast path: the step's weight-tensor tuple and requires_grad flags -> packs; a hit skips rebuilding
# the named list (7.5 -> 5 us per step).  A weak-keyed side table, not a module attribute: the
# packs hold non-leaf tensors, which would break copy.deepcopy(model)
_PACKS_FAST: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


_SHORT_TO_NAME = {v: k for k, v in S.GRAD_FIELDS.items()}


def param_packs(model: nn.Module, tensors: dict | None = None):
    """(core, graph) packs of the model's trainable parameters that the step backward produces
    (GRAD_FIELDS; ``gate_mlp`` and the frozen perception are never in a pack, so they keep
    ``grad=None`` as in the reference).  ``tensors``: the step's weight tensors by short name
    (``run_step`` has them already; walking ``named_parameters`` costs ~30 us per step).  Cached
    per module: the token only routes gradients, so it stays valid across optimiser steps as
    long as the parameter objects are the same."""
    if tensors is not None:   # fast path: the same parameter objects and requires_grad flags
        vals = tuple(tensors.values())
        flags = tuple(t.requires_grad for t in vals)
        fast = _PACKS_FAST.get(model)
        if fast is not None and fast[0] == flags and len(fast[1]) == len(vals) and \
                all(a is b for a, b in zip(fast[1], vals)):
            return fast[2]
    if tensors is None:
        named = [(n, p) for n, p in model.named_parameters() if n in S.GRAD_FIELDS]
    else:
        named = [(_SHORT_TO_NAME[k], t) for k, t in tensors.items() if k in _SHORT_TO_NAME]
    named = [(n, p) for n, p in named if p.requires_grad]
    dev = named[0][1].device if named else None
    hit = _PACKS.get(model)
    if hit is not None and len(hit[0]) == len(named) and all(a is b for a, (_, b) in zip(hit[0], named)) \
            and hit[2] == dev:
        if tensors is not None:
            _PACKS_FAST[model] = (flags, vals, hit[1])
        return hit[1]
    core = [(n, p) for n, p in named if not n.startswith("graph.")]
    graph = [(n, p) for n, p in named if n.startswith("graph.")]
    packs = (_Pack(core) if core else None, _Pack(graph) if graph else None)
    _PACKS[model] = (tuple(p for _, p in named), packs, dev)
    if tensors is not None:
        _PACKS_FAST[model] = (flags, vals, packs)
    return packs


class _StepFn(torch.autograd.Function):
    """The HIP step as an autograd node (BPTT through the trainers' rollouts).

    Forward: ``gnca_step_f32`` into a workspace that the node keeps (the step's update field and
    GroupNorm partials, ~one state of memory).  Backward: ``gnca_step_bwd_f32`` on that saved
    workspace; everything else (perception, hidden layer, message) is recomputed from the input
    state, so a rollout keeps two state-sized tensors per step alive, far less than the
    reference's per-op activations.  Gradients follow the
    reference's graph of tensors: masks are constants, the perception weight is frozen,
    ``gate_mlp`` is never used (None), and the graph parameters get None when no offsets were
    drawn (``graph_augmentation.py:141-147`` returns zeros without touching them).  Parameter
    gradients leave as one flat tensor per pack (see ``_ParamPack``), written in place by the
    backward's reduce kernel."""

    @staticmethod
    def forward(ctx, x, desc, weights, keep, fire, want_attn, active, core, graph, tok_core, tok_graph,
                tensors=None):
        ws = S.workspace(desc, x.device)   # kept: the backward reuses its update field
        out, attn = S.step(desc, weights, x, fire=fire, want_attention=want_attn, ws=ws, active=active)
        if attn is not None:
            ctx.mark_non_differentiable(attn)
        ctx.save_for_backward(x)
        ctx.desc, ctx.weights, ctx.keep, ctx.fire = desc, weights, keep, fire
        ctx.ws = ws
        ctx.active = active
        ctx.packs = (core, graph)
        # the weights are passed to the kernels as raw pointers (not saved tensors), so autograd's
        # version check would not see an in-place update between forward and backward (an
        # optimizer step, load_state_dict, EMA swap): record the versions and check them ourselves
        ctx.versions = tuple((t, t._version) for t in (tensors or {}).values())
        return out, attn

    @staticmethod
    def backward(ctx, gout, gattn):
        (x,) = ctx.saved_tensors
        for t, v in ctx.versions:
            if t._version != v:
                raise RuntimeError(
                    "one of the variables needed for gradient computation has been modified by an "
                    f"inplace operation: a step weight of shape {tuple(t.shape)} is at version "
                    f"{t._version}; expected version {v} instead")
        desc = ctx.desc
        no_graph_use = (desc.flags & L.GRAPH) and desc.num_offsets == 0
        want, views, flats = {}, {}, [None, None]
        for i, pack in enumerate(ctx.packs):
            if pack is None or not ctx.needs_input_grad[9 + i] or (i == 1 and no_graph_use):
                continue
            flats[i] = torch.empty(sum(pack.sizes), dtype=torch.float32, device=x.device)
            views.update(pack.views(flats[i]))
            want.update(zip(pack.names, pack.params))
        gx, _ = S.step_backward(desc, ctx.weights, x, gout.contiguous(), fire=ctx.fire, want=want,
                                saved=ctx.ws, active=ctx.active, out=views)
        ctx.ws = None
        return (gx if ctx.needs_input_grad[0] else None, None, None, None, None, None, None, None, None,
                flats[0], flats[1], None)


def apply_step(model: nn.Module, x, desc, weights, keep, fire, want_attn=False, active=None, tensors=None):
    """One differentiable step: the HIP forward, and the HIP backward into the model's packs."""
    core, graph = param_packs(model, tensors)
    tc = core.token if core is not None else None
    tg = graph.token if graph is not None else None
    return _StepFn.apply(x, desc, weights, keep, fire, want_attn, active, core, graph, tc, tg, tensors)


def _step_tensors(model: nn.Module, graph) -> dict:
    """The step's weight tensors by short name, read straight from the modules' parameter dicts
    (``nn.Module.__getattr__`` costs ~1 us per attribute: building this dict through it was ~30 us
    of host time per step at the trainer's size, more than the step's kernels)."""
    mods = model._modules
    up = mods["update_net"]._modules
    l1, l2 = up["0"]._parameters, up["2"]._parameters
    t = {"perception": mods["perception"]._modules["conv"]._parameters["weight"],
         "w1": l1["weight"], "b1": l1["bias"], "w2": l2["weight"]}
    norm = mods["norm"]
    if isinstance(norm, nn.GroupNorm):
        t["gn_weight"] = norm._parameters["weight"]
        t["gn_bias"] = norm._parameters["bias"]
    if graph is not None:
        gm = graph._modules
        q, k, m = (gm[n]._parameters for n in ("query_proj", "key_proj", "msg_proj"))
        t.update(wq=q["weight"], bq=q["bias"], wk=k["weight"], bk=k["bias"], wm=m["weight"], bm=m["bias"],
                 scaling=graph._parameters["scaling"])
    return t


_DESC_TEMPLATES: dict = {}


def _step_desc(key, chosen, message_gain, fire_rate, fire_mode):
    """A fresh descriptor: the fields fixed by (shape, flags, model constants) copied from a cached
    template, then this call's offsets, message gain and fire fields (make_desc was ~10 us)."""
    tpl = _DESC_TEMPLATES.get(key)
    if tpl is None:
        B, C, H, W, hidden, d_model, flags, update_gain, alpha_thr, graph_thr, eps = key
        tpl = S.make_desc(B=B, C=C, H=H, W=W, hidden=hidden, d_model=d_model, offsets=[], flags=flags,
                          update_gain=update_gain, alpha_thr=alpha_thr, graph_alpha_thr=graph_thr,
                          message_gain=0.0, fire_rate=1.0, fire_mode=L.FIRE_NONE, gn_eps=eps)
        if len(_DESC_TEMPLATES) >= 256:
            _DESC_TEMPLATES.clear()
        _DESC_TEMPLATES[key] = tpl
    d = L.StepDesc.from_buffer_copy(tpl)
    if chosen:
        if len(chosen) > L.MAX_OFFSETS:
            raise ValueError(f"at most {L.MAX_OFFSETS} offsets per step (got {len(chosen)})")
        flat = [v for o in chosen for v in o]
        if min(flat) < -127 or max(flat) > 127:
            raise ValueError(f"offsets {chosen} out of int8 range")
        d.num_offsets = len(chosen)
        d.offsets[:len(flat)] = flat
    d.message_gain = float(message_gain)
    d.fire_rate = float(fire_rate)
    d.fire_mode = fire_mode
    return d


def run_step(model: nn.Module, x: torch.Tensor, fire_rate: float, graph, chosen, message_gain,
             hidden_only: bool, return_attention: bool, active=None):
    x = S.check_state(x, model.n_channels)
    B, C, H, W = x.shape
    flags = 0
    norm = model._modules["norm"]
    eps = 1e-3
    if isinstance(norm, nn.GroupNorm):
        if norm.num_groups != 1 or not norm.affine:
            raise ValueError("only GroupNorm(1, C, affine=True) is supported (ncagraph.py:68)")
        flags |= L.USE_GROUPNORM
        eps = norm.eps
    elif not isinstance(norm, nn.Identity):
        raise ValueError(f"unsupported norm module {type(norm).__name__}")
    tensors = _step_tensors(model, graph)
    d_model = 1
    graph_thr = None
    if graph is not None:
        flags |= graph.flags(return_attention)
        if hidden_only:
            flags |= L.HIDDEN_ONLY
        d_model = graph.d_model
        graph_thr = graph.alpha_thr
    # stochastic fire mask: the reference's torch.rand draw, on x.device (ncagraph.py:144-146)
    fire = None
    fire_mode = L.FIRE_NONE
    if fire_rate < 1.0:
        fire = torch.rand(B, 1, H, W, device=x.device)
        fire_mode = L.FIRE_RAND_F32
    alpha_thr = float(model.alpha_thr)
    key = (B, C, H, W, tensors["w1"].shape[0], d_model, flags, float(model.update_gain), alpha_thr,
           alpha_thr if graph_thr is None else float(graph_thr), float(eps))
    desc = _step_desc(key, chosen, message_gain, fire_rate, fire_mode)
    w, keep = S.make_weights(tensors)
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in tensors.values())):
        out, attn = apply_step(model, x, desc, w, keep, fire, return_attention, active, tensors)
    else:
        out, attn = S.step(desc, w, x, fire=fire, want_attention=return_attention, active=active)
    return out, attn


class _RolloutFn(torch.autograd.Function):
    """A whole rollout as ONE autograd node: ``gnca_rollout_fwd_f32`` with a tape forward,
    ``gnca_rollout_bwd_f32`` backward.  The weight-gradient partials are accumulated across the
    steps on the device and reduced once, so the parameter gradients leave as one flat tensor per
    pack per rollout (``_ParamPack``), not one per step."""

    @staticmethod
    def forward(ctx, x, call, weights, keep, core, graph, tok_core, tok_graph, tensors=None):
        out, tape = call.forward(weights, x, want_tape=True)
        ctx.call, ctx.weights, ctx.keep, ctx.tape = call, weights, keep, tape
        ctx.packs = (core, graph)
        # raw weight pointers: check the versions ourselves, as _StepFn does
        ctx.versions = tuple((t, t._version) for t in (tensors or {}).values())
        return out

    @staticmethod
    def backward(ctx, gout):
        for t, v in ctx.versions:
            if t._version != v:
                raise RuntimeError(
                    "one of the variables needed for gradient computation has been modified by an "
                    f"inplace operation: a rollout weight of shape {tuple(t.shape)} is at version "
                    f"{t._version}; expected version {v} instead")
        if ctx.tape is None:
            raise RuntimeError("rollout: backward through the same rollout a second time (its tape was freed)")
        desc = ctx.call.desc
        no_graph_use = (desc.flags & L.GRAPH) and desc.num_offsets == 0
        want, views, flats = {}, {}, [None, None]
        for i, pack in enumerate(ctx.packs):
            if pack is None or not ctx.needs_input_grad[6 + i] or (i == 1 and no_graph_use):
                continue
            flats[i] = torch.empty(sum(pack.sizes), dtype=torch.float32, device=gout.device)
            views.update(pack.views(flats[i]))
            want.update(zip(pack.names, pack.params))
        gx, _ = ctx.call.backward(ctx.weights, ctx.tape, gout.contiguous(), want=want, out=views)
        ctx.tape = None
        return (gx if ctx.needs_input_grad[0] else None, None, None, None, None, None, flats[0], flats[1], None)


def _rollout_desc(model: nn.Module, x, steps: int, graph, hidden_only: bool, sched):
    """(desc, weights, keep, tensors) of a rollout of ``sched`` on ``x``: the shared front of
    ``run_rollout`` and ``run_trace``."""
    desc, tensors = _rollout_desc_host(model, tuple(x.shape), steps, graph, hidden_only, sched)
    w, keep = S.make_weights(tensors)
    return desc, w, keep, tensors


def _rollout_desc_host(model: nn.Module, shape, steps: int, graph, hidden_only: bool, sched):
    """(desc, tensors): the descriptor alone, from the state's shape (no device pointer is taken)."""
    B, C, H, W = shape
    flags, eps = _check_norm(model)
    tensors = _step_tensors(model, graph)
    d_model = 1
    graph_thr = None
    if graph is not None:
        flags |= graph.flags(False)
        if hidden_only:
            flags |= L.HIDDEN_ONLY
        d_model = graph.d_model
        graph_thr = graph.alpha_thr
    alpha_thr = float(model.alpha_thr)
    key = (B, C, H, W, tensors["w1"].shape[0], d_model, flags, float(model.update_gain), alpha_thr,
           alpha_thr if graph_thr is None else float(graph_thr), float(eps))
    first = sched.offsets[0] if sched.offsets and steps > 0 else None
    desc = _step_desc(key, first, sched.gains[0] if sched.gains and steps > 0 else 0.0,
                      sched.fire_rates[0] if steps > 0 else 1.0, sched.fire_mode)
    desc.num_offsets = sched.k
    if steps == 0 and graph is not None:
        # nothing was drawn: keep the count forward() would draw, so that the (all-zero) graph
        # gradients are tensors, as after a rollout of message-off steps
        desc.num_offsets = min(graph.num_neighbors, len(graph.offsets))
    desc.rng_seed = sched.seed & 0xFFFFFFFFFFFFFFFF
    desc.sample_base = sched.sample_base
    return desc, tensors


def _check_norm(model: nn.Module):
    """(flags, eps) of the model's norm module, or ValueError for one the step does not support."""
    norm = model._modules["norm"]
    if isinstance(norm, nn.GroupNorm):
        if norm.num_groups != 1 or not norm.affine:
            raise ValueError("only GroupNorm(1, C, affine=True) is supported (ncagraph.py:68)")
        return L.USE_GROUPNORM, norm.eps
    if not isinstance(norm, nn.Identity):
        raise ValueError(f"unsupported norm module {type(norm).__name__}")
    return 0, 1e-3


def run_rollout(model: nn.Module, x: torch.Tensor, steps: int, graph, hidden_only: bool, *, fire_rate=1.0,
                message_gain=None, nsteps=None, min_steps=0, fire=None, seed=None, sample_base=0, offsets=None,
                recompute=False, checkpoint_every=None):
    """``steps`` CA steps in one native call (and, with grad, one autograd node): the shared body of
    ``NeuralCA.rollout`` / ``NeuralCAGraph.rollout``."""
    S.checkpoint_interval(checkpoint_every, steps if isinstance(steps, int) else 0)   # (pure Python, first)
    x = S.check_state(x, model.n_channels)
    B, C, H, W = x.shape
    _check_norm(model)   # (before the schedule draws its offsets)
    sched = S.build_schedule(steps=steps, B=B, H=H, W=W, device=x.device, fire_rate=fire_rate,
                             message_gain=message_gain, nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                             sample_base=sample_base, offsets=offsets,
                             sample_offsets=None if graph is None else graph.sample_offsets, recompute=recompute,
                             checkpoint_every=checkpoint_every)
    desc, w, keep, tensors = _rollout_desc(model, x, steps, graph, hidden_only, sched)
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in tensors.values())):
        core, gpack = param_packs(model, tensors)
        tc = core.token if core is not None else None
        tg = gpack.token if gpack is not None else None
        return _RolloutFn.apply(x, S.RolloutCall(desc, sched), w, keep, core, gpack, tc, tg, tensors)
    if sched.uniform and steps > 0:
        # the no-grad pipeline (compact update field, sub-batch streams, the fold, alive hand-over)
        return S.rollout(desc, w, x, steps, sched.offsets or [])
    out, _ = S.RolloutCall(desc, sched).forward(w, x, want_tape=False)
    return out


def _shape_and_device(model: nn.Module, x_or_shape, nsteps, fire):
    """(shape, device) of a state given as a tensor or as its shape (then the device of ``nsteps`` or ``fire``,
    else the CPU); ValueError unless it is a [B,C,H,W] of the model's channel count."""
    if isinstance(x_or_shape, torch.Tensor):
        shape, device = tuple(x_or_shape.shape), x_or_shape.device
    else:
        shape = tuple(int(v) for v in x_or_shape)
        given = nsteps if nsteps is not None else fire
        device = given.device if isinstance(given, torch.Tensor) else torch.device("cpu")
    if len(shape) != 4:
        raise ValueError(f"state must be [B,C,H,W], got {shape}")
    if shape[1] != model.n_channels:
        raise ValueError(f"state has {shape[1]} channels, model expects {model.n_channels}")
    return shape, device


@contextlib.contextmanager
def _rng_restored():
    """Python's and torch's CPU RNG states are put back on the way out."""
    py_state, torch_state = random.getstate(), torch.get_rng_state()
    try:
        yield
    finally:
        random.setstate(py_state)
        torch.set_rng_state(torch_state)


def _steps_int(steps, minimum: int) -> None:
    """ValueError unless ``steps`` is an int >= ``minimum`` (0 or 1)."""
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < minimum:
        raise ValueError(f"steps must be a {'positive' if minimum else 'non-negative'} int, got {steps!r}")


def run_rollout_memory(model: nn.Module, x_or_shape, steps: int, graph, hidden_only: bool, *, fire_rate=1.0,
                       message_gain=None, nsteps=None, min_steps=0, fire=None, seed=None, sample_base=0,
                       offsets=None, recompute=False, checkpoint_every=None) -> dict:
    """The shared body of ``rollout_memory``: the schedule ``rollout()`` would build for these
    arguments, asked for its sizes.  Host-only; Python's and torch's RNG states are put back."""
    shape, device = _shape_and_device(model, x_or_shape, nsteps, fire)
    B, C, H, W = shape
    _check_norm(model)
    with _rng_restored():
        sched = S.build_schedule(steps=steps, B=B, H=H, W=W, device=device, fire_rate=fire_rate,
                                 message_gain=message_gain, nsteps=nsteps, min_steps=min_steps, fire=fire,
                                 seed=seed, sample_base=sample_base, offsets=offsets,
                                 sample_offsets=None if graph is None else graph.sample_offsets,
                                 recompute=recompute, checkpoint_every=checkpoint_every)
    desc, _ = _rollout_desc_host(model, shape, steps, graph, hidden_only, sched)
    return S.RolloutCall(desc, sched).memory()


def _tap_knobs(loss: str, alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb):
    """The masked tap loss's four numbers, checked (ValueError), or None for the premultiplied kind."""
    from .. import loss as LS
    if loss != "masked":
        return None
    return (LS._number(alpha_thr, "alpha_thr"), LS._number(lam_area, "lam_area"),
            LS._number(lam_bg_alpha, "lam_bg_alpha"), LS._number(lam_bg_rgb, "lam_bg_rgb"))


def _tap_target(target: torch.Tensor, device) -> torch.Tensor:
    """The prepared target as the kernels read it: float32, contiguous, on ``device``; one sample when it is
    broadcast over the batch."""
    tgt = target.detach().to(device, torch.float32)
    return tgt[:1].contiguous() if tgt.shape[0] == 1 or tgt.stride(0) == 0 else tgt.contiguous()


class _RolloutObjectiveFn(torch.autograd.Function):
    """A whole rollout AND the per-sample losses of its tapped states as ONE autograd node with two
    outputs: ``gnca_rollout_fwd_f32`` with a tape and ``gnca_rollout_tap_loss`` on that tape forward,
    ``gnca_rollout_bwd_taps`` backward.  Either output's cotangent may be absent (no zero tensor is
    made for it); the parameter gradients leave through the packs as in ``_RolloutFn``.  With
    ``checkpoint_every`` the forward is ``gnca_rollout_fwd_taps``: the losses are written as the states are
    produced, since the checkpointed tape keeps only every k-th of them."""

    @staticmethod
    def forward(ctx, x, call, taps, weights, keep, core, graph, tok_core, tok_graph, tensors=None):
        ctx.set_materialize_grads(False)
        if call.schedule.checkpoint_every is not None:
            # most tapped states never reach a checkpointed tape: the forward writes their losses
            out, tape, losses, alive = call.forward_taps(weights, taps, x, want_tape=True)
        else:
            out, tape = call.forward(weights, x, want_tape=True)
            losses, alive = call.tap_losses(taps, tape, out)
        ctx.call, ctx.taps, ctx.weights, ctx.keep, ctx.tape, ctx.alive = call, taps, weights, keep, tape, alive
        ctx.packs = (core, graph)
        ctx.save_for_backward(out)   # (the state of a tap at the last step: it is not on the tape)
        ctx.versions = tuple((t, t._version) for t in (tensors or {}).values())
        return out, losses

    @staticmethod
    def backward(ctx, g_final, g_losses):
        for t, v in ctx.versions:
            if t._version != v:
                raise RuntimeError(
                    "one of the variables needed for gradient computation has been modified by an "
                    f"inplace operation: a rollout weight of shape {tuple(t.shape)} is at version "
                    f"{t._version}; expected version {v} instead")
        if ctx.tape is None:
            raise RuntimeError("rollout_objective: backward through the same rollout a second time "
                               "(its tape was freed)")
        if g_final is None and g_losses is None:
            ctx.tape = None
            return (None,) * 10
        (x_final,) = ctx.saved_tensors
        desc = ctx.call.desc
        no_graph_use = (desc.flags & L.GRAPH) and desc.num_offsets == 0
        want, views, flats = {}, {}, [None, None]
        for i, pack in enumerate(ctx.packs):
            if pack is None or not ctx.needs_input_grad[7 + i] or (i == 1 and no_graph_use):
                continue
            flats[i] = torch.empty(sum(pack.sizes), dtype=torch.float32, device=x_final.device)
            views.update(pack.views(flats[i]))
            want.update(zip(pack.names, pack.params))
        gx, _ = ctx.call.backward_taps(ctx.weights, ctx.taps, ctx.tape, x_final,
                                       None if g_final is None else g_final.contiguous(),
                                       None if g_losses is None else g_losses.contiguous(), ctx.alive,
                                       want=want, out=views)
        ctx.tape = None
        return (gx if ctx.needs_input_grad[0] else None, None, None, None, None, None, None, flats[0], flats[1],
                None)


class RolloutObjective:
    """What ``rollout_objective()`` returns: ``x_final`` [B,C,H,W], exactly ``rollout()``'s result;
    ``losses`` float32 [R,B], the per-sample loss of the state after each tapped step; ``steps``, the R
    tapped step indices (from 1).  ``x_final`` and ``losses`` are the two outputs of one autograd node."""

    __slots__ = ("x_final", "losses", "steps")

    def __init__(self, x_final, losses, steps):
        self.x_final, self.losses, self.steps = x_final, losses, steps

    def __repr__(self):
        return f"RolloutObjective(steps={self.steps}, losses={tuple(self.losses.shape)})"


def run_rollout_objective(model: nn.Module, x: torch.Tensor, steps: int, target, graph, hidden_only: bool, *,
                          every=1, record=None, loss="premult", alpha_thr=0.2, lam_area=5e-5, lam_bg_alpha=0.0,
                          lam_bg_rgb=0.0, fire_rate=1.0, message_gain=None, nsteps=None, min_steps=0, fire=None,
                          seed=None, sample_base=0, offsets=None, recompute=False,
                          checkpoint_every=None) -> RolloutObjective:
    """The shared body of ``NeuralCA.rollout_objective`` / ``NeuralCAGraph.rollout_objective``."""
    from .. import loss as LS
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"state must be [B,C,H,W], got {tuple(getattr(x, 'shape', ()))}")
    B, C, H, W = x.shape
    _check_norm(model)
    # validation first (pure Python): nothing below runs, and no offsets are drawn, on a bad call
    if loss not in S.TAP_KINDS:
        raise ValueError(f"loss must be one of {sorted(S.TAP_KINDS)}, got {loss!r}")
    if C < 4:
        raise ValueError(f"the losses read channels 0..3 of the state, which has {C}")
    _, target = LS._prepare(x[:, :4], target)
    knobs = _tap_knobs(loss, alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb)
    _steps_int(steps, 1)
    rec = S.expand_record(steps, every, record)
    if not rec:
        raise ValueError("record is empty: a rollout objective needs at least one tapped step")
    S.checkpoint_interval(checkpoint_every, steps)
    x = S.check_state(x, model.n_channels)   # (channels, device, dtype: before the schedule draws its offsets)
    tensors = _step_tensors(model, graph)
    grad = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in tensors.values()))
    # (without grad the tape is only read by the loss kernel: states alone)
    sched = S.build_schedule(steps=steps, B=B, H=H, W=W, device=x.device, fire_rate=fire_rate,
                             message_gain=message_gain, nsteps=nsteps, min_steps=min_steps, fire=fire, seed=seed,
                             sample_base=sample_base, offsets=offsets,
                             sample_offsets=None if graph is None else graph.sample_offsets,
                             recompute=recompute if grad else True, checkpoint_every=checkpoint_every)
    desc, w, keep, tensors = _rollout_desc(model, x, steps, graph, hidden_only, sched)
    tgt = _tap_target(target, x.device)
    call, taps = S.RolloutCall(desc, sched), S.RolloutTaps(desc, rec, loss, knobs, tgt)
    if grad:
        core, gpack = param_packs(model, tensors)
        tc = core.token if core is not None else None
        tg = gpack.token if gpack is not None else None
        out, losses = _RolloutObjectiveFn.apply(x, call, taps, w, keep, core, gpack, tc, tg, tensors)
    elif checkpoint_every is not None:
        out, _, losses, _ = call.forward_taps(w, taps, x, want_tape=False)   # (no tape at all)
    else:
        out, tape = call.forward(w, x, want_tape=True)
        losses, _ = call.tap_losses(taps, tape, out)
        del tape
    return RolloutObjective(out, losses, list(rec))


class TraceResult:
    """What ``trace()`` returns: ``x_final`` [B,C,H,W], ``frames`` [R,B,channels,H,W] (the state after
    each recorded step), ``steps`` (the R recorded step indices, counted from 1 within this call) and
    ``attention`` [R,B,H,W] (the map of each recorded step) or None; ``metrics``, an ``ImageMetrics``
    of shape [R,B] (the state after each recorded step against ``target``) or None.  ``frames`` is
    None for a trace with ``frames=False``.  ``diagnostics``: a ``GraphDiagnostics`` whose fields lead
    with the R axis (each recorded step's input state with that step's offsets) or None.  With
    ``render``: ``rgb_u8`` uint8 [R,B,H*s,W*s,3|4], the frames as images (``render.render_rgb``), and
    ``attention_u8`` uint8 [R,B,H,W,3], the attention maps as colour images (``render.colorize``), or
    None.  ``vitals``: a ``StateVitals`` of shape [R,B] (``vitals.state_vitals`` of the whole state after
    each recorded step) or None.  All detached."""

    __slots__ = ("x_final", "frames", "steps", "attention", "metrics", "rgb_u8", "attention_u8", "vitals",
                 "diagnostics")

    def __init__(self, x_final, frames, steps, attention, metrics=None, diagnostics=None, *, rgb_u8=None,
                 attention_u8=None, vitals=None):
        self.x_final, self.frames, self.steps, self.attention = x_final, frames, steps, attention
        self.metrics = metrics
        self.diagnostics = diagnostics
        self.rgb_u8, self.attention_u8 = rgb_u8, attention_u8
        self.vitals = vitals

    def __repr__(self):
        shape = lambda t: None if t is None else tuple(t.shape)
        return (f"TraceResult(steps={self.steps}, frames={shape(self.frames)}, "
                f"attention={shape(self.attention)}, "
                f"metrics={None if self.metrics is None else shape(self.metrics.stacked)}"
                + ("" if self.rgb_u8 is None else f", rgb_u8={shape(self.rgb_u8)}")
                + ("" if self.attention_u8 is None else f", attention_u8={shape(self.attention_u8)}")
                + ("" if self.diagnostics is None else ", diagnostics")
                + ("" if self.vitals is None else f", vitals={shape(self.vitals.stacked)}") + ")")


def run_trace(model: nn.Module, x: torch.Tensor, steps: int, graph, hidden_only: bool, *, every=1, record=None,
              channels=4, return_attention=False, fire_rate=1.0, message_gain=None, seed=None, sample_base=0,
              first_step=0, offsets=None, target=None, frames=True, diagnostics=False,
              per_offset=False, render=None, vitals=False) -> TraceResult:
    """The shared body of ``NeuralCA.trace`` / ``NeuralCAGraph.trace``: a no-grad rollout that records
    frames (and attention maps, image metrics against ``target`` and graph diagnostics) in one native
    call; ``render`` adds one launch over all recorded frames and one over all attention maps."""
    if x.dim() != 4:
        raise ValueError(f"state must be [B,C,H,W], got {tuple(x.shape)}")
    B, C, H, W = x.shape
    _check_norm(model)
    if not isinstance(frames, bool):
        raise ValueError(f"frames must be a bool, got {frames!r}")
    if not isinstance(diagnostics, bool) or not isinstance(per_offset, bool):
        raise ValueError(f"diagnostics and per_offset must be bools, got {diagnostics!r}, {per_offset!r}")
    if diagnostics and graph is None:
        raise ValueError("diagnostics needs the graph term: this model has none")
    if per_offset and not diagnostics:
        raise ValueError("per_offset is part of the diagnostics: pass diagnostics=True")
    if target is not None:
        target = M.check_target(target, B, H, W)
    vitals_thr = None   # vitals: False, True (the model's alpha_thr) or the threshold itself
    if vitals is True:
        vitals_thr = V.check_alpha_thr(model.alpha_thr, "the model's alpha_thr")
    elif vitals is not False:
        vitals_thr = V.check_alpha_thr(vitals, "vitals (a bool, or the alpha threshold)")
    render = R.check_trace_render(render, model.alpha_thr, channels, frames)
    # validation first (pure Python): nothing below runs, and no offsets are drawn, on a bad call
    plan = S.build_trace(steps=steps, B=B, C=C, H=H, W=W, device=x.device, every=every, record=record,
                         channels=channels, return_attention=return_attention, fire_rate=fire_rate,
                         message_gain=message_gain, seed=seed, sample_base=sample_base, first_step=first_step,
                         offsets=offsets, sample_offsets=None if graph is None else graph.sample_offsets)
    with torch.no_grad():
        x = S.check_state(x.detach(), model.n_channels)
        sched = plan.schedule
        desc, w, keep, _ = _rollout_desc(model, x, steps, graph, hidden_only, sched)
        desc.rng_step = plan.first_step
        met = diag = vit = None
        if vitals_thr is not None:
            tgt, tbs = (None, 0) if target is None else M.device_target(target, x.device)
            out, frm, attn, met, diag, vit = S.trace_vitals(desc, w, x, steps, sched.offsets or [], plan.record,
                                                            plan.channels, vitals_thr, tgt, tbs,
                                                            want_attention=plan.attention, want_frames=frames,
                                                            diagnostics=diagnostics, per_offset=per_offset)
            met = None if met is None else M.ImageMetrics(met)
            vit = V.StateVitals(vit)
        elif diagnostics:
            tgt, tbs = (None, 0) if target is None else M.device_target(target, x.device)
            out, frm, attn, met, diag = S.trace_diag(desc, w, x, steps, sched.offsets or [], plan.record,
                                                     plan.channels, tgt, tbs, want_attention=plan.attention,
                                                     want_frames=frames, per_offset=per_offset)
            met = None if met is None else M.ImageMetrics(met)
        elif target is None and frames:
            out, frm, attn = S.trace(desc, w, x, steps, sched.offsets or [], plan.record, plan.channels,
                                     want_attention=plan.attention)
        else:
            tgt, tbs = (None, 0) if target is None else M.device_target(target, x.device)
            out, frm, attn, met = S.trace_metrics(desc, w, x, steps, sched.offsets or [], plan.record,
                                                  plan.channels, tgt, tbs, want_attention=plan.attention,
                                                  want_frames=frames)
            met = None if met is None else M.ImageMetrics(met)
        del keep
        rgb_u8 = attn_u8 = None
        if render is not None:
            rgb_u8 = R.render_rgb(frm, render["alpha_thr"], render["upscale"], render["mode"])
            if attn is not None:
                attn_u8 = R.colorize(attn, render["cmap"])
    return TraceResult(out, frm, list(plan.record), attn, met, diag, rgb_u8=rgb_u8, attention_u8=attn_u8,
                       vitals=vit)


# ---------------------------------------------------------------------------------------------
# Forward-mode tangent: where a nudge of the state is after the step / the rollout, no tape
# ---------------------------------------------------------------------------------------------
class TangentResult:
    """What ``rollout_tangent()`` returns: ``x_final`` [B,C,H,W], exactly the no-grad ``rollout()``'s
    result; ``v_final`` [B,C,H,W], the tangent after the last step (renormalised at every recorded step
    with ``renormalize=True``); ``steps``, the R recorded step indices (from 1); ``log_norm`` float64
    [R,B], the natural log of the 2-norm the tangent of each sample would have after each recorded step
    had it never been renormalised (``-inf`` for a zero tangent).  All detached."""

    __slots__ = ("x_final", "v_final", "steps", "log_norm")

    def __init__(self, x_final, v_final, steps, log_norm):
        self.x_final, self.v_final, self.steps, self.log_norm = x_final, v_final, steps, log_norm

    def __repr__(self):
        return f"TangentResult(steps={self.steps}, log_norm={tuple(self.log_norm.shape)})"


def _check_tangent_pair(model: nn.Module, x, v):
    """ValueError unless x and v are two [B,C,H,W] tensors of one shape, device and dtype (pure Python)."""
    for name, t in (("state", x), ("tangent", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be [B,C,H,W], got {tuple(getattr(t, 'shape', ()))}")
    if x.shape[1] != model.n_channels:
        raise ValueError(f"state has {x.shape[1]} channels, model expects {model.n_channels}")
    if x.shape[1] < 4:
        raise ValueError("the alive mask reads channel 3: n_channels must be >= 4")
    if v.shape != x.shape:
        raise ValueError(f"the tangent has shape {tuple(v.shape)}, the state {tuple(x.shape)}")
    if v.device != x.device:
        raise ValueError(f"the tangent is on {v.device}, the state on {x.device}")
    if v.dtype != x.dtype:
        raise ValueError(f"the tangent is {v.dtype}, the state {x.dtype}")


def _tangent_flags(model: nn.Module, graph, hidden_only: bool):
    """(flags, eps, k) of the model's steps, refusing what the tangent does not cover (ValueError)."""
    flags, eps = _check_norm(model)
    k = 0
    if graph is not None:
        flags |= graph.flags(False)
        if hidden_only:
            flags |= L.HIDDEN_ONLY
        k = min(graph.num_neighbors, len(graph.offsets))
    S.check_tangent_desc(flags, k)
    return flags, eps, k


# graph parameters whose direction is accepted and ignored: in torus mode (the only mode the tangent serves) the
# offset weights are the constant 1/k, so the query, key and scaling directions have exactly zero effect, as the
# backward's exactly-zero gradients there; gate_mlp is never used by the step
_IGNORED_DIRECTIONS = ("graph.query_proj.", "graph.key_proj.", "graph.scaling", "graph.gate_mlp.")


def param_direction(model: nn.Module, fill: float = 0.0) -> dict:
    """A correctly shaped ``dparams`` dict: one tensor per parameter a direction may perturb, filled with
    ``fill``, on the parameter's device."""
    return {n: torch.full_like(p.detach(), float(fill)) for n, p in model.named_parameters()
            if n in S.DIRECTION_FIELDS}


def _check_dparams(model: nn.Module, dparams) -> dict:
    """ValueError unless ``dparams`` is a dict of directions for the model's parameters (pure Python, nothing is
    drawn); returns {gnca_weights field: tensor} of the entries the kernels read."""
    if not isinstance(dparams, dict):
        raise ValueError(f"dparams must be a dict keyed by named_parameters() names, got {type(dparams).__name__}")
    params = dict(model.named_parameters())
    out = {}
    for name, t in dparams.items():
        if name == "perception.conv.weight":
            raise ValueError("perception.conv.weight is frozen: the tangent carries no direction for it")
        if name not in params:
            if isinstance(name, str) and name.startswith("norm."):
                raise ValueError(f"{name}: the model has no GroupNorm")
            raise ValueError(f"unknown parameter {name!r}")
        p = params[name]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(p.shape):
            raise ValueError(f"the direction of {name} has shape {tuple(getattr(t, 'shape', ()))}, the parameter "
                             f"{tuple(p.shape)}")
        if t.dtype != p.dtype:
            raise ValueError(f"the direction of {name} is {t.dtype}, the parameter {p.dtype}")
        if t.device != p.device:
            raise ValueError(f"the direction of {name} is on {t.device}, the parameter on {p.device}")
        if name in S.DIRECTION_FIELDS:
            out[S.DIRECTION_FIELDS[name]] = t
        elif not name.startswith(_IGNORED_DIRECTIONS):
            raise ValueError(f"unknown parameter {name!r}")
    return out


def _direction_weights(fields: dict):
    """(Weights struct, tensors to keep alive) of a checked direction; a missing tensor is a zero direction."""
    return S.make_weights({k: t.detach() for k, t in fields.items()})


def _check_dparams_block(model: nn.Module, dparams, allow_single: bool) -> list:
    """``_check_dparams`` of each of the K directions of a block; ``allow_single``: one dict stands for K = 1."""
    if allow_single and isinstance(dparams, dict):
        dparams = [dparams]
    if not isinstance(dparams, (list, tuple)) or not 1 <= len(dparams) <= L.TANGENT_MAX_DIRS:
        raise ValueError(f"dparams must be a {'dict or a ' if allow_single else ''}list of K dicts, "
                         f"1 <= K <= {L.TANGENT_MAX_DIRS}")
    return [_check_dparams(model, d) for d in dparams]


def _direction_block(dfields):
    """(K Weights structs, their tensors to keep alive) of a checked block of directions, or (None, None)."""
    if dfields is None:
        return None, None
    pairs = [_direction_weights(f) for f in dfields]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _draw_schedule(x, steps, graph, *, seed=None, offsets=None, **schedule_kw):
    """``S.build_schedule`` for the state ``x``, with the graph's offsets drawn only once every other schedule
    argument has passed (and before a seed is drawn): a rejected call leaves Python's and torch's generators
    alone."""
    B, _, H, W = x.shape
    kw = dict(steps=steps, B=B, H=H, W=W, device=x.device, **schedule_kw)
    if graph is not None and offsets is None:
        S.build_schedule(seed=0 if seed is None else seed, offsets=[[] for _ in range(steps)], **kw)
    return S.build_schedule(seed=seed, offsets=offsets,
                            sample_offsets=None if graph is None else graph.sample_offsets, **kw)


def run_tangent_step(model: nn.Module, x, v, fire_rate, graph, message_gain, hidden_only: bool, *, active=None,
                     offsets=None, fire=None, dparams=None):
    """The shared body of ``NeuralCA.tangent_step`` / ``NeuralCAGraph.tangent_step``."""
    if v is None and dparams is None:
        raise ValueError("v=None (a zero tangent) is allowed only together with dparams")
    _check_tangent_pair(model, x, x if v is None else v)
    dfields = None if dparams is None else _check_dparams(model, dparams)
    B, C, H, W = x.shape
    flags, eps, _ = _tangent_flags(model, graph, hidden_only)
    if isinstance(fire_rate, bool) or not isinstance(fire_rate, (int, float)):
        raise ValueError(f"fire_rate must be a number, got {fire_rate!r}")
    if offsets is not None:
        if graph is None:
            raise ValueError("offsets given for a model without the graph term")
        try:
            offsets = [tuple(o) for o in offsets]
        except TypeError:
            raise ValueError(f"offsets must be a sequence of (dy, dx) pairs, got {offsets!r}") from None
        for pair in offsets:
            if len(pair) != 2 or not all(isinstance(q, int) and -127 <= q <= 127 for q in pair):
                raise ValueError(f"offset {pair!r} is not a (dy, dx) pair in the int8 range")
        if len(offsets) > L.MAX_OFFSETS:
            raise ValueError(f"at most {L.MAX_OFFSETS} offsets per step (got {len(offsets)})")
    fire_mode = L.FIRE_NONE
    if fire is not None:
        if not isinstance(fire, torch.Tensor) or tuple(fire.shape) != (B, 1, H, W):
            raise ValueError(f"fire must be a tensor of shape ({B}, 1, {H}, {W})")
        if fire.device != x.device:
            raise ValueError(f"fire is on {fire.device}, the state on {x.device}")
        if fire.dtype == torch.float32:
            fire_mode = L.FIRE_RAND_F32
        elif fire.dtype in (torch.uint8, torch.bool):
            fire_mode = L.FIRE_MASK_U8
        else:
            raise ValueError(f"fire must be float32 uniforms or a uint8 / bool mask, got {fire.dtype}")
    if active is not None and (not isinstance(active, torch.Tensor) or active.device != x.device or
                               active.dtype not in (torch.bool, torch.uint8) or tuple(active.shape) != (B,)):
        raise ValueError("active must be a [B] bool/uint8 tensor on the state's device")
    with torch.no_grad():
        x = S.check_state(x.detach(), model.n_channels)
        v = torch.zeros_like(x) if v is None else S._dev_f32(v.detach(), "tangent")
        # the draws of forward(): one random.sample, then (rate below 1) one torch.rand on x.device
        chosen = None
        if graph is not None:
            chosen = graph.sample_offsets() if offsets is None else offsets
        if fire is None and fire_rate < 1.0:
            fire = torch.rand(B, 1, H, W, device=x.device)
            fire_mode = L.FIRE_RAND_F32
        elif fire is not None:
            fire = fire.contiguous()
            fire = fire.view(torch.uint8) if fire.dtype == torch.bool else fire
        tensors = _step_tensors(model, graph)
        alpha_thr = float(model.alpha_thr)
        key = (B, C, H, W, tensors["w1"].shape[0], 1 if graph is None else graph.d_model, flags,
               float(model.update_gain), alpha_thr, alpha_thr if graph is None else float(graph.alpha_thr),
               float(eps))
        desc = _step_desc(key, chosen, message_gain, fire_rate, fire_mode)
        w, keep = S.make_weights(tensors)
        if dfields is None:
            out = S.step_tangent(desc, w, x, v, fire=fire, active=active)
        else:
            dw, dkeep = _direction_weights(dfields)
            out = S.step_tangent(desc, w, x, v, fire=fire, active=active, dweights=dw)
            del dkeep
        del keep
    return out


def run_rollout_tangent(model: nn.Module, x, v, steps, graph, hidden_only: bool, *, every=None, record=None,
                        renormalize=False, fire_rate=1.0, message_gain=None, nsteps=None, min_steps=0, fire=None,
                        seed=None, sample_base=0, offsets=None, dparams=None) -> TangentResult:
    """The shared body of ``NeuralCA.rollout_tangent`` / ``NeuralCAGraph.rollout_tangent``."""
    if v is None and dparams is None:
        raise ValueError("v=None (a zero tangent) is allowed only together with dparams")
    _check_tangent_pair(model, x, x if v is None else v)
    dfields = None if dparams is None else _check_dparams(model, dparams)
    _tangent_flags(model, graph, hidden_only)
    _steps_int(steps, 0)
    if not isinstance(renormalize, bool):
        raise ValueError(f"renormalize must be a bool, got {renormalize!r}")
    if renormalize and dfields is not None:
        raise ValueError("renormalize=True with a parameter direction: rescaling v alone breaks linearity in the "
                         "pair (v, dparams)")
    # the taps follow trace()'s rules; neither every nor record: nothing is recorded
    rec = [] if every is None and record is None else S.expand_record(steps, 1 if every is None else every, record)
    with torch.no_grad():
        x = S.check_state(x.detach(), model.n_channels)   # (before the schedule draws its offsets)
        v = torch.zeros_like(x) if v is None else S._dev_f32(v.detach(), "tangent")
        sched = _draw_schedule(x, steps, graph, fire_rate=fire_rate, message_gain=message_gain, nsteps=nsteps,
                               min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base, offsets=offsets)
        desc, w, keep, _ = _rollout_desc(model, x, steps, graph, hidden_only, sched)
        dw, dkeep = (None, None) if dfields is None else _direction_weights(dfields)
        x_final, v_final, log_norm = S.rollout_tangent(S.RolloutCall(desc, sched), w, x, v, rec, renormalize,
                                                       dweights=dw)
        del keep, dkeep
    return TangentResult(x_final, v_final, list(rec), log_norm)


class TangentBlockResult:
    """What ``rollout_tangent_block()`` returns: ``x_final`` [B,C,H,W], exactly the no-grad ``rollout()``'s
    result; ``v_final`` [K,B,C,H,W], the block after the last step; ``steps``, the R recorded step indices
    (from 1); ``log_r`` float64 [R,B,K].  With ``orthonormalize=True`` ``log_r[r,b,j]`` is the running sum of
    ``log R_jj`` over the QR factorisations up to recorded step r (``-inf`` from the record at which
    direction j was dropped); without, it is direction j's own log norm.  All detached."""

    __slots__ = ("x_final", "v_final", "steps", "log_r")

    def __init__(self, x_final, v_final, steps, log_r):
        self.x_final, self.v_final, self.steps, self.log_r = x_final, v_final, steps, log_r

    def exponents(self):
        """``log_r[-1] / steps[-1]``, float64 [B,K]: the finite-time Lyapunov spectrum over the whole
        rollout, per step, largest first for a generic block.  A sample that ``nsteps`` stopped early ran
        fewer steps than ``steps[-1]``: dividing its row by its own step count is the caller's."""
        if not self.steps:
            raise ValueError("nothing was recorded: pass every= or record=")
        return self.log_r[-1] / self.steps[-1]

    def __repr__(self):
        return f"TangentBlockResult(steps={self.steps}, log_r={tuple(self.log_r.shape)})"


def run_rollout_tangent_block(model: nn.Module, x, V, steps, graph, hidden_only: bool, *, every=None, record=None,
                              orthonormalize=True, fire_rate=1.0, message_gain=None, nsteps=None, min_steps=0,
                              fire=None, seed=None, sample_base=0, offsets=None,
                              dparams=None) -> TangentBlockResult:
    """The shared body of ``NeuralCA.rollout_tangent_block`` / ``NeuralCAGraph.rollout_tangent_block``."""
    dfields = None
    if dparams is not None:
        dfields = _check_dparams_block(model, dparams, allow_single=False)
        if isinstance(V, torch.Tensor) and V.dim() == 5 and V.shape[0] != len(dparams):
            raise ValueError(f"{len(dparams)} parameter directions for a block of {V.shape[0]} tangents")
        if orthonormalize is True:
            raise ValueError("orthonormalize=True with parameter directions: mixing the tangents alone breaks "
                             "linearity in the pairs (V[j], dparams[j]); pass orthonormalize=False")
    zero_block = V is None and dfields is not None
    if V is None and dfields is None:
        raise ValueError("V=None (zero tangents) is allowed only together with dparams")
    if zero_block:
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"state must be [B,C,H,W], got {tuple(getattr(x, 'shape', ()))}")
        V = x.new_zeros((len(dfields),) + tuple(x.shape))
    if not isinstance(V, torch.Tensor) or V.dim() != 5:
        raise ValueError(f"the tangent block must be [K,B,C,H,W], got {tuple(getattr(V, 'shape', ()))}")
    if not 1 <= V.shape[0] <= L.TANGENT_MAX_DIRS:
        raise ValueError(f"the block holds {V.shape[0]} directions; 1 <= K <= {L.TANGENT_MAX_DIRS}")
    _check_tangent_pair(model, x, V[0])
    _tangent_flags(model, graph, hidden_only)
    _steps_int(steps, 0)
    if not isinstance(orthonormalize, bool):
        raise ValueError(f"orthonormalize must be a bool, got {orthonormalize!r}")
    rec = [] if every is None and record is None else S.expand_record(steps, 1 if every is None else every, record)
    with torch.no_grad():
        x = S.check_state(x.detach(), model.n_channels)   # (before the schedule draws its offsets)
        V = S._dev_f32(V.detach(), "tangent block")
        sched = _draw_schedule(x, steps, graph, fire_rate=fire_rate, message_gain=message_gain, nsteps=nsteps,
                               min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base, offsets=offsets)
        desc, w, keep, _ = _rollout_desc(model, x, steps, graph, hidden_only, sched)
        dws, dkeep = _direction_block(dfields)
        x_final, v_final, log_r = S.rollout_tangent_block(S.RolloutCall(desc, sched), w, x, V, rec, orthonormalize,
                                                          dweights=dws)
        del keep, dkeep
    return TangentBlockResult(x_final, v_final, list(rec), log_r)


# ---------------------------------------------------------------------------------------------
# A forward-mode objective: the tap losses and their directional derivatives along K tangents, no tape
# ---------------------------------------------------------------------------------------------
class ObjectiveTangent:
    """What ``rollout_objective_tangent()`` returns: ``x_final`` [B,C,H,W], exactly the no-grad ``rollout()``'s
    result; ``losses`` float32 [R,B], exactly ``rollout_objective()``'s; ``dlosses`` float64 [R,K,B], the
    derivative of ``losses[r,b]`` along direction k; ``steps``, the R tapped step indices (from 1); ``v_final``
    [K,B,C,H,W] with ``return_tangents=True``, else None.  All detached."""

    __slots__ = ("x_final", "losses", "dlosses", "steps", "v_final")

    def __init__(self, x_final, losses, dlosses, steps, v_final=None):
        self.x_final, self.losses, self.dlosses, self.steps, self.v_final = x_final, losses, dlosses, steps, v_final

    def __repr__(self):
        return f"ObjectiveTangent(steps={self.steps}, dlosses={tuple(self.dlosses.shape)})"


def run_rollout_objective_tangent(model: nn.Module, x, steps, target, graph, hidden_only: bool, *, V=None,
                                  dparams=None, every=1, record=None, loss="premult", alpha_thr=0.2, lam_area=5e-5,
                                  lam_bg_alpha=0.0, lam_bg_rgb=0.0, fire_rate=1.0, message_gain=None, nsteps=None,
                                  min_steps=0, fire=None, seed=None, sample_base=0, offsets=None,
                                  return_tangents=False) -> ObjectiveTangent:
    """The shared body of ``NeuralCA.rollout_objective_tangent`` / ``NeuralCAGraph.rollout_objective_tangent``."""
    from .. import loss as LS
    # validation first (pure Python): nothing below runs, and nothing is drawn, on a bad call
    if V is None and dparams is None:
        raise ValueError("at least one of V (state tangents) and dparams (weight directions) must be given")
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"state must be [B,C,H,W], got {tuple(getattr(x, 'shape', ()))}")
    dfields = None
    if dparams is not None:
        dfields = _check_dparams_block(model, dparams, allow_single=True)
    if V is not None:
        if not isinstance(V, torch.Tensor) or V.dim() != 5:
            raise ValueError(f"the tangent block must be [K,B,C,H,W], got {tuple(getattr(V, 'shape', ()))}")
        if not 1 <= V.shape[0] <= L.TANGENT_MAX_DIRS:
            raise ValueError(f"the block holds {V.shape[0]} directions; 1 <= K <= {L.TANGENT_MAX_DIRS}")
        if dfields is not None and V.shape[0] != len(dfields):
            raise ValueError(f"{len(dfields)} parameter directions for a block of {V.shape[0]} tangents")
    _check_tangent_pair(model, x, x if V is None else V[0])
    K = len(dfields) if V is None else V.shape[0]
    _tangent_flags(model, graph, hidden_only)
    if loss not in S.TAP_KINDS:
        raise ValueError(f"loss must be one of {sorted(S.TAP_KINDS)}, got {loss!r}")
    _, target = LS._prepare(x[:, :4], target)
    knobs = _tap_knobs(loss, alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb)
    _steps_int(steps, 1)
    rec = S.expand_record(steps, every, record)
    if not rec:
        raise ValueError("record is empty: a rollout objective needs at least one tapped step")
    if not isinstance(return_tangents, bool):
        raise ValueError(f"return_tangents must be a bool, got {return_tangents!r}")
    with torch.no_grad():
        x = S.check_state(x.detach(), model.n_channels)   # (before the schedule draws its offsets)
        if V is not None:
            V = S._dev_f32(V.detach(), "tangent block")
        sched = _draw_schedule(x, steps, graph, fire_rate=fire_rate, message_gain=message_gain, nsteps=nsteps,
                               min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base, offsets=offsets)
        desc, w, keep, _ = _rollout_desc(model, x, steps, graph, hidden_only, sched)
        tgt = _tap_target(target, x.device)
        dws, dkeep = _direction_block(dfields)
        x_final, losses, dlosses, v_final = S.rollout_objective_tangent(
            S.RolloutCall(desc, sched), S.RolloutTaps(desc, rec, loss, knobs, tgt), w, x, V, K, dweights=dws,
            want_tangents=return_tangents)
        del keep, dkeep
    return ObjectiveTangent(x_final, losses, dlosses, list(rec), v_final)


# ---------------------------------------------------------------------------------------------
# Gauss-Newton curvature-vector products of the tap objective: one tangent forward that leaves a tape and the
# taps' curvature fields, one BPTT that injects them
# ---------------------------------------------------------------------------------------------
class GaussNewtonProduct:
    """What ``rollout_gauss_newton()`` returns: ``x_final`` [B,C,H,W], exactly the no-grad ``rollout()``'s result;
    ``losses`` float32 [R,B], exactly ``rollout_objective()``'s; ``dlosses`` float64 [R,B], exactly
    ``rollout_objective_tangent()``'s for this one direction; ``quad`` float64 [R,B], the loss curvature's
    quadratic form in the tangent of each tapped state; ``steps``, the R tapped step indices (from 1);
    ``product``, a dict keyed like ``param_direction()`` with ``G_tt dparams + G_tx v`` in the shape of each
    parameter; ``gx`` [B,C,H,W], ``G_xt dparams + G_xx v``; ``energy``, the device float64 scalar
    ``sum_r scale_r sum_b quad[r,b]``, which equals ``<dparams, product> + <v, gx>`` in exact arithmetic;
    ``fields`` float32 [R,B,4,H,W] with ``return_fields=True`` (each tap's curvature field, before its scale),
    else None.  All detached."""

    __slots__ = ("x_final", "losses", "dlosses", "quad", "steps", "product", "gx", "energy", "fields")

    def __init__(self, x_final, losses, dlosses, quad, steps, product, gx, energy, fields=None):
        self.x_final, self.losses, self.dlosses, self.quad, self.steps = x_final, losses, dlosses, quad, steps
        self.product, self.gx, self.energy, self.fields = product, gx, energy, fields

    def product_flat(self) -> torch.Tensor:
        """``product`` as one float32 vector [P] in ``forward_grad.ParamDirections`` order."""
        return torch.cat([self.product[n].reshape(-1) for n in S.DIRECTION_FIELDS if n in self.product])

    def __repr__(self):
        return f"GaussNewtonProduct(steps={self.steps}, tensors={len(self.product)})"


def _gauss_newton_front(model: nn.Module, x, steps, target, graph, hidden_only: bool, dparams, v, every, record, loss,
                        alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb, tap_weights, checkpoint_every):
    """The pure-Python validation of ``rollout_gauss_newton``: (dfields, target, knobs, rec, scale)."""
    from .. import loss as LS
    if v is None and dparams is None:
        raise ValueError("at least one of v (a state tangent) and dparams (a weight direction) must be given")
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"state must be [B,C,H,W], got {tuple(getattr(x, 'shape', ()))}")
    dfields = None
    if dparams is not None:
        if not isinstance(dparams, dict):
            raise ValueError("dparams must be ONE dict of weight directions: a Gauss-Newton product takes one "
                             "direction per call")
        dfields = _check_dparams(model, dparams)
    _check_tangent_pair(model, x, x if v is None else v)
    B = x.shape[0]
    _tangent_flags(model, graph, hidden_only)
    if loss not in S.TAP_KINDS:
        raise ValueError(f"loss must be one of {sorted(S.TAP_KINDS)}, got {loss!r}")
    _, target = LS._prepare(x[:, :4], target)
    knobs = _tap_knobs(loss, alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb)
    _steps_int(steps, 1)
    rec = S.expand_record(steps, every, record)
    if not rec:
        raise ValueError("record is empty: a Gauss-Newton product needs at least one tapped step")
    S.checkpoint_interval(checkpoint_every, steps)
    if tap_weights is None:
        weights = [1.0] * len(rec)
    else:
        if isinstance(tap_weights, (torch.Tensor, str)) or not hasattr(tap_weights, "__len__"):
            raise ValueError("tap_weights must be a sequence of R host numbers (they travel as kernel arguments)")
        weights = [LS._number(t, "tap weight") for t in tap_weights]
        if len(weights) != len(rec):
            raise ValueError(f"{len(weights)} tap weights for {len(rec)} taps")
    # scale_r as the float32 the injection kernel takes
    scale = [ctypes.c_float(t / B).value for t in weights]
    return dfields, target, knobs, rec, scale


def run_rollout_gauss_newton(model: nn.Module, x, steps, target, graph, hidden_only: bool, *, dparams=None, v=None,
                             every=1, record=None, loss="premult", alpha_thr=0.2, lam_area=5e-5, lam_bg_alpha=0.0,
                             lam_bg_rgb=0.0, tap_weights=None, checkpoint_every=None, fire_rate=1.0,
                             message_gain=None, nsteps=None, min_steps=0, fire=None, seed=None, sample_base=0,
                             offsets=None, return_fields=False) -> GaussNewtonProduct:
    """The shared body of ``NeuralCA.rollout_gauss_newton`` / ``NeuralCAGraph.rollout_gauss_newton``."""
    if not isinstance(return_fields, bool):
        raise ValueError(f"return_fields must be a bool, got {return_fields!r}")
    # validation first (pure Python): nothing below runs, and nothing is drawn, on a bad call
    dfields, target, knobs, rec, scale = _gauss_newton_front(
        model, x, steps, target, graph, hidden_only, dparams, v, every, record, loss, alpha_thr, lam_area,
        lam_bg_alpha, lam_bg_rgb, tap_weights, checkpoint_every)
    with torch.no_grad():
        x = S.check_state(x.detach(), model.n_channels)   # (before the schedule draws its offsets)
        if v is not None:
            v = S._dev_f32(v.detach(), "tangent")
        sched = _draw_schedule(x, steps, graph, fire_rate=fire_rate, message_gain=message_gain, nsteps=nsteps,
                               min_steps=min_steps, fire=fire, seed=seed, sample_base=sample_base, offsets=offsets,
                               recompute=True, checkpoint_every=checkpoint_every)
        desc, w, keep, _ = _rollout_desc(model, x, steps, graph, hidden_only, sched)
        tgt = _tap_target(target, x.device)
        dw, dkeep = (None, None) if dfields is None else _direction_weights(dfields)
        call, taps = S.RolloutCall(desc, sched), S.RolloutTaps(desc, rec, loss, knobs, tgt)
        x_final, tape, fields, losses, dlosses, quad = S.rollout_gn_forward(call, taps, w, x, v, dweights=dw)
        want = {n: p for n, p in model.named_parameters() if n in S.DIRECTION_FIELDS}
        gx, product = S.rollout_gn_backward(call, taps, w, tape, fields, scale, x, want=want)
        del tape, keep, dkeep
        per_tap = quad.sum(dim=1)
        if len(set(scale)) == 1:
            energy = per_tap.sum() * scale[0]
        else:
            energy = sum(per_tap[r] * s for r, s in enumerate(scale))
    return GaussNewtonProduct(x_final, losses, dlosses, quad, list(rec), product, gx, energy,
                              fields if return_fields else None)


def run_gauss_newton_memory(model: nn.Module, x_or_shape, steps: int, graph, hidden_only: bool, *, every=1,
                            record=None, checkpoint_every=None, fire_rate=1.0, message_gain=None, nsteps=None,
                            min_steps=0, fire=None, seed=None, sample_base=0, offsets=None) -> dict:
    """The shared body of ``gauss_newton_memory``: bytes of the tape, the two workspaces and the fields of the
    product ``rollout_gauss_newton()`` would run for these arguments.  Host-only; Python's and torch's RNG states
    are put back."""
    shape, device = _shape_and_device(model, x_or_shape, nsteps, fire)
    B, C, H, W = shape
    _tangent_flags(model, graph, hidden_only)
    _steps_int(steps, 1)
    rec = S.expand_record(steps, every, record)
    if not rec:
        raise ValueError("record is empty: a Gauss-Newton product needs at least one tapped step")
    with _rng_restored():
        sched = S.build_schedule(steps=steps, B=B, H=H, W=W, device=device, fire_rate=fire_rate,
                                 message_gain=message_gain, nsteps=nsteps, min_steps=min_steps, fire=fire,
                                 seed=seed, sample_base=sample_base, offsets=offsets,
                                 sample_offsets=None if graph is None else graph.sample_offsets,
                                 recompute=True, checkpoint_every=checkpoint_every)
    desc, _ = _rollout_desc_host(model, shape, steps, graph, hidden_only, sched)
    # (the sizes do not depend on the loss kind or on the target: a one-float placeholder stands for it)
    taps = S.RolloutTaps(desc, rec, "premult", None, torch.zeros(1, 4, 1, 1))
    return S.gn_memory(S.RolloutCall(desc, sched), taps)
