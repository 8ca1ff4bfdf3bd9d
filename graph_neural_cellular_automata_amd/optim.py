"""The trainers' gradient policy and ``optimizer.step()`` as one HIP launch (``gnca_optim_step``).

The graph trainer normalises every gradient by its own 2-norm and steps Adam
(``src/training/train_graph_augmented_nca.py:367-375``); the classic trainer clips the global norm
at 0.5 first (``src/training/train_intermediate_loss.py:280-283``).  With 12 trainable tensors and
~11k parameters that is a few dozen launches that move 43 KB.  ``FusedAdam`` is
``torch.optim.Adam`` with ``step()`` replaced: the policy and torch's non-amsgrad Adam update with L2
weight decay run in one launch over a table of tensors that travels as the kernel argument (nothing
is copied to the device per step).  ``param_groups``, ``state_dict``, ``load_state_dict``,
``zero_grad`` and the LR schedulers are inherited and the state layout is torch's (a 0-dim float32
CPU ``step`` per parameter, ``exp_avg`` and ``exp_avg_sq`` shaped like it), so a reference
checkpoint's ``optimizer_state`` loads into it and its own loads into ``torch.optim.Adam``::

    opt = FusedAdam(model.parameters(), lr=2e-4, weight_decay=1e-5, grad_policy="normalize")
    ...
    dp.train_step(model, opt, loss, policy="none")     # backward -> all-reduce -> opt.step()

``p.grad`` is READ, never written, on the device path: the reference normalises (clips) it in
place, but nothing reads it between that and the next ``zero_grad``.  A parameter whose ``.grad`` is
``None`` is skipped entirely: no state is created and its step count does not advance.

Parameters that are not on a ROCm device, or not contiguous float32 (they, their gradients or their
state), take the torch path instead, ``dp.POLICIES[...]`` (which does write ``p.grad``) and then
``torch.optim.Adam.step``; so do parameters spread over several devices.  That keeps the class usable
on the CPU.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from . import dp
from .step import stream_ptr

_POLICY = {None: L.OPTIM_POLICY_NONE, "none": L.OPTIM_POLICY_NONE, "normalize": L.OPTIM_POLICY_NORMALIZE,
           "clip": L.OPTIM_POLICY_CLIP}
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _native_ok(t: torch.Tensor, dev) -> bool:
    return t.device == dev and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous() \
        and t.numel() > 0


class FusedAdam(torch.optim.Adam):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` whose ``step()`` first applies
    ``grad_policy`` and is one launch for up to 24 tensors (two once they hold more than 65536
    elements together; more tensors take more launches of the same kernels).

    ``grad_policy="normalize"``: per tensor ``g / (||g|| + norm_eps)`` (``norm_eps`` defaults to the
    graph trainer's 1e-8).  ``"clip"``: ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` over every
    tensor that has a gradient, across all param groups.  ``None``: plain Adam.  The weight decay is
    added after the policy, as in the trainers.  ``p.grad`` is read, never written (module docstring).
    ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, a tensor ``lr`` and
    ``decoupled_weight_decay`` raise ``ValueError``.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 grad_policy=None, max_norm=0.5, norm_eps=None, foreach=None, maximize=False, capturable=False,
                 differentiable=False, decoupled_weight_decay=False):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable,
                     decoupled_weight_decay=decoupled_weight_decay)
        for name in _UNSUPPORTED:
            if given[name]:
                raise ValueError(f"FusedAdam does not support {name}")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam does not support a tensor lr")
        if grad_policy not in _POLICY:
            raise ValueError(f"grad_policy must be None, 'normalize' or 'clip', got {grad_policy!r}")
        self.grad_policy = None if grad_policy == "none" else grad_policy
        self.max_norm = float(max_norm)
        self.norm_eps = 1e-8 if norm_eps is None else float(norm_eps)
        if not self.max_norm >= 0.0 or not self.norm_eps >= 0.0:
            raise ValueError("max_norm and norm_eps must be non-negative")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=foreach)
        self._desc = L.OptimDesc()

    def _check_groups(self):
        # (load_state_dict replaces the groups' options: checked at every step, not only here)
        for group in self.param_groups:
            for name in _UNSUPPORTED:
                if group.get(name, False):
                    raise ValueError(f"FusedAdam does not support {name}")
            if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
                raise ValueError("FusedAdam does not support a tensor lr or tensor betas")

    def _torch_step(self, params):
        if self.grad_policy == "normalize":
            dp.normalize_gradients_(params, eps=self.norm_eps)
        elif self.grad_policy == "clip":
            dp.clip_gradients_(params, max_norm=self.max_norm)
        torch.optim.Adam.step(self)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        work = [(p, group) for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not work:
            return loss
        dev = work[0][0].device
        native = dev.type == "cuda" and all(_native_ok(p, dev) and _native_ok(p.grad, dev) for p, _ in work)
        for p, _ in work:
            st = self.state[p]
            if len(st) == 0 and native:
                # torch's layout (torch/optim/adam.py), created directly
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif native:
                native = _native_ok(st["exp_avg"], dev) and _native_ok(st["exp_avg_sq"], dev) and \
                    isinstance(st["step"], torch.Tensor) and st["step"].device.type == "cpu"
            if not native:
                break
        if not native:
            # (states created above are zeros at step 0, which is what torch would create)
            self._torch_step([p for p, _ in work])
            return loss
        self._native_step(work, dev)
        return loss

    def _fill(self, d, chunk, base, advance):
        """The table of ``chunk``; ``advance``: count the step (once per ``step()`` and parameter)."""
        d.num_tensors, d.sumsq_base = len(chunk), base
        for i, (p, group) in enumerate(chunk):
            st = self.state[p]
            if advance:
                st["step"] += 1
            t = float(st["step"])
            beta1, beta2 = group["betas"]
            e = d.t[i]
            e.p, e.g, e.m, e.v = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            e.numel = p.numel()
            e.lr, e.weight_decay = float(group["lr"]), float(group["weight_decay"])
            e.bias1, e.bias2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t

    def _native_step(self, work, dev):
        fn = getattr(L.load(), "gnca_optim_step", None)
        if fn is None:
            raise L.GncaError(f"libgnca.so at {L.LIB_PATH} has no gnca_optim_step; rebuild it")
        stream = stream_ptr(dev)
        policy = _POLICY[self.grad_policy]
        # the kernels take one (beta1, beta2, eps) per call: tensors are batched per such triple
        batches = {}
        for p, group in work:
            key = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            batches.setdefault(key, []).append((p, group))
        n = len(work)
        total = sum(p.numel() for p, _ in work)
        chunks = [(key, items[i:i + L.OPTIM_MAX_TENSORS]) for key, items in batches.items()
                  for i in range(0, len(items), L.OPTIM_MAX_TENSORS)]
        # one launch while one call sees every tensor its sums need and they are small; else the sums of
        # squares go through an fp64 workspace (clip: shared by all calls, so the total covers all tensors)
        split = policy != L.OPTIM_POLICY_NONE and (
            total > L.OPTIM_ONE_LAUNCH_MAX or (policy == L.OPTIM_POLICY_CLIP and len(chunks) > 1))
        ws = torch.empty(n, dtype=torch.float64, device=dev) if split else None
        d = self._desc
        d.policy, d.max_norm, d.norm_eps = policy, self.max_norm, self.norm_eps
        d.sumsq, d.sumsq_count = (ws.data_ptr(), n) if split else (None, 0)
        two_pass = split and policy == L.OPTIM_POLICY_CLIP and len(chunks) > 1
        passes = (L.OPTIM_SUMSQ, L.OPTIM_UPDATE) if two_pass else (0,)
        for flags in passes:
            base = 0
            for (beta1, beta2, eps), chunk in chunks:
                d.beta1, d.beta2, d.eps, d.flags = beta1, beta2, eps, flags
                self._fill(d, chunk, base, advance=flags != L.OPTIM_UPDATE)
                L.check(fn(ctypes.byref(d), stream), "gnca_optim_step")
                base += len(chunk)
