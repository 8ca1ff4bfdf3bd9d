"""Damage curriculum on the device: the reference's ``utils.damage``
(``src/utils/damage.py:15-138``) with the same function names, arguments and effects, each one
HIP launch over the whole batch (``gnca_damage_f32``).

RNG: ``alpha_dropout_``, ``salt_pepper_alpha_`` and ``hidden_scramble_`` draw exactly what the
reference draws (``torch.rand_like`` / ``torch.randn`` of the same shapes), and ``stripe_wipe_``
/ ``apply_damage_policy_`` consume Python ``random`` as the reference does.  The per-sample
positions of the square / circle / gaussian kinds are drawn for the whole batch in one
``torch.randint`` call on the device instead of one host-synchronising call per sample, so their
values differ from the reference's for the same seed (their ranges are the same).

``DamagePolicy`` / ``regrow_trace`` (below the reference's functions) are the policy with ALL its draws
on the device (``gnca_damage_policy``): one launch, no host wait, a kind per sample, a counter RNG
keyed by the global sample index instead of torch's and Python's generators.
"""
from __future__ import annotations

import ctypes
import random

import torch

from . import _lib as L
from .step import stream_ptr


def _launch(state, kind, size=0, pos=None, noise=None, p=0.0, alpha_thr=0.1, softness=0.35, sigma=0.0):
    if state.device.type != "cuda" or state.dtype != torch.float32 or not state.is_contiguous():
        raise RuntimeError("damage ops run in place on a contiguous float32 ROCm state (no CPU path)")
    B, C, H, W = state.shape
    d = L.DamageDesc(B=B, C=C, H=H, W=W, kind=kind, size=int(size), p=float(p),
                     alpha_thr=float(alpha_thr), softness=float(softness), sigma=float(sigma))
    pos_t = None if pos is None else pos.to(device=state.device, dtype=torch.int32).contiguous()
    noise_t = None if noise is None else noise.to(device=state.device, dtype=torch.float32).contiguous()
    rc = L.load().gnca_damage_f32(ctypes.byref(d), state.data_ptr(),
                                  None if pos_t is None else pos_t.data_ptr(),
                                  None if noise_t is None else noise_t.data_ptr(), stream_ptr(state.device))
    L.check(rc, "gnca_damage_f32")


def _centres(B, H, W, r, device):
    cy = torch.randint(r, max(r + 1, H - r), (B,), device=device)
    cx = torch.randint(r, max(r + 1, W - r), (B,), device=device)
    return torch.stack([cy, cx], 1)


@torch.no_grad()
def cutout_square_(state, size: int):
    """Zero all channels in a random size x size square per sample (damage.py:15-23)."""
    B, C, H, W = state.shape
    if size <= 0:
        return
    y = torch.randint(0, max(1, H - size + 1), (B,), device=state.device)
    x = torch.randint(0, max(1, W - size + 1), (B,), device=state.device)
    _launch(state, L.DMG_SQUARE, size, pos=torch.stack([y, x], 1))


@torch.no_grad()
def cutout_circle_(state, radius: int):
    """Zero all channels inside a random circle of radius R per sample (damage.py:25-36)."""
    B, C, H, W = state.shape
    if radius <= 0:
        return
    _launch(state, L.DMG_CIRCLE, radius, pos=_centres(B, H, W, radius, state.device))


@torch.no_grad()
def stripe_wipe_(state, width: int, orientation: str = "auto"):
    """Zero one random horizontal or vertical band, shared by the batch (damage.py:38-50)."""
    B, C, H, W = state.shape
    if width <= 0:
        return
    if orientation == "auto":
        orientation = "h" if random.random() < 0.5 else "v"
    if orientation == "h":
        y0 = torch.randint(0, max(1, H - width + 1), (1,), device=state.device)
        pos = torch.stack([y0.expand(B), torch.zeros_like(y0).expand(B)], 1)
        _launch(state, L.DMG_STRIPE_H, width, pos=pos)
    else:
        x0 = torch.randint(0, max(1, W - width + 1), (1,), device=state.device)
        pos = torch.stack([torch.zeros_like(x0).expand(B), x0.expand(B)], 1)
        _launch(state, L.DMG_STRIPE_V, width, pos=pos)


@torch.no_grad()
def alpha_dropout_(state, p: float, alpha_thr: float = 0.1, hard: bool = True):
    """Kill a fraction p of the alive alpha pixels (damage.py:52-65)."""
    if p <= 0:
        return
    u = torch.rand_like(state[:, 3:4])
    _launch(state, L.DMG_ALPHA_DROP if hard else L.DMG_ALPHA_DROP_SOFT, noise=u, p=p, alpha_thr=alpha_thr)


@torch.no_grad()
def salt_pepper_alpha_(state, p: float):
    """Zero alpha at random pixels (damage.py:67-72)."""
    if p <= 0:
        return
    _launch(state, L.DMG_SALT_PEPPER, noise=torch.rand_like(state[:, 3:4]), p=p)


@torch.no_grad()
def hidden_scramble_(state, sigma: float = 0.2):
    """Noise on the hidden channels, clamped to [0, 1] (damage.py:74-80)."""
    B, C, H, W = state.shape
    if C <= 4 or sigma <= 0:
        return
    _launch(state, L.DMG_HIDDEN_NOISE, noise=torch.randn(B, C - 4, H, W, device=state.device), sigma=sigma)


@torch.no_grad()
def gaussian_hole_(state, radius: int, softness: float = 0.35):
    """Multiply all channels by 1 - a soft disk per sample (damage.py:82-97)."""
    B, C, H, W = state.shape
    if radius <= 0:
        return
    _launch(state, L.DMG_GAUSSIAN, radius, pos=_centres(B, H, W, radius, state.device), softness=softness)


def _cfg(cfg: dict, key: str, legacy: str | None, default):
    """``cfg[key]``, else the older key name the reference also accepts, else ``default``."""
    if key in cfg:
        return cfg[key]
    if legacy is not None and legacy in cfg:
        return cfg[legacy]
    return default


# kind -> launcher(state, size, knobs).  ``size`` is the policy's sampled patch size; ``knobs``
# the parsed config (damage.py:118-136 maps each kind to one of the primitives above).
_KINDS = {
    "square": lambda st, n, k: cutout_square_(st, n),
    "circle": lambda st, n, k: cutout_circle_(st, n // 2 if n > 1 else 1),
    "stripes": lambda st, n, k: stripe_wipe_(st, k["stripe_width"], orientation="auto"),
    "alpha_drop": lambda st, n, k: alpha_dropout_(st, k["alpha_dropout_p"], alpha_thr=k["alpha_thr"], hard=True),
    "saltpepper": lambda st, n, k: salt_pepper_alpha_(st, k["salt_pepper_p"]),
    "gaussian": lambda st, n, k: gaussian_hole_(st, radius=max(1, n // 2), softness=k["gaussian_softness"]),
    "hidden_noise": lambda st, n, k: hidden_scramble_(st, sigma=k["hidden_noise_sigma"]),
}


@torch.no_grad()
def apply_damage_policy_(state, dmg_cfg: dict, epoch: int):
    """The reference's policy (damage.py:99-138): from ``start_epoch`` on, with probability
    ``prob`` (one device ``torch.rand(1)``), ONE kind for the whole batch drawn by
    ``random.choices`` over ``kinds``, a patch size by ``random.randint(size_min, size_max)``, then
    that kind's primitive; an unknown kind falls back to the square cut-out.  Same draws, in the
    same order, as the reference."""
    if epoch < int(_cfg(dmg_cfg, "start_epoch", "damage_start_epoch", 100)):
        return
    prob = float(_cfg(dmg_cfg, "prob", "damage_prob", 0.0))
    if prob <= 0 or torch.rand(1, device=state.device).item() > prob:
        return
    table = dmg_cfg.get("kinds", {"square": 1.0})
    kind = random.choices(list(table.keys()), weights=list(table.values()), k=1)[0]
    lo = int(_cfg(dmg_cfg, "size_min", "damage_patch_size", 8))
    size = int(random.randint(lo, int(_cfg(dmg_cfg, "size_max", None, max(lo, 14)))))
    knobs = {"alpha_thr": float(dmg_cfg.get("alpha_thr", 0.1)),
             "alpha_dropout_p": float(dmg_cfg.get("alpha_dropout_p", 0.1)),
             "stripe_width": int(dmg_cfg.get("stripe_width", size)),
             "salt_pepper_p": float(dmg_cfg.get("salt_pepper_p", 0.02)),
             "hidden_noise_sigma": float(dmg_cfg.get("hidden_noise_sigma", 0.0)),
             "gaussian_softness": float(dmg_cfg.get("gaussian_softness", 0.35))}
    _KINDS.get(kind, _KINDS["square"])(state, size, knobs)


# ---------------------------------------------------------------------------------------------
# The policy with its draws on the device (gnca_damage_policy): no host draw, no noise tensor, no
# host wait, a kind per sample.  Its RNG is the project's own counter RNG (include/gnca.h), keyed by
# (seed, event, global sample), so a sharded batch draws what the whole batch draws.
# ---------------------------------------------------------------------------------------------
KIND_CODES = {"square": L.DMG_SQUARE, "circle": L.DMG_CIRCLE, "stripe_h": L.DMG_STRIPE_H,
              "stripe_v": L.DMG_STRIPE_V, "alpha_drop": L.DMG_ALPHA_DROP, "alpha_drop_soft": L.DMG_ALPHA_DROP_SOFT,
              "saltpepper": L.DMG_SALT_PEPPER, "gaussian": L.DMG_GAUSSIAN, "hidden_noise": L.DMG_HIDDEN_NOISE,
              "stripes": L.DMG_STRIPES_AUTO}
SCOPES = {"batch": L.DMG_SCOPE_BATCH, "sample": L.DMG_SCOPE_SAMPLE}


def _entry(name: str):
    fn = getattr(L.load(), name, None)
    if fn is None:
        raise L.GncaError(f"libgnca.so at {L.LIB_PATH} has no {name}; rebuild it")
    return fn


class DamagePolicy:
    """The reference's damage config block (``apply_damage_policy_`` above reads the same keys, the
    legacy ``damage_start_epoch`` / ``damage_prob`` / ``damage_patch_size`` among them), parsed once on
    the host; ``apply_`` is then ONE launch that draws and damages on the device.

    ``scope="batch"`` keeps the reference's structure: one gate, kind, size, stripe orientation and
    stripe origin for the batch, positions per sample, noise per cell.  ``scope="sample"`` draws
    everything per sample: the batch gate on ``prob``, then a gate per sample on ``per_sample_prob``
    (the config key the reference's regeneration script sets and its ``utils.damage`` ignores;
    default 1.0).  What differs from ``apply_damage_policy_``: the RNG (neither torch's nor Python's is
    consumed), and in the table of kinds: a name that is no kind counts as ``square`` (the reference's
    fallback), entries of one kind are merged, zero-weight kinds are dropped, and a ``stripe_width``
    that is absent or <= 0 means the drawn size."""

    def __init__(self, cfg: dict, seed: int, scope: str = "batch"):
        if scope not in SCOPES:
            raise ValueError(f"scope must be one of {sorted(SCOPES)}, got {scope!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
        self.scope, self.seed = scope, seed
        self.start_epoch = int(_cfg(cfg, "start_epoch", "damage_start_epoch", 100))
        self.prob = float(_cfg(cfg, "prob", "damage_prob", 0.0))
        self.per_sample_prob = float(cfg.get("per_sample_prob", 1.0))
        self.size_min = int(_cfg(cfg, "size_min", "damage_patch_size", 8))
        self.size_max = int(_cfg(cfg, "size_max", None, max(self.size_min, 14)))
        if self.size_max < self.size_min:
            raise ValueError(f"size_max {self.size_max} < size_min {self.size_min}")
        self.stripe_width = max(0, int(cfg.get("stripe_width", 0)))
        self.alpha_thr = float(cfg.get("alpha_thr", 0.1))
        self.alpha_dropout_p = float(cfg.get("alpha_dropout_p", 0.1))
        self.salt_pepper_p = float(cfg.get("salt_pepper_p", 0.02))
        self.hidden_sigma = float(cfg.get("hidden_noise_sigma", 0.0))
        self.gaussian_softness = float(cfg.get("gaussian_softness", 0.35))
        weights: dict = {}
        for name, w in cfg.get("kinds", {"square": 1.0}).items():
            w = float(w)
            if not 0.0 <= w < float("inf"):
                raise ValueError(f"the weight of kind {name!r} must be a finite number >= 0, got {w!r}")
            code = KIND_CODES.get(name, L.DMG_SQUARE)
            weights[code] = weights.get(code, 0.0) + w
        weights = {c: w for c, w in weights.items() if w > 0.0}
        if not weights:
            raise ValueError("the kinds table holds no kind with a positive weight")
        self.kinds = list(weights)
        total, run, cum = sum(weights.values()), 0.0, []
        for w in weights.values():
            run += w
            cum.append(run / total)
        cum[-1] = 1.0
        self.cum = [ctypes.c_float(c).value for c in cum]     # fp32 of the fp64 running sums

    @staticmethod
    def codes(names, device=None) -> torch.Tensor:
        """int32 [B] tensor of kind codes for ``apply_(kinds=...)``: a name per sample, ``None`` (code
        -1) for a sample to leave untouched; a name that is no kind counts as ``square``."""
        vals = [-1 if n is None else KIND_CODES.get(n, L.DMG_SQUARE) for n in names]
        return torch.tensor(vals, dtype=torch.int32, device=device)

    def desc(self, B: int, C: int, H: int, W: int, event: int = 0, sample_base: int = 0) -> L.DamagePolicyDesc:
        d = L.DamagePolicyDesc(B=B, C=C, H=H, W=W, scope=SCOPES[self.scope], prob=self.prob,
                               per_sample_prob=self.per_sample_prob, n_kinds=len(self.kinds),
                               size_min=self.size_min, size_max=self.size_max, stripe_width=self.stripe_width,
                               alpha_thr=self.alpha_thr, alpha_dropout_p=self.alpha_dropout_p,
                               salt_pepper_p=self.salt_pepper_p, hidden_sigma=self.hidden_sigma,
                               gaussian_softness=self.gaussian_softness, seed=self.seed, event=int(event),
                               sample_base=int(sample_base))
        for k, (code, c) in enumerate(zip(self.kinds, self.cum)):
            d.kinds[k], d.cum[k] = code, c
        return d

    @torch.no_grad()
    def apply_(self, state, epoch: int, event, *, sample_base: int = 0, kinds=None, return_draws: bool = False,
               return_noise: bool = False):
        """Damage ``state`` [B,C,H,W] in place: one launch on the current stream, no host wait.

        ``event`` numbers the call (a training iteration, say): an int, or a 1-element int64 device
        tensor that the kernel reads, so that a captured loop draws afresh on every replay.  The same
        ``(seed, event, sample_base)`` gives the same damage.  ``kinds``: an int32 [B] device tensor of
        codes (``DamagePolicy.codes``) or a list of names / None, which is uploaded first; a given kind
        replaces the gates and the kind draw of its sample, -1 / None leaves the sample untouched.

        Returns None when ``epoch < start_epoch`` or ``prob <= 0`` (nothing is launched), else
        ``(draws, noise)``: ``draws`` int32 [B,8] = (applied, primitive kind, size argument, y, x, 0, 0, 0)
        per sample with ``return_draws`` and ``noise`` [B,max(1,C-4),H,W] with ``return_noise`` (written
        only where a noise kind applied), else None; both stay on the device."""
        if not isinstance(state, torch.Tensor) or state.dim() != 4:
            raise ValueError("state must be a [B,C,H,W] tensor")
        B, C, H, W = state.shape
        if C < 4 or H < 1 or W < 1:
            raise ValueError(f"state must have >= 4 channels and a non-empty field, got {tuple(state.shape)}")
        for name, v in (("epoch", epoch), ("sample_base", sample_base)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an int, got {v!r}")
        if sample_base < 0 or sample_base + B > L.DMG_SHARED_SAMPLE:
            raise ValueError(f"sample_base must be in [0, 2^32 - 1 - B], got {sample_base}")
        event_t = None
        if isinstance(event, torch.Tensor):
            if event.dtype != torch.int64 or event.numel() != 1 or event.device != state.device:
                raise ValueError("a tensor event must hold one int64 on the state's device")
            event_t, event = event, 0
        elif isinstance(event, bool) or not isinstance(event, int) or not -(1 << 63) <= event < 1 << 63:
            raise ValueError(f"event must be an int64 value or a 1-element int64 device tensor, got {event!r}")
        if kinds is not None and not isinstance(kinds, torch.Tensor):
            kinds = list(kinds)
            if len(kinds) != B or not all(n is None or isinstance(n, str) for n in kinds):
                raise ValueError(f"kinds must name {B} samples (a str or None each), got {kinds!r}")
        elif kinds is not None and (kinds.dtype != torch.int32 or tuple(kinds.shape) != (B,)
                                    or kinds.device != state.device or not kinds.is_contiguous()):
            raise ValueError(f"kinds must be a contiguous int32 tensor of shape ({B},) on the state's device")
        if state.device.type != "cuda" or state.dtype != torch.float32 or not state.is_contiguous():
            raise RuntimeError("damage ops run in place on a contiguous float32 ROCm state (no CPU path)")
        if isinstance(kinds, list):
            kinds = self.codes(kinds, state.device)
        if epoch < self.start_epoch or self.prob <= 0:
            return None
        d = self.desc(B, C, H, W, event, sample_base)
        d.stream = stream_ptr(state.device)
        draws = torch.empty(B, 8, dtype=torch.int32, device=state.device) if return_draws else None
        noise = torch.empty(B, max(1, C - 4), H, W, dtype=torch.float32, device=state.device) if return_noise else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = _entry("gnca_damage_policy")(ctypes.byref(d), state.data_ptr(), ptr(kinds), ptr(event_t), ptr(draws),
                                          ptr(noise))
        L.check(rc, "gnca_damage_policy")
        return draws, noise


def _cat(parts):
    parts = [p for p in parts if p is not None]
    return torch.cat(parts, 0) if parts else None


def split_record(steps: int, damage_step: int, every=1, record=None):
    """The recorded steps of a ``steps``-step run cut at ``damage_step``: (the indices up to it, the
    later ones counted from it).  Raises ``ValueError`` as ``trace`` does."""
    from .step import expand_record
    rec = expand_record(steps, every, record)
    return [r for r in rec if r <= damage_step], [r - damage_step for r in rec if r > damage_step]


def regrow_trace(model, x, steps: int, policy: DamagePolicy, damage_step: int, *, event=0, kinds=None, epoch=None,
                 **trace_kwargs):
    """Grow, damage, regrow as one ``TraceResult``: ``model.trace`` for ``damage_step`` steps,
    ``policy.apply_`` on its ``x_final`` (``epoch=None``: the policy's ``start_epoch``; ``sample_base``
    as the trace's), then ``model.trace`` for the remaining steps with ``first_step`` advanced by
    ``damage_step`` and the matching part of ``offsets`` / ``record`` / ``every``.  Every recorded field
    is concatenated along R and ``steps`` counts over the whole run.  ``damage_step=0`` damages (a copy
    of) ``x`` before the first step; the native trace cannot be interrupted, so this is two native calls
    by design.  Bad arguments raise ``ValueError`` before anything is drawn or launched."""
    from .metrics import ImageMetrics
    from .modules._stepper import TraceResult
    from .step import GraphDiagnostics
    from .vitals import StateVitals
    for name, v in (("steps", steps), ("damage_step", damage_step)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    if damage_step >= steps:
        raise ValueError(f"damage_step {damage_step} must be below steps {steps}: nothing would regrow")
    if not isinstance(policy, DamagePolicy):
        raise ValueError("policy must be a DamagePolicy")
    kw = dict(trace_kwargs)
    rec1, rec2 = split_record(steps, damage_step, kw.pop("every", 1), kw.pop("record", None))
    first = kw.pop("first_step", 0)
    if isinstance(first, bool) or not isinstance(first, int) or first < 0:
        raise ValueError(f"first_step must be a non-negative int, got {first!r}")
    offsets = kw.pop("offsets", None)
    if offsets is not None:
        offsets = list(offsets)
        if len(offsets) != steps:
            raise ValueError(f"offsets has {len(offsets)} entries for {steps} steps")
    if kinds is not None and not isinstance(kinds, torch.Tensor):
        kinds = list(kinds)
        if len(kinds) != x.shape[0]:
            raise ValueError(f"kinds names {len(kinds)} samples, the batch holds {x.shape[0]}")
        kinds = DamagePolicy.codes(kinds, x.device)
    epoch = policy.start_epoch if epoch is None else epoch
    if damage_step > 0:
        a = model.trace(x, damage_step, record=rec1, first_step=first,
                        offsets=None if offsets is None else offsets[:damage_step], **kw)
        mid = a.x_final
    else:
        a, mid = None, x.detach().clone()
    policy.apply_(mid, epoch, event, sample_base=kw.get("sample_base", 0), kinds=kinds)
    b = model.trace(mid, steps - damage_step, record=rec2, first_step=first + damage_step,
                    offsets=None if offsets is None else offsets[damage_step:], **kw)
    if a is None:
        return b
    metrics = None if b.metrics is None else ImageMetrics(torch.cat([a.metrics.stacked, b.metrics.stacked], 0))
    diag = None
    if b.diagnostics is not None:
        da, db = a.diagnostics, b.diagnostics
        diag = GraphDiagnostics(offsets=list(da.offsets or []) + list(db.offsets or []),
                                **{n: _cat([getattr(da, n), getattr(db, n)]) for n in L.DIAG_FIELDS})
    vitals = None if b.vitals is None else StateVitals(torch.cat([a.vitals.stacked, b.vitals.stacked], 0))
    return TraceResult(b.x_final, _cat([a.frames, b.frames]), rec1 + [r + damage_step for r in rec2],
                       _cat([a.attention, b.attention]), metrics, diag, rgb_u8=_cat([a.rgb_u8, b.rgb_u8]),
                       attention_u8=_cat([a.attention_u8, b.attention_u8]), vitals=vitals)
