"""Functional host layer over the C ABI: build descriptors from module state and launch.

Everything here is plumbing around ``libgnca.so``; the arithmetic is in the HIP kernels.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.device.type != "cuda":
        raise RuntimeError(
            f"graph_neural_cellular_automata_amd: {name} is on {t.device}; the NCA step runs only "
            f"on a ROCm GPU (move the model and the state to 'cuda'). There is no CPU path.")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def check_state(x: torch.Tensor, C: int) -> torch.Tensor:
    if x.dim() != 4:
        raise ValueError(f"state must be [B,C,H,W], got {tuple(x.shape)}")
    if x.shape[1] != C:
        raise ValueError(f"state has {x.shape[1]} channels, model expects {C}")
    if C < 4:
        raise ValueError("the alive mask reads channel 3: n_channels must be >= 4")
    return _dev_f32(x, "state")


def make_desc(*, B, C, H, W, hidden, d_model, offsets, flags, update_gain, alpha_thr,
              message_gain, fire_rate, fire_mode, gn_eps=1e-3, rng_seed=0, rng_step=0,
              sample_base=0, graph_alpha_thr=None) -> L.StepDesc:
    d = L.StepDesc()
    d.B, d.C, d.H, d.W = int(B), int(C), int(H), int(W)
    d.hidden, d.d_model = int(hidden), int(d_model)
    if len(offsets) > L.MAX_OFFSETS:
        raise ValueError(f"at most {L.MAX_OFFSETS} offsets per step (got {len(offsets)})")
    d.num_offsets = len(offsets)
    for o, (dy, dx) in enumerate(offsets):
        if not (-127 <= dy <= 127 and -127 <= dx <= 127):
            raise ValueError(f"offset {(dy, dx)} out of int8 range")
        d.offsets[2 * o] = int(dy)
        d.offsets[2 * o + 1] = int(dx)
    d.flags = int(flags)
    d.update_gain = float(update_gain)
    d.alpha_thr = float(alpha_thr)
    d.graph_alpha_thr = float(alpha_thr if graph_alpha_thr is None else graph_alpha_thr)
    d.message_gain = float(message_gain)
    d.gn_eps = float(gn_eps)
    d.fire_rate = float(fire_rate)
    d.fire_mode = int(fire_mode)
    d.rng_seed = int(rng_seed) & 0xFFFFFFFFFFFFFFFF
    d.rng_step = int(rng_step)
    d.sample_base = int(sample_base)
    return d


_WCACHE: dict = {}


def _dev_index(device) -> int:
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def make_weights(tensors: dict) -> tuple[L.Weights, list]:
    """tensors: name -> device tensor (reference layouts).  Returns the struct and the list of
    contiguous tensors that must stay alive until the launch is enqueued.

    When every tensor is already a contiguous float32 device tensor the struct holds exactly their
    addresses, so it is cached by (name, device, address, shape): a hit rebuilds nothing (in-place
    updates such as optimiser steps keep the addresses).  Only such tensors are looked up or
    stored: the check runs BEFORE the lookup, so a non-contiguous view or a tensor of another dtype
    that happens to sit at a cached address never returns a cached struct.  For cacheable tensors
    the struct is a pure function of the key, so the cache holds no tensor references (the weights
    of a deleted model are freed; a later tensor at the same address gets the same, correct
    struct).  Building the struct was ~20 us of host time per step at the trainer's size."""
    keep = [t for t in tensors.values() if t is not None]
    cacheable = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in keep)
    key = None
    if cacheable:
        key = tuple((name, t.device.index, t.data_ptr(), tuple(t.shape))
                    for name, t in tensors.items() if t is not None)
        hit = _WCACHE.get(key)
        if hit is not None:
            return hit, keep
    w = L.Weights()
    conv = []
    for name, t in tensors.items():
        if t is None:
            continue
        t = _dev_f32(t.detach(), name)
        conv.append(t)
        setattr(w, name, t.data_ptr())
    if cacheable:
        if len(_WCACHE) >= 256:
            _WCACHE.clear()
        _WCACHE[key] = w
        return w, keep
    return w, conv


_WS_BYTES: dict = {}

# the shape classes libgnca.so is compiled for (find_variant in gnca_step.hip)
SUPPORT_SET = "supported: 4 <= C <= 32; hidden <= 128, or hidden <= 256 for 13 <= C <= 16"


def _entry(name: str):
    """The library's entry point ``name``; a library built before it was added names what is missing."""
    fn = getattr(L.load(), name, None)
    if fn is None:
        raise L.GncaError(f"libgnca.so at {L.LIB_PATH} has no {name}: rebuild it (python -c 'import __graft_entry__ "
                          f"as g; g.build(force=True)')")
    return fn


def _sized(n: int, what: str, desc, device=None, extra: str = "", K=None):
    """The uint8 workspace for a size query's answer ``n`` (``device`` None: ``n`` itself).  0 is the query's
    refusal: ``GncaError`` "unsupported ``what``: [K=..] B=.. (the support set``extra``)"."""
    if n == 0:
        k = "" if K is None else f"K={K} "
        raise L.GncaError(f"unsupported {what}: {k}B={desc.B} C={desc.C} H={desc.H} W={desc.W} "
                          f"hidden={desc.hidden} ({SUPPORT_SET}{extra})")
    return n if device is None else torch.empty(n, dtype=torch.uint8, device=device)


def _k1_info(desc) -> tuple[str, int]:
    """(kernel name, arith bits) of gnca_k1_variant for ``desc``."""
    buf = ctypes.create_string_buffer(128)
    arith = ctypes.c_int32(0)
    L.check(L.load().gnca_k1_variant(ctypes.byref(desc), buf, 128, ctypes.byref(arith)), "gnca_k1_variant")
    return buf.value.decode(), arith.value


def _flat_offsets(desc, steps: int, offsets_per_step: list):
    """``offsets_per_step`` as the int8 array [steps][k][2] of the C calls, or None when there are none."""
    flat = [v for offs in offsets_per_step for o in offs for v in o]
    if (desc.flags & L.GRAPH) and desc.num_offsets > 0 and len(flat) != steps * 2 * desc.num_offsets:
        raise ValueError("offsets_per_step must hold k pairs for every step")
    return (ctypes.c_int8 * len(flat))(*flat) if flat else None


def _records(record: list):
    """The recorded step indices as an int32 array (one unused element when there are none)."""
    return (ctypes.c_int32 * max(1, len(record)))(*record)


def _grad_buffers(want: dict | None, out: dict | None, device):
    """(``L.Grads``, {name: tensor}) for the ``want``ed parameters: the caller's ``out`` tensors where given,
    fresh float32 ones elsewhere."""
    g, grads = L.Grads(), {}
    given = out or {}
    for name, p in (want or {}).items():
        t = given.get(name)
        if t is None:
            t = torch.empty(p.shape, dtype=torch.float32, device=device)
        elif t.shape != p.shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"gradient buffer for {name} must be contiguous float32 {tuple(p.shape)}")
        grads[name] = t
        setattr(g, GRAD_FIELDS[name], t.data_ptr())
    return g, grads


def _tape(call: "RolloutCall", device) -> torch.Tensor:
    """The tape of ``call``'s schedule (0 steps record nothing: 256 bytes keep the pointer valid)."""
    nb = L.load().gnca_rollout_tape_bytes(ctypes.byref(call.desc), ctypes.byref(call.c))
    return torch.empty(max(nb, 256), dtype=torch.uint8, device=device)


def workspace(desc: L.StepDesc, device) -> torch.Tensor:
    # the size depends on the shape class and the offsets' radius (the tile plan), not on the
    # offsets themselves or the knobs' values
    o = desc.offsets[:2 * desc.num_offsets]
    # (the plan also depends on the device's CU count: keyed by device)
    key = (_dev_index(device), desc.B, desc.C, desc.H, desc.W, desc.hidden, desc.d_model, desc.num_offsets, desc.flags,
           desc.message_gain != 0.0, desc.fire_mode,
           max((abs(v) for v in o[0::2]), default=0), max((abs(v) for v in o[1::2]), default=0))
    n = _WS_BYTES.get(key)
    if n is None:
        n = L.load().gnca_workspace_bytes(ctypes.byref(desc))
        if n and len(_WS_BYTES) < 256:
            _WS_BYTES[key] = n
    return _sized(n, "step shape", desc, device)


def k1_variant(desc: L.StepDesc) -> tuple[str, str]:
    """(kernel name, MFMA arithmetic) of the K1 the plan for ``desc`` launches: arithmetic "f32"
    (fp32 MFMA) or "bf16x6" (bf16 MFMA on exact 3-way splits, 6 products per fp32 product)."""
    name, arith = _k1_info(desc)
    return name, ("bf16x6" if arith & 1 else "f32")


def bb_variant(desc: L.StepDesc) -> str:
    """The backward MLP kernel (BB) the backward plan for ``desc`` launches, as
    "gnca_b_mlp<CP,HB,FULL,TH,TW,RY,RX,K,LEAN>" (gnca_bb_variant, host-only)."""
    buf = ctypes.create_string_buffer(128)
    L.check(L.load().gnca_bb_variant(ctypes.byref(desc), buf, 128), "gnca_bb_variant")
    return buf.value.decode()


def k2_variant(desc: L.StepDesc, co: int = 0) -> str:
    """The K2 (finalize) kernel a step of ``desc`` launches (gnca_k2_variant, host-only):
    "gnca_k2_finalize_flat<V,CU>" or the band kernel "gnca_k2_finalize<V,COMPACT,CU,ROWS>".  ``co``: 1 = a
    step of a rollout's sub-batch pipeline (K2 beside the other sub-batch's K1), 0 = a rollout step with
    K2 alone on the chip, -1 = a single (or masked) step."""
    lib = L.load()
    lib.gnca_k2_variant.restype = ctypes.c_int
    lib.gnca_k2_variant.argtypes = [ctypes.POINTER(L.StepDesc), ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]
    buf = ctypes.create_string_buffer(128)
    L.check(lib.gnca_k2_variant(ctypes.byref(desc), int(co), buf, 128), "gnca_k2_variant")
    return buf.value.decode()


def rollout_compact(desc: L.StepDesc) -> bool:
    """True when a rollout of ``desc``'s shape runs on the compact update field (K1 packs the live
    cells' dx per tile, K2 unpacks them: GNCA_PHASE_COMPACT)."""
    return bool(_k1_info(desc)[1] & 2)


def rollout_subs(desc: L.StepDesc) -> int:
    """Concurrent sub-batches a rollout of ``desc``'s shape runs as (2: one sub-batch's K2 beside
    the other's K1 on two streams; 1: one stream)."""
    return 2 if _k1_info(desc)[1] & 4 else 1


def rollout_fold(desc: L.StepDesc, possible: bool = False) -> bool:
    """True when a rollout of ``desc``'s shape folds each step's finish (GroupNorm, tanh * gain,
    residual, post-update alpha gate) into the next step's K1, so one K1 launch per step plus one
    K2 at the end of the rollout (gnca_k1_variant arith bit 8).  ``possible``: whether it can, on
    request (``rollout(..., fold=True)``; arith bit 16) where it is not the default."""
    return bool(_k1_info(desc)[1] & (16 if possible else 8))


_MULTI_GPU = None


def stream_ptr(device) -> int:
    """The current stream of ``device`` as the C ABI's ``void* stream``.

    The null stream (pointer 0) names no device: the library would launch on whichever device is
    current.  So a tensor on a device that is not the current one, on that device's default stream,
    is refused instead of launched on the wrong device."""
    ptr = torch.cuda.current_stream(device).cuda_stream
    if ptr == 0 and _MULTI_GPU is not False:
        _refuse_foreign_default_stream(device)
    return ptr


def _refuse_foreign_default_stream(device) -> None:
    global _MULTI_GPU
    if _MULTI_GPU is None:
        _MULTI_GPU = torch.cuda.device_count() > 1
    if not _MULTI_GPU:
        return
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    if idx is None:      # "cuda" without an index is the current device
        return
    cur = torch.cuda.current_device()
    if idx != cur:
        raise ValueError(
            f"the tensors are on cuda:{idx} but the current device is cuda:{cur}, and cuda:{idx}'s "
            f"current stream is its default stream, which does not name a device: the kernels would "
            f"launch on cuda:{cur}.  Enter `with torch.cuda.device({idx}):` around the call, or use a "
            f"stream of cuda:{idx} (`with torch.cuda.stream(torch.cuda.Stream({idx})):`)")


def _active_u8(active, B, device):
    if active is None:
        return None
    if active.device != device or active.dtype not in (torch.bool, torch.uint8) or active.shape != (B,):
        raise ValueError("active must be a [B] bool/uint8 tensor on the state's device")
    active = active.contiguous()
    # a bool tensor is one byte of 0/1 per element: reinterpret, no conversion launch
    return active.view(torch.uint8) if active.dtype == torch.bool else active


def step(desc, weights, x, fire=None, want_attention=False, ws=None, active=None):
    """One step: returns (x_out, attn_or_None).  ``ws``: an optional caller-owned workspace
    (``workspace(desc)``); after the call it holds what ``step_backward(saved=ws)`` reuses.
    ``active``: optional [B] bool/uint8 device mask; inactive samples pass through unchanged
    (gnca_step_masked_f32)."""
    lib = L.load()
    x_out = torch.empty_like(x)
    attn = torch.empty(desc.B, desc.H, desc.W, dtype=torch.float32, device=x.device) \
        if want_attention else None
    if ws is None:
        ws = workspace(desc, x.device)
    act = _active_u8(active, desc.B, x.device)
    if act is not None:
        if want_attention:
            raise ValueError("return_attention is not supported with an active-sample mask")
        rc = lib.gnca_step_masked_f32(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(),
                                      x_out.data_ptr(), _ptr(fire), act.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream_ptr(x.device))
        L.check(rc, "gnca_step_masked_f32")
        return x_out, None
    rc = lib.gnca_step_f32(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(),
                           x_out.data_ptr(), _ptr(fire), _ptr(attn), ws.data_ptr(), ws.numel(),
                           stream_ptr(x.device))
    L.check(rc, "gnca_step_f32")
    return x_out, attn


def message(desc, weights, x, want_attention=False):
    lib = L.load()
    m = torch.empty_like(x)
    attn = torch.empty(desc.B, desc.H, desc.W, dtype=torch.float32, device=x.device) \
        if want_attention else None
    ws = workspace(desc, x.device)
    rc = lib.gnca_message_f32(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(),
                              m.data_ptr(), _ptr(attn), ws.data_ptr(), ws.numel(),
                              stream_ptr(x.device))
    L.check(rc, "gnca_message_f32")
    return m, attn


def perceive(weight, x):
    lib = L.load()
    B, C, H, W = x.shape
    w = _dev_f32(weight.detach(), "perception weight")
    y = torch.empty(B, 3 * C, H, W, dtype=torch.float32, device=x.device)
    rc = lib.gnca_perceive_f32(B, C, H, W, w.data_ptr(), x.data_ptr(), y.data_ptr(),
                               stream_ptr(x.device))
    L.check(rc, "gnca_perceive_f32")
    return y


def fire_mask(desc, device) -> torch.Tensor:
    """The [B,1,H,W] uint8 fire mask a GNCA_FIRE_HASH step with ``desc`` draws."""
    m = torch.empty(desc.B, 1, desc.H, desc.W, dtype=torch.uint8, device=device)
    L.check(L.load().gnca_fire_mask_u8(ctypes.byref(desc), m.data_ptr(), stream_ptr(device)),
            "gnca_fire_mask_u8")
    return m


def rollout(desc, weights, x, steps: int, offsets_per_step: list, fold: bool = False):
    """``steps`` no-grad steps (GNCA_FIRE_HASH / NONE) in one C call.  ``fold``: fold each step's
    finish into the next K1 even where that is not the default (GNCA_ROLLOUT_FOLD)."""
    lib = L.load()
    arr = _flat_offsets(desc, steps, offsets_per_step)
    out = torch.empty_like(x)
    scratch = torch.empty_like(x)
    ws = workspace(desc, x.device)
    rc = lib.gnca_rollout_ex_f32(ctypes.byref(desc), ctypes.byref(weights), int(steps), arr,
                                 x.data_ptr(), out.data_ptr(), scratch.data_ptr(), ws.data_ptr(),
                                 ws.numel(), L.ROLLOUT_FOLD if fold else 0, stream_ptr(x.device))
    L.check(rc, "gnca_rollout_ex_f32")
    return out


# parameter name (state_dict suffix) -> gnca_grads field
GRAD_FIELDS = {
    "update_net.0.weight": "w1", "update_net.0.bias": "b1", "update_net.2.weight": "w2",
    "norm.weight": "gn_weight", "norm.bias": "gn_bias",
    "graph.query_proj.weight": "wq", "graph.query_proj.bias": "bq",
    "graph.key_proj.weight": "wk", "graph.key_proj.bias": "bk",
    "graph.msg_proj.weight": "wm", "graph.msg_proj.bias": "bm", "graph.scaling": "scaling",
}


def step_backward(desc, weights, x, gy, fire=None, want: dict | None = None, saved=None, active=None,
                  out: dict | None = None):
    """Vector-Jacobian product of one step (gnca_step_bwd_f32).

    ``want`` maps state_dict names (GRAD_FIELDS keys) to the parameter tensors whose gradients
    are wanted; returns ``(gx, {name: grad})`` with grads shaped like the parameters.
    ``saved``: the workspace of the forward ``step(..., ws=saved)`` call on the same inputs
    (skips recomputing the forward's update field).  ``out``: preallocated float32 gradient
    tensors (e.g. views of one flat buffer) for some of the ``want`` names."""
    lib = L.load()
    gy = _dev_f32(gy, "grad_output")
    gx = torch.empty_like(x)
    g, out = _grad_buffers(want, out, x.device)
    ws = _sized(lib.gnca_bwd_workspace_bytes(ctypes.byref(desc)), "step shape for the backward", desc, x.device)
    act = _active_u8(active, desc.B, x.device)
    rc = lib.gnca_step_bwd_f32(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(), _ptr(fire),
                               _ptr(act), gy.data_ptr(), gx.data_ptr(), ctypes.byref(g), _ptr(saved),
                               ws.data_ptr(), ws.numel(), stream_ptr(x.device))
    L.check(rc, "gnca_step_bwd_f32")
    return gx, out


# ---------------------------------------------------------------------------------------------
# Whole-rollout schedule (gnca_rollout_fwd_f32 / gnca_rollout_bwd_f32)
# ---------------------------------------------------------------------------------------------
class Schedule:
    """A validated per-step schedule of one rollout (``build_schedule``): plain Python values and
    the caller's device tensors; ``RolloutCall`` turns it into the C struct."""

    __slots__ = ("steps", "full_steps", "recompute", "offsets", "k", "fire_rates", "gains", "nsteps",
                 "fire", "fire_mode", "seed", "sample_base", "checkpoint_every")

    @property
    def uniform(self) -> bool:
        """One rate, one gain, every sample every step, hash or no fire: the schedule the no-grad
        pipeline of ``gnca_rollout_ex_f32`` runs."""
        return (self.nsteps is None and self.fire is None and len(set(self.fire_rates)) <= 1
                and (self.gains is None or len(set(self.gains)) <= 1))


def _per_step(value, steps: int, name: str) -> list:
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        return [float(value)] * steps
    try:
        vals = [float(v) for v in value]
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or a sequence of {steps} numbers") from None
    if len(vals) != steps:
        raise ValueError(f"{name} has {len(vals)} entries for {steps} steps")
    return vals


def checkpoint_interval(checkpoint_every, steps: int):
    """``checkpoint_every`` validated: None (no checkpointing), an int >= 1, or ``"auto"`` =
    ``ceil(sqrt(steps))``, which minimises the ``steps / k`` anchors plus the ``k`` segment states."""
    if checkpoint_every is None:
        return None
    if isinstance(checkpoint_every, str):
        if checkpoint_every != "auto":
            raise ValueError(f"checkpoint_every must be None, an int >= 1 or 'auto', got {checkpoint_every!r}")
        k = math.isqrt(max(int(steps), 1))
        return max(k if k * k >= steps else k + 1, 1)
    if isinstance(checkpoint_every, bool) or not isinstance(checkpoint_every, int) or checkpoint_every < 1:
        raise ValueError(f"checkpoint_every must be None, an int >= 1 or 'auto', got {checkpoint_every!r}")
    return checkpoint_every


def build_schedule(*, steps, B, H, W, device, fire_rate=1.0, message_gain=None, nsteps=None, min_steps=0,
                   fire=None, seed=None, sample_base=0, offsets=None, sample_offsets=None,
                   recompute=False, checkpoint_every=None) -> Schedule:
    """Validate a rollout's arguments and build its schedule.  Pure Python: needs neither the
    library nor a GPU, and raises ``ValueError`` before anything is launched.

    ``message_gain``: None for a model without the graph term, else a number or ``steps`` numbers.
    ``offsets``: ``steps`` lists of (dy, dx) pairs (the same count every step), or None to call
    ``sample_offsets()`` once per step in step order (``GraphAugmentation.sample_offsets``: the
    draws ``steps`` forward calls would make from Python's ``random``, message-off steps included).
    ``fire``: None (hash masks from ``seed`` when any rate is below 1; ``seed=None`` draws one
    integer from torch's default CPU generator) or a [steps,B,1,H,W] tensor on ``device``: float32
    uniforms or uint8 / bool masks.
    ``checkpoint_every``: None, an int >= 1 or ``"auto"`` (``checkpoint_interval``): the tape keeps
    every k-th state and the backward re-runs one segment of k steps at a time."""
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise ValueError(f"steps must be a non-negative int, got {steps!r}")
    if isinstance(min_steps, bool) or not isinstance(min_steps, int) or min_steps < 0:
        raise ValueError(f"min_steps must be a non-negative int, got {min_steps!r}")
    ckpt = checkpoint_interval(checkpoint_every, steps)   # (before any offset is drawn)
    device = torch.device(device)
    s = Schedule()
    s.checkpoint_every = ckpt
    s.steps, s.full_steps, s.recompute = steps, min(min_steps, steps), bool(recompute)
    s.sample_base = int(sample_base)
    s.fire_rates = _per_step(fire_rate, steps, "fire_rate")
    s.gains = None if message_gain is None else _per_step(message_gain, steps, "message_gain")
    # offsets
    if offsets is None:
        offsets = [sample_offsets() for _ in range(steps)] if sample_offsets is not None else None
    elif s.gains is None:
        raise ValueError("offsets given for a model without the graph term")
    if offsets is None:
        s.offsets, s.k = None, 0
    else:
        offsets = [list(o) for o in offsets]
        if len(offsets) != steps:
            raise ValueError(f"offsets has {len(offsets)} entries for {steps} steps")
        ks = {len(o) for o in offsets}
        if len(ks) > 1:
            raise ValueError(f"every step must draw the same number of offsets, got {sorted(ks)}")
        s.k = ks.pop() if ks else 0
        if s.k > L.MAX_OFFSETS:
            raise ValueError(f"at most {L.MAX_OFFSETS} offsets per step (got {s.k})")
        for o in offsets:
            for pair in o:
                if len(pair) != 2 or not all(isinstance(v, int) and -127 <= v <= 127 for v in pair):
                    raise ValueError(f"offset {pair!r} is not a (dy, dx) pair in the int8 range")
        s.offsets = [[(int(dy), int(dx)) for dy, dx in o] for o in offsets]
    # active steps per sample
    if nsteps is not None:
        if not isinstance(nsteps, torch.Tensor) or nsteps.dtype != torch.int32 or tuple(nsteps.shape) != (B,):
            raise ValueError(f"nsteps must be an int32 tensor of shape ({B},)")
        if nsteps.device != device:
            raise ValueError(f"nsteps is on {nsteps.device}, the state on {device}")
        nsteps = nsteps.contiguous()
    s.nsteps = nsteps
    # fire
    s.seed = 0
    if fire is not None:
        if not isinstance(fire, torch.Tensor) or tuple(fire.shape) != (steps, B, 1, H, W):
            raise ValueError(f"fire must be a tensor of shape ({steps}, {B}, 1, {H}, {W})")
        if fire.device != device:
            raise ValueError(f"fire is on {fire.device}, the state on {device}")
        if fire.dtype == torch.float32:
            s.fire_mode = L.FIRE_RAND_F32
        elif fire.dtype in (torch.uint8, torch.bool):
            s.fire_mode = L.FIRE_MASK_U8
        else:
            raise ValueError(f"fire must be float32 uniforms or uint8 / bool masks, got {fire.dtype}")
        fire = fire.contiguous()
        s.fire = fire.view(torch.uint8) if fire.dtype == torch.bool else fire
    else:
        s.fire = None
        if any(r < 1.0 for r in s.fire_rates):
            s.fire_mode = L.FIRE_HASH
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            elif isinstance(seed, bool) or not isinstance(seed, int):
                raise ValueError(f"seed must be an int, got {seed!r}")
            s.seed = seed
        else:
            s.fire_mode = L.FIRE_NONE
    return s


def expand_record(steps: int, every=1, record=None) -> list:
    """The recorded step indices of a trace: ``record`` as given (strictly increasing, in
    ``1..steps``), else ``every, 2*every, ...`` and also ``steps`` when it is not a multiple."""
    if record is not None:
        if every != 1:
            raise ValueError("give either every or record, not both")
        try:
            rec = list(record)
        except TypeError:
            raise ValueError(f"record must be a sequence of step indices, got {record!r}") from None
        for r in rec:
            if isinstance(r, bool) or not isinstance(r, int):
                raise ValueError(f"record entries must be ints, got {r!r}")
            if not 1 <= r <= steps:
                raise ValueError(f"record entry {r} is outside 1..{steps}")
        if any(b <= a for a, b in zip(rec, rec[1:])):
            raise ValueError(f"record must be strictly increasing, got {rec}")
        return rec
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"every must be a positive int, got {every!r}")
    rec = list(range(every, steps + 1, every))
    if steps > 0 and steps % every:
        rec.append(steps)
    return rec


class TracePlan:
    """A validated trace (``build_trace``): the uniform schedule, the recorded step indices, the
    frame channel count, the hash-RNG step base and whether maps are wanted."""

    __slots__ = ("schedule", "record", "channels", "first_step", "attention")


def build_trace(*, steps, B, C, H, W, device, every=1, record=None, channels=4, return_attention=False,
                fire_rate=1.0, message_gain=None, seed=None, sample_base=0, first_step=0, offsets=None,
                sample_offsets=None) -> TracePlan:
    """Validate a trace's arguments and build its plan.  Pure Python, like ``build_schedule`` (which
    validates the shared arguments and draws the offsets): raises ``ValueError`` before the library is
    loaded.  A trace runs the no-grad rollout pipeline, so its schedule must be uniform: one fire
    rate and one message gain for every step (a per-step list must hold one value), hash or no fire
    masks."""
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= C:
        raise ValueError(f"channels must be an int in 1..{C} (the state's channel count), got {channels!r}")
    if isinstance(first_step, bool) or not isinstance(first_step, int) or first_step < 0:
        raise ValueError(f"first_step must be a non-negative int, got {first_step!r}")
    if return_attention and message_gain is None:
        raise ValueError("return_attention needs the graph term: this model has none")
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise ValueError(f"steps must be a non-negative int, got {steps!r}")
    rec = expand_record(steps, every, record)
    # (before the offsets are drawn: a rejected call leaves Python's random state alone)
    for name, v in (("fire_rate", fire_rate), ("message_gain", message_gain)):
        if v is not None and len(set(_per_step(v, steps, name))) > 1:
            raise ValueError(f"a trace needs a uniform schedule: {name} must be one value for every step")
    s = build_schedule(steps=steps, B=B, H=H, W=W, device=device, fire_rate=fire_rate, message_gain=message_gain,
                       seed=seed, sample_base=sample_base, offsets=offsets, sample_offsets=sample_offsets)
    if not s.uniform:
        raise ValueError("a trace needs a uniform schedule")
    p = TracePlan()
    p.schedule, p.record, p.channels, p.first_step, p.attention = s, rec, channels, first_step, bool(return_attention)
    return p


def attention_map(desc, weights, x):
    """The normalised attention map [B,H,W] of state ``x`` for ``desc``'s offsets
    (gnca_attention_f32): a side computation, no step."""
    lib = L.load()
    attn = torch.empty(desc.B, desc.H, desc.W, dtype=torch.float32, device=x.device)
    n = lib.gnca_attention_workspace_bytes(ctypes.byref(desc))
    if n == 0:
        raise L.GncaError(f"unsupported attention-map shape: B={desc.B} C={desc.C} H={desc.H} W={desc.W} "
                          f"k={desc.num_offsets}")
    ws = torch.empty(n, dtype=torch.uint8, device=x.device)
    rc = lib.gnca_attention_f32(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(), attn.data_ptr(),
                                ws.data_ptr(), ws.numel(), stream_ptr(x.device))
    L.check(rc, "gnca_attention_f32")
    return attn


def trace(desc, weights, x, steps: int, offsets_per_step: list, record: list, channels: int,
          want_attention: bool = False):
    """``steps`` no-grad steps in one C call that also records (gnca_rollout_trace_f32): returns
    ``(x_final, frames [R,B,channels,H,W], attention [R,B,H,W] or None)``."""
    lib = L.load()
    arr = _flat_offsets(desc, steps, offsets_per_step)
    R = len(record)
    rec = _records(record)
    out = torch.empty_like(x)
    frames = torch.empty(R, desc.B, channels, desc.H, desc.W, dtype=torch.float32, device=x.device)
    attn = torch.empty(R, desc.B, desc.H, desc.W, dtype=torch.float32, device=x.device) if want_attention else None
    a = L.TraceArgs()
    a.steps, a.num_records, a.frame_channels, a.flags = int(steps), R, int(channels), 0
    a.offsets = ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None
    a.record = ctypes.cast(rec, ctypes.c_void_p)
    # (an empty tensor's data_ptr is 0: no record points, nothing is written)
    a.frames = frames.data_ptr() if R else None
    a.attn = attn.data_ptr() if (attn is not None and R) else None
    ws = _sized(lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(desc), ctypes.byref(a)), "trace shape", desc,
                x.device)
    rc = lib.gnca_rollout_trace_f32(ctypes.byref(desc), ctypes.byref(weights), ctypes.byref(a), x.data_ptr(),
                                    out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(x.device))
    L.check(rc, "gnca_rollout_trace_f32")
    return out, frames, attn


def trace_metrics(desc, weights, x, steps: int, offsets_per_step: list, record: list, channels: int,
                  target, target_bstride: int, want_attention: bool = False, want_frames: bool = True):
    """``trace`` that also measures (gnca_rollout_trace_metrics_f32): the image metrics of channels
    0..3 of the state after each recorded step against ``target`` (a contiguous float32 device tensor
    of premultiplied RGBA with sample stride ``target_bstride``, 0 = broadcast; None: nothing is
    measured).  Returns ``(x_final, frames or None, attention or None, metrics [R,B,4] or None)``;
    without ``want_frames`` no frame buffer is allocated."""
    return _trace_measured(desc, weights, x, steps, offsets_per_step, record, channels, target, target_bstride,
                           want_attention, want_frames, None)[:4]


def trace_diag(desc, weights, x, steps: int, offsets_per_step: list, record: list, channels: int,
               target=None, target_bstride: int = 0, want_attention: bool = False, want_frames: bool = True,
               per_offset: bool = False):
    """``trace_metrics`` that also records the diagnostics of every recorded step
    (gnca_rollout_trace_diag), computed from that step's input state with that step's offsets.
    Returns ``(x_final, frames or None, attention or None, metrics [R,B,4] or None, GraphDiagnostics
    with [R,...]-leading fields)``."""
    return _trace_measured(desc, weights, x, steps, offsets_per_step, record, channels, target, target_bstride,
                           want_attention, want_frames, bool(per_offset))[:5]


def trace_vitals(desc, weights, x, steps: int, offsets_per_step: list, record: list, channels: int,
                 alpha_thr: float, target=None, target_bstride: int = 0, want_attention: bool = False,
                 want_frames: bool = True, diagnostics: bool = False, per_offset: bool = False):
    """``trace_metrics`` / ``trace_diag`` that also takes the vitals of the state after each recorded
    step (gnca_rollout_trace_vitals; ``vitals.state_vitals`` of all C channels, against ``alpha_thr``).
    Returns ``(x_final, frames or None, attention or None, metrics [R,B,4] or None, GraphDiagnostics or
    None, vitals [R,B,13] float64)``."""
    return _trace_measured(desc, weights, x, steps, offsets_per_step, record, channels, target, target_bstride,
                           want_attention, want_frames, bool(per_offset) if diagnostics else None,
                           vitals_thr=float(alpha_thr))


def _trace_measured(desc, weights, x, steps, offsets_per_step, record, channels, target, target_bstride,
                    want_attention, want_frames, diag_taps, vitals_thr=None):
    """The shared body of ``trace_metrics`` (``diag_taps`` None), ``trace_diag`` (``diag_taps``: whether
    the per-offset stack is recorded too) and ``trace_vitals`` (``vitals_thr`` set, beside either)."""
    lib = L.load()
    fn = _entry("gnca_rollout_trace_diag") if diag_taps is not None else None
    if vitals_thr is not None:
        fn = _entry("gnca_rollout_trace_vitals")
    arr = _flat_offsets(desc, steps, offsets_per_step)
    R = len(record)
    rec = _records(record)
    out = torch.empty_like(x)
    frames = None
    if want_frames:
        frames = torch.empty(R, desc.B, channels, desc.H, desc.W, dtype=torch.float32, device=x.device)
    attn = torch.empty(R, desc.B, desc.H, desc.W, dtype=torch.float32, device=x.device) if want_attention else None
    met = None if target is None else torch.empty(R, desc.B, 4, dtype=torch.float32, device=x.device)
    a = L.TraceArgs()
    a.steps, a.num_records, a.frame_channels, a.flags = int(steps), R, int(channels), 0
    a.offsets = ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None
    a.record = ctypes.cast(rec, ctypes.c_void_p)
    a.frames = frames.data_ptr() if (frames is not None and R) else None
    a.attn = attn.data_ptr() if (attn is not None and R) else None
    m = L.TraceMetrics()
    if met is not None:
        # (R = 0: a placeholder element keeps both pointers set; nothing is written)
        keep_out = met if R else torch.empty(4, dtype=torch.float32, device=x.device)
        m.target, m.target_bstride, m.out = target.data_ptr(), int(target_bstride), keep_out.data_ptr()
    if vitals_thr is not None:
        t, o = _diag_buffers(desc, x.device, diag_taps, lead=(R,)) if diag_taps is not None else (None, None)
        op = None if o is None else ctypes.byref(o)
        n = lib.gnca_rollout_trace_vitals_workspace_bytes(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(m), op)
    else:
        size = (lib.gnca_rollout_trace_metrics_workspace_bytes if fn is None
                else lib.gnca_rollout_trace_diag_workspace_bytes)
        n = size(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(m))
    ws = _sized(n, "trace shape", desc, x.device)
    if vitals_thr is not None:
        vit = torch.empty(R, desc.B, len(L.VITALS_FIELDS), dtype=torch.float64, device=x.device)
        v = L.TraceVitals()
        v.alpha_thr, v.out = float(vitals_thr), (vit.data_ptr() if R else None)
        rc = fn(ctypes.byref(desc), ctypes.byref(weights), ctypes.byref(a), ctypes.byref(m), op, ctypes.byref(v),
                x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(x.device))
        L.check(rc, "gnca_rollout_trace_vitals")
        diag = None if t is None else _trace_diagnostics(desc, offsets_per_step, record, t)
        return out, frames, attn, met, diag, vit
    if fn is None:
        rc = lib.gnca_rollout_trace_metrics_f32(ctypes.byref(desc), ctypes.byref(weights), ctypes.byref(a),
                                                ctypes.byref(m), x.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                ws.numel(), stream_ptr(x.device))
        L.check(rc, "gnca_rollout_trace_metrics_f32")
        return out, frames, attn, met, None, None
    t, o = _diag_buffers(desc, x.device, diag_taps, lead=(R,))
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), ctypes.byref(a), ctypes.byref(m), ctypes.byref(o),
            x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(x.device))
    L.check(rc, "gnca_rollout_trace_diag")
    return out, frames, attn, met, _trace_diagnostics(desc, offsets_per_step, record, t), None


def _trace_diagnostics(desc, offsets_per_step, record, fields):
    """A trace's ``GraphDiagnostics``: the recorded steps' offsets beside the [R,...]-leading fields."""
    has = (desc.flags & L.GRAPH) and desc.num_offsets > 0
    offs = [[tuple(p) for p in offsets_per_step[r - 1]] if has else [] for r in record]
    return GraphDiagnostics(offs, **fields)


class GraphDiagnostics:
    """The decomposition of the attention map (``GraphAugmentation.diagnostics``, ``trace(diagnostics=True)``;
    include/gnca.h, gnca_graph_diag_out).  With ``m = msg_proj(x)``, ``src`` the sender mask (1 without
    ``alive_to_alive``), ``w_o`` the step's offset weights and ``S = src * mean_c |m_c|``, per sample
    (a trace adds a leading ``R`` axis to every field):

    ``magnitude`` [B,3,H,W]   mean |m_c| over the channels 0..2 / 3 / 4.. (unmasked, unweighted)
    ``groups`` [B,3,H,W]      sum_o w_o shift_o(src * magnitude)
    ``per_offset`` [B,k,H,W]  w_o shift_o(S), in offset order (None when not requested)
    ``raw`` [B,H,W]           sum_o w_o shift_o(S): the un-normalised map
    ``attention`` [B,H,W]     raw min-max normalised per sample: ``attention_map``, bitwise
    ``sender_union`` [B,H,W]  {0,1}: max_o shift_o(src) with ``alive_to_alive``, else zeros
    ``receiver`` [B,H,W]      {0,1}: the alive mask of the state
    ``weights`` [B,k]         w_o
    ``offsets``               the (dy, dx) pairs (a trace: one list per recorded step)

    All detached float32 device tensors."""

    __slots__ = L.DIAG_FIELDS + ("offsets",)

    def __init__(self, offsets=None, **fields):
        for n in L.DIAG_FIELDS:
            setattr(self, n, fields.get(n))
        self.offsets = offsets

    def __repr__(self):
        shape = lambda t: None if t is None else tuple(t.shape)
        return "GraphDiagnostics(" + ", ".join(f"{n}={shape(getattr(self, n))}" for n in L.DIAG_FIELDS) + ")"


def _diag_buffers(desc, device, per_offset: bool, lead: tuple = ()):
    """The output tensors of one diagnostics call (``lead``: a trace's record axis) and their struct."""
    B, H, W = desc.B, desc.H, desc.W
    k = desc.num_offsets if (desc.flags & L.GRAPH) else 0
    f32 = torch.float32
    t = {
        "magnitude": torch.empty(*lead, B, 3, H, W, dtype=f32, device=device),
        "groups": torch.empty(*lead, B, 3, H, W, dtype=f32, device=device),
        "per_offset": torch.empty(*lead, B, k, H, W, dtype=f32, device=device) if per_offset else None,
        "raw": torch.empty(*lead, B, H, W, dtype=f32, device=device),
        "attention": torch.empty(*lead, B, H, W, dtype=f32, device=device),
        "sender_union": torch.empty(*lead, B, H, W, dtype=f32, device=device),
        "receiver": torch.empty(*lead, B, H, W, dtype=f32, device=device),
        "weights": torch.empty(*lead, B, k, dtype=f32, device=device),
    }
    o = L.GraphDiagOut()
    for n, v in t.items():
        # (an empty tensor's data_ptr is 0: nothing is written)
        setattr(o, n, v.data_ptr() if (v is not None and v.numel()) else None)
    return t, o


def graph_diagnostics(desc, weights, x, per_offset: bool = True) -> GraphDiagnostics:
    """The diagnostics of state ``x`` for ``desc``'s offsets (gnca_graph_diag): a side computation, no
    step."""
    fn = _entry("gnca_graph_diag")
    lib = L.load()
    t, o = _diag_buffers(desc, x.device, per_offset)
    n = lib.gnca_graph_diag_workspace_bytes(ctypes.byref(desc))
    if n == 0:
        raise L.GncaError(f"unsupported diagnostics shape: B={desc.B} C={desc.C} H={desc.H} W={desc.W} "
                          f"k={desc.num_offsets}")
    ws = torch.empty(n, dtype=torch.uint8, device=x.device)
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(), ctypes.byref(o), ws.data_ptr(), ws.numel(),
            stream_ptr(x.device))
    L.check(rc, "gnca_graph_diag")
    k = desc.num_offsets if (desc.flags & L.GRAPH) else 0
    offs = [(int(desc.offsets[2 * i]), int(desc.offsets[2 * i + 1])) for i in range(k)]
    return GraphDiagnostics(offs, **t)


class RolloutCall:
    """A schedule bound to a descriptor: the C struct with its host arrays kept alive."""

    def __init__(self, desc: L.StepDesc, sched: Schedule):
        T, k = sched.steps, desc.num_offsets
        self.desc, self.schedule = desc, sched
        c = L.RolloutSched()
        c.steps, c.full_steps = T, sched.full_steps
        c.flags = L.SCHED_RECOMPUTE if sched.recompute else 0
        if sched.checkpoint_every is not None:
            c.flags |= L.SCHED_CHECKPOINT
            c.ckpt_every = sched.checkpoint_every
        self._keep = []
        if sched.offsets is not None and k > 0 and T > 0:
            flat = [v for o in sched.offsets for pair in o for v in pair]
            arr = (ctypes.c_int8 * len(flat))(*flat)
            self._keep.append(arr)
            c.offsets = ctypes.cast(arr, ctypes.c_void_p)
        if T > 0:
            fr = (ctypes.c_float * T)(*sched.fire_rates)
            self._keep.append(fr)
            c.fire_rate = ctypes.cast(fr, ctypes.c_void_p)
            if sched.gains is not None:
                mg = (ctypes.c_float * T)(*sched.gains)
                self._keep.append(mg)
                c.message_gain = ctypes.cast(mg, ctypes.c_void_p)
        c.nsteps = _ptr(sched.nsteps)
        c.fire = _ptr(sched.fire)
        self.c = c

    def _sizes(self, fn):
        return _sized(fn(ctypes.byref(self.desc), ctypes.byref(self.c)), "rollout shape", self.desc)

    def forward(self, weights, x, want_tape: bool):
        """(x_final, tape or None).  ``want_tape=False`` is the no-grad form of the same schedule."""
        lib = L.load()
        out = torch.empty_like(x)
        tape = _tape(self, x.device) if want_tape else None
        ws = torch.empty(self._sizes(lib.gnca_rollout_fwd_workspace_bytes), dtype=torch.uint8, device=x.device)
        rc = lib.gnca_rollout_fwd_f32(ctypes.byref(self.desc), ctypes.byref(weights), ctypes.byref(self.c),
                                      x.data_ptr(), out.data_ptr(), _ptr(tape), 0 if tape is None else tape.numel(),
                                      ws.data_ptr(), ws.numel(), stream_ptr(x.device))
        L.check(rc, "gnca_rollout_fwd_f32")
        return out, tape

    def memory(self) -> dict:
        """Bytes of the tape and of the two workspaces of this schedule, from the three host-only size
        queries: no GPU is touched."""
        lib = L.load()
        return {"tape": lib.gnca_rollout_tape_bytes(ctypes.byref(self.desc), ctypes.byref(self.c)),
                "forward_workspace": self._sizes(lib.gnca_rollout_fwd_workspace_bytes),
                "backward_workspace": self._sizes(lib.gnca_rollout_bwd_workspace_bytes)}

    def forward_taps(self, weights, taps: "RolloutTaps", x, want_tape: bool):
        """(x_final, tape or None, losses [R,B], alive_count [B] or None): ``forward`` that also writes
        the losses of the tapped states as they are produced (``gnca_rollout_fwd_taps``), so it serves
        a checkpointed tape, which holds few of them, and the no-grad form, which has no tape."""
        fn = _entry("gnca_rollout_fwd_taps")
        lib = L.load()
        B, dev = self.desc.B, x.device
        out = torch.empty_like(x)
        tape = _tape(self, dev) if want_tape else None
        losses = torch.empty(taps.c.n, B, dtype=torch.float32, device=dev)
        alive = torch.empty(B, dtype=torch.int32, device=dev) if taps.c.kind == L.TAP_MASKED else None
        ws = torch.empty(self._sizes(lib.gnca_rollout_fwd_workspace_bytes), dtype=torch.uint8, device=dev)
        taps.c.stream = stream_ptr(dev)
        rc = fn(ctypes.byref(self.desc), ctypes.byref(weights), ctypes.byref(self.c), ctypes.byref(taps.c),
                x.data_ptr(), out.data_ptr(), _ptr(tape), 0 if tape is None else tape.numel(), losses.data_ptr(),
                _ptr(alive), ws.data_ptr(), ws.numel())
        L.check(rc, "gnca_rollout_fwd_taps")
        return out, tape, losses, alive

    def backward(self, weights, tape, gy, want: dict | None = None, out: dict | None = None):
        """(gx, {name: grad}) of the rollout that recorded ``tape`` (``want`` / ``out`` as in
        ``step_backward``)."""
        lib = L.load()
        gy = _dev_f32(gy, "grad_output")
        gx = torch.empty_like(gy)
        g, grads = _grad_buffers(want, out, gy.device)
        ws = torch.empty(self._sizes(lib.gnca_rollout_bwd_workspace_bytes), dtype=torch.uint8, device=gy.device)
        rc = lib.gnca_rollout_bwd_f32(ctypes.byref(self.desc), ctypes.byref(weights), ctypes.byref(self.c),
                                      tape.data_ptr(), tape.numel(), gy.data_ptr(), gx.data_ptr(), ctypes.byref(g),
                                      ws.data_ptr(), ws.numel(), stream_ptr(gy.device))
        L.check(rc, "gnca_rollout_bwd_f32")
        return gx, grads

    # -----------------------------------------------------------------------------------------
    # taps: losses of intermediate states read from the tape (gnca_rollout_tap_loss) and the BPTT
    # that adds their gradients between two steps (gnca_rollout_bwd_taps)
    # -----------------------------------------------------------------------------------------
    def tap_losses(self, taps: "RolloutTaps", tape, x_final):
        """(losses [R,B], alive_count [B] or None) of the tapped states of the rollout that recorded
        ``tape`` and returned ``x_final``."""
        fn = _entry("gnca_rollout_tap_loss")
        B, dev = self.desc.B, x_final.device
        losses = torch.empty(taps.c.n, B, dtype=torch.float32, device=dev)
        alive = torch.empty(B, dtype=torch.int32, device=dev) if taps.c.kind == L.TAP_MASKED else None
        taps.c.stream = stream_ptr(dev)
        rc = fn(ctypes.byref(self.desc), ctypes.byref(self.c), ctypes.byref(taps.c), tape.data_ptr(), tape.numel(),
                x_final.data_ptr(), losses.data_ptr(), _ptr(alive))
        L.check(rc, "gnca_rollout_tap_loss")
        return losses, alive

    def backward_taps(self, weights, taps: "RolloutTaps", tape, x_final, gy, g_losses, alive,
                      want: dict | None = None, out: dict | None = None):
        """(gx, {name: grad}) of ``sum(g_losses * losses) + sum(gy * x_final)``; either cotangent may be
        None (not both).  ``want`` / ``out`` as in ``backward``."""
        fn = _entry("gnca_rollout_bwd_taps")
        if gy is None and g_losses is None:
            raise ValueError("backward_taps needs gy, g_losses or both")
        dev = x_final.device
        gy = None if gy is None else _dev_f32(gy, "grad_output")
        if g_losses is not None:
            g_losses = _dev_f32(g_losses, "grad_losses")
            if tuple(g_losses.shape) != (taps.c.n, self.desc.B):
                raise ValueError(f"grad_losses must be [{taps.c.n},{self.desc.B}], got {tuple(g_losses.shape)}")
        gx = torch.empty_like(x_final)
        g, grads = _grad_buffers(want, out, dev)
        ws = torch.empty(self._sizes(L.load().gnca_rollout_bwd_workspace_bytes), dtype=torch.uint8, device=dev)
        taps.c.stream = stream_ptr(dev)
        rc = fn(ctypes.byref(self.desc), ctypes.byref(weights), ctypes.byref(self.c), ctypes.byref(taps.c),
                tape.data_ptr(), tape.numel(), x_final.data_ptr(), _ptr(gy), _ptr(g_losses), _ptr(alive),
                gx.data_ptr(), ctypes.byref(g), ws.data_ptr(), ws.numel())
        L.check(rc, "gnca_rollout_bwd_taps")
        return gx, grads


TAP_KINDS = {"premult": L.TAP_PREMULT, "masked": L.TAP_MASKED}


class RolloutTaps:
    """The taps of one ``rollout_objective`` call: the C struct with its host step list and the device
    target kept alive.  ``record``: the tapped step indices (``expand_record``); ``kind``: a key of
    ``TAP_KINDS``; ``knobs``: (alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb) of the masked kind;
    ``target``: float32 [B or 1,4,H,W] on the state's device, contiguous."""

    def __init__(self, desc: L.StepDesc, record: list, kind: str, knobs, target: torch.Tensor):
        if not record:
            raise ValueError("a rollout objective needs at least one tapped step")
        c = L.RolloutTaps()
        c.n = len(record)
        arr = _records(record)
        c.steps = ctypes.cast(arr, ctypes.c_void_p)
        c.kind = TAP_KINDS[kind]
        c.masked.B, c.masked.H, c.masked.W = desc.B, desc.H, desc.W
        if knobs is not None:
            c.masked.alpha_thr, c.masked.lam_area, c.masked.lam_bg_alpha, c.masked.lam_bg_rgb = knobs
        c.target = target.data_ptr()
        c.target_bstride = 0 if target.shape[0] == 1 else target.stride(0)
        self.c, self.record, self._keep = c, list(record), (arr, target)


# ---------------------------------------------------------------------------------------------
# Forward-mode tangent (gnca_step_tangent / gnca_rollout_tangent)
# ---------------------------------------------------------------------------------------------
ZERO_PAD_TANGENT = ("the tangent of the zero-padded shift is not implemented: its offset weights depend on the "
                    "state through the pooled logits, so its tangent needs a second reduction pass over v; "
                    "build the model with graph_zero_padded_shift=False (torus mode)")


def check_tangent_desc(flags: int, num_offsets: int) -> None:
    """ValueError for what the tangent entry points refuse, before anything is drawn or launched."""
    if (flags & L.GRAPH) and (flags & L.ZERO_PAD_SHIFT) and num_offsets > 0:
        raise ValueError(ZERO_PAD_TANGENT)


# the parameters a direction may perturb (state_dict name -> gnca_weights field): GRAD_FIELDS without the query,
# key and scaling entries, whose directions have exactly zero effect in torus mode
DIRECTION_FIELDS = {"update_net.0.weight": "w1", "update_net.0.bias": "b1", "update_net.2.weight": "w2",
                    "norm.weight": "gn_weight", "norm.bias": "gn_bias",
                    "graph.msg_proj.weight": "wm", "graph.msg_proj.bias": "bm"}


def step_tangent(desc, weights, x, v, fire=None, active=None, ws=None, dweights=None):
    """One step and its Jacobian-vector product: (x_out, v_out), x_out bitwise ``step``'s.  ``dweights``: a
    ``Weights`` struct holding a parameter direction (``gnca_step_tangent_params``)."""
    fn = _entry("gnca_step_tangent" if dweights is None else "gnca_step_tangent_params")
    lib = L.load()
    x_out, v_out = torch.empty_like(x), torch.empty_like(v)
    if ws is None:
        ws = _sized(lib.gnca_step_tangent_workspace_bytes(ctypes.byref(desc)), "tangent step", desc, x.device,
                    "; torus mode")
    act = _active_u8(active, desc.B, x.device)
    dw = () if dweights is None else (ctypes.byref(dweights),)
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), *dw, x.data_ptr(), _ptr(fire), _ptr(act), v.data_ptr(),
            x_out.data_ptr(), v_out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(x.device))
    L.check(rc, "gnca_step_tangent" if dweights is None else "gnca_step_tangent_params")
    return x_out, v_out


def rollout_tangent(call: "RolloutCall", weights, x, v, record: list, renormalize: bool, dweights=None):
    """(x_final, v_final, log_norm float64 [R,B]) of the schedule bound in ``call``.  ``dweights``: a ``Weights``
    struct holding a parameter direction (``gnca_rollout_tangent_params``)."""
    fn = _entry("gnca_rollout_tangent" if dweights is None else "gnca_rollout_tangent_params")
    lib = L.load()
    desc, dev = call.desc, x.device
    a = L.TangentArgs()
    a.num_records = len(record)
    arr = _records(record)
    a.record = ctypes.cast(arr, ctypes.c_void_p) if record else None
    a.flags = L.TANGENT_RENORM if renormalize else 0
    log_norm = torch.empty(len(record), desc.B, dtype=torch.float64, device=dev)
    a.log_norm = log_norm.data_ptr() if record else None
    a.stream = stream_ptr(dev)
    n = lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(desc), ctypes.byref(call.c), ctypes.byref(a))
    ws = _sized(n, "tangent rollout", desc, dev, "; torus mode")
    x_final, v_final = torch.empty_like(x), torch.empty_like(v)
    dw = () if dweights is None else (ctypes.byref(dweights),)
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), *dw, ctypes.byref(call.c), ctypes.byref(a), x.data_ptr(),
            v.data_ptr(), x_final.data_ptr(), v_final.data_ptr(), ws.data_ptr(), ws.numel())
    L.check(rc, "gnca_rollout_tangent" if dweights is None else "gnca_rollout_tangent_params")
    return x_final, v_final, log_norm


# ---------------------------------------------------------------------------------------------
# A block of K tangents (gnca_tangent_qr / gnca_rollout_tangent_block)
# ---------------------------------------------------------------------------------------------
def tangent_qr(v, want_r: bool = True, ws=None):
    """The thin QR of the block ``v`` [K,B,...] (float32, contiguous, on the GPU), IN PLACE: ``v`` becomes Q.
    Returns (r float64 [B,K,K] or None, log_diag float64 [B,K], ws); the workspace begins with the Gram
    partials, float64 [B][nchunk][K(K+1)/2] (include/gnca.h)."""
    fn = _entry("gnca_tangent_qr")
    lib = L.load()
    K, B = v.shape[0], v.shape[1]
    n = v[0, 0].numel()
    if ws is None:
        nb = lib.gnca_tangent_qr_workspace_bytes(K, B, n)
        if nb == 0:
            raise L.GncaError(f"gnca_tangent_qr: no workspace for K={K} B={B} n={n} "
                              f"(1 <= K <= {L.TANGENT_MAX_DIRS}, B >= 1, n >= 1)")
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
    r = torch.empty(B, K, K, dtype=torch.float64, device=v.device) if want_r else None
    log_diag = torch.empty(B, K, dtype=torch.float64, device=v.device)
    rc = fn(K, B, n, v.data_ptr(), _ptr(r), log_diag.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(v.device))
    L.check(rc, "gnca_tangent_qr")
    return r, log_diag, ws


def rollout_tangent_block(call: "RolloutCall", weights, x, v, record: list, orthonormalize: bool, dweights=None):
    """(x_final, v_final [K,B,C,H,W], log_r float64 [R,B,K]) of the schedule bound in ``call``.  ``dweights``: K
    ``Weights`` structs, direction j's parameter direction (``gnca_rollout_tangent_block_params``)."""
    fn = _entry("gnca_rollout_tangent_block" if dweights is None else "gnca_rollout_tangent_block_params")
    lib = L.load()
    desc, dev = call.desc, x.device
    K = v.shape[0]
    a = L.TangentBlockArgs()
    a.num_dirs = K
    a.num_records = len(record)
    arr = _records(record)
    a.record = ctypes.cast(arr, ctypes.c_void_p) if record else None
    a.flags = L.TBLOCK_ORTHO if orthonormalize else 0
    log_r = torch.empty(len(record), desc.B, K, dtype=torch.float64, device=dev)
    a.log_r = log_r.data_ptr() if record else None
    a.stream = stream_ptr(dev)
    n = lib.gnca_rollout_tangent_block_workspace_bytes(ctypes.byref(desc), ctypes.byref(call.c), ctypes.byref(a))
    ws = _sized(n, "tangent block rollout", desc, dev, "; torus mode", K=K)
    x_final, v_final = torch.empty_like(x), torch.empty_like(v)
    dw = ()
    if dweights is not None:
        if len(dweights) != K:
            raise ValueError(f"{len(dweights)} parameter directions for a block of {K} tangents")
        dw = ((L.Weights * K)(*dweights),)
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), *dw, ctypes.byref(call.c), ctypes.byref(a), x.data_ptr(),
            v.data_ptr(), x_final.data_ptr(), v_final.data_ptr(), ws.data_ptr(), ws.numel())
    L.check(rc, "gnca_rollout_tangent_block" if dweights is None else "gnca_rollout_tangent_block_params")
    return x_final, v_final, log_r


# ---------------------------------------------------------------------------------------------
# A forward-mode objective (gnca_rollout_objective_tangent): tap losses and their directional derivatives
# ---------------------------------------------------------------------------------------------
def rollout_objective_tangent(call: "RolloutCall", taps: "RolloutTaps", weights, x, v, K: int, dweights=None,
                              want_tangents: bool = False):
    """(x_final, losses float32 [R,B], dlosses float64 [R,K,B], v_final [K,B,C,H,W] or None) of the schedule
    bound in ``call``.  ``v``: the block [K,B,C,H,W] or None (zeros, made on the device); ``dweights``: K
    ``Weights`` structs or None."""
    fn = _entry("gnca_rollout_objective_tangent")
    lib = L.load()
    desc, dev = call.desc, x.device
    R, B = taps.c.n, desc.B
    if dweights is not None and len(dweights) != K:
        raise ValueError(f"{len(dweights)} parameter directions for a block of {K} tangents")
    taps.c.stream = stream_ptr(dev)
    n = lib.gnca_rollout_objective_tangent_workspace_bytes(ctypes.byref(desc), ctypes.byref(call.c),
                                                           ctypes.byref(taps.c), K)
    ws = _sized(n, "objective tangent rollout", desc, dev, "; torus mode", K=K)
    x_final = torch.empty_like(x)
    v_final = torch.empty((K,) + tuple(x.shape), dtype=torch.float32, device=dev) if want_tangents else None
    losses = torch.empty(R, B, dtype=torch.float32, device=dev)
    dlosses = torch.empty(R, K, B, dtype=torch.float64, device=dev)
    alive = torch.empty(B, dtype=torch.int32, device=dev) if taps.c.kind == L.TAP_MASKED else None
    dw = None if dweights is None else (L.Weights * K)(*dweights)
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), dw, ctypes.byref(call.c), ctypes.byref(taps.c), K,
            x.data_ptr(), _ptr(v), x_final.data_ptr(), _ptr(v_final), losses.data_ptr(), dlosses.data_ptr(),
            _ptr(alive), ws.data_ptr(), ws.numel())
    L.check(rc, "gnca_rollout_objective_tangent")
    return x_final, losses, dlosses, v_final


# ---------------------------------------------------------------------------------------------
# Gauss-Newton products (gnca_rollout_gn_fwd / gnca_rollout_gn_bwd): the tangent forward that leaves a tape and
# the curvature fields of the taps, and the BPTT that injects them
# ---------------------------------------------------------------------------------------------
def gn_memory(call: "RolloutCall", taps: "RolloutTaps") -> dict:
    """Bytes of one Gauss-Newton product of the schedule bound in ``call``, from the host-only size queries."""
    fn = _entry("gnca_rollout_gn_fwd_workspace_bytes")
    lib = L.load()
    desc = call.desc
    n = _sized(fn(ctypes.byref(desc), ctypes.byref(call.c), ctypes.byref(taps.c)), "Gauss-Newton rollout", desc,
               extra="; torus mode; a states-only tape")
    return {"tape": lib.gnca_rollout_tape_bytes(ctypes.byref(desc), ctypes.byref(call.c)),
            "forward_workspace": n,
            "backward_workspace": call._sizes(lib.gnca_rollout_bwd_workspace_bytes),
            "fields": taps.c.n * desc.B * 4 * desc.H * desc.W * 4}


def rollout_gn_forward(call: "RolloutCall", taps: "RolloutTaps", weights, x, v, dweights=None):
    """(x_final, tape, fields float32 [R,B,4,H,W], losses float32 [R,B], dlosses float64 [R,B], quad float64 [R,B])
    of the schedule bound in ``call`` (``recompute=True``).  ``v``: [B,C,H,W] or None (zeros, made on the device);
    ``dweights``: a ``Weights`` struct holding the parameter direction, or None."""
    fn = _entry("gnca_rollout_gn_fwd")
    desc, dev = call.desc, x.device
    R, B = taps.c.n, desc.B
    taps.c.stream = stream_ptr(dev)
    mem = gn_memory(call, taps)
    ws = torch.empty(mem["forward_workspace"], dtype=torch.uint8, device=dev)
    tape = torch.empty(max(mem["tape"], 256), dtype=torch.uint8, device=dev)
    x_final = torch.empty_like(x)
    fields = torch.empty(R, B, 4, desc.H, desc.W, dtype=torch.float32, device=dev)
    losses = torch.empty(R, B, dtype=torch.float32, device=dev)
    dlosses = torch.empty(R, B, dtype=torch.float64, device=dev)
    quad = torch.empty(R, B, dtype=torch.float64, device=dev)
    alive = torch.empty(B, dtype=torch.int32, device=dev) if taps.c.kind == L.TAP_MASKED else None
    rc = fn(ctypes.byref(desc), ctypes.byref(weights), None if dweights is None else ctypes.byref(dweights),
            ctypes.byref(call.c), ctypes.byref(taps.c), x.data_ptr(), _ptr(v), x_final.data_ptr(), tape.data_ptr(),
            tape.numel(), fields.data_ptr(), losses.data_ptr(), dlosses.data_ptr(), quad.data_ptr(), _ptr(alive),
            ws.data_ptr(), ws.numel())
    L.check(rc, "gnca_rollout_gn_fwd")
    return x_final, tape, fields, losses, dlosses, quad


def rollout_gn_backward(call: "RolloutCall", taps: "RolloutTaps", weights, tape, fields, scale: list, like,
                        want: dict | None = None):
    """(gx, {name: grad}) of the BPTT that injects ``scale[r] * fields[r]`` at tap r on the tape of
    ``rollout_gn_forward``.  ``scale``: R host numbers; ``like``: a tensor of the state's shape; ``want`` as in
    ``RolloutCall.backward``."""
    fn = _entry("gnca_rollout_gn_bwd")
    dev = fields.device
    if len(scale) != taps.c.n:
        raise ValueError(f"{len(scale)} scales for {taps.c.n} taps")
    sc = (ctypes.c_float * len(scale))(*scale)
    gx = torch.empty_like(like)
    g, grads = _grad_buffers(want, None, dev)
    ws = torch.empty(call._sizes(L.load().gnca_rollout_bwd_workspace_bytes), dtype=torch.uint8, device=dev)
    taps.c.stream = stream_ptr(dev)
    rc = fn(ctypes.byref(call.desc), ctypes.byref(weights), ctypes.byref(call.c), ctypes.byref(taps.c),
            tape.data_ptr(), tape.numel(), fields.data_ptr(), sc, gx.data_ptr(), ctypes.byref(g), ws.data_ptr(),
            ws.numel())
    L.check(rc, "gnca_rollout_gn_bwd")
    return gx, grads
