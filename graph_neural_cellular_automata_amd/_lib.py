"""ctypes binding of libgnca.so (include/gnca.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950) and
loaded from this package directory.  There is no fallback: if the library is missing or does
not match the ABI version, every op raises.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  — load torch's HIP runtime first; libgnca.so binds to it by soname

_HERE = os.path.dirname(os.path.abspath(__file__))
# GNCA_LIB_PATH: an alternative build of the same library (A/B measurement runs only)
LIB_PATH = os.environ.get("GNCA_LIB_PATH") or os.path.join(_HERE, "libgnca.so")

ABI_VERSION = 5
MAX_OFFSETS = 128

GRAPH = 1 << 0
USE_GROUPNORM = 1 << 1
HIDDEN_ONLY = 1 << 2
ALIVE_TO_ALIVE = 1 << 3
ZERO_PAD_SHIFT = 1 << 4
ATTENTION = 1 << 5

FIRE_NONE = 0
FIRE_RAND_F32 = 1
FIRE_MASK_U8 = 2
FIRE_HASH = 3


class StepDesc(ctypes.Structure):
    """Mirror of gnca_step_desc (include/gnca.h)."""
    _fields_ = [
        ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("hidden", ctypes.c_int32), ("d_model", ctypes.c_int32), ("num_offsets", ctypes.c_int32),
        ("fire_mode", ctypes.c_int32), ("flags", ctypes.c_uint32),
        ("update_gain", ctypes.c_float), ("alpha_thr", ctypes.c_float),
        ("graph_alpha_thr", ctypes.c_float),
        ("message_gain", ctypes.c_float), ("gn_eps", ctypes.c_float), ("fire_rate", ctypes.c_float),
        ("rng_seed", ctypes.c_uint64), ("rng_step", ctypes.c_int64), ("sample_base", ctypes.c_int64),
        ("offsets", ctypes.c_int8 * (2 * MAX_OFFSETS)),
    ]


class Weights(ctypes.Structure):
    """Mirror of gnca_weights (include/gnca.h): device pointers in reference layouts."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "perception", "w1", "b1", "w2", "gn_weight", "gn_bias",
        "wq", "bq", "wk", "bk", "wm", "bm", "scaling")]


class Grads(ctypes.Structure):
    """Mirror of gnca_grads (include/gnca.h): device output pointers in reference layouts."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "w1", "b1", "w2", "gn_weight", "gn_bias", "wq", "bq", "wk", "bk", "wm", "bm", "scaling")]


class RolloutSched(ctypes.Structure):
    """Mirror of gnca_rollout_sched (include/gnca.h): offsets / fire_rate / message_gain are HOST
    arrays read during the call, nsteps / fire are device pointers; ckpt_every (read only with
    SCHED_CHECKPOINT) sits in what was the padding after flags."""
    _fields_ = [("steps", ctypes.c_int32), ("full_steps", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("ckpt_every", ctypes.c_int32), ("offsets", ctypes.c_void_p), ("fire_rate", ctypes.c_void_p),
                ("message_gain", ctypes.c_void_p), ("nsteps", ctypes.c_void_p), ("fire", ctypes.c_void_p)]


SCHED_RECOMPUTE = 1 << 0
SCHED_CHECKPOINT = 1 << 1   # the tape keeps every ckpt_every-th state; the backward re-runs segments


class TraceArgs(ctypes.Structure):
    """Mirror of gnca_trace_args (include/gnca.h): offsets / record are HOST arrays read during the
    call, frames / attn are device pointers."""
    _fields_ = [("steps", ctypes.c_int32), ("num_records", ctypes.c_int32),
                ("frame_channels", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("offsets", ctypes.c_void_p), ("record", ctypes.c_void_p),
                ("frames", ctypes.c_void_p), ("attn", ctypes.c_void_p)]


class TraceMetrics(ctypes.Structure):
    """Mirror of gnca_trace_metrics (include/gnca.h): device pointers and the target's sample stride."""
    _fields_ = [("target", ctypes.c_void_p), ("target_bstride", ctypes.c_int64), ("out", ctypes.c_void_p)]


DIAG_FIELDS = ("magnitude", "groups", "per_offset", "raw", "attention", "sender_union", "receiver", "weights")


class GraphDiagOut(ctypes.Structure):
    """Mirror of gnca_graph_diag_out (include/gnca.h): device output pointers, NULL = skipped."""
    _fields_ = [(n, ctypes.c_void_p) for n in DIAG_FIELDS]


VITALS_FIELDS = ("alive", "mature", "alpha_sum", "mass", "cy", "cx", "y0", "y1", "x0", "x1", "max_abs",
                 "nonfinite", "hidden_rms")
VITALS_BAND_ROWS, VITALS_TILE_COLS = 8, 256   # the tile of one sample that one workgroup of gnca_state_vitals
                                              # reads (include/gnca.h)


class TraceVitals(ctypes.Structure):
    """Mirror of gnca_trace_vitals (include/gnca.h): the threshold and the device output [R,B,13]."""
    _fields_ = [("alpha_thr", ctypes.c_float), ("out", ctypes.c_void_p)]


class DamageDesc(ctypes.Structure):
    """Mirror of gnca_damage_desc (include/gnca.h)."""
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("size", ctypes.c_int32), ("p", ctypes.c_float),
                ("alpha_thr", ctypes.c_float), ("softness", ctypes.c_float), ("sigma", ctypes.c_float)]


class MaskedLossDesc(ctypes.Structure):
    """Mirror of gnca_masked_loss_desc (include/gnca.h)."""
    _fields_ = [("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("alpha_thr", ctypes.c_float), ("lam_area", ctypes.c_float), ("lam_bg_alpha", ctypes.c_float),
                ("lam_bg_rgb", ctypes.c_float), ("close_thresh", ctypes.c_float), ("close_steps", ctypes.c_int32)]


TAP_PREMULT, TAP_MASKED = 0, 1
TAP_CHUNK = 32   # taps per launch of the tap loss kernel (include/gnca.h)


class RolloutTaps(ctypes.Structure):
    """Mirror of gnca_rollout_taps (include/gnca.h): steps is a HOST array read during the call, target a
    device pointer; the stream travels in the descriptor."""
    _fields_ = [("n", ctypes.c_int32), ("steps", ctypes.c_void_p), ("kind", ctypes.c_int32),
                ("masked", MaskedLossDesc), ("target", ctypes.c_void_p), ("target_bstride", ctypes.c_int64),
                ("stream", ctypes.c_void_p)]


TANGENT_RENORM = 1 << 0   # gnca_tangent_args.flags: renormalise the tangent at every recorded step


class TangentArgs(ctypes.Structure):
    """Mirror of gnca_tangent_args (include/gnca.h): record is a HOST array read during the call, log_norm
    a device pointer; the stream travels in the struct."""
    _fields_ = [("num_records", ctypes.c_int32), ("record", ctypes.c_void_p), ("flags", ctypes.c_uint32),
                ("log_norm", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


TANGENT_MAX_DIRS = 16          # GNCA_TANGENT_MAX_DIRS: directions of a tangent block
TANGENT_QR_CHUNK = 4096        # GNCA_TANGENT_QR_CHUNK: elements of one sample per Gram partial
TBLOCK_ORTHO = 1 << 0          # gnca_tangent_block_args.flags: replace the block by Q at every recorded step


class TangentBlockArgs(ctypes.Structure):
    """Mirror of gnca_tangent_block_args (include/gnca.h): record is a HOST array read during the call, log_r a
    device pointer; the stream travels in the struct."""
    _fields_ = [("num_dirs", ctypes.c_int32), ("num_records", ctypes.c_int32), ("record", ctypes.c_void_p),
                ("flags", ctypes.c_uint32), ("log_r", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


OPTIM_MAX_TENSORS = 24
OPTIM_ONE_LAUNCH_MAX = 65536   # elements a one-launch gnca_optim_step call may hold (include/gnca.h)
OPTIM_POLICY_NONE, OPTIM_POLICY_NORMALIZE, OPTIM_POLICY_CLIP = 0, 1, 2
OPTIM_SUMSQ, OPTIM_UPDATE = 1, 2


class OptimTensor(ctypes.Structure):
    """Mirror of gnca_optim_tensor (include/gnca.h): device pointers and the host-computed knobs."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("lr", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("bias1", ctypes.c_double), ("bias2", ctypes.c_double)]


class OptimDesc(ctypes.Structure):
    """Mirror of gnca_optim_desc (include/gnca.h): passed by value to the kernels."""
    _fields_ = [("policy", ctypes.c_int32), ("num_tensors", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("sumsq_base", ctypes.c_int32), ("sumsq_count", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("sumsq", ctypes.c_void_p), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("max_norm", ctypes.c_double), ("norm_eps", ctypes.c_double),
                ("t", OptimTensor * OPTIM_MAX_TENSORS)]


LOSS_TANGENT_DIRS = 4    # GNCA_LOSS_TANGENT_DIRS: directions one workgroup of the loss tangent kernel serves
FGRAD_ACCUMULATE = 1 << 0


class ForwardGradTensor(ctypes.Structure):
    """Mirror of gnca_forward_grad_tensor (include/gnca.h): direction k of the tensor is at dir + k * dir_stride."""
    _fields_ = [("g", ctypes.c_void_p), ("dir", ctypes.c_void_p), ("dir_stride", ctypes.c_int64),
                ("numel", ctypes.c_int64)]


class ForwardGradDesc(ctypes.Structure):
    """Mirror of gnca_forward_grad_desc (include/gnca.h): passed by value to the kernels."""
    _fields_ = [("K", ctypes.c_int32), ("R", ctypes.c_int32), ("B", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("dlosses", ctypes.c_void_p), ("tap_weight", ctypes.c_void_p), ("scale", ctypes.c_double),
                ("coef", ctypes.c_void_p), ("num_tensors", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("t", ForwardGradTensor * OPTIM_MAX_TENSORS)]


class PoolCommitDesc(ctypes.Structure):
    """Mirror of gnca_pool_commit_desc (include/gnca.h)."""
    _fields_ = [("pool_slots", ctypes.c_int64), ("sample_elems", ctypes.c_int64), ("B", ctypes.c_int32),
                ("n_reset", ctypes.c_int32)]


RENDER_RGB, RENDER_RGBA = 0, 1
RENDER_BAND_ROWS = 8   # source rows one workgroup of gnca_render_u8 renders (include/gnca.h)
NORM_MAX, NORM_MINMAX = 0, 1


class RenderDesc(ctypes.Structure):
    """Mirror of gnca_render_desc (include/gnca.h): the stream travels in the descriptor."""
    _fields_ = [("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("upscale", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("alpha_thr", ctypes.c_float), ("src_nstride", ctypes.c_int64),
                ("stream", ctypes.c_void_p)]


class ColorizeDesc(ctypes.Structure):
    """Mirror of gnca_colorize_desc (include/gnca.h): the stream travels in the descriptor."""
    _fields_ = [("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("norm", ctypes.c_int32),
                ("stream", ctypes.c_void_p)]


DMG_SQUARE, DMG_CIRCLE, DMG_STRIPE_H, DMG_STRIPE_V = 0, 1, 2, 3
DMG_ALPHA_DROP, DMG_ALPHA_DROP_SOFT, DMG_SALT_PEPPER, DMG_GAUSSIAN, DMG_HIDDEN_NOISE = 4, 5, 6, 7, 8
DMG_STRIPES_AUTO = 9           # gnca_damage_policy only: the orientation is drawn
DMG_MAX_KINDS = 10
DMG_SCOPE_BATCH, DMG_SCOPE_SAMPLE = 0, 1
DMG_SHARED_SAMPLE = 0xFFFFFFFF
DMG_RNG_STREAMS = ("gate", "sample_gate", "kind", "size", "orient", "y", "x", "cell", "normal_u1", "normal_u2")


class DamagePolicyDesc(ctypes.Structure):
    """Mirror of gnca_damage_policy_desc (include/gnca.h): the stream travels in the descriptor."""
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("scope", ctypes.c_int32), ("prob", ctypes.c_float), ("per_sample_prob", ctypes.c_float),
                ("n_kinds", ctypes.c_int32), ("kinds", ctypes.c_int32 * DMG_MAX_KINDS),
                ("cum", ctypes.c_float * DMG_MAX_KINDS), ("size_min", ctypes.c_int32), ("size_max", ctypes.c_int32),
                ("stripe_width", ctypes.c_int32), ("alpha_thr", ctypes.c_float), ("alpha_dropout_p", ctypes.c_float),
                ("salt_pepper_p", ctypes.c_float), ("hidden_sigma", ctypes.c_float),
                ("gaussian_softness", ctypes.c_float), ("seed", ctypes.c_uint64), ("event", ctypes.c_int64),
                ("sample_base", ctypes.c_int64), ("stream", ctypes.c_void_p)]


EXPORTS = ("gnca_abi_version", "gnca_status_string", "gnca_last_hip_error",
           "gnca_workspace_bytes", "gnca_step_f32", "gnca_step_phases_f32", "gnca_message_f32",
           "gnca_perceive_f32", "gnca_rollout_f32", "gnca_bwd_workspace_bytes", "gnca_step_bwd_f32",
           "gnca_fire_mask_u8", "gnca_step_masked_f32", "gnca_damage_f32", "gnca_loss_premult_f32",
           "gnca_loss_premult_bwd_f32", "gnca_k1_variant", "gnca_rollout_stamped_f32",
           "gnca_rollout_ex_f32", "gnca_bb_variant", "gnca_rollout_tape_bytes",
           "gnca_rollout_fwd_workspace_bytes", "gnca_rollout_bwd_workspace_bytes",
           "gnca_rollout_fwd_f32", "gnca_rollout_bwd_f32", "gnca_attention_workspace_bytes",
           "gnca_attention_f32", "gnca_rollout_trace_workspace_bytes", "gnca_rollout_trace_f32",
           "gnca_image_metrics_workspace_bytes", "gnca_image_metrics_f32",
           "gnca_rollout_trace_metrics_workspace_bytes", "gnca_rollout_trace_metrics_f32",
           "gnca_loss_masked_f32", "gnca_loss_masked_bwd_f32", "gnca_loss_stability_workspace_bytes",
           "gnca_loss_stability_f32", "gnca_loss_stability_bwd_f32", "gnca_optim_step", "gnca_pool_commit",
           "gnca_graph_diag_workspace_bytes", "gnca_graph_diag", "gnca_rollout_trace_diag_workspace_bytes",
           "gnca_rollout_trace_diag", "gnca_render_u8", "gnca_colorize_u8", "gnca_damage_policy",
           "gnca_state_vitals_workspace_bytes", "gnca_state_vitals",
           "gnca_rollout_trace_vitals_workspace_bytes", "gnca_rollout_trace_vitals",
           "gnca_rollout_tap_loss", "gnca_rollout_bwd_taps", "gnca_rollout_fwd_taps",
           "gnca_step_tangent_workspace_bytes", "gnca_step_tangent",
           "gnca_rollout_tangent_workspace_bytes", "gnca_rollout_tangent",
           "gnca_tangent_qr_workspace_bytes", "gnca_tangent_qr",
           "gnca_rollout_tangent_block_workspace_bytes", "gnca_rollout_tangent_block",
           "gnca_k2_variant",
           "gnca_step_tangent_params", "gnca_rollout_tangent_params", "gnca_rollout_tangent_block_params",
           "gnca_loss_tangent", "gnca_rollout_objective_tangent_workspace_bytes", "gnca_rollout_objective_tangent",
           "gnca_forward_grad",
           "gnca_loss_curvature", "gnca_rollout_gn_fwd_workspace_bytes", "gnca_rollout_gn_fwd",
           "gnca_rollout_gn_bwd")

PHASE_K0, PHASE_K1, PHASE_K2 = 1, 2, 4
PHASE_ALL = 7
PHASE_ALIVE = 8   # rollout mode: K2 hands the next step's alive masks to K1 (include/gnca.h)
ROLLOUT_ALIVE_IN, ROLLOUT_ALIVE_OUT = 1, 2   # gnca_rollout_ex_f32 pieces (include/gnca.h)
ROLLOUT_PENDING_IN, ROLLOUT_PENDING_OUT = 4, 8   # fold rollouts: the last step handed over unfinished
ROLLOUT_FOLD = 16   # request the fold on the compact field too (include/gnca.h)
PHASE_COMPACT = 16   # rollout mode: K1 packs the live cells' dx per tile, K2 unpacks (include/gnca.h)

_lib = None


class GncaError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load libgnca.so (raises if absent or ABI-mismatched — there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise GncaError(
            f"libgnca.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950). The NCA step has no CPU fallback.")
    lib = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.gnca_abi_version.restype = ctypes.c_int
    lib.gnca_status_string.restype = ctypes.c_char_p
    lib.gnca_status_string.argtypes = [ctypes.c_int]
    lib.gnca_last_hip_error.restype = ctypes.c_int
    lib.gnca_workspace_bytes.restype = sz
    lib.gnca_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc)]
    lib.gnca_step_f32.restype = ctypes.c_int
    lib.gnca_step_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp, vp,
                                  vp, vp, sz, vp]
    lib.gnca_step_phases_f32.restype = ctypes.c_int
    lib.gnca_step_phases_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp,
                                         vp, vp, vp, sz, vp, ctypes.c_uint32]
    lib.gnca_message_f32.restype = ctypes.c_int
    lib.gnca_message_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp,
                                     vp, vp, sz, vp]
    lib.gnca_perceive_f32.restype = ctypes.c_int
    lib.gnca_perceive_f32.argtypes = [ctypes.c_int32] * 4 + [vp, vp, vp, vp]
    lib.gnca_rollout_f32.restype = ctypes.c_int
    lib.gnca_rollout_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                     ctypes.c_int32, vp, vp, vp, vp, vp, sz, vp]
    lib.gnca_rollout_ex_f32.restype = ctypes.c_int
    lib.gnca_rollout_ex_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                        ctypes.c_int32, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp]
    lib.gnca_rollout_stamped_f32.restype = ctypes.c_int
    lib.gnca_rollout_stamped_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                             ctypes.c_int32, vp, vp, vp, vp, vp, sz, vp,
                                             ctypes.c_int32, vp]
    lib.gnca_fire_mask_u8.restype = ctypes.c_int
    lib.gnca_fire_mask_u8.argtypes = [ctypes.POINTER(StepDesc), vp, vp]
    lib.gnca_bwd_workspace_bytes.restype = sz
    lib.gnca_bwd_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc)]
    lib.gnca_step_bwd_f32.restype = ctypes.c_int
    lib.gnca_step_bwd_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp, vp,
                                      vp, vp, ctypes.POINTER(Grads), vp, vp, sz, vp]
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    lib.gnca_loss_premult_f32.restype = ctypes.c_int
    lib.gnca_loss_premult_f32.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, vp]
    lib.gnca_loss_premult_bwd_f32.restype = ctypes.c_int
    lib.gnca_loss_premult_bwd_f32.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, vp, i64, vp]
    lib.gnca_damage_f32.restype = ctypes.c_int
    lib.gnca_damage_f32.argtypes = [ctypes.POINTER(DamageDesc), vp, vp, vp, vp]
    lib.gnca_k1_variant.restype = ctypes.c_int
    lib.gnca_k1_variant.argtypes = [ctypes.POINTER(StepDesc), ctypes.c_char_p, i32, ctypes.POINTER(ctypes.c_int32)]
    lib.gnca_bb_variant.restype = ctypes.c_int
    lib.gnca_bb_variant.argtypes = [ctypes.POINTER(StepDesc), ctypes.c_char_p, i32]
    lib.gnca_step_masked_f32.restype = ctypes.c_int
    lib.gnca_step_masked_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp, vp,
                                         vp, vp, sz, vp]
    for name in ("gnca_rollout_tape_bytes", "gnca_rollout_fwd_workspace_bytes",
                 "gnca_rollout_bwd_workspace_bytes"):
        getattr(lib, name).restype = sz
        getattr(lib, name).argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(RolloutSched)]
    lib.gnca_rollout_fwd_f32.restype = ctypes.c_int
    lib.gnca_rollout_fwd_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                         ctypes.POINTER(RolloutSched), vp, vp, vp, sz, vp, sz, vp]
    lib.gnca_rollout_bwd_f32.restype = ctypes.c_int
    lib.gnca_rollout_bwd_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                         ctypes.POINTER(RolloutSched), vp, sz, vp, vp,
                                         ctypes.POINTER(Grads), vp, sz, vp]
    v = lib.gnca_abi_version()
    if v == ABI_VERSION:   # (an older library lacks these symbols: report the version instead)
        lib.gnca_attention_workspace_bytes.restype = sz
        lib.gnca_attention_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc)]
        lib.gnca_attention_f32.restype = ctypes.c_int
        lib.gnca_attention_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp, vp, sz, vp]
        lib.gnca_rollout_trace_workspace_bytes.restype = sz
        lib.gnca_rollout_trace_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(TraceArgs)]
        lib.gnca_rollout_trace_f32.restype = ctypes.c_int
        lib.gnca_rollout_trace_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                               ctypes.POINTER(TraceArgs), vp, vp, vp, sz, vp]
        lib.gnca_image_metrics_workspace_bytes.restype = sz
        lib.gnca_image_metrics_workspace_bytes.argtypes = [i32, i32, i32]
        lib.gnca_image_metrics_f32.restype = ctypes.c_int
        lib.gnca_image_metrics_f32.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, vp, sz, vp]
        lib.gnca_rollout_trace_metrics_workspace_bytes.restype = sz
        lib.gnca_rollout_trace_metrics_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(TraceArgs),
                                                                   ctypes.POINTER(TraceMetrics)]
        lib.gnca_rollout_trace_metrics_f32.restype = ctypes.c_int
        lib.gnca_rollout_trace_metrics_f32.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                       ctypes.POINTER(TraceArgs), ctypes.POINTER(TraceMetrics),
                                                       vp, vp, vp, sz, vp]
        if hasattr(lib, "gnca_loss_masked_f32"):   # (a version-5 library from before these additions lacks them)
            md = ctypes.POINTER(MaskedLossDesc)
            lib.gnca_loss_masked_f32.restype = ctypes.c_int
            lib.gnca_loss_masked_f32.argtypes = [md, vp, i64, vp, i64, vp, vp, vp, vp]
            lib.gnca_loss_masked_bwd_f32.restype = ctypes.c_int
            lib.gnca_loss_masked_bwd_f32.argtypes = [md, vp, i64, vp, i64, vp, vp, vp, i64, vp]
            lib.gnca_loss_stability_workspace_bytes.restype = sz
            lib.gnca_loss_stability_workspace_bytes.argtypes = [i32]
            lib.gnca_loss_stability_f32.restype = ctypes.c_int
            lib.gnca_loss_stability_f32.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, sz, vp]
            lib.gnca_loss_stability_bwd_f32.restype = ctypes.c_int
            lib.gnca_loss_stability_bwd_f32.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp]
        if hasattr(lib, "gnca_optim_step"):   # (likewise: loss._entry-style callers name what is missing)
            lib.gnca_optim_step.restype = ctypes.c_int
            lib.gnca_optim_step.argtypes = [ctypes.POINTER(OptimDesc), vp]
            lib.gnca_pool_commit.restype = ctypes.c_int
            lib.gnca_pool_commit.argtypes = [ctypes.POINTER(PoolCommitDesc), vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(lib, "gnca_graph_diag"):   # (likewise)
            do = ctypes.POINTER(GraphDiagOut)
            lib.gnca_graph_diag_workspace_bytes.restype = sz
            lib.gnca_graph_diag_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc)]
            lib.gnca_graph_diag.restype = ctypes.c_int
            lib.gnca_graph_diag.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, do, vp, sz, vp]
            lib.gnca_rollout_trace_diag_workspace_bytes.restype = sz
            lib.gnca_rollout_trace_diag_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(TraceArgs),
                                                                    ctypes.POINTER(TraceMetrics)]
            lib.gnca_rollout_trace_diag.restype = ctypes.c_int
            lib.gnca_rollout_trace_diag.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                    ctypes.POINTER(TraceArgs), ctypes.POINTER(TraceMetrics), do,
                                                    vp, vp, vp, sz, vp]
        if hasattr(lib, "gnca_render_u8"):   # (likewise)
            lib.gnca_render_u8.restype = ctypes.c_int
            lib.gnca_render_u8.argtypes = [ctypes.POINTER(RenderDesc), vp, vp]
            lib.gnca_colorize_u8.restype = ctypes.c_int
            lib.gnca_colorize_u8.argtypes = [ctypes.POINTER(ColorizeDesc), vp, vp, vp]
        if hasattr(lib, "gnca_damage_policy"):   # (likewise)
            lib.gnca_damage_policy.restype = ctypes.c_int
            lib.gnca_damage_policy.argtypes = [ctypes.POINTER(DamagePolicyDesc), vp, vp, vp, vp, vp]
        if hasattr(lib, "gnca_state_vitals"):   # (likewise)
            do = ctypes.POINTER(GraphDiagOut)
            lib.gnca_state_vitals_workspace_bytes.restype = sz
            lib.gnca_state_vitals_workspace_bytes.argtypes = [i32, i32, i32, i32]
            lib.gnca_state_vitals.restype = ctypes.c_int
            lib.gnca_state_vitals.argtypes = [i32, i32, i32, i32, vp, i64, ctypes.c_float, vp, vp, sz, vp]
            lib.gnca_rollout_trace_vitals_workspace_bytes.restype = sz
            lib.gnca_rollout_trace_vitals_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc),
                                                                      ctypes.POINTER(TraceArgs),
                                                                      ctypes.POINTER(TraceMetrics), do]
            lib.gnca_rollout_trace_vitals.restype = ctypes.c_int
            lib.gnca_rollout_trace_vitals.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                      ctypes.POINTER(TraceArgs), ctypes.POINTER(TraceMetrics), do,
                                                      ctypes.POINTER(TraceVitals), vp, vp, vp, sz, vp]
        if hasattr(lib, "gnca_rollout_tap_loss"):   # (likewise)
            tp = ctypes.POINTER(RolloutTaps)
            lib.gnca_rollout_tap_loss.restype = ctypes.c_int
            lib.gnca_rollout_tap_loss.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(RolloutSched), tp, vp, sz,
                                                  vp, vp, vp]
            lib.gnca_rollout_bwd_taps.restype = ctypes.c_int
            lib.gnca_rollout_bwd_taps.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                  ctypes.POINTER(RolloutSched), tp, vp, sz, vp, vp, vp, vp, vp,
                                                  ctypes.POINTER(Grads), vp, sz]
        if hasattr(lib, "gnca_rollout_fwd_taps"):   # (likewise)
            lib.gnca_rollout_fwd_taps.restype = ctypes.c_int
            lib.gnca_rollout_fwd_taps.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                  ctypes.POINTER(RolloutSched), ctypes.POINTER(RolloutTaps),
                                                  vp, vp, vp, sz, vp, vp, vp, sz]
        if hasattr(lib, "gnca_step_tangent"):   # (likewise)
            ta = ctypes.POINTER(TangentArgs)
            lib.gnca_step_tangent_workspace_bytes.restype = sz
            lib.gnca_step_tangent_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc)]
            lib.gnca_step_tangent.restype = ctypes.c_int
            lib.gnca_step_tangent.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights), vp, vp, vp, vp, vp,
                                              vp, vp, sz, vp]
            lib.gnca_rollout_tangent_workspace_bytes.restype = sz
            lib.gnca_rollout_tangent_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc),
                                                                 ctypes.POINTER(RolloutSched), ta]
            lib.gnca_rollout_tangent.restype = ctypes.c_int
            lib.gnca_rollout_tangent.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                 ctypes.POINTER(RolloutSched), ta, vp, vp, vp, vp, vp, sz]
        if hasattr(lib, "gnca_tangent_qr"):   # (likewise)
            tb = ctypes.POINTER(TangentBlockArgs)
            lib.gnca_tangent_qr_workspace_bytes.restype = sz
            lib.gnca_tangent_qr_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
            lib.gnca_tangent_qr.restype = ctypes.c_int
            lib.gnca_tangent_qr.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, vp, vp, vp, vp, sz, vp]
            lib.gnca_rollout_tangent_block_workspace_bytes.restype = sz
            lib.gnca_rollout_tangent_block_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc),
                                                                       ctypes.POINTER(RolloutSched), tb]
            lib.gnca_rollout_tangent_block.restype = ctypes.c_int
            lib.gnca_rollout_tangent_block.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(Weights),
                                                       ctypes.POINTER(RolloutSched), tb, vp, vp, vp, vp, vp, sz]
        if hasattr(lib, "gnca_step_tangent_params"):   # (likewise); dw is a Weights, or an array of K for the block
            wp = ctypes.POINTER(Weights)
            lib.gnca_step_tangent_params.restype = ctypes.c_int
            lib.gnca_step_tangent_params.argtypes = [ctypes.POINTER(StepDesc), wp, wp, vp, vp, vp, vp, vp, vp, vp, sz,
                                                     vp]
            lib.gnca_rollout_tangent_params.restype = ctypes.c_int
            lib.gnca_rollout_tangent_params.argtypes = [ctypes.POINTER(StepDesc), wp, wp, ctypes.POINTER(RolloutSched),
                                                        ctypes.POINTER(TangentArgs), vp, vp, vp, vp, vp, sz]
            lib.gnca_rollout_tangent_block_params.restype = ctypes.c_int
            lib.gnca_rollout_tangent_block_params.argtypes = [ctypes.POINTER(StepDesc), wp, wp,
                                                              ctypes.POINTER(RolloutSched),
                                                              ctypes.POINTER(TangentBlockArgs), vp, vp, vp, vp, vp, sz]
        if hasattr(lib, "gnca_rollout_objective_tangent"):   # (likewise)
            wp, tp = ctypes.POINTER(Weights), ctypes.POINTER(RolloutTaps)
            lib.gnca_loss_tangent.restype = ctypes.c_int
            lib.gnca_loss_tangent.argtypes = [i32, ctypes.POINTER(MaskedLossDesc), i32, vp, i64, vp, i64, i64, vp, i64,
                                              vp, vp, vp]
            lib.gnca_rollout_objective_tangent_workspace_bytes.restype = sz
            lib.gnca_rollout_objective_tangent_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc),
                                                                           ctypes.POINTER(RolloutSched), tp, i32]
            lib.gnca_rollout_objective_tangent.restype = ctypes.c_int
            lib.gnca_rollout_objective_tangent.argtypes = [ctypes.POINTER(StepDesc), wp, wp,
                                                           ctypes.POINTER(RolloutSched), tp, i32, vp, vp, vp, vp, vp,
                                                           vp, vp, vp, sz]
            lib.gnca_forward_grad.restype = ctypes.c_int
            lib.gnca_forward_grad.argtypes = [ctypes.POINTER(ForwardGradDesc), vp]
        if hasattr(lib, "gnca_rollout_gn_fwd"):   # (likewise)
            wp, tp = ctypes.POINTER(Weights), ctypes.POINTER(RolloutTaps)
            lib.gnca_loss_curvature.restype = ctypes.c_int
            lib.gnca_loss_curvature.argtypes = [i32, ctypes.POINTER(MaskedLossDesc), vp, i64, vp, i64, vp, i64, vp, vp,
                                                vp, vp, i64, vp]
            lib.gnca_rollout_gn_fwd_workspace_bytes.restype = sz
            lib.gnca_rollout_gn_fwd_workspace_bytes.argtypes = [ctypes.POINTER(StepDesc), ctypes.POINTER(RolloutSched),
                                                                tp]
            lib.gnca_rollout_gn_fwd.restype = ctypes.c_int
            lib.gnca_rollout_gn_fwd.argtypes = [ctypes.POINTER(StepDesc), wp, wp, ctypes.POINTER(RolloutSched), tp,
                                                vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, sz]
            lib.gnca_rollout_gn_bwd.restype = ctypes.c_int
            lib.gnca_rollout_gn_bwd.argtypes = [ctypes.POINTER(StepDesc), wp, ctypes.POINTER(RolloutSched), tp, vp, sz,
                                                vp, ctypes.POINTER(ctypes.c_float), vp, ctypes.POINTER(Grads), vp, sz]
    if v != ABI_VERSION:
        raise GncaError(f"libgnca.so ABI version {v} != expected {ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        lib = load()
        msg = lib.gnca_status_string(rc).decode()
        hip = lib.gnca_last_hip_error()
        raise GncaError(f"{what} failed: {msg} (status {rc}, hipError {hip})")
