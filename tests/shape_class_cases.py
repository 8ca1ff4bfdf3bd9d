"""Shape-class cases: the case table and the shared helpers of tests/test_shape_class_cases_cpu.py
and tests/test_gpu_shape_classes.py (test infrastructure only; importable without a GPU).

Every other step, backward, rollout, attention-map and diagnostics test uses a channel count that is
a multiple of 4.  The library accepts any 4 <= C <= 32: the plans pad to ``CP = (C + 3) & ~3``, the
attention and diagnostics kernels to 16 or 32, and about 45 guarded branches of the kernels
(``c < C``, ``co < C``, ``min(c, C - 1)``) keep the padded channels out of the sums.  A C that is no
multiple of 4 also takes the weight row stride ``3 * C``, the gradient-partial column count and the
sample stride ``C * H * W`` off their 16-byte alignment, selects the runtime-C backward kernel, and
must keep a 13..15 / 29..31-channel model off the bf16-split K1s.  The ``p*`` cases run that; the
``q*`` cases reach the rows of the two kernel tables that no other test reaches for certain:
together the cases plan every runtime-geometry ``gnca_k1_update<CP,HDP>`` row of ``kVariants``
(gnca_step.hip) and every ``(CP,HB)`` row of ``kBB`` (gnca_bwd.hip), which
tests/test_shape_class_cases_cpu.py asserts against the two lists below.

Each case: B <= 3, canvas <= 24x24.  ``k1`` is the ``(CP, HDP)`` of the planned
``gnca_k1_update<CP,HDP,...>``, ``bb`` the ``(CP, HB, slices)`` of the planned
``gnca_b_mlp<CP,HB,FULL,...>`` with ``slices = ceil(hidden / HB)``; FULL (the C == CP instance) is 1
exactly for C = 16 and C = 32.

Models are built as tests/test_gpu_fuzz.py builds them, with every parameter that the reference
initialises to zero scaled (``update_net[2]``, ``query_proj`` / ``key_proj``), states drawn as there:
RGB and alpha uniform, hidden channels normal (and a dead band: ``state``).
"""
from __future__ import annotations

import copy
import random

import numpy as np
import torch

SEED0 = 4100          # seed of case i: SEED0 + i
FIRE_SEED = 9         # the hash fire masks of the rollouts
GAIN, THR, MSG = 0.05, 0.12, 0.25


def _c(kind, C, hidden, H, W, k1, bb, *, B=2, r=2, K=4, d=16, zp=False, gn=True, ho=True, a2a=True, fire=1.0):
    return dict(graph=kind == "graph", C=C, hidden=hidden, B=B, H=H, W=W, radius=r, K=K, d_model=d, zp=zp, gn=gn,
                hidden_only=ho, a2a=a2a, fire_rate=fire, msg=MSG, gain=GAIN, thr=THR, k1=k1, bb=bb)


CASES = {
    # padded channel counts
    "p5": _c("classic", 5, 20, 11, 13, (8, 32), (8, 32, 1), B=3, fire=0.5),            # odd W: 4-byte staging
    "p6": _c("graph", 6, 40, 12, 16, (8, 64), (8, 64, 1), d=8, ho=False),              # W % 4 == 0: 16-byte staging
    "p7": _c("graph", 7, 64, 9, 10, (8, 64), (8, 64, 1), B=3, zp=True, a2a=False, fire=0.5),
    "p10": _c("graph", 10, 128, 13, 18, (12, 128), (12, 64, 2), r=3, K=8, gn=False),
    "p13": _c("graph", 13, 128, 24, 24, (16, 128), (16, 128, 1), r=4, K=8, fire=0.5),   # whole 8x24 tiles
    "p15": _c("classic", 15, 256, 10, 12, (16, 256), (16, 128, 2), gn=False),
    "p17": _c("graph", 17, 100, 12, 12, (20, 128), (20, 64, 2), r=3, K=8, zp=True, ho=False, fire=0.5),
    "p22": _c("graph", 22, 128, 8, 12, (24, 128), (24, 64, 2), a2a=False),
    "p27": _c("graph", 27, 96, 10, 9, (28, 128), (28, 64, 2), B=1, r=3, K=8, gn=False, fire=0.5),
    # the split32 shape but for C; with 16 offsets inside radius 5 no (32,64) tile fits LDS: four 32-unit slices
    "p31": _c("graph", 31, 128, 16, 16, (32, 128), (32, 32, 4), r=5, K=16, fire=0.5),
    # unreached rows of the kernel tables
    "q4": _c("graph", 4, 32, 8, 8, (4, 32), (4, 32, 1), d=4),       # hidden_only on 4 channels: no message at all
    "q4h64": _c("classic", 4, 64, 6, 10, (4, 64), (4, 64, 1), fire=0.5),
    "q4h128": _c("classic", 4, 128, 7, 9, (4, 128), (4, 64, 2)),
    "q8h1": _c("classic", 8, 1, 6, 8, (8, 32), (8, 32, 1), B=1),
    "q8h128": _c("graph", 8, 128, 8, 8, (8, 128), (8, 64, 2), d=8, fire=0.5),
    "q12h32": _c("graph", 12, 32, 10, 10, (12, 64), (12, 32, 1)),
    "q16h32": _c("classic", 16, 32, 8, 8, (16, 32), (16, 32, 1), fire=0.5),
    "q16h64": _c("graph", 16, 64, 12, 8, (16, 64), (16, 64, 1), zp=True),
    "q16h200": _c("graph", 16, 200, 16, 24, (16, 256), (16, 128, 2), r=4, K=8, fire=0.5),
    "q16h256": _c("graph", 16, 256, 12, 12, (16, 256), (16, 128, 2)),
    "q20h32": _c("graph", 20, 32, 8, 12, (20, 128), (20, 32, 1), ho=False),
    "q24h32": _c("graph", 24, 32, 8, 8, (24, 128), (24, 32, 1), fire=0.5),
    "q24h128": _c("classic", 24, 128, 8, 8, (24, 128), (24, 64, 2), fire=0.5),
    "q28h32": _c("classic", 28, 32, 8, 8, (28, 128), (28, 32, 1)),
    "q28h128": _c("graph", 28, 128, 8, 8, (28, 128), (28, 64, 2), zp=True, fire=0.5),
    "q32h32": _c("graph", 32, 32, 8, 8, (32, 64), (32, 32, 1)),
    "q32h64": _c("graph", 32, 64, 8, 8, (32, 64), (32, 64, 1), a2a=False, fire=0.5),
}
IDS = tuple(CASES)
GRAPH_IDS = tuple(n for n in IDS if CASES[n]["graph"])
PADDED_IDS = tuple(n for n in IDS if CASES[n]["C"] % 4)
ANCHOR_IDS = ("p5", "p6", "p10", "p13", "p17")                  # the CPU oracle anchor
BPTT_IDS = ("p6", "p13", "p17", "q16h200", "q24h128")           # model.rollout with grad and nsteps
TRACE_IDS = ("p6", "p13")

# the runtime-geometry rows of kVariants (gnca_step.hip) and the rows of kBB (gnca_bwd.hip)
K1_ROWS = {(4, 32), (4, 64), (4, 128), (8, 32), (8, 64), (8, 128), (12, 64), (12, 128), (16, 32), (16, 64),
           (16, 128), (16, 256), (20, 128), (24, 128), (28, 128), (32, 64), (32, 128)}
BB_ROWS = {(16, 128), (4, 32), (8, 32), (16, 32), (4, 64), (8, 64), (12, 64), (16, 64), (20, 64), (24, 64), (28, 64),
           (32, 64), (12, 32), (20, 32), (24, 32), (28, 32), (32, 32)}
# shapes outside the support set: (C, hidden)
UNSUPPORTED = [(33, 128), (16, 257)] + [(C, 129) for C in (4, 8, 12, 17, 24, 28, 32)]


def seed(name: str) -> int:
    return SEED0 + IDS.index(name)


def k1_name(name: str) -> str:
    """The prefix of the K1 the case plans (the name goes on with the geometry and thread count)."""
    return "gnca_k1_update<%d,%d," % CASES[name]["k1"]


def bb_name(name: str) -> str:
    c = CASES[name]
    return "gnca_b_mlp<%d,%d,%d,0,0,0,0,-1,0>" % (c["bb"][0], c["bb"][1], 1 if c["C"] in (16, 32) else 0)


_MODELS: dict = {}


def model(name: str, dev=None):
    """The case's module (seeded; built on the CPU once, copied to ``dev``)."""
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    c = CASES[name]
    if name not in _MODELS:
        torch.manual_seed(seed(name))
        if c["graph"]:
            m = NeuralCAGraph(c["C"], c["hidden"], update_gain=c["gain"], alpha_thr=c["thr"], use_groupnorm=c["gn"],
                              message_gain=c["msg"], hidden_only=c["hidden_only"], graph_d_model=c["d_model"],
                              graph_attention_radius=c["radius"], graph_num_neighbors=c["K"],
                              graph_alive_to_alive=c["a2a"], graph_zero_padded_shift=c["zp"])
        else:
            m = NeuralCA(c["C"], c["hidden"], update_gain=c["gain"], alpha_thr=c["thr"], use_groupnorm=c["gn"])
        with torch.no_grad():
            m.update_net[2].weight.normal_(0, 0.05)
            if c["gn"]:
                m.norm.weight.uniform_(0.5, 1.5)
                m.norm.bias.uniform_(-0.2, 0.2)
            if c["graph"]:
                m.graph.query_proj.weight.normal_(0, 0.3)
                m.graph.key_proj.weight.normal_(0, 0.3)
        _MODELS[name] = m.eval()
    m = copy.deepcopy(_MODELS[name])
    return m if dev is None else m.to(dev)


def params64(name: str) -> dict:
    return {k: v.detach().numpy().astype(np.float64) for k, v in model(name).state_dict().items()}


def state(name: str, B=None) -> torch.Tensor:
    """The seeded CPU state [B,C,H,W]: RGB and alpha ~ U(0,1), hidden channels ~ N(0,1); alpha is 0 on
    the upper third of the canvas, so that the alive masks (pre- and post-update, senders) matter."""
    c = CASES[name]
    B = c["B"] if B is None else B
    g = torch.Generator().manual_seed(seed(name))
    x = torch.rand(B, c["C"], c["H"], c["W"], generator=g)
    if c["C"] > 4:
        x[:, 4:] = torch.randn(B, c["C"] - 4, c["H"], c["W"], generator=g)
    x[:, 3, :c["H"] // 3] = 0.0
    return x


def cotangent(name: str, B=None) -> torch.Tensor:
    c = CASES[name]
    g = torch.Generator().manual_seed(77 + seed(name))
    return torch.randn(c["B"] if B is None else B, c["C"], c["H"], c["W"], generator=g)


def all_offsets(name: str) -> list:
    r = CASES[name]["radius"]
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if not (abs(dy) <= 1 and abs(dx) <= 1)]


def offsets(name: str, steps: int = 1) -> list:
    """``steps`` seeded draws of the case's K offsets ([] per step for a classic case)."""
    c = CASES[name]
    if not c["graph"]:
        return [[] for _ in range(steps)]
    rr = random.Random(seed(name))
    pool = all_offsets(name)
    return [rr.sample(pool, min(c["K"], len(pool))) for _ in range(steps)]


def fire_mask(name: str, B=None):
    """The seeded {0,1} fire mask [B,1,H,W] uint8 of the one-step tests, or None at fire rate 1."""
    c = CASES[name]
    if c["fire_rate"] >= 1.0:
        return None
    g = torch.Generator().manual_seed(13 + seed(name))
    return (torch.rand(c["B"] if B is None else B, 1, c["H"], c["W"], generator=g) <= c["fire_rate"]).to(torch.uint8)


def oracle_cfg(name: str) -> dict:
    c = CASES[name]
    return dict(update_gain=c["gain"], alpha_thr=c["thr"], use_groupnorm=c["gn"], graph=c["graph"],
                message_gain=c["msg"], hidden_only=c["hidden_only"], zero_padded_shift=c["zp"],
                alive_to_alive=c["a2a"])


def flags(name: str, attention: bool = False) -> int:
    from graph_neural_cellular_automata_amd import _lib as L
    c = CASES[name]
    f = L.USE_GROUPNORM if c["gn"] else 0
    if c["graph"]:
        f |= L.GRAPH | (L.ALIVE_TO_ALIVE if c["a2a"] else 0) | (L.ZERO_PAD_SHIFT if c["zp"] else 0) | \
            (L.HIDDEN_ONLY if c["hidden_only"] else 0) | (L.ATTENTION if attention else 0)
    return f


def desc(name: str, offs=None, *, B=None, fire_mode=None, fire_rate=None, rng_step=0, message_gain=None,
         attention=False, **over):
    """The case's descriptor: its first seeded offsets and FIRE_MASK_U8 / FIRE_NONE by default."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    c = CASES[name]
    if fire_mode is None:
        fire_mode = L.FIRE_MASK_U8 if c["fire_rate"] < 1.0 else L.FIRE_NONE
    kw = dict(B=c["B"] if B is None else B, C=c["C"], H=c["H"], W=c["W"], hidden=c["hidden"],
              d_model=c["d_model"] if c["graph"] else 1, offsets=offsets(name)[0] if offs is None else offs,
              flags=flags(name, attention), update_gain=c["gain"], alpha_thr=c["thr"],
              message_gain=(c["msg"] if c["graph"] else 0.0) if message_gain is None else message_gain,
              fire_rate=c["fire_rate"] if fire_rate is None else fire_rate, fire_mode=fire_mode,
              rng_seed=FIRE_SEED, rng_step=rng_step)
    kw.update(over)
    return S.make_desc(**kw)


def bare_desc(C: int, hidden: int):
    """A small graph descriptor of any (C, hidden), for the support-set boundary."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    return S.make_desc(B=2, C=C, H=8, W=8, hidden=hidden, d_model=16, offsets=[(2, 0), (0, -2)],
                       flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY, update_gain=GAIN,
                       alpha_thr=THR, message_gain=MSG, fire_rate=1.0, fire_mode=L.FIRE_NONE)


def weight_tensors(m) -> dict:
    """The module's step weights by their gnca_weights field names."""
    t = dict(perception=m.perception.conv.weight, w1=m.update_net[0].weight, b1=m.update_net[0].bias,
             w2=m.update_net[2].weight)
    if hasattr(m, "graph"):
        t.update(m.graph.weight_tensors())
    if isinstance(m.norm, torch.nn.GroupNorm):
        t.update(gn_weight=m.norm.weight, gn_bias=m.norm.bias)
    return t


_REF: dict = {}


def reference(name: str, fire=None) -> dict:
    """One step and its VJP on the float64 oracle, computed once per case and left unchanged:
    ``out``, ``attn`` (graph cases), ``gx`` and ``grads`` for the case's state, first offsets, fire mask
    and cotangent.  ``fire``: a {0,1} array [B,1,H,W] that replaces ``fire_mask(name)`` (the GPU
    tests pass the mask the module's ``torch.rand`` draws on the device; kept apart in the cache)."""
    key = (name, fire is not None)
    if key in _REF:
        return _REF[key]
    from oracle import nca_oracle as O
    from oracle import nca_oracle_vjp as V
    c = CASES[name]
    x = state(name).numpy().astype(np.float64)
    p, cfg = params64(name), oracle_cfg(name)
    chosen = offsets(name)[0] if c["graph"] else None
    f = fire_mask(name) if fire is None else torch.as_tensor(fire)
    f = None if f is None else f.numpy().astype(np.float64)
    r = {}
    if c["graph"]:
        r["out"], r["attn"] = O.nca_step(x, p, cfg, chosen=chosen, fire_mask=f, return_attention=True)
    else:
        r["out"] = O.nca_step(x, p, cfg, chosen=chosen, fire_mask=f)
    r["gx"], r["grads"] = V.nca_step_vjp(x, p, cfg, cotangent(name).numpy().astype(np.float64), chosen=chosen,
                                         fire_mask=f)
    for v in [r["out"], r["gx"], *r["grads"].values()] + ([r["attn"]] if "attn" in r else []):
        v.setflags(write=False)
    _REF[key] = r
    return r
