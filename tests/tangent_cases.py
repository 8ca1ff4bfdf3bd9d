"""The cases of the tangent tests (tests/test_gpu_tangent.py, tests/test_tangent_api_cpu.py): test
infrastructure only, importable without a GPU.

Every torus (non-zero-pad) case of tests/shape_class_cases.py, derived from its table (B <= 3, canvas <=
24x24: padded channel counts, the hidden-sliced class p31, classic models, GroupNorm off, hidden 200 / 256,
every fire rate), one case of the trainers' class (16 channels, hidden 128, r = 4, K = 8, torus, B = 2 at
72x72) and one case with a negative alive threshold.  Models, states,
offsets and fire masks are built as tests/shape_class_cases.py builds them.
"""
from __future__ import annotations

import copy
import random

import numpy as np
import torch

from tests import shape_class_cases as SC

T72 = dict(SC.CASES["p13"], C=16, hidden=128, B=2, H=72, W=72, radius=4, K=8, fire_rate=0.5)
# "neg": p6 with a NEGATIVE alive threshold and an alpha plane shifted to [-0.5, 0.5): the post mask cannot be read
# off the gated alpha of the new state there (a gated +-0 exceeds the threshold), TB recomputes the updated alpha
NEG = dict(SC.CASES["p6"], thr=-0.05)
SC_IDS = tuple(n for n in SC.IDS if not SC.CASES[n]["zp"])      # every torus case of the table
IDS = SC_IDS + ("t72", "neg")
SEED_T72, SEED_NEG = 4777, 4888


def case(name: str) -> dict:
    return T72 if name == "t72" else NEG if name == "neg" else SC.CASES[name]


def seed(name: str) -> int:
    return SEED_T72 if name == "t72" else SEED_NEG if name == "neg" else SC.seed(name)


_MODELS: dict = {}


def model(name: str, dev=None):
    if name not in ("t72", "neg"):
        return SC.model(name, dev)
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    c = case(name)
    if name not in _MODELS:
        torch.manual_seed(seed(name))
        m = NeuralCAGraph(c["C"], c["hidden"], update_gain=c["gain"], alpha_thr=c["thr"], use_groupnorm=True,
                          message_gain=c["msg"], hidden_only=c["hidden_only"], graph_d_model=c["d_model"],
                          graph_attention_radius=c["radius"], graph_num_neighbors=c["K"],
                          graph_alive_to_alive=True, graph_zero_padded_shift=False)
        with torch.no_grad():
            m.update_net[2].weight.normal_(0, 0.05)
            m.norm.weight.uniform_(0.5, 1.5)
            m.norm.bias.uniform_(-0.2, 0.2)
        _MODELS[name] = m.eval()
    m = copy.deepcopy(_MODELS[name])
    return m if dev is None else m.to(dev)


def params64(name: str) -> dict:
    return {k: v.detach().numpy().astype(np.float64) for k, v in model(name).state_dict().items()}


def state(name: str, B=None, extra: int = 0) -> torch.Tensor:
    """RGB and alpha ~ U(0,1), hidden ~ N(0,1), alpha 0 on the upper third (SC.state); ``extra``: another draw."""
    c = case(name)
    B = c["B"] if B is None else B
    g = torch.Generator().manual_seed(seed(name) + 1000 * extra)
    x = torch.rand(B, c["C"], c["H"], c["W"], generator=g)
    if c["C"] > 4:
        x[:, 4:] = torch.randn(B, c["C"] - 4, c["H"], c["W"], generator=g)
    x[:, 3, :c["H"] // 3] = 0.0
    if c["thr"] < 0:
        x[:, 3] -= 0.5          # dead band at -0.5, the rest in [-0.5, 0.5): both sides of the negative threshold
    return x


def tangent(name: str, B=None, extra: int = 0) -> torch.Tensor:
    c = case(name)
    g = torch.Generator().manual_seed(555 + seed(name) + 1000 * extra)
    return torch.randn(c["B"] if B is None else B, c["C"], c["H"], c["W"], generator=g)


def cotangent(name: str) -> torch.Tensor:
    c = case(name)
    g = torch.Generator().manual_seed(77 + seed(name))
    return torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g)


def offsets(name: str, steps: int = 1) -> list:
    c = case(name)
    if not c["graph"]:
        return [[] for _ in range(steps)]
    r = c["radius"]
    pool = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if not (abs(dy) <= 1 and abs(dx) <= 1)]
    rr = random.Random(seed(name))
    return [rr.sample(pool, min(c["K"], len(pool))) for _ in range(steps)]


def fire_mask(name: str, B=None, extra: int = 0):
    """The seeded {0,1} uint8 fire mask [B,1,H,W] of the one-step tests, or None at fire rate 1."""
    c = case(name)
    if c["fire_rate"] >= 1.0:
        return None
    g = torch.Generator().manual_seed(13 + seed(name) + 1000 * extra)
    return (torch.rand(c["B"] if B is None else B, 1, c["H"], c["W"], generator=g) <= c["fire_rate"]).to(torch.uint8)


def oracle_cfg(name: str) -> dict:
    c = case(name)
    return dict(update_gain=c["gain"], alpha_thr=c["thr"], use_groupnorm=c["gn"], graph=c["graph"],
                message_gain=c["msg"], hidden_only=c["hidden_only"], zero_padded_shift=c["zp"],
                alive_to_alive=c["a2a"])


def desc(name: str, offs, *, fire_mode, fire_rate=None, message_gain=None):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    c = case(name)
    f = L.USE_GROUPNORM if c["gn"] else 0
    if c["graph"]:
        f |= L.GRAPH | (L.ALIVE_TO_ALIVE if c["a2a"] else 0) | (L.ZERO_PAD_SHIFT if c["zp"] else 0) | \
            (L.HIDDEN_ONLY if c["hidden_only"] else 0)
    return S.make_desc(B=c["B"], C=c["C"], H=c["H"], W=c["W"], hidden=c["hidden"],
                       d_model=c["d_model"] if c["graph"] else 1, offsets=offs, flags=f, update_gain=c["gain"],
                       alpha_thr=c["thr"],
                       message_gain=(c["msg"] if c["graph"] else 0.0) if message_gain is None else message_gain,
                       fire_rate=c["fire_rate"] if fire_rate is None else fire_rate, fire_mode=fire_mode)
