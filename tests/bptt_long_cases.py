"""Trainer-length BPTT cases: the case table, schedule builder, seed-state builder and the float64
oracle chain of tests/test_bptt_long_cases_cpu.py and tests/test_gpu_bptt_long.py (test
infrastructure only).

The trainers back-propagate through 48-80 steps of a state grown from one seed cell; every other
BPTT test stops at 4 steps of a seeded random state (alpha ~ U(0,1): all alive).  The cases here
run that workload: a state that goes from under 1 % alive to over a third, so that every backward
step sees another live-tile list, other per-tile live counts and other GroupNorm statistics, over
enough steps that the rollout's accumulating rows, tape slots, gradient ping-pong and [T][B] mask
block leave their first few entries.

All cases share:

* the seed state: zeros, alpha and the hidden channels of one cell set to 1 (the trainers' seed);
  the cell is the centre moved by (b, -b) per sample (wrapped), so the samples differ;
* GNCA_FIRE_HASH masks, rate 0.5, seed ``FIRE_SEED``, ``rng_step = t``;
* the message on every third step (t % 3 == 0), off otherwise;
* offsets drawn per step by ``random.sample`` of a ``random.Random`` with a fixed seed; two
  message-on steps (one in the unmasked prefix, one in the masked tail where the case has both) and
  one message-off step draw inside radius 2 and one message-on step inside radius 3, so that the
  rollout layouts' set of (message on/off, max |dy|, max |dx|) keys holds several entries;
* a seeded normal cotangent of the state's shape.
"""
from __future__ import annotations

import random

import numpy as np

from oracle import nca_oracle as O
from oracle import nca_oracle_vjp as V
from tests.golden_io import Case
from tests.liveness_cases import MARGIN, pooled, tile_live_counts

FIRE_SEED = 9
FIRE_RATE = 0.5
OFFSET_SEED = 2024
COT_SEED = 77

_TORUS = "grad_graph_torus_latest_grown_b2_40"
# name -> weights fixture, B, H, W, T, per-sample step counts, min_steps (the unmasked prefix),
# oracle: compared with the float64 VJP (lean72 is too large for the CPU oracle)
CASES = {
    "torus40": dict(fixture=_TORUS, B=4, H=40, W=40, T=72, nsteps=[72, 48, 61, 55], min_steps=48, oracle=True),
    "zeropad40": dict(fixture="grad_graph_zeropad_latest_grown_b2_40", B=3, H=40, W=40, T=49,
                      nsteps=[49, 33, 40], min_steps=0, oracle=True),
    "classic20": dict(fixture="grad_classic_c12_hd48_nogn_b2_20", B=2, H=20, W=22, T=64, nsteps=[64, 50],
                      min_steps=50, oracle=True),
    "lean72": dict(fixture=_TORUS, B=104, H=72, W=72, T=24, nsteps=[24 if b % 2 == 0 else 12 for b in range(104)],
                   min_steps=12, oracle=False),
}
ORACLE_CASES = tuple(n for n, k in CASES.items() if k["oracle"])

# The kernels each case means to run (S.k1_variant / S.bb_variant of a step's descriptor), for a
# message-on and a message-off step.  gnca_bb_variant names the plan of the step WITHOUT an
# active-sample mask; a masked step of the same descriptor never takes the lean 24x24 tiles
# (bwd_plan's lean_ok), so lean72's masked tail runs the 8x24 instance that B = 128 plans
# (liveness_cases.BWD_FAMILIES "8x24") behind gnca_b_actlist.
PLANS = {
    "torus40": dict(k1_on="gnca_k1_split<8,20,4,4,8>", k1_off="gnca_k1_split<8,20,1,4,0>",
                    bb_on="gnca_b_mlp<16,128,1,0,0,0,0,-1,0>", bb_off="gnca_b_mlp<16,128,1,0,0,0,0,-1,0>"),
    "zeropad40": dict(k1_on="gnca_k1_split<8,20,4,4,8>", k1_off="gnca_k1_split<8,20,1,4,0>",
                      bb_on="gnca_b_mlp<16,128,1,0,0,0,0,-1,0>", bb_off="gnca_b_mlp<16,128,1,0,0,0,0,-1,0>"),
    "classic20": dict(k1_on="gnca_k1_update<12,64,", k1_off="gnca_k1_update<12,64,",
                      bb_on="gnca_b_mlp<12,64,0,0,0,0,0,-1,0>", bb_off="gnca_b_mlp<12,64,0,0,0,0,0,-1,0>"),
    "lean72": dict(k1_on="gnca_k1_split<24,36,4,4,8>", k1_off="gnca_k1_split<24,36,1,4,0>",
                   bb_on="gnca_b_mlp<16,128,1,24,24,4,4,8,1>", bb_off="gnca_b_mlp<16,128,1,24,24,1,4,0,1>"),
}

_FIX: dict = {}


def fixture(name: str) -> Case:
    fx = CASES[name]["fixture"]
    if fx not in _FIX:
        _FIX[fx] = Case(fx)
    return _FIX[fx]


def nsteps(name: str) -> np.ndarray:
    return np.asarray(CASES[name]["nsteps"], np.int32)


def _within(r: int, radius: int) -> list:
    return [o for o in O.build_offsets(radius) if max(abs(o[0]), abs(o[1])) <= r]


def small_steps(T: int) -> dict:
    """step -> radius of the steps that draw inside a smaller radius: the second and the
    last-but-one message-on step and the message-off step 4 inside 2, the third message-on step
    inside 3."""
    on = list(range(0, T, 3))
    return {on[1]: 2, on[-2]: 2, 4: 2, on[2]: 3}


def schedule(name: str):
    """(offsets per step, message gain per step); (None, None) for the classic model."""
    m = fixture(name).meta
    T = CASES[name]["T"]
    if not m["graph"]:
        return None, None
    rnd = random.Random(OFFSET_SEED + list(CASES).index(name))
    small = small_steps(T)
    offs = []
    for t in range(T):
        pool = _within(small[t], m["r"]) if t in small else O.build_offsets(m["r"])
        offs.append(rnd.sample(pool, m["K"]))
    gains = [float(m["message_gain"]) if t % 3 == 0 else 0.0 for t in range(T)]
    return offs, gains


def seen_keys(offs, gains) -> set:
    """The keys the rollout layouts size a step's workspace by (roll_bwd_layout: message on/off,
    max |dy|, max |dx| of the step's offsets)."""
    if offs is None:
        return {(False, 0, 0)}
    return {(g != 0.0, max(abs(dy) for dy, _ in o), max(abs(dx) for _, dx in o)) for o, g in zip(offs, gains)}


def seed_state(name: str) -> np.ndarray:
    k = CASES[name]
    C = fixture(name).meta["C"]
    x = np.zeros((k["B"], C, k["H"], k["W"]), np.float32)
    for b in range(k["B"]):
        x[b, 3:, (k["H"] // 2 + b) % k["H"], (k["W"] // 2 - b) % k["W"]] = 1.0
    return x


def cotangent(name: str) -> np.ndarray:
    k = CASES[name]
    g = np.random.default_rng([COT_SEED, list(CASES).index(name)])
    return g.standard_normal((k["B"], fixture(name).meta["C"], k["H"], k["W"]), dtype=np.float32)


def fire(name: str, t: int, samples) -> np.ndarray:
    """The hashed fire masks [n,1,H,W] of ``samples`` (global sample indices) at step ``t``."""
    k = CASES[name]
    return np.concatenate([O.hash_fire_mask(FIRE_SEED, t, int(b), 1, k["H"], k["W"], FIRE_RATE) for b in samples])


def cfg(name: str, gain: float) -> dict:
    return dict(fixture(name).cfg(), message_gain=gain)


def params64(name: str) -> dict:
    return {k: np.asarray(v, np.float64) for k, v in fixture(name).weights.items()}


def doubtful(xt: np.ndarray, thr: float) -> np.ndarray:
    """bool [n,1,H,W]: the cells whose post-update mask a float32 run within the forward parity
    bound may decide the other way: the 3x3-pooled alpha of ``xt`` (the float64 updated state
    before the post gate) lies within MARGIN (10 x the forward atol) of float32(thr)."""
    d = np.abs(pooled(np.asarray(xt, np.float64)[:, 3]) - np.float64(np.float32(thr)))
    return (d <= MARGIN)[:, None]


def step_args(name: str, t: int, offs, gains):
    """(cfg, chosen) of step ``t`` for the oracle."""
    return cfg(name, gains[t] if gains else 0.0), (offs[t] if offs else None)


def desc(name: str, t: int, offs, gains):
    """The descriptor of step ``t``, as the rollout's schedule gives it to the kernels."""
    from graph_neural_cellular_automata_amd import _lib as L
    from tests.fixture_run import desc_for
    k = CASES[name]
    return desc_for(fixture(name), k["B"], k["H"], k["W"], offs[t] if offs else [], L.FIRE_HASH, fire_rate=FIRE_RATE,
                    rng_seed=FIRE_SEED, rng_step=t, message_gain=gains[t] if gains else 0.0)


def plan_steps(name: str) -> tuple:
    """(a message-on step of the unmasked prefix, or step 0 where the case has none; the first
    message-off step of the masked tail): the two descriptors whose plans a case asserts."""
    t = max(CASES[name]["min_steps"], 1)
    while t % 3 == 0:
        t += 1
    return 0, t


def check_plans(name: str) -> tuple:
    """Assert the kernels the case means to run (PLANS) and return them for the assertion
    messages."""
    from graph_neural_cellular_automata_amd import step as S
    offs, gains = schedule(name)
    t_on, t_off = plan_steps(name)
    assert CASES[name]["min_steps"] <= t_off < CASES[name]["T"], (name, t_off)
    d_on, d_off = desc(name, t_on, offs, gains), desc(name, t_off, offs, gains)
    got = dict(k1_on=S.k1_variant(d_on)[0], k1_off=S.k1_variant(d_off)[0], bb_on=S.bb_variant(d_on),
               bb_off=S.bb_variant(d_off))
    for key, want in PLANS[name].items():
        assert got[key].startswith(want), (name, key, got)
    return tuple(sorted(got.items()))


_CHAIN: dict = {}


def oracle_chain(name: str) -> dict:
    """The case on the float64 oracle alone: the masked forward (inactive samples pass through),
    then the chained VJP of the cotangent.  Returns per-step lists: ``alive`` (alive fraction of the
    state after t steps, T + 1 entries), ``gmax`` (max |g| after the backward of step t), ``keep``
    (the keep masks alive AND fire of all samples, inactive ones included), and the counts
    ``doubtful`` / ``triples`` over the (active sample, step, cell) triples."""
    if name in _CHAIN:
        return _CHAIN[name]
    k = CASES[name]
    T, ns, thr = k["T"], nsteps(name), fixture(name).meta["alpha_thr"]
    p = params64(name)
    offs, gains = schedule(name)
    x = seed_state(name).astype(np.float64)
    states, alive, keep, nd, ntr = [x], [float(O.alive_mask(x, thr).mean())], [], 0, 0
    for t in range(T):
        idx = np.flatnonzero(ns > t)
        c, ch = step_args(name, t, offs, gains)
        keep.append(O.alive_mask(x, thr) * fire(name, t, range(k["B"])))
        xt, _ = O.nca_update(x[idx], p, c, chosen=ch, fire_mask=fire(name, t, idx))
        nd += int(doubtful(xt, thr).sum())
        ntr += idx.size * k["H"] * k["W"]
        xt[:, 3:4] *= O.alive_mask(xt, thr)
        x = x.copy()
        x[idx] = xt
        states.append(x)
        alive.append(float(O.alive_mask(x, thr).mean()))
    g = cotangent(name).astype(np.float64)
    gmax = [0.0] * T
    for t in reversed(range(T)):
        idx = np.flatnonzero(ns > t)
        c, ch = step_args(name, t, offs, gains)
        gx, _ = V.nca_step_vjp(states[t][idx], p, c, g[idx], chosen=ch, fire_mask=fire(name, t, idx))
        g = g.copy()
        g[idx] = gx
        gmax[t] = float(np.abs(g).max())
    _CHAIN[name] = dict(alive=alive, gmax=gmax, keep=keep, doubtful=nd, triples=ntr)
    return _CHAIN[name]


def empty_tile_rows(keep: np.ndarray, tile=(4, 8)) -> int:
    """Tile rows of a keep mask [n,1,H,W] without one kept cell, over the samples."""
    return int((tile_live_counts(keep, tile).sum(axis=2) == 0).sum())
