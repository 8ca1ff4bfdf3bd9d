#!/usr/bin/env python
"""A/B of one training iteration's rollout + BPTT: the per-step loop (one autograd node per step,
``apply_step`` with ``active = nsteps > t``) against ``model.rollout`` (one node per rollout), in
ONE process, alternating, on identical seeded schedules (hash fire masks, fixed per-sample lengths).

Each repeat times a window of at least ``--window`` seconds per path: forward and backward are
bracketed by device synchronises, and the per-iteration means are printed per repeat (the spread)
with their median, then the maximum gradient difference between the two paths.

    python tools/bench_rollout_bptt.py [--shape trainer|reference|both] [--repeats 5] [--window 1.0]
    python tools/bench_rollout_bptt.py --profile-backward    # three rollout iterations only (for a kernel trace)
    python tools/bench_rollout_bptt.py --shape trainer --checkpoint-every auto [--recompute] [--steps 200 400]

With ``--checkpoint-every`` the two alternating paths are ``model.rollout`` without and with
``checkpoint_every`` (same windows, same schedule): the checkpointed backward re-runs the forward, so the
yardstick printed beside it is the same run's plain backward plus plain forward.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_neural_cellular_automata_amd import NeuralCAGraph  # noqa: E402
from graph_neural_cellular_automata_amd import _lib as L  # noqa: E402
from graph_neural_cellular_automata_amd import step as S  # noqa: E402
from graph_neural_cellular_automata_amd.modules import _stepper as ST  # noqa: E402

SHAPES = {"trainer": dict(B=128, H=72), "reference": dict(B=16, H=40)}
LO, HI, SEED, RATE, GAIN = 48, 80, 17, 0.5, 0.25


def setup(B, H, dev):
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=GAIN,
                          graph_zero_padded_shift=False).to(dev)
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.02)
    x = torch.zeros(B, 16, H, H, device=dev)
    x[:, 3:, H // 2 - 4:H // 2 + 4, H // 2 - 4:H // 2 + 4] = 1.0   # a grown-ish seed patch
    x[:, 4:] += 0.1 * torch.randn(B, 12, H, H, device=dev)
    gy = torch.randn(B, 16, H, H, device=dev) / (B * H * H)
    rng = random.Random(5)
    nsteps = [rng.randint(LO, HI) for _ in range(B)]
    random.seed(6)
    offs = [model.graph.sample_offsets() for _ in range(HI)]
    gains = [GAIN if t % 3 == 0 else 0.0 for t in range(HI)]
    return model, x, gy, torch.tensor(nsteps, dtype=torch.int32, device=dev), offs, gains


def per_step_forward(model, x, ns, offs, gains):
    """The per-step path: one masked step node per CA step, on the rollout's descriptors."""
    B, C, H, W = x.shape
    tensors = ST._step_tensors(model, model.graph)
    flags = L.USE_GROUPNORM | model.graph.flags(False) | L.HIDDEN_ONLY
    key = (B, C, H, W, 128, model.graph.d_model, flags, float(model.update_gain), float(model.alpha_thr),
           float(model.graph.alpha_thr), 1e-3)
    w, keep = S.make_weights(tensors)
    s = x
    for t in range(HI):
        d = ST._step_desc(key, offs[t], gains[t], RATE, L.FIRE_HASH)
        d.rng_seed, d.rng_step = SEED, t
        # (the trainers skip the mask while every sample is active: t < LO)
        s, _ = ST.apply_step(model, s, d, w, keep, None, False, None if t < LO else ns > t, tensors)
    return s


ROLLOUT_KW = {}   # --recompute


def rollout_forward(model, x, ns, offs, gains, **kw):
    return model.rollout(x, HI, fire_rate=RATE, message_gain=gains, nsteps=ns, min_steps=LO, seed=SEED, offsets=offs,
                         **ROLLOUT_KW, **kw)


def one_iteration(fwd, model, x, gy, ns, offs, gains):
    model.zero_grad(set_to_none=True)
    leaf = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fwd(model, leaf, ns, offs, gains)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    (out * gy).sum().backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, leaf.grad, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def bench(name, repeats, window, dev, checkpoint_every=None):
    cfg = SHAPES[name]
    args = setup(cfg["B"], cfg["H"], dev)
    paths = {"per_step": per_step_forward, "rollout": rollout_forward}
    if checkpoint_every is not None:
        paths = {"per_step": rollout_forward,    # (the baseline's slot: the plain rollout)
                 "rollout": lambda *a: rollout_forward(*a, checkpoint_every=checkpoint_every)}
    grads = {}
    for p, fn in paths.items():   # warm-up (plans, workspaces, allocator)
        for _ in range(2):
            *_, gx, g = one_iteration(fn, *args)
        grads[p] = dict(g, gx=gx)
    diff = {k: float((grads["per_step"][k] - grads["rollout"][k]).abs().max()) for k in grads["per_step"]}
    scale = {k: float(grads["per_step"][k].abs().max()) for k in grads["per_step"]}
    rows = {p: [] for p in paths}
    for _ in range(repeats):
        for p, fn in paths.items():
            f = b = 0.0
            n = 0
            t_end = time.perf_counter() + window
            while time.perf_counter() < t_end or n == 0:
                tf, tb, *_ = one_iteration(fn, *args)
                f += tf; b += tb; n += 1
            rows[p].append((1e3 * f / n, 1e3 * b / n, n))
    res = dict(shape=name, B=cfg["B"], H=cfg["H"], steps=[LO, HI], message_every=3, repeats=repeats, window_s=window)
    for p in paths:
        res[p] = dict(fwd_ms=[round(r[0], 3) for r in rows[p]], bwd_ms=[round(r[1], 3) for r in rows[p]],
                      iters=[r[2] for r in rows[p]],
                      fwd_ms_median=round(statistics.median(r[0] for r in rows[p]), 3),
                      bwd_ms_median=round(statistics.median(r[1] for r in rows[p]), 3))
    res["max_grad_diff"] = {k: f"{diff[k]:.3e} (max|g| {scale[k]:.3e})" for k in diff}
    if checkpoint_every is not None:
        res["plain"], res["checkpointed"] = res.pop("per_step"), res.pop("rollout")
        res["checkpoint_every"], res["recompute"] = checkpoint_every, bool(ROLLOUT_KW.get("recompute"))
        res["memory_bytes"] = {
            tag: args[0].rollout_memory(args[1], HI, fire_rate=RATE, message_gain=args[5], min_steps=LO, seed=SEED,
                                        offsets=args[4], **ROLLOUT_KW, **kw)
            for tag, kw in (("plain", {}), ("checkpointed", dict(checkpoint_every=checkpoint_every)))}
        want = res["plain"]["bwd_ms_median"] + res["plain"]["fwd_ms_median"]
        res["bwd_yardstick_ms"] = round(want, 3)     # plain backward + plain tape forward
        res["bwd_over_yardstick"] = round(res["checkpointed"]["bwd_ms_median"] / want, 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["trainer", "reference", "both"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--profile-backward", action="store_true",
                    help="three rollout iterations at the trainer shape and nothing else (for a kernel trace)")
    ap.add_argument("--profile-per-step", action="store_true",
                    help="the same three iterations on the per-step path")
    ap.add_argument("--checkpoint-every", default=None,
                    help="an int >= 1 or 'auto': time model.rollout without and with checkpoint_every")
    ap.add_argument("--recompute", action="store_true", help="recompute=True on both rollout paths")
    ap.add_argument("--steps", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help="per-sample rollout lengths are drawn from LO..HI (default 48 80)")
    a = ap.parse_args()
    global LO, HI
    if a.steps:
        LO, HI = a.steps
        if not 1 <= LO <= HI:
            ap.error("--steps needs 1 <= LO <= HI")
    if a.recompute:
        ROLLOUT_KW["recompute"] = True
    ck = a.checkpoint_every
    if ck is not None and ck != "auto":
        ck = int(ck)
    dev = torch.device("cuda:0")
    if a.profile_backward or a.profile_per_step:
        args = setup(SHAPES["trainer"]["B"], SHAPES["trainer"]["H"], dev)
        for _ in range(3):
            one_iteration(rollout_forward if a.profile_backward else per_step_forward, *args)
        return
    for name in (["trainer", "reference"] if a.shape == "both" else [a.shape]):
        bench(name, a.repeats, a.window, dev, ck)


if __name__ == "__main__":
    main()
