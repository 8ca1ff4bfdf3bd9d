#!/usr/bin/env python
"""A/B of one training iteration with losses at intermediate steps: ``model.rollout_objective`` (one
autograd node for the rollout and every tapped loss) against the chain of ``model.rollout`` segments
with a loss node on each segment's end, in ONE process, alternating, on identical seeded schedules
(hash fire masks cannot be chained, so both paths take the same explicit uint8 masks).

T = 64 steps, the message on every third step; taps ``every=8`` (8 taps), then the single final tap.
Each repeat times a window of at least ``--window`` seconds per path; an iteration is forward, the
scalar ``losses.mean()`` and backward, bracketed by device synchronises.  Per shape and tap list one
JSON line: the per-repeat means, their median and min-max, and the largest difference between the two
paths' gradients.

    python tools/bench_rollout_objective.py [--shape reference|trainer|both] [--repeats 5] [--window 1.0]
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
from graph_neural_cellular_automata_amd.loss import masked_loss  # noqa: E402

SHAPES = {"reference": dict(B=16, H=40), "trainer": dict(B=128, H=72)}
T, EVERY, RATE, GAIN = 64, 8, 0.5, 0.25
KNOBS = (0.2, 5e-5, 1e-3, 2e-4)


def setup(B, H, dev):
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=GAIN,
                          graph_zero_padded_shift=False).to(dev)
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.02)
    x = torch.zeros(B, 16, H, H, device=dev)
    x[:, 3:, H // 2 - 4:H // 2 + 4, H // 2 - 4:H // 2 + 4] = 1.0   # a grown-ish seed patch
    x[:, 4:] += 0.1 * torch.randn(B, 12, H, H, device=dev)
    target = torch.rand(4, H, H, device=dev)
    target[3, : H // 3] = 0.0
    fire = (torch.rand(T, B, 1, H, H, device=dev) <= RATE).to(torch.uint8)
    random.seed(6)
    offs = [model.graph.sample_offsets() for _ in range(T)]
    gains = [GAIN if t % 3 == 0 else 0.0 for t in range(T)]
    return model, x, target, fire, offs, gains


def fused(model, leaf, target, fire, offs, gains, taps):
    res = model.rollout_objective(leaf, T, target, record=taps, loss="masked", alpha_thr=KNOBS[0], lam_area=KNOBS[1],
                                  lam_bg_alpha=KNOBS[2], lam_bg_rgb=KNOBS[3], fire_rate=RATE, message_gain=gains,
                                  fire=fire, offsets=offs)
    return res.losses


def chain(model, leaf, target, fire, offs, gains, taps):
    state, lo, losses = leaf, 0, []
    for t in taps:
        state = model.rollout(state, t - lo, fire_rate=RATE, message_gain=gains[lo:t], fire=fire[lo:t],
                              offsets=offs[lo:t])
        losses.append(masked_loss(state[:, :4], target, *KNOBS))
        lo = t
    return torch.stack(losses)


def one_iteration(fn, model, x, target, fire, offs, gains, taps):
    model.zero_grad(set_to_none=True)
    leaf = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = fn(model, leaf, target, fire, offs, gains, taps)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    losses.mean().backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return t1 - t0, t2 - t1, dict(grads, gx=leaf.grad, losses=losses.detach())


def bench(name, taps_name, taps, repeats, window, dev):
    cfg = SHAPES[name]
    args = setup(cfg["B"], cfg["H"], dev)
    paths = {"chain": chain, "fused": fused}
    last = {}
    for p, fn in paths.items():   # warm-up (plans, workspaces, allocator)
        for _ in range(2):
            *_, last[p] = one_iteration(fn, *args, taps)
    diff = {k: float((last["chain"][k] - last["fused"][k]).abs().max()) for k in last["chain"]}
    scale = {k: float(last["chain"][k].abs().max()) for k in last["chain"]}
    rows = {p: [] for p in paths}
    for _ in range(repeats):
        for p, fn in paths.items():
            f = b = 0.0
            n = 0
            t_end = time.perf_counter() + window
            while time.perf_counter() < t_end or n == 0:
                tf, tb, _ = one_iteration(fn, *args, taps)
                f += tf; b += tb; n += 1
            rows[p].append((1e3 * f / n, 1e3 * b / n, n))
    res = dict(shape=name, B=cfg["B"], H=cfg["H"], steps=T, message_every=3, taps=taps_name, num_taps=len(taps),
               loss="masked", repeats=repeats, window_s=window)
    for p in paths:
        tot = [r[0] + r[1] for r in rows[p]]
        res[p] = dict(fwd_ms=[round(r[0], 3) for r in rows[p]], bwd_ms=[round(r[1], 3) for r in rows[p]],
                      iters=[r[2] for r in rows[p]],
                      fwd_ms_median=round(statistics.median(r[0] for r in rows[p]), 3),
                      bwd_ms_median=round(statistics.median(r[1] for r in rows[p]), 3),
                      total_ms_median=round(statistics.median(tot), 3),
                      total_ms_min=round(min(tot), 3), total_ms_max=round(max(tot), 3))
    res["fused_over_chain"] = round(res["fused"]["total_ms_median"] / res["chain"]["total_ms_median"], 4)
    res["max_diff"] = {k: f"{diff[k]:.3e} (max|chain| {scale[k]:.3e})" for k in diff}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["reference", "trainer", "both"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in (["reference", "trainer"] if a.shape == "both" else [a.shape]):
        bench(name, f"every={EVERY}", list(range(EVERY, T + 1, EVERY)), a.repeats, a.window, dev)
        bench(name, "final", [T], a.repeats, a.window, dev)


if __name__ == "__main__":
    main()
