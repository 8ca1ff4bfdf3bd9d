#!/usr/bin/env python
"""What the forward-mode objective costs: ``model.rollout_objective_tangent`` with K = 8 weight directions and a
tap at every step, and with one tap at T, against ``model.rollout_tangent_block(dparams, orthonormalize=False)``
at the same K (the same rollout without the loss kernel: the per-tap overhead is the difference divided by R),
against ``model.rollout_objective(checkpoint_every="auto")`` forward plus backward (the reverse-mode yardstick
for ONE gradient), and ``forward_gradient_`` alone at K = 16, in ONE process, alternating.

The setup is tools/bench_tangent.py's (16 channels, 72x72, torus r = 4 K = 8, hash fire 0.5, T = 32, a fully
alive canvas, an all-true ``nsteps``) at B = 128 and B = 1024; every timed call is bracketed by device
synchronises; a repeat is the mean over a window of at least ``--window`` seconds per path; per batch size one
JSON line with the per-repeat values, their median and min-max.  The rollouts are in ms per step, forward_grad
in ms per call.

    python tools/bench_objective_tangent.py [--batch 128 1024] [--repeats 5] [--window 1.0] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_neural_cellular_automata_amd import ParamDirections, forward_gradient_  # noqa: E402
from tools.bench_tangent import H, T, setup, timed  # noqa: E402

K = 8


def paths(model, x, kw, dev):
    B = x.shape[0]
    g = torch.Generator(device=dev).manual_seed(77)
    target = torch.rand(B, 4, H, H, device=dev, generator=g)
    dirs = ParamDirections(model, K, seed=1).normal_(0.0, 0.01)
    dps = dirs.dicts()
    dirs16 = ParamDirections(model, 16, seed=2).normal_()
    dl16 = torch.randn(T, 16, B, dtype=torch.float64, device=dev, generator=g)

    def objective(every):
        return lambda: model.rollout_objective_tangent(x, T, target, dparams=dps, every=every, **kw).dlosses

    def block():
        return model.rollout_tangent_block(x, None, T, orthonormalize=False, dparams=dps, **kw).v_final

    def reverse():
        model.zero_grad(set_to_none=True)
        out = model.rollout_objective(x, T, target, every=1, checkpoint_every="auto", **kw)
        out.losses.sum(0).mean().backward()

    def fgrad():
        return forward_gradient_(model, dl16, dirs16)

    return {"objective_tangent_every1": (objective(1), T), "objective_tangent_everyT": (objective(T), T),
            "tangent_block": (block, T), "rollout_objective_fwd_bwd": (reverse, T), "forward_gradient_K16": (fgrad, 1)}


def bench(B, repeats, window, dev):
    model, x, _, kw = setup(B, dev)
    P = paths(model, x, kw, dev)
    for fn, _ in P.values():   # warm-up: plans, workspaces, function attributes, the allocator
        for _ in range(2):
            timed(fn)
    rows = {p: [] for p in P}
    for _ in range(repeats):
        for p, (fn, div) in P.items():
            tot, n = 0.0, 0
            t_end = time.perf_counter() + window
            while time.perf_counter() < t_end or n == 0:
                tot += timed(fn)
                n += 1
            rows[p].append(1e3 * tot / n / div)
    res = dict(B=B, C=16, H=H, W=H, hidden=128, radius=4, K_offsets=8, dirs=K, fire_rate=0.5, steps=T, repeats=repeats,
               window_s=window, unit="ms per step (forward_gradient_K16: ms per call)")
    for p in P:
        res[p] = dict(per_repeat=[round(r, 4) for r in rows[p]], median=round(statistics.median(rows[p]), 4),
                      min=round(min(rows[p]), 4), max=round(max(rows[p]), 4))
    m = lambda p: res[p]["median"]   # noqa: E731
    # per tap: (every = 1 minus the block) is R = T taps over T steps, so the per-step difference IS the per-tap cost
    res["per_tap_ms"] = round(m("objective_tangent_every1") - m("tangent_block"), 4)
    res["tap_share_of_every1"] = round(res["per_tap_ms"] / m("objective_tangent_every1"), 4)
    res["every1_over_reverse"] = round(m("objective_tangent_every1") / m("rollout_objective_fwd_bwd"), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective_tangent needs a ROCm GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    for B in a.batch:
        line = json.dumps(bench(B, a.repeats, a.window, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
