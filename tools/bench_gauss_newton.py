#!/usr/bin/env python
"""What one Gauss-Newton product costs: ``model.rollout_gauss_newton(dparams=)`` (a) against the two calls a caller
would otherwise chain for it, ``model.rollout_tangent(dparams=)`` (b, the forward half) and
``model.rollout_objective(recompute=True)`` forward plus backward (c, the tape and the BPTT), on the same schedule,
in ONE process, alternating.  The product shares one primal forward with the tape, so the design predicts
a / (b + c) below 1.

The setup is tools/bench_tangent.py's (16 channels, 72x72, torus r = 4 K = 8, hash fire 0.5, T = 32, a fully
alive canvas, an all-true ``nsteps``) with a tap every 8 steps, at B = 128 and B = 1024; every timed call is
bracketed by device synchronises; a repeat is the mean over a window of at least ``--window`` seconds per path;
per batch size one JSON line with the per-repeat values, their median and min-max, in ms per step.

    python tools/bench_gauss_newton.py [--batch 128 1024] [--repeats 5] [--window 1.0] [--out FILE]
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

from tools.bench_tangent import H, T, direction, setup, timed  # noqa: E402

EVERY = 8


def paths(model, x, kw, dev):
    B = x.shape[0]
    g = torch.Generator(device=dev).manual_seed(77)
    target = torch.rand(B, 4, H, H, device=dev, generator=g)
    dp = direction(model, dev)

    def product():
        return model.rollout_gauss_newton(x, T, target, dparams=dp, every=EVERY, **kw).product

    def tangent():
        return model.rollout_tangent(x, None, T, dparams=dp, **kw).v_final

    def reverse():
        model.zero_grad(set_to_none=True)
        out = model.rollout_objective(x, T, target, every=EVERY, recompute=True, **kw)
        out.losses.sum(0).mean().backward()

    return {"gauss_newton_product": product, "rollout_tangent_dparams": tangent,
            "rollout_objective_recompute_fwd_bwd": reverse}


def bench(B, repeats, window, dev):
    model, x, _, kw = setup(B, dev)
    P = paths(model, x, kw, dev)
    for fn in P.values():   # warm-up: plans, workspaces, function attributes, the allocator
        for _ in range(2):
            timed(fn)
    rows = {p: [] for p in P}
    for _ in range(repeats):
        for p, fn in P.items():
            tot, n = 0.0, 0
            t_end = time.perf_counter() + window
            while time.perf_counter() < t_end or n == 0:
                tot += timed(fn)
                n += 1
            rows[p].append(1e3 * tot / n / T)
    res = dict(B=B, C=16, H=H, W=H, hidden=128, radius=4, K_offsets=8, fire_rate=0.5, steps=T, every=EVERY,
               repeats=repeats, window_s=window, unit="ms per step")
    for p in P:
        res[p] = dict(per_repeat=[round(r, 4) for r in rows[p]], median=round(statistics.median(rows[p]), 4),
                      min=round(min(rows[p]), 4), max=round(max(rows[p]), 4))
    a, b, c = (rows[p] for p in P)
    ratios = [a[i] / (b[i] + c[i]) for i in range(repeats)]
    res["a_over_b_plus_c"] = dict(per_repeat=[round(r, 4) for r in ratios], median=round(statistics.median(ratios), 4),
                                  min=round(min(ratios), 4), max=round(max(ratios), 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gauss_newton needs a ROCm GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    for B in a.batch:
        line = json.dumps(bench(B, a.repeats, a.window, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
