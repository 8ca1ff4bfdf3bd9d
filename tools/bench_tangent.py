#!/usr/bin/env python
"""What a tangent step costs: ``model.rollout_tangent`` against the no-grad scheduled ``model.rollout``
and against ``model.rollout`` with grad (forward with a tape, plus backward), in ONE process,
alternating, on identical seeded schedules.

16 channels, 72x72, torus, r = 4, K = 8, fire rate 0.5 (hash masks), T = 32, a fully alive canvas
(the flagship's state: RGB and alpha uniform, hidden channels normal), at B = 128 and B = 1024.  The
schedule carries an all-true ``nsteps`` so that all three paths run the scheduled entry points
(gnca_rollout_fwd_f32 / gnca_rollout_bwd_f32 / gnca_rollout_tangent) and not the uniform no-grad
pipeline.  Every timed call is bracketed by device synchronises; a repeat is the mean over a window of
at least ``--window`` seconds per path; per batch size one JSON line with the per-repeat values, their
median and min-max, in ms per step.  The yardstick of the tangent is the forward-plus-backward per step.
``--dparams`` adds a fourth leg, ``tangent_dparams``: the same rollout_tangent with a dense direction of every
weight carried beside ``v`` (gnca_rollout_tangent_params).

    python tools/bench_tangent.py [--batch 128 1024] [--repeats 5] [--window 1.0] [--dparams]
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

T, H, RATE, GAIN, SEED = 32, 72, 0.5, 0.25, 11


def setup(B, dev):
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=GAIN, graph_attention_radius=4,
                          graph_num_neighbors=8, graph_zero_padded_shift=False).to(dev)
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.02)
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.rand(B, 16, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, 12, H, H, device=dev, generator=g)
    v = torch.randn(B, 16, H, H, device=dev, generator=g)
    random.seed(6)
    offs = [model.graph.sample_offsets() for _ in range(T)]
    nsteps = torch.full((B,), T, dtype=torch.int32, device=dev)
    kw = dict(fire_rate=RATE, seed=SEED, offsets=offs, nsteps=nsteps)
    return model, x, v, kw


def direction(model, dev):
    """A dense N(0, 0.01) direction of every weight a direction may perturb."""
    g = torch.Generator(device=dev).manual_seed(4321)
    return {n: 0.01 * torch.randn(t.shape, device=dev, generator=g) for n, t in model.param_direction().items()}


def run_tangent(model, x, v, kw):
    return model.rollout_tangent(x, v, T, **kw).v_final


def run_tangent_dparams(model, x, v, kw):
    return model.rollout_tangent(x, v, T, dparams=model._bench_direction, **kw).v_final


def run_nograd(model, x, v, kw):
    with torch.no_grad():
        return model.rollout(x, T, **kw)


def run_grad(model, x, v, kw):
    model.zero_grad(set_to_none=True)
    leaf = x.clone().requires_grad_(True)
    out = model.rollout(leaf, T, **kw)
    out.backward(v)
    return leaf.grad


PATHS = {"tangent": run_tangent, "rollout_nograd": run_nograd, "rollout_fwd_bwd": run_grad}


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(B, repeats, window, dev):
    args = setup(B, dev)
    if "tangent_dparams" in PATHS:
        args[0]._bench_direction = direction(args[0], dev)
    for fn in PATHS.values():   # warm-up: plans, workspaces, function attributes, the allocator
        for _ in range(2):
            timed(fn, *args)
    rows = {p: [] for p in PATHS}
    for _ in range(repeats):
        for p, fn in PATHS.items():
            tot, n = 0.0, 0
            t_end = time.perf_counter() + window
            while time.perf_counter() < t_end or n == 0:
                tot += timed(fn, *args)
                n += 1
            rows[p].append(1e3 * tot / n / T)
    res = dict(B=B, C=16, H=H, W=H, hidden=128, radius=4, K=8, fire_rate=RATE, steps=T, repeats=repeats, window_s=window,
               unit="ms per step")
    for p in PATHS:
        res[p] = dict(per_repeat=[round(r, 4) for r in rows[p]], median=round(statistics.median(rows[p]), 4),
                      min=round(min(rows[p]), 4), max=round(max(rows[p]), 4))
    res["tangent_over_fwd_bwd"] = round(res["tangent"]["median"] / res["rollout_fwd_bwd"]["median"], 4)
    res["tangent_over_nograd"] = round(res["tangent"]["median"] / res["rollout_nograd"]["median"], 4)
    if "tangent_dparams" in PATHS:
        res["dparams_over_tangent"] = round(res["tangent_dparams"]["median"] / res["tangent"]["median"], 4)
        res["dparams_over_fwd_bwd"] = round(res["tangent_dparams"]["median"] / res["rollout_fwd_bwd"]["median"], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--only", default=None, choices=list(PATHS) + ["tangent_dparams"],
                    help="run one path once per batch size (for a kernel trace)")
    ap.add_argument("--dparams", action="store_true", help="add the weight-direction leg (tangent_dparams)")
    a = ap.parse_args()
    if a.dparams or a.only == "tangent_dparams":
        PATHS["tangent_dparams"] = run_tangent_dparams
    if not torch.cuda.is_available():
        raise SystemExit("bench_tangent needs a ROCm GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    for B in a.batch:
        if a.only:
            args = setup(B, dev)
            if a.only == "tangent_dparams":
                args[0]._bench_direction = direction(args[0], dev)
            for _ in range(3):
                timed(PATHS[a.only], *args)
            continue
        bench(B, a.repeats, a.window, dev)


if __name__ == "__main__":
    main()
