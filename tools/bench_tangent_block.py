#!/usr/bin/env python
"""What a direction of a tangent block costs: ``model.rollout_tangent_block`` (K directions beside one
primal state, re-orthonormalised on the device at every recorded step) against the only way to carry K
directions without it, K separate ``model.rollout_tangent(renormalize=True)`` calls, in ONE process,
alternating, on identical seeded schedules.

16 channels, 72x72, torus, r = 4, 8 offsets per step, fire rate 0.5 (hash masks), T = 32, recorded
every 8 steps, a fully alive canvas (RGB and alpha uniform, hidden channels normal), B = 128, blocks
of K = 1, 4 and 8 directions.  Every timed call is bracketed by device synchronises; a repeat is the
mean over a window of at least ``--window`` seconds per path; per K one JSON line with the per-repeat
values, their median and min-max, in ms per step per direction.

    python tools/bench_tangent_block.py [--dirs 1 4 8] [--batch 128] [--repeats 5] [--window 1.0]
    python tools/bench_tangent_block.py --only block --dirs 8      # three calls, for a kernel trace
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

T, EVERY, H, RATE, GAIN, SEED = 32, 8, 72, 0.5, 0.25, 11


def setup(B, K, dev):
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=GAIN, graph_attention_radius=4,
                          graph_num_neighbors=8, graph_zero_padded_shift=False).to(dev)
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.02)
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.rand(B, 16, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, 12, H, H, device=dev, generator=g)
    V = torch.randn(K, B, 16, H, H, device=dev, generator=g)
    random.seed(6)
    offs = [model.graph.sample_offsets() for _ in range(T)]
    nsteps = torch.full((B,), T, dtype=torch.int32, device=dev)
    kw = dict(fire_rate=RATE, seed=SEED, offsets=offs, nsteps=nsteps, every=EVERY)
    return model, x, V, kw


def run_block(model, x, V, kw):
    return model.rollout_tangent_block(x, V, T, **kw).log_r


def run_separate(model, x, V, kw):
    return [model.rollout_tangent(x, V[j], T, renormalize=True, **kw).log_norm for j in range(V.shape[0])]


PATHS = {"block": run_block, "separate": run_separate}


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(B, K, repeats, window, dev):
    args = setup(B, K, dev)
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
            rows[p].append(1e3 * tot / n / T / K)
    res = dict(B=B, dirs=K, C=16, H=H, W=H, hidden=128, radius=4, K_offsets=8, fire_rate=RATE, steps=T, every=EVERY,
               repeats=repeats, window_s=window, unit="ms per step per direction")
    for p in PATHS:
        res[p] = dict(per_repeat=[round(r, 4) for r in rows[p]], median=round(statistics.median(rows[p]), 4),
                      min=round(min(rows[p]), 4), max=round(max(rows[p]), 4))
    res["block_over_separate"] = round(res["block"]["median"] / res["separate"]["median"], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dirs", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--only", default=None, choices=list(PATHS), help="run one path three times per K (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tangent_block needs a ROCm GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    for K in a.dirs:
        if a.only:
            args = setup(a.batch, K, dev)
            for _ in range(3):
                timed(PATHS[a.only], *args)
            continue
        bench(a.batch, K, a.repeats, a.window, dev)


if __name__ == "__main__":
    main()
