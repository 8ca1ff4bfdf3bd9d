#!/usr/bin/env python
"""What the device state vitals cost, in ONE process on one GPU:

(a) ``state_vitals(x)``: one pass over the state, B*C*H*W*4 bytes read once;
(b) the same 13 fields composed from torch ops on the device (``torch_vitals`` below);
(c) ``x.clone()``: the copy yardstick (the same bytes read, and written once more);

at B=1024 x 16 x 72^2 (340 MB) and B=128 x 32 x 128^2 (268 MB), and what ``vitals=True`` adds per step
to a 96-step ``trace(every=1, frames=False)`` at B=128 x 16 x 72^2 (torus r=4, K=8, fire 0.5), against
the same trace without it.

Each repeat times a window of at least ``--window`` seconds per path, alternating, every call ending in
a device synchronise; per-repeat means (the spread) and their median are printed.  The number to read:
``vitals_share_of_clone`` = (a)'s bytes/s over (c)'s read bytes/s (the same bytes over each one's time).

    python tools/bench_vitals.py [--repeats 5] [--window 1.0] [--out profiles/vitals.json]
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_neural_cellular_automata_amd import NeuralCAGraph, state_vitals  # noqa: E402

THR, RATE, SEED = 0.12, 0.5, 17


def torch_vitals(x, thr):
    """The 13 fields from torch ops, float64 sums, no host synchronisation: [B,13]."""
    B, C, H, W = x.shape
    a = x[:, 3]
    alive = (F.max_pool2d(x[:, 3:4], 3, 1, 1) > thr).sum((1, 2, 3), dtype=torch.float64)
    m = a > thr
    mature = m.sum((1, 2), dtype=torch.float64)
    asum = a.sum((1, 2), dtype=torch.float64)
    clip = a.clamp(0, 1).double()
    mass = clip.sum((1, 2))
    ii = torch.arange(H, device=x.device, dtype=torch.float64)
    jj = torch.arange(W, device=x.device, dtype=torch.float64)
    cy = (clip.sum(2) * ii).sum(1) / mass
    cx = (clip.sum(1) * jj).sum(1) / mass
    rows, cols = m.any(2), m.any(1)
    none = mature == 0
    big = torch.full_like(ii, float(H + W))
    y0 = torch.where(rows, ii, big[:H]).amin(1)
    y1 = torch.where(rows, ii, -big[:H]).amax(1)
    x0 = torch.where(cols, jj, torch.full_like(jj, float(H + W))).amin(1)
    x1 = torch.where(cols, jj, torch.full_like(jj, -float(H + W))).amax(1)
    neg = -torch.ones_like(y0)
    fin = torch.isfinite(x)
    max_abs = torch.where(fin, x.abs(), torch.zeros_like(x)).amax((1, 2, 3)).double()
    nonfinite = (~fin).sum((1, 2, 3), dtype=torch.float64)
    h = torch.where(fin[:, 4:], x[:, 4:], torch.zeros_like(x[:, 4:]))
    rms = ((h.double() ** 2).sum((1, 2, 3)) / max(1, (C - 4) * H * W)).sqrt()
    return torch.stack([alive, mature, asum, mass, cy, cx, torch.where(none, neg, y0), torch.where(none, neg, y1),
                        torch.where(none, neg, x0), torch.where(none, neg, x1), max_abs, nonfinite, rms], 1)


def windows(paths, repeats, window):
    """paths: name -> zero-argument callable.  Per repeat and path: (mean seconds per call, calls)."""
    for fn in paths.values():   # warm-up (workspaces, allocator, code objects)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = {p: [] for p in paths}
    for _ in range(repeats):
        for p, fn in paths.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < window or n == 0:
                fn()
                torch.cuda.synchronize()
                n += 1
            rows[p].append(((time.perf_counter() - t0) / n, n))
    return rows


def bench_kernel(B, C, H, repeats, window, dev, inner=20):
    g = torch.Generator(device=dev).manual_seed(31)
    x = torch.randn(B, C, H, H, device=dev, generator=g)
    x[:, 3] = torch.rand(B, H, H, device=dev, generator=g) * 1.4 - 0.2
    got, ref = state_vitals(x, THR).stacked, torch_vitals(x, THR)
    exact = [0, 1, 6, 7, 8, 9, 10, 11]
    assert torch.equal(got[:, exact], ref[:, exact]), "state_vitals and its torch composition disagree"
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-9, equal_nan=True)

    def rep(fn):
        def call():
            for _ in range(inner):
                fn()
        return call

    paths = {"state_vitals": rep(lambda: state_vitals(x, THR)), "torch_ops": rep(lambda: torch_vitals(x, THR)),
             "clone": rep(lambda: x.clone())}
    with torch.no_grad():
        rows = windows(paths, repeats, window)
    mb = B * C * H * H * 4 / 1e6
    res = dict(bench="state_vitals", B=B, C=C, H=H, W=H, state_mb=round(mb, 1), repeats=repeats, window_s=window,
               calls_per_sync=inner)
    for p, r in rows.items():
        us = [1e6 * s / inner for s, _ in r]
        med = statistics.median(us)
        res[p] = dict(us_per_call=[round(v, 2) for v in us], us_per_call_median=round(med, 2),
                      state_gb_per_s_median=round(mb / med * 1e3, 1))
    med = lambda p: res[p]["us_per_call_median"]
    res["vitals_share_of_clone"] = round(med("clone") / med("state_vitals"), 3)
    res["torch_ops_over_vitals"] = round(med("torch_ops") / med("state_vitals"), 2)
    return res


def bench_trace(B, T, repeats, window, dev, H=72):
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=THR, message_gain=0.25,
                          graph_zero_padded_shift=False).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.02)
    g = torch.Generator(device=dev).manual_seed(31)
    x = torch.rand(B, 16, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, 12, H, H, device=dev, generator=g)
    random.seed(6)
    kw = dict(every=1, frames=False, fire_rate=RATE, seed=SEED)
    paths = {"trace_bare": lambda: model.trace(x, T, **kw),
             "trace_vitals": lambda: model.trace(x, T, vitals=True, **kw)}
    rows = windows(paths, repeats, window)
    res = dict(bench="trace_vitals", B=B, C=16, H=H, steps=T, every=1, fire_rate=RATE, repeats=repeats,
               window_s=window, state_mb=round(B * 16 * H * H * 4 / 1e6, 1))
    for p, r in rows.items():
        us = [1e6 * s / T for s, _ in r]
        res[p] = dict(us_per_step=[round(v, 2) for v in us], calls=[n for _, n in r],
                      us_per_step_median=round(statistics.median(us), 2))
    med = lambda p: res[p]["us_per_step_median"]
    res["vitals_us_per_step"] = round(med("trace_vitals") - med("trace_bare"), 2)
    res["vitals_per_step_fraction"] = round(res["vitals_us_per_step"] / med("trace_bare"), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of at least 5 windows)")
    if a.window < 1.0:
        ap.error("--window must be at least 1 second")
    if not torch.cuda.is_available():
        sys.exit("bench_vitals.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    results = []
    for B, C, H in ((1024, 16, 72), (128, 32, 128)):
        results.append(bench_kernel(B, C, H, a.repeats, a.window, dev))
        print(json.dumps(results[-1]), flush=True)
    results.append(bench_trace(128, a.steps, a.repeats, a.window, dev))
    print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
