#!/usr/bin/env python
"""A/B of a recorded rollout: ``model.trace(every=1, return_attention=True)`` (one native call on
the rollout pipeline plus the standalone attention-map kernels) against the per-step loop it replaces
(``model(x, fire_rate, return_attention=True)`` once per CA step, keeping the RGBA frame and the map,
as the regeneration diagnostic and the video generators do), in ONE process, alternating.  Also
``graph.attention_map(x)`` against ``graph(x, return_attention_map=True)``.

Shape: 16 channels, 72^2, r=4, K=8, fire 0.5, torus; B=1 and B=8 for the rollouts, B=1 and B=128 for
the map alone.  Each repeat times a window of at least ``--window`` seconds per path, every call ending
in a device synchronise; the per-call means are printed per repeat (the spread) with their median.

    python tools/bench_trace.py [--steps 64] [--repeats 5] [--window 1.0] [--out profiles/trace.json]
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

H, RATE, SEED = 72, 0.5, 17


def setup(B, dev):
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=0.25,
                          graph_zero_padded_shift=False).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.02)
    g = torch.Generator(device=dev).manual_seed(31)
    x = torch.rand(B, 16, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, 12, H, H, device=dev, generator=g)
    return model, x


def per_step_loop(model, x, T):
    frames, maps = [], []
    with torch.no_grad():
        for _ in range(T):
            x, attn = model(x, RATE, return_attention=True)
            frames.append(x[:, :4].clone())
            maps.append(attn)
    return x, frames, maps


def trace_call(model, x, T):
    tr = model.trace(x, T, every=1, return_attention=True, fire_rate=RATE, seed=SEED)
    return tr.x_final, tr.frames, tr.attention


def windows(paths, repeats, window):
    """paths: name -> zero-argument callable.  Per repeat and path: (mean seconds per call, calls)."""
    for fn in paths.values():   # warm-up (plans, workspaces, allocator, code objects)
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


def bench_rollout(B, T, repeats, window, dev):
    model, x = setup(B, dev)
    random.seed(6)
    rows = windows({"per_step": lambda: per_step_loop(model, x, T), "trace": lambda: trace_call(model, x, T)},
                   repeats, window)
    res = dict(bench="trace_vs_per_step", B=B, C=16, H=H, steps=T, fire_rate=RATE, repeats=repeats, window_s=window)
    for p, r in rows.items():
        us = [1e6 * s / T for s, _ in r]
        res[p] = dict(us_per_step=[round(v, 2) for v in us], calls=[n for _, n in r],
                      us_per_step_median=round(statistics.median(us), 2),
                      mcell_updates_per_s_median=round(B * H * H / statistics.median(us), 1))
    res["speedup_median"] = round(res["per_step"]["us_per_step_median"] / res["trace"]["us_per_step_median"], 2)
    return res


def bench_map(B, repeats, window, dev, inner=50):
    model, x = setup(B, dev)
    graph = model.graph
    random.seed(6)

    def message_path():
        with torch.no_grad():
            for _ in range(inner):
                graph(x, return_attention_map=True)

    def map_path():
        for _ in range(inner):
            graph.attention_map(x)

    rows = windows({"message_with_map": message_path, "attention_map": map_path}, repeats, window)
    res = dict(bench="attention_map_vs_message", B=B, C=16, H=H, repeats=repeats, window_s=window,
               calls_per_sync=inner)
    for p, r in rows.items():
        us = [1e6 * s / inner for s, _ in r]
        res[p] = dict(us_per_call=[round(v, 2) for v in us], us_per_call_median=round(statistics.median(us), 2))
    res["speedup_median"] = round(res["message_with_map"]["us_per_call_median"] /
                                  res["attention_map"]["us_per_call_median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of at least 5 windows)")
    if not torch.cuda.is_available():
        sys.exit("bench_trace.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    results = []
    for B in (1, 8):
        results.append(bench_rollout(B, a.steps, a.repeats, a.window, dev))
        print(json.dumps(results[-1]), flush=True)
    for B in (1, 128):
        results.append(bench_map(B, a.repeats, a.window, dev))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
