#!/usr/bin/env python
"""A/B of the graph diagnostics: ``graph.diagnostics(x)`` (gnca_graph_diag: field, gather and finish
kernels) against ``graph.attention_map(x)`` alone (what the extra planes cost on top of the map) and
against a torch-op restatement of the same decomposition on the device, written from the formulas of
include/gnca.h and looping over the samples, as a user who wants these panels must today (the
reference's debugger asserts B == 1).  ONE process, alternating paths.

Shape: 16 channels, 72^2, r=4, K=8, torus; B = 1, 8, 128.  Each repeat times a window of at least
``--window`` seconds per path, every timed unit ending in a device synchronise; the per-call means are
printed per repeat (the spread) with their median.

    python tools/bench_diag.py [--repeats 5] [--window 1.0] [--out profiles/diag.json]
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

from graph_neural_cellular_automata_amd import GraphAugmentation  # noqa: E402

H, C, K = 72, 16, 8


def setup(B, dev):
    torch.manual_seed(0)
    graph = GraphAugmentation(C, d_model=16, attention_radius=4, num_neighbors=K, alive_to_alive=True,
                              zero_padded_shift=False, alpha_thr=0.12).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(31)
    x = torch.rand(B, C, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, C - 4, H, H, device=dev, generator=g)
    x[:, 3, : H // 3] = 0.0      # a dead region: the sender mask matters
    return graph, x


@torch.no_grad()
def torch_restatement(graph, x, chosen):
    """The fields of ``GraphDiagnostics`` in torch ops, one sample at a time (torus: w_o = 1/k)."""
    k = len(chosen)
    w = 1.0 / k
    out = []
    for b in range(x.shape[0]):
        xb = x[b:b + 1]
        m = graph.msg_proj(xb).abs()
        alive = (F.max_pool2d(xb[:, 3:4], 3, 1, 1) > graph.alpha_thr).float()
        src = alive if graph.alive_to_alive else torch.ones_like(alive)
        G = torch.cat([m[:, :3].mean(1, keepdim=True), m[:, 3:4], m[:, 4:].mean(1, keepdim=True)], 1)
        S = src * m.mean(1, keepdim=True)
        planes = torch.cat([S, src * G, src], 1)                     # [1,5,H,W]: one roll per offset
        rolled = torch.stack([torch.roll(planes, (dy, dx), (2, 3)) for dy, dx in chosen], 0)[:, 0]   # [k,5,H,W]
        taps = w * rolled[:, 0]
        raw = taps.sum(0)
        groups = w * rolled[:, 1:4].sum(0)
        union = rolled[:, 4].amax(0) if graph.alive_to_alive else torch.zeros_like(raw)
        attn = (raw - raw.min()) / (raw.max() - raw.min() + 1e-8)
        out.append((G[0], groups, taps, raw, attn, union, alive[0, 0]))
    return [torch.stack(f, 0) for f in zip(*out)]


def windows(paths, repeats, window):
    """paths: name -> (zero-argument callable, calls it makes).  Per repeat and path: seconds per call."""
    for fn, _ in paths.values():   # warm-up (workspaces, allocator, code objects)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = {p: [] for p in paths}
    for _ in range(repeats):
        for p, (fn, inner) in paths.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < window or n == 0:
                fn()
                torch.cuda.synchronize()
                n += 1
            rows[p].append((time.perf_counter() - t0) / (n * inner))
    return rows


def bench(B, repeats, window, dev, inner=20):
    graph, x = setup(B, dev)
    random.seed(6)
    chosen = graph.sample_offsets()

    def many(fn):
        def run():
            for _ in range(inner):
                fn()
        return run

    # the restatement agrees with the op (loosely: this is a benchmark, tests/test_gpu_diag.py is the test)
    d = graph.diagnostics(x, offsets=chosen)
    ref = torch_restatement(graph, x, chosen)
    for got, want in zip((d.magnitude, d.groups, d.per_offset, d.raw, d.attention, d.sender_union, d.receiver), ref):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), "restatement"
    paths = {"attention_map": (many(lambda: graph.attention_map(x, offsets=chosen)), inner),
             "diagnostics": (many(lambda: graph.diagnostics(x, offsets=chosen)), inner),
             "diagnostics_no_taps": (many(lambda: graph.diagnostics(x, offsets=chosen, per_offset=False)), inner),
             "torch_per_sample": (lambda: torch_restatement(graph, x, chosen), 1)}
    rows = windows(paths, repeats, window)
    res = dict(bench="graph_diagnostics", B=B, C=C, H=H, k=K, shift="torus", repeats=repeats, window_s=window,
               calls_per_sync=inner)
    for p, r in rows.items():
        us = [1e6 * s for s in r]
        res[p] = dict(us_per_call=[round(v, 2) for v in us], us_per_call_median=round(statistics.median(us), 2))
    med = lambda p: res[p]["us_per_call_median"]
    res["diagnostics_over_attention_map"] = round(med("diagnostics") / med("attention_map"), 2)
    res["torch_over_diagnostics"] = round(med("torch_per_sample") / med("diagnostics"), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of at least 5 windows)")
    if not torch.cuda.is_available():
        sys.exit("bench_diag.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    results = []
    for B in (1, 8, 128):
        results.append(bench(B, a.repeats, a.window, dev))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
