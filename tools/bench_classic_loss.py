#!/usr/bin/env python
"""What the classic trainer's objective costs on the device, fused against the torch formulas, in ONE
process on one GPU:

(a) forward + backward of ``masked_loss(state[:, :4], target).mean()`` (gnca_loss_masked_f32 and its
    backward: one launch each) against the same formula as a chain of torch ops
    (``train_intermediate_loss.py:37-51``), on the same device tensors;
(b) forward + backward of ``stability_loss(state[:, :4], target, close)`` with half the batch close against
    ``if close.any(): F.mse_loss(state[close, :4], target[close])`` (the boolean-index gathers and the
    host wait of ``:256-267``),

at B=16 x 40^2 (the config's shape), B=128 x 72^2 and B=1024 x 72^2, 16-channel states.

Each repeat times a window of at least ``--window`` seconds per path, the two paths alternating, every
window ending in a device synchronise (``--inner`` iterations between synchronises, so that the host's
launch cost shows where it binds); per-repeat means (the spread) and their median are printed.

    python tools/bench_classic_loss.py [--repeats 5] [--window 1.0] [--out profiles/classic_loss.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_neural_cellular_automata_amd.loss import masked_loss, stability_loss  # noqa: E402

SHAPES = [(16, 40), (128, 72), (1024, 72)]


def torch_masked(pred, target, alpha_thr=0.2, lam_area=5e-5):
    mask = (target[:, 3:4] > alpha_thr).float()
    per = (((pred - target) ** 2) * mask).sum(dim=(1, 2, 3)) / (mask.sum(dim=(1, 2, 3)) + 1e-8)
    return per + lam_area * pred[:, 3:4].mean(dim=(1, 2, 3))


def torch_stability(pred, target, close):
    if close.any():   # the trainer's host wait
        return F.mse_loss(pred[close], target[close])
    return pred.sum() * 0.0


def windows(paths, repeats, window, inner):
    """paths: name -> zero-argument callable.  Per repeat and path: mean seconds per call."""
    for fn in paths.values():   # warm-up (allocator, code objects)
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rows = {p: [] for p in paths}
    for _ in range(repeats):
        for p, fn in paths.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < window or n == 0:
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                n += inner
            rows[p].append((time.perf_counter() - t0) / n)
    return rows


def bench(B, H, repeats, window, inner, dev):
    g = torch.Generator(device=dev).manual_seed(31)
    state = torch.rand(B, 16, H, H, device=dev, generator=g).requires_grad_(True)
    target = torch.rand(B, 4, H, H, device=dev, generator=g)     # per-sample targets: both paths read B of them
    close = torch.arange(B, device=dev) % 2 == 0

    def run(loss_fn):
        def call():
            state.grad = None
            loss_fn().backward()
        return call

    paths = {
        "masked_fused": run(lambda: masked_loss(state[:, :4], target).mean()),
        "masked_torch": run(lambda: torch_masked(state[:, :4], target).mean()),
        "stability_fused": run(lambda: stability_loss(state[:, :4], target, close)),
        "stability_torch": run(lambda: torch_stability(state[:, :4], target, close)),
    }
    rows = windows(paths, repeats, window, inner)
    res = dict(bench="classic_loss", B=B, C=16, H=H, W=H, repeats=repeats, window_s=window, calls_per_sync=inner,
               what="forward + backward to state.grad, microseconds per iteration")
    for p, r in rows.items():
        us = [1e6 * s for s in r]
        res[p] = dict(us=[round(v, 2) for v in us], us_median=round(statistics.median(us), 2),
                      us_min=round(min(us), 2), us_max=round(max(us), 2))
    for k in ("masked", "stability"):
        res[f"{k}_torch_over_fused"] = round(res[f"{k}_torch"]["us_median"] / res[f"{k}_fused"]["us_median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--inner", type=int, default=20, help="iterations between device synchronises")
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of at least 5 windows)")
    if not torch.cuda.is_available():
        sys.exit("bench_classic_loss.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    results = []
    for B, H in SHAPES:
        results.append(bench(B, H, a.repeats, a.window, a.inner, dev))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
