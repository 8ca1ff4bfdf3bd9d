#!/usr/bin/env python
"""A/B of one training iteration's tail: gradient policy + optimiser step + pool write-back.

ONE process alternates two paths on the same model, the same gradients and the same pool batch:

  parent   dp.normalize_gradients_ + torch.optim.Adam.step, then the reference's write-back written
           with torch ops (topk, randint().item(), clone, two assignments, index_copy_)
  new      optim.FusedAdam(grad_policy="normalize").step + SamplePool.commit

at the reference's default shape (B=16, 40x40) and the trainer shape (B=128, 72x72), 16 channels,
n_reset = int(0.1 B), with and without the random reseed (the parent's ``.item()`` host wait happens
only with it).  Per repeat and path, ``--calls`` tails are enqueued back to back between two device
synchronises and two events:

  host_us  host wall time per call until the call returns (the enqueue; the parent's includes its
           host wait, which here has only the tail's own work to wait for: in a trainer it would wait
           for everything queued before it)
  done_us  host wall time per call until the device has finished
  gpu_us   device time per call between the events

Medians over ``--repeats`` alternating repeats are printed as one JSON line per shape, after a check
that both paths leave the same parameters (to rounding) and the same pool (bitwise) from one start.

    python tools/bench_trainer_tail.py [--repeats 15] [--calls 20]
    python tools/bench_trainer_tail.py --profile new|parent --calls N   # N tails of one path and nothing
                                        # else, for a kernel trace (two N: the launches per tail)
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

from graph_neural_cellular_automata_amd import NeuralCAGraph, dp  # noqa: E402
from graph_neural_cellular_automata_amd.optim import FusedAdam  # noqa: E402
from graph_neural_cellular_automata_amd.pool import SamplePool  # noqa: E402

SHAPES = {"reference": dict(B=16, H=40, P=1024), "trainer": dict(B=128, H=72, P=256)}
C = 16
OPT = dict(lr=2e-4, weight_decay=1e-5)


class Tail:
    """One path's model, optimiser and pool, with fixed gradients and a fixed sampled batch."""

    def __init__(self, new: bool, B: int, H: int, P: int, dev):
        self.new, self.B, self.dev = new, B, dev
        torch.manual_seed(0)
        random.seed(0)
        self.model = NeuralCAGraph(C, 128, update_gain=0.05, alpha_thr=0.12, message_gain=0.25).to(dev)
        self.params = [p for n, p in self.model.named_parameters()
                       if p.requires_grad and "gate_mlp" not in n]     # the 12 tensors that get gradients
        g = torch.Generator(device=dev).manual_seed(1)
        for p in self.params:
            p.grad = torch.randn(p.shape, device=dev, generator=g)
        self.opt = (FusedAdam(self.model.parameters(), grad_policy="normalize", **OPT) if new
                    else torch.optim.Adam(self.model.parameters(), **OPT))

        def seed_fn(batch_size=1):
            s = torch.zeros(batch_size, C, H, H, device=dev)
            s[:, 3:4, H // 2, H // 2] = 1.0
            return s
        self.seed_fn = seed_fn
        self.pool = SamplePool(P, seed_fn, device=dev)
        self.idx, batch = self.pool.sample(B)
        self.state = batch + 0.5
        self.per = torch.rand(B, device=dev, generator=g)
        self.n_reset = int(0.1 * B)

    def __call__(self, reseed: bool):
        if self.new:
            self.opt.step()
            self.pool.commit(self.idx, self.state, self.per, n_reset=self.n_reset, seed_fn=self.seed_fn,
                             reseed=reseed)
            return
        dp.normalize_gradients_(self.params)
        self.opt.step()
        # train_graph_augmented_nca.py:377-391
        worst = torch.topk(self.per, self.n_reset).indices if self.n_reset > 0 else None
        rand_idx = torch.randint(0, self.B, (1,), device=self.dev).item() if reseed else None
        sfp = self.state.detach()
        if worst is not None or reseed:
            sfp = sfp.clone()
            if worst is not None:
                sfp[worst] = self.seed_fn(len(worst)).detach()
            if reseed:
                sfp[rand_idx:rand_idx + 1] = self.seed_fn(1).detach()
        self.pool.replace(self.idx, sfp)


def agreement(cfg, dev):
    """One tail of each path from the same start: max parameter difference, pool equality."""
    a, b = Tail(False, dev=dev, **cfg), Tail(True, dev=dev, **cfg)
    for t in (a, b):
        torch.manual_seed(3)
        t(True)
    torch.cuda.synchronize()
    dparam = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.model.parameters(), b.model.parameters()))
    return dparam, bool(torch.equal(a.pool.states, b.pool.states))


def timed(tail, reseed, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        tail(reseed)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e6 * (t1 - t0) / calls, 1e6 * (t2 - t0) / calls, 1e3 * e0.elapsed_time(e1) / calls


def bench(name, repeats, calls, dev):
    cfg = SHAPES[name]
    dparam, same_pool = agreement(cfg, dev)
    tails = {"parent": Tail(False, dev=dev, **cfg), "new": Tail(True, dev=dev, **cfg)}
    res = dict(shape=name, B=cfg["B"], H=cfg["H"], channels=C, n_reset=int(0.1 * cfg["B"]), repeats=repeats,
               calls=calls, max_param_diff=f"{dparam:.3e}", pool_bitwise_equal=same_pool)
    for reseed in (False, True):
        for t in tails.values():            # warm-up: code objects, optimiser state, allocator
            for _ in range(5):
                t(reseed)
        rows = {k: [] for k in tails}
        for _ in range(repeats):
            for k, t in tails.items():
                rows[k].append(timed(t, reseed, calls))
        for k in tails:
            med = [round(statistics.median(r[i] for r in rows[k]), 1) for i in range(3)]
            lo = [round(min(r[i] for r in rows[k]), 1) for i in range(3)]
            hi = [round(max(r[i] for r in rows[k]), 1) for i in range(3)]
            res[f"{k}_reseed{int(reseed)}"] = dict(host_us=med[0], done_us=med[1], gpu_us=med[2],
                                                   min=lo, max=hi)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["trainer", "reference", "both"])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--profile", choices=["new", "parent"],
                    help="--calls tails (reseed on) of one path at the reference shape and nothing else")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trainer_tail.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    if a.profile:
        t = Tail(a.profile == "new", dev=dev, **SHAPES["reference"])
        for _ in range(a.calls):
            t(True)
        torch.cuda.synchronize()
        return
    for name in (["reference", "trainer"] if a.shape == "both" else [a.shape]):
        bench(name, a.repeats, a.calls, dev)


if __name__ == "__main__":
    main()
