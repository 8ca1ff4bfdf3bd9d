#!/usr/bin/env python
"""A/B of the damage policy in ONE process, alternating the two paths on identical states:

  old   ``damage.apply_damage_policy_`` (host draws, ``torch.rand(1).item()``, torch RNG launches for the
        positions / noise tensors, then ``gnca_damage_f32``), its config forced to one kind;
  new   ``damage.DamagePolicy.apply_`` (``gnca_damage_policy``: one launch, draws on the device), forced
        to the same kind.

Shapes: B=128 x 16 ch x 72^2 and B=16 x 32 ch x 128^2.  Per kind and path, every repeat's figure (the
spread) and the median of:

  device_us   device time per call from device events, with the calls queued behind a blocker kernel so
              that the device runs them back to back: for ``old`` the kind's launches alone (the torch RNG
              launches and ``gnca_damage_f32``, i.e. the primitive without the policy's ``.item()``);
  span_us     ``old`` only: device events around the whole ``apply_damage_policy_`` calls, host round
              trips included (what the stream sees);
  host_us     host time per call on an idle stream (for ``old`` it includes the wait of ``.item()``);
  behind_rollout_us   host time until the call returns when the stream already holds a queued 50-step
              rollout of the same batch: ``old`` waits for the rollout, ``new`` should not.

Every timed call damages a fresh copy of the state (the copies are made outside the timed region), so
the work does not shrink as cells die.

    python tools/bench_damage_policy.py [--repeats 5] [--calls 20] [--out profiles/pr_damage_policy.txt]
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
from graph_neural_cellular_automata_amd import damage as D  # noqa: E402

SHAPES = ((128, 16, 72, 72), (16, 32, 128, 128))
KINDS = ("square", "circle", "stripes", "alpha_drop", "saltpepper", "gaussian", "hidden_noise")
BASE = {"start_epoch": 0, "prob": 1.0, "size_min": 8, "size_max": 14, "alpha_thr": 0.1, "alpha_dropout_p": 0.1,
        "salt_pepper_p": 0.02, "hidden_noise_sigma": 0.1, "gaussian_softness": 0.35}
ROLLOUT_STEPS = 50


def blocker(ms: float) -> None:
    """Keep the stream busy for about ``ms`` so that what is enqueued next runs back to back."""
    a = blocker.a
    for _ in range(max(1, int(ms / blocker.one_ms))):
        torch.mm(a, a, out=blocker.out)


def prepare_blocker(dev) -> None:
    blocker.a = torch.randn(4096, 4096, device=dev)
    blocker.out = torch.empty_like(blocker.a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(blocker.a, blocker.a, out=blocker.out)
    torch.cuda.synchronize()
    e0.record()
    torch.mm(blocker.a, blocker.a, out=blocker.out)
    e1.record()
    torch.cuda.synchronize()
    blocker.one_ms = max(e0.elapsed_time(e1), 1e-3)


def copies(x, n):
    return [x.clone() for _ in range(n)]


def host_us(fn, states) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for st in states:
        fn(st)
    t = time.perf_counter() - t0
    torch.cuda.synchronize()
    return 1e6 * t / len(states)


def device_us(fn, states, hold_ms: float, blocked: bool = True) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if blocked:
        blocker(hold_ms)
    e0.record()
    for st in states:
        fn(st)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / len(states)


def behind_rollout_us(fn, state, model, x) -> float:
    torch.cuda.synchronize()
    with torch.no_grad():
        model.rollout(x, ROLLOUT_STEPS, fire_rate=0.5, seed=1)
    t0 = time.perf_counter()
    fn(state)
    t = time.perf_counter() - t0
    torch.cuda.synchronize()
    return 1e6 * t


def bench_kind(shape, kind, model, x, repeats, calls, dev):
    cfg = dict(BASE, kinds={kind: 1.0})
    policy = D.DamagePolicy(cfg, seed=7, scope="batch")
    forced = D.DamagePolicy.codes([kind] * shape[0], dev)
    event = [0]

    def new(st):
        event[0] += 1
        policy.apply_(st, 0, event[0], kinds=forced)

    def old(st):
        D.apply_damage_policy_(st, cfg, 0)

    knobs = {"alpha_thr": cfg["alpha_thr"], "alpha_dropout_p": cfg["alpha_dropout_p"], "stripe_width": 11,
             "salt_pepper_p": cfg["salt_pepper_p"], "hidden_noise_sigma": cfg["hidden_noise_sigma"],
             "gaussian_softness": cfg["gaussian_softness"]}

    def old_launches(st):          # the kind's launches alone: no .item(), so they can queue behind the blocker
        D._KINDS[kind](st, 11, knobs)

    for fn in (new, old, old_launches):      # warm-up: code objects, allocator
        for st in copies(x, 3):
            fn(st)
    torch.cuda.synchronize()
    rows = {k: [] for k in ("old_device_us", "new_device_us", "old_span_us", "old_host_us", "new_host_us",
                            "old_behind_rollout_us", "new_behind_rollout_us")}
    for _ in range(repeats):
        h_old = host_us(old, copies(x, calls))
        h_new = host_us(new, copies(x, calls))
        rows["old_host_us"].append(h_old)
        rows["new_host_us"].append(h_new)
        hold = 2.0 * calls * max(host_us(old_launches, copies(x, calls)), h_new) / 1e3 + 2.0
        rows["old_device_us"].append(device_us(old_launches, copies(x, calls), hold))
        rows["new_device_us"].append(device_us(new, copies(x, calls), hold))
        rows["old_span_us"].append(device_us(old, copies(x, calls), 0.0, blocked=False))
        rows["old_behind_rollout_us"].append(behind_rollout_us(old, x.clone(), model, x))
        rows["new_behind_rollout_us"].append(behind_rollout_us(new, x.clone(), model, x))
    res = dict(bench="damage_policy", B=shape[0], C=shape[1], H=shape[2], W=shape[3], kind=kind, repeats=repeats,
               calls_per_window=calls)
    for k, v in rows.items():
        res[k] = [round(t, 2) for t in v]
        res[k + "_median"] = round(statistics.median(v), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls (and state copies) per timed window")
    ap.add_argument("--out", default=None, help="also write the table and the result lines to this text file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_damage_policy.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    prepare_blocker(dev)
    results = []
    for shape in SHAPES:
        B, C, H, W = shape
        torch.manual_seed(0)
        random.seed(0)
        model = NeuralCAGraph(C, 128, update_gain=0.05, alpha_thr=0.1, message_gain=0.25).to(dev).eval()
        g = torch.Generator(device=dev).manual_seed(5)
        x = torch.rand(B, C, H, W, device=dev, generator=g)
        for kind in KINDS:
            results.append(bench_kind(shape, kind, model, x, a.repeats, a.calls, dev))
            print(json.dumps(results[-1]), flush=True)
    head = (f"{'shape':>16} {'kind':>12} | {'old dev us':>10} {'new dev us':>10} | {'old span':>9} | "
            f"{'old host':>9} {'new host':>9} | {'old behind':>10} {'new behind':>10}")
    lines = [f"device: {torch.cuda.get_device_name(0)}; medians of {a.repeats} alternating windows of {a.calls} calls; "
             f"microseconds per call; 'behind': host time of one call behind a queued {ROLLOUT_STEPS}-step rollout",
             head, "-" * len(head)]
    for r in results:
        lines.append(f"{r['B']:>4}x{r['C']}x{r['H']}x{r['W']:<4} {r['kind']:>12} | {r['old_device_us_median']:>10.2f} "
                     f"{r['new_device_us_median']:>10.2f} | {r['old_span_us_median']:>9.2f} | "
                     f"{r['old_host_us_median']:>9.2f} {r['new_host_us_median']:>9.2f} | "
                     f"{r['old_behind_rollout_us_median']:>10.1f} {r['new_behind_rollout_us_median']:>10.1f}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n\nper-window figures (the spread):\n")
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
