#!/usr/bin/env python
"""A/B of the uint8 rendering (``render.render_rgb`` / ``render.colorize``, one HIP launch each) against
what a user could do before it, in ONE process, alternating, on identical inputs:

  new    the new launch;
  torch  the same frame composed from torch device ops (mul, clamp, F.interpolate, clamp, mul(255),
         .to(uint8), permute().contiguous(); for maps: amax, div, clamp, mul(256), .long(), table index);
  host   the per-frame host path of the reference's scripts, for context: copy the frame to the CPU, mask,
         clip, F.interpolate, clip, ``(img * 255).astype(np.uint8)``; for maps: divide by the maximum, clip,
         matplotlib's viridis (a numpy table lookup where matplotlib is not installed), times 255, astype.
         Timed on at most ``HOST_FRAMES`` frames of the batch, reported per frame.

Shapes (72^2, the scripts' grid): frames N=1 s=4 (the scripts' own case), N=512 s=4 (a recorded trace of
64 steps x 8 samples), N=1024 s=1; maps N=1 and N=512.  Each repeat times a window of at least
``--window`` seconds per path; a call ends in a device synchronise every ``calls_per_sync`` calls.  Per
path: the per-call microseconds of every repeat (the spread), their median and, for ``new`` and ``torch``,
the achieved output GB/s (output bytes over the call time: an end-to-end figure that includes the launch
and the allocation, not a kernel's share of the HBM peak).  ``differing_bytes`` counts the bytes in which
``new`` and ``torch`` disagree on the timed input.

    python tools/bench_render.py [--repeats 5] [--window 1.0] [--out profiles/render.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_neural_cellular_automata_amd import CMAPS, colorize, render_rgb  # noqa: E402

H, THR, HOST_FRAMES = 72, 0.1, 8
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E, for the table's last column


def torch_frames(x4, s):
    rgb = (x4[:, :3] * (x4[:, 3:4] > THR).float()).clamp(0, 1)
    if s > 1:
        rgb = F.interpolate(rgb, scale_factor=s, mode="bilinear", align_corners=False).clamp(0, 1)
    return rgb.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def host_frames(x4, s):
    out = []
    for f in x4[:HOST_FRAMES]:
        f = f.cpu()
        img = (f[:3] * (f[3:4] > THR).float()).permute(1, 2, 0).numpy().clip(0, 1)
        if s > 1:
            t = F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], scale_factor=s, mode="bilinear",
                              align_corners=False)[0]
            img = t.permute(1, 2, 0).numpy().clip(0, 1)
        out.append((img * 255).astype(np.uint8))
    return out


def torch_maps(a, table):
    vmax = a.amax(dim=(-2, -1), keepdim=True)
    z = (a / (vmax + 1e-8)).clamp(0, 1)
    return table[(z * 256).long().clamp(max=255)]


def host_maps(a, cm):
    out = []
    for m in a[:HOST_FRAMES]:
        m = m.cpu().numpy()
        z = np.clip(m / (m.max() + 1e-8), 0, 1)
        rgb = cm(z)[..., :3] if callable(cm) else cm[np.minimum((z * 256).astype(np.int64), 255)] / 255.0
        out.append((rgb * 255).astype(np.uint8))
    return out


def windows(paths, repeats, window, inner):
    for fn in paths.values():   # warm-up (code objects, allocator)
        for _ in range(3):
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
            rows[p].append(((time.perf_counter() - t0) / n, n))
    return rows


def report(res, rows, out_bytes, host_n):
    for p, r in rows.items():
        per = host_n if p == "host" else 1
        us = [1e6 * s / per for s, _ in r]
        key = "us_per_frame" if p == "host" else "us_per_call"
        res[p] = {key: [round(v, 2) for v in us], key + "_median": round(statistics.median(us), 2),
                  "calls": [n for _, n in r]}
        if p != "host":
            res[p]["output_gb_per_s_median"] = round(out_bytes / statistics.median(us) / 1e3, 2)
            res[p]["share_of_hbm_peak"] = round(out_bytes / statistics.median(us) / 1e3 / HBM_PEAK_GBS, 4)
    res["new_over_torch_speedup_median"] = round(res["torch"]["us_per_call_median"] / res["new"]["us_per_call_median"], 2)
    return res


def bench_frames(N, s, repeats, window, dev):
    g = torch.Generator(device=dev).manual_seed(31)
    x = torch.rand(N, 16, H, H, device=dev, generator=g) * 1.4 - 0.2
    x4 = x[:, :4]
    inner = 20 if N == 1 else 1
    a, b = render_rgb(x4, THR, s), torch_frames(x4, s)
    differ = int((a != b).sum())
    del a, b
    rows = windows({"new": lambda: render_rgb(x4, THR, s), "torch": lambda: torch_frames(x4, s),
                    "host": lambda: host_frames(x4, s)}, repeats, window, inner)
    out_bytes = N * H * s * H * s * 3
    res = dict(bench="render_rgb", N=N, H=H, W=H, upscale=s, mode="rgb", output_bytes=out_bytes, repeats=repeats,
               window_s=window, calls_per_sync=inner, differing_bytes=differ)
    return report(res, rows, out_bytes, min(N, HOST_FRAMES))


def bench_maps(N, repeats, window, dev):
    g = torch.Generator(device=dev).manual_seed(32)
    a = torch.rand(N, H, H, device=dev, generator=g) * torch.rand(N, 1, 1, device=dev, generator=g)
    table = CMAPS["viridis"].to(dev)
    try:
        from matplotlib import colormaps
        cm = colormaps["viridis"]
    except ImportError:
        cm = CMAPS["viridis"].numpy()
    inner = 20 if N == 1 else 1
    differ = int((colorize(a) != torch_maps(a, table)).sum())
    rows = windows({"new": lambda: colorize(a), "torch": lambda: torch_maps(a, table),
                    "host": lambda: host_maps(a, cm)}, repeats, window, inner)
    out_bytes = N * H * H * 3
    res = dict(bench="colorize", N=N, H=H, W=H, cmap="viridis", norm="max", output_bytes=out_bytes, repeats=repeats,
               window_s=window, calls_per_sync=inner, differing_bytes=differ,
               host_colormap="matplotlib" if callable(cm) else "numpy table")
    return report(res, rows, out_bytes, min(N, HOST_FRAMES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of at least 5 windows)")
    if not torch.cuda.is_available():
        sys.exit("bench_render.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    results = []
    for N, s in ((1, 4), (512, 4), (1024, 1)):
        results.append(bench_frames(N, s, a.repeats, a.window, dev))
        print(json.dumps(results[-1]), flush=True)
    for N in (1, 512):
        results.append(bench_maps(N, a.repeats, a.window, dev))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
