"""The float64 oracle of the state vitals (include/gnca.h, gnca_state_vitals): a numpy restatement of
the 13 definitions.  ``alive`` goes through ``torch.nn.functional.max_pool2d`` on the CPU, which is the
model's own ``_alive_mask``.  Comparisons are float32 against the float32 threshold, sums float64."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

FIELDS = ("alive", "mature", "alpha_sum", "mass", "cy", "cx", "y0", "y1", "x0", "x1", "max_abs", "nonfinite",
          "hidden_rms")
SUM_FIELDS = ("alpha_sum", "mass", "cy", "cx", "hidden_rms")


def alive_mask(x: np.ndarray, alpha_thr: float) -> np.ndarray:
    """[B,H,W] bool: ``max_pool2d(alpha, 3, 1, 1) > alpha_thr`` (the padding never wins: -inf)."""
    a = torch.from_numpy(np.ascontiguousarray(x[:, 3:4], dtype=np.float32))
    return (F.max_pool2d(a, 3, stride=1, padding=1) > float(np.float32(alpha_thr)))[:, 0].numpy()


def state_vitals(x: np.ndarray, alpha_thr: float) -> np.ndarray:
    """[B,13] float64 for the float32 state ``x`` [B,C>=4,H,W]."""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    thr = np.float32(alpha_thr)
    out = np.zeros((B, len(FIELDS)), dtype=np.float64)
    alive = alive_mask(x, alpha_thr)
    ii, jj = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            a = x[b, 3]
            mature = a > thr
            clip = np.clip(a, np.float32(0), np.float32(1)).astype(np.float64)
            mass = clip.sum()
            out[b, 0] = alive[b].sum()
            out[b, 1] = mature.sum()
            out[b, 2] = a.astype(np.float64).sum()
            out[b, 3] = mass
            out[b, 4] = np.float64((clip * ii).sum()) / np.float64(mass)
            out[b, 5] = np.float64((clip * jj).sum()) / np.float64(mass)
            if mature.any():
                rows, cols = np.nonzero(mature.any(axis=1))[0], np.nonzero(mature.any(axis=0))[0]
                out[b, 6:10] = rows[0], rows[-1], cols[0], cols[-1]
            else:
                out[b, 6:10] = -1
            v = x[b].astype(np.float64)
            fin = np.isfinite(v)
            out[b, 10] = np.abs(v[fin]).max() if fin.any() else 0.0
            out[b, 11] = (~fin).sum()
            if C > 4:
                h = np.where(fin[4:], v[4:], 0.0)
                out[b, 12] = np.sqrt((h * h).sum() / (np.float64(C - 4) * H * W))
    return out


def sum_terms(x: np.ndarray) -> dict:
    """For each sum behind a SUM_FIELDS entry of sample-batch ``x``: (number of terms, [B] sum of the
    terms' magnitudes), the two factors of the rounding bound n * 2^-52 * sum|term|."""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    a = x[:, 3].astype(np.float64)
    clip = np.clip(x[:, 3], np.float32(0), np.float32(1)).astype(np.float64)
    ii, jj = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    h = x[:, 4:].astype(np.float64)
    h = np.where(np.isfinite(h), h, 0.0)
    return {"alpha_sum": (H * W, np.abs(a).sum(axis=(1, 2))),
            "mass": (H * W, clip.sum(axis=(1, 2))),
            "sy": (H * W, (clip * ii).sum(axis=(1, 2))),
            "sx": (H * W, (clip * jj).sum(axis=(1, 2))),
            "hidden_sq": ((C - 4) * H * W, (h * h).sum(axis=(1, 2, 3)))}
