"""Generate tests/golden/loss/loss_*.npz by running the REFERENCE trainers' ``masked_loss`` functions
(src/training/train_intermediate_loss.py:37-51, src/training/train_graph_augmented_nca.py:30-49) and,
for the stability term, ``F.mse_loss`` on the boolean-indexed tensors as the trainers do (:256-267).

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss.py

The trainer modules import tensorboard, skimage, matplotlib and tqdm at their top; whichever of those
is not installed gets an empty stand-in module before the import (the loss functions use none of them).

Each fixture: the inputs (pred, target, close, g), the knobs, the reference's float32 value and autograd
gradient, and the same from the same functions on a float64 ``pred`` (the target stays float32 where
the reference compares it with ``alpha_thr``, so the alive mask is the float32 code's).  Data only.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src"))
sys.dont_write_bytecode = True
# a folder of their own: the forward-fixture tests take every tests/golden/*.npz for a step fixture
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loss")


def _stand_in(name, **attrs):
    """An empty module under ``name`` (and its parents) unless the real one imports."""
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sub = ".".join(parts[:i])
        if sub not in sys.modules or i == len(parts):
            m = types.ModuleType(sub)
            m.__path__ = []
            sys.modules[sub] = m
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], m)
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


_stand_in("torch.utils.tensorboard", SummaryWriter=object)
_stand_in("skimage.metrics", peak_signal_noise_ratio=None, structural_similarity=None)
_stand_in("matplotlib.pyplot")
_stand_in("tqdm", trange=range)

from training import train_graph_augmented_nca as TG  # noqa: E402  (reference)
from training import train_intermediate_loss as TC  # noqa: E402  (reference)

B, H, W = 3, 9, 13


def inputs(seed, alpha_thr):
    """pred in [-0.2, 1.2]; target 0 mixed with one alpha cell exactly float32(alpha_thr) (dead), target 1
    with no alive cell, target 2 alive everywhere; dead cells of sample 0 with rgb exactly 0 and negative."""
    rng = np.random.default_rng(seed)
    pred = (rng.random((B, 4, H, W), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
    target = rng.random((B, 4, H, W), dtype=np.float32)
    thr32 = np.float32(alpha_thr)
    target[1, 3] = target[1, 3] * thr32 * np.float32(0.99)          # all <= thr: nothing alive
    target[2, 3] = np.float32(0.5) + np.float32(0.5) * target[2, 3]  # all alive
    target[0, 3, 2, 5] = thr32                                       # equal: dead in float32
    target[0, 3, 4, 4] = np.nextafter(thr32, np.float32(1))          # one ulp above: alive
    target[0, 3, 0, :4] = 0                                          # dead cells ...
    pred[0, :3, 0, 0] = 0                                            # ... with rgb exactly 0,
    pred[0, 1, 0, 1] = 0
    pred[0, :3, 0, 2] = np.float32(-0.15)                            # ... negative,
    pred[0, 2, 0, 3] = np.float32(-0.0)                              # ... and a negative zero
    pred[0, 0, 2, 5] = 0                                             # (the threshold cell: dead, rgb 0)
    assert (pred < 0).any() and (pred.min() >= -0.2) and (pred.max() <= 1.2)
    alive = target[:, 3] > thr32
    assert alive[0].any() and not alive[0].all() and not alive[1].any() and alive[2].all()
    assert not alive[0, 2, 5] and alive[0, 4, 4]
    if alpha_thr == 0.2:   # float32(0.2) > 0.2: a float64 comparison calls the threshold cell alive
        assert float(target[0, 3, 2, 5]) > alpha_thr
    return pred, target


def run(fn, pred, target, g, dtype, *knobs):
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    per = fn(p, torch.from_numpy(target), *knobs)
    (per * torch.from_numpy(g).to(per.dtype)).sum().backward()
    return per.detach().numpy(), p.grad.numpy()


def stability(pred, target, close, gs, dtype):
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    t = torch.from_numpy(target).to(dtype)
    idx = torch.from_numpy(close)
    loss = F.mse_loss(p[idx, :4], t[idx])
    (loss * gs).backward()
    return loss.detach().numpy(), p.grad.numpy()


def make(name, seed, trainer, alpha_thr, lam_area, lam_bg_alpha=None, lam_bg_rgb=None):
    pred, target = inputs(seed, alpha_thr)
    g = np.arange(1, B + 1, dtype=np.float32) * np.float32(0.5)
    knobs = (alpha_thr, lam_area) if trainer == "classic" else (alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb)
    fn = TC.masked_loss if trainer == "classic" else TG.masked_loss
    v32, g32 = run(fn, pred, target, g, torch.float32, *knobs)
    v64, g64 = run(fn, pred, target, g, torch.float64, *knobs)
    assert v32.dtype == np.float32 and v64.dtype == np.float64 and g64.dtype == np.float64
    if trainer == "classic":   # the classic function is the graph function with zero background knobs
        w32, h32 = run(TG.masked_loss, pred, target, g, torch.float32, alpha_thr, lam_area, 0.0, 0.0)
        assert np.array_equal(v32, w32) and np.array_equal(g32, h32)
    close = np.array([True, False, True])
    gs = 0.5
    s32, sg32 = stability(pred, target, close, gs, torch.float32)
    s64, sg64 = stability(pred, target, close, gs, torch.float64)
    meta = dict(trainer=trainer, alpha_thr=alpha_thr, lam_area=lam_area, lam_bg_alpha=lam_bg_alpha or 0.0,
                lam_bg_rgb=lam_bg_rgb or 0.0, stability_g=gs)
    np.savez_compressed(os.path.join(OUT, f"loss_{name}.npz"), pred=pred, target=target, g=g, close=close,
                        meta=np.array(json.dumps(meta)), value_f32=v32, grad_f32=g32, value_f64=v64, grad_f64=g64,
                        stab_f32=s32, stab_grad_f32=sg32, stab_f64=s64, stab_grad_f64=sg64)
    print(name, meta, v32, float(np.abs(v32 - v64).max() / np.abs(v64).max()))


def main():
    os.makedirs(OUT, exist_ok=True)
    make("knobs_b3_9x13", 1, "graph", 0.2, 0.3, 0.7, 0.4)          # every term visible
    make("config_b3_9x13", 2, "graph", 0.12, 0.0, 0.0, 0.0)        # configs/config.json's values
    make("graphdef_b3_9x13", 3, "graph", 0.2, 5e-5, 1e-3, 2e-4)    # the graph trainer's defaults
    make("classic_b3_9x13", 4, "classic", 0.2, 5e-5)               # the classic trainer's function and defaults


if __name__ == "__main__":
    main()
