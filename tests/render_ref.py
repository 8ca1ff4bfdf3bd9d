"""Torch-CPU restatement of the uint8 rendering (include/gnca.h, gnca_render_u8 / gnca_colorize_u8).

Everything is float32, as the kernels' arithmetic: the alive mask ``alpha > float32(thr)`` (strict),
the pre-clip of the ``rgb`` mode, bilinear resampling with half-pixel centres written out tap by tap
(``src = max((dst + 0.5) / s - 0.5, 0)``; rows first horizontally, then vertically, the nesting of
``F.interpolate``'s CPU kernel), the clip and ``trunc(255 v)``.  ``colorize`` is ``attn_to_rgb``'s
normalisation per map and the table lookup ``min(int(256 z), 255)``.
"""
import numpy as np
import torch


def axis_taps(n: int, s: int):
    """(i0, i1, l0, l1) of the n*s output positions of one axis: int64 / float32 tensors."""
    dst = torch.arange(n * s, dtype=torch.float32)
    src = torch.clamp((dst + 0.5) / float(s) - 0.5, min=0.0)
    i0 = src.floor().long()
    i1 = torch.clamp(i0 + 1, max=n - 1)
    l1 = src - i0.float()
    return i0, i1, 1.0 - l1, l1


def resample(v: torch.Tensor, s: int) -> torch.Tensor:
    """[..., H, W] float32 -> [..., H*s, W*s]."""
    H, W = v.shape[-2:]
    y0, y1, ly0, ly1 = axis_taps(H, s)
    x0, x1, lx0, lx1 = axis_taps(W, s)
    top, bot = v[..., y0, :], v[..., y1, :]
    h0 = lx0 * top[..., x0] + lx1 * top[..., x1]
    h1 = lx0 * bot[..., x0] + lx1 * bot[..., x1]
    return ly0[:, None] * h0 + ly1[:, None] * h1


def to_u8(v: torch.Tensor) -> torch.Tensor:
    return (torch.clamp(v, 0.0, 1.0) * 255.0).to(torch.int32).to(torch.uint8)     # truncation


def render_rgb(state, alpha_thr=0.1, upscale=1, mode="rgb") -> torch.Tensor:
    """uint8 [..., H*s, W*s, 3|4] of a float32 [..., C>=4, H, W] state."""
    x = torch.as_tensor(state, dtype=torch.float32)
    thr = torch.tensor(float(alpha_thr), dtype=torch.float32)
    m = (x[..., 3:4, :, :] > thr).float()
    rgb = x[..., :3, :, :] * m
    v = torch.clamp(rgb, 0.0, 1.0) if mode == "rgb" else torch.cat([rgb, m], dim=-3)
    return to_u8(resample(v, int(upscale))).movedim(-3, -1).contiguous()


def lut_index(maps, norm="max") -> torch.Tensor:
    """int64 [..., H, W] table indices; every [H,W] map normalises on its own."""
    a = torch.as_tensor(maps, dtype=torch.float32)
    mx = a.amax(dim=(-2, -1), keepdim=True)
    if norm == "max":
        z = torch.clamp(a / (mx + torch.tensor(1e-8, dtype=torch.float32)), 0.0, 1.0)
        z = torch.where(mx > 0, z, torch.zeros_like(z))
    else:
        mn = a.amin(dim=(-2, -1), keepdim=True)
        den = mx - mn
        z = torch.where(den > 0, (a - mn) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(a))
    return torch.clamp((z * 256.0).to(torch.int64), max=255)


def colorize(maps, table, norm="max") -> torch.Tensor:
    """uint8 [..., H, W, 3]: ``table`` is a uint8 [256,3] tensor."""
    return torch.as_tensor(table)[lut_index(maps, norm)]


def count_diff(got, want):
    """(bytes that differ, largest |difference|) of two uint8 arrays of one shape."""
    g, w = np.asarray(got).astype(np.int16), np.asarray(want).astype(np.int16)
    assert g.shape == w.shape, (g.shape, w.shape)
    d = np.abs(g - w)
    return int((d != 0).sum()), int(d.max()) if d.size else 0
