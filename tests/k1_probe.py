"""Read K1's update field before GroupNorm and tanh — shared by the K1 precision tests.

``gnca_step_phases_f32`` with K0 and K1 only (no K2, no compact field) leaves the dense update field
``(dl + tanh(m + bm S) message_gain) keep`` in the step workspace, where the backward already reads it
(``fwd_layout``).  ``fast_tanh`` and the update gain hide K1's last bits at the step's output; here
they are visible.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_cpu_ref as T
from tests import split_emul as E

# Byte offset of the dense update field (B*C*H*W floats, NCHW) in the step workspace: ``off_dx`` is the
# first carve of ``make_plan`` (gnca_step.hip), handed to the backward by ``fwd_layout`` (FwdLayout::off_dx)
DX_OFFSET_BYTES = 0


def probe_dx(desc, weights, x: torch.Tensor, fire=None) -> torch.Tensor:
    """The [B,C,H,W] float32 update field K1 writes for state ``x``.  The workspace is filled with
    0xFF bytes (NaNs) first, so every value returned, the dead cells' zeros included, was written by
    this launch."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    ws = S.workspace(desc, x.device)
    ws.fill_(0xFF)
    scratch = torch.empty_like(x)
    rc = L.load().gnca_step_phases_f32(ctypes.byref(desc), ctypes.byref(weights), x.data_ptr(), scratch.data_ptr(),
                                       None if fire is None else fire.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                       S.stream_ptr(x.device), L.PHASE_K0 | L.PHASE_K1)
    L.check(rc, "gnca_step_phases_f32")
    n = 4 * x.numel()
    return ws[DX_OFFSET_BYTES:DX_OFFSET_BYTES + n].view(torch.float32).view(x.shape).clone()


class Probe:
    """One K1 variant of ``split_emul.VARIANTS`` on the device: its descriptor (GroupNorm off,
    FIRE_NONE), device weight tensors that are updated in place (the weights struct is built once),
    and the plan's assertion by name."""

    def __init__(self, vid: str, dev, *, message_gain: float = 1.0, offsets=None, a2a: bool = True,
                 hidden_only: bool = True, fire_mask: bool = False):
        from graph_neural_cellular_automata_amd import _lib as L
        from graph_neural_cellular_automata_amd import step as S
        self.vid = vid
        self.name, self.arith, C, HD, H, W, B, nb, k, zp = E.VARIANTS[vid]
        self.C, self.HD, self.H, self.W, self.B, self.nb, self.k, self.zp = C, HD, H, W, B, nb, k, zp
        self.dev = dev
        self.offsets = E.variant_offsets(vid) if offsets is None else offsets
        flags = 0
        if k:
            flags = L.GRAPH | (L.ALIVE_TO_ALIVE if a2a else 0) | (L.HIDDEN_ONLY if hidden_only else 0) | \
                (L.ZERO_PAD_SHIFT if zp else 0)
        self.desc = S.make_desc(B=B, C=C, H=H, W=W, hidden=HD, d_model=16, offsets=self.offsets, flags=flags,
                                update_gain=0.05, alpha_thr=E.ALPHA_THR, message_gain=message_gain, fire_rate=1.0,
                                fire_mode=L.FIRE_MASK_U8 if fire_mask else L.FIRE_NONE)
        planned = S.k1_variant(self.desc)
        assert planned == (self.name, self.arith), f"{vid}: the plan launches {planned}"
        f32 = dict(dtype=torch.float32, device=dev)
        self.t = dict(perception=T.sobel_bank(C).to(dev), w1=torch.zeros(HD, 3 * C, 1, 1, **f32),
                      b1=torch.zeros(HD, **f32), w2=torch.zeros(C, HD, 1, 1, **f32))
        if k:
            g = torch.Generator().manual_seed(3)
            self.t.update(wm=torch.zeros(C, C, 1, 1, **f32), bm=torch.zeros(C, **f32),
                          wq=(torch.randn(16, C, 1, 1, generator=g) * 0.2).to(dev),
                          bq=(torch.randn(16, generator=g) * 0.1).to(dev),
                          wk=(torch.randn(16, C, 1, 1, generator=g) * 0.2).to(dev),
                          bk=(torch.randn(16, generator=g) * 0.1).to(dev), scaling=torch.ones(1, **f32))
        self.w, self._keep = S.make_weights(self.t)

    def set(self, **arrays):
        """Overwrite device weights in place from numpy arrays (w1, b1, w2, wm, bm)."""
        for name, a in arrays.items():
            t = self.t[name]
            t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).view(t.shape))

    def state(self, x_base: np.ndarray) -> torch.Tensor:
        """The batch on the device: the ``nb`` distinct samples repeated to ``B``."""
        xb = torch.from_numpy(np.ascontiguousarray(x_base, np.float32)).to(self.dev)
        assert xb.shape[0] == self.nb and self.B % self.nb == 0
        return xb.repeat(self.B // self.nb, 1, 1, 1).contiguous()

    def dx(self, x: torch.Tensor, fire=None) -> torch.Tensor:
        return probe_dx(self.desc, self.w, x, fire)

    def mismatches(self, dx: torch.Tensor, expect: np.ndarray) -> torch.Tensor:
        """Device count of values of ``dx`` [B,...] that differ from ``expect`` [nb,...] (fp32, every
        repeat of the distinct samples compared; NaNs count as differing)."""
        e = torch.from_numpy(np.ascontiguousarray(expect, np.float32)).to(self.dev)
        return (dx.view(self.B // self.nb, *e.shape) != e[None]).sum()


def torch_ref_dl32(x, W1, b1, W2) -> np.ndarray:
    """The fp32 reference of the error budget: oracle/torch_cpu_ref.py's update on CPU ATen kernels
    (TorchCpuStep.__call__'s perception, reorder and the two 1x1 convolutions), before the masks."""
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    B, C, H, W = xt.shape
    with torch.no_grad():
        y = F.conv2d(xt, T.sobel_bank(C), padding=1, groups=C)
        y = y.view(B, C, 3, H, W).transpose(1, 2).reshape(B, 3 * C, H, W)
        h = torch.relu(F.conv2d(y, torch.from_numpy(W1)[:, :, None, None], torch.from_numpy(b1)))
        return F.conv2d(h, torch.from_numpy(W2)[:, :, None, None]).numpy()
