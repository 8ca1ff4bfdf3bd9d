"""CPU-side checks of the image-metrics ABI (gnca_image_metrics_f32 / gnca_rollout_trace_metrics_f32):
the ctypes mirror of gnca_trace_metrics matches the header, the library exports the new symbols, the
host-only size functions behave, bad arguments are rejected before any launch, ``image_metrics`` and
``trace(target=...)`` validate shapes before the library is touched, and the float64 oracle
(tests/metrics_ref.py) agrees with a direct valid-window restatement of SSIM.  No GPU needed."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnca_image_metrics_workspace_bytes", "gnca_image_metrics_f32",
               "gnca_rollout_trace_metrics_workspace_bytes", "gnca_rollout_trace_metrics_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_trace_metrics_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.TraceMetrics._fields_]
    assert fields == ["target", "target_bstride", "out"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_trace_metrics));',
             'printf("args %zu\\n", sizeof(gnca_trace_args));',
             'printf("abi %d\\n", GNCA_ABI_VERSION);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_trace_metrics, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.TraceMetrics)
    assert int(got["args"]) == ctypes.sizeof(L.TraceArgs)      # gnca_trace_args is unchanged
    assert int(got["abi"]) == L.ABI_VERSION == 5
    for f in fields:
        assert int(got[f]) == getattr(L.TraceMetrics, f).offset, f


def test_exports_new_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTS
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert hasattr(lib, n)


def test_image_metrics_workspace_bytes_host_only(lib):
    size = lib.gnca_image_metrics_workspace_bytes
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert size(*bad) == 0
    # a function of the image count and the shape; a taller image never needs less
    assert size(8, 72, 72) == 8 * size(1, 72, 72)
    assert size(1, 4096, 72) >= size(1, 72, 72)
    assert size(1, 4096, 72) % 8 == 0


def test_image_metrics_rejects_bad_args_without_touching_gpu(lib):
    f = lib.gnca_image_metrics_f32
    big = 1 << 40
    assert f(0, 8, 8, 4096, 256, 8192, 0, 12288, 16384, big, None) == -1
    assert f(2, 0, 8, 4096, 256, 8192, 0, 12288, 16384, big, None) == -1
    assert f(2, 8, -3, 4096, 256, 8192, 0, 12288, 16384, big, None) == -1
    assert f(2, 8, 8, None, 256, 8192, 0, 12288, 16384, big, None) == -1
    assert f(2, 8, 8, 4096, 256, None, 0, 12288, 16384, big, None) == -1
    assert f(2, 8, 8, 4096, 256, 8192, 0, None, 16384, big, None) == -1
    assert f(2, 8, 8, 4096, -1, 8192, 0, 12288, 16384, big, None) == -1
    need = lib.gnca_image_metrics_workspace_bytes(2, 4096, 8)
    assert need > 0
    assert f(2, 4096, 8, 4096, 4 * 4096 * 8, 8192, 0, 12288, 16384, need - 1, None) == -3
    assert f(2, 4096, 8, 4096, 4 * 4096 * 8, 8192, 0, 12288, None, big, None) == -3


R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]


def _desc(**kw):
    base = dict(B=4, C=16, H=72, W=72, hidden=128, d_model=16, offsets=R4[:8],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY,
                update_gain=0.05, alpha_thr=0.12, message_gain=0.25, fire_rate=0.5, fire_mode=L.FIRE_HASH)
    base.update(kw)
    return S.make_desc(**base)


def _args(steps, record, keep, channels=4, frames=None):
    a = L.TraceArgs()
    a.steps, a.num_records, a.frame_channels = steps, len(record), channels
    rec = (ctypes.c_int32 * max(1, len(record)))(*record)
    keep.append(rec)
    a.record = ctypes.cast(rec, ctypes.c_void_p)
    offs = (ctypes.c_int8 * max(1, steps * 16))(*([2, 3] * (steps * 8)))   # host: 8 pairs per step
    keep.append(offs)
    a.offsets = ctypes.cast(offs, ctypes.c_void_p)
    a.frames = frames
    return a


def _met(target=4096, out=8192, tbs=0):
    m = L.TraceMetrics()
    m.target, m.target_bstride, m.out = target, tbs, out
    return m


def test_trace_metrics_workspace_bytes_host_only(lib):
    keep = []
    d = _desc()
    a = _args(6, [2, 6], keep)
    plain = lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), ctypes.byref(a))
    size = lib.gnca_rollout_trace_metrics_workspace_bytes
    with_m = size(ctypes.byref(d), ctypes.byref(a), ctypes.byref(_met()))
    assert with_m >= plain + lib.gnca_image_metrics_workspace_bytes(4, 72, 72)
    assert size(ctypes.byref(d), ctypes.byref(a), None) == 0
    assert size(None, ctypes.byref(a), ctypes.byref(_met())) == 0
    assert size(ctypes.byref(d), None, ctypes.byref(_met())) == 0
    assert size(ctypes.byref(d), ctypes.byref(_args(6, [6, 2], keep)), ctypes.byref(_met())) == 0


def test_trace_metrics_rejects_bad_args_without_touching_gpu(lib):
    keep = []
    d, w = _desc(), L.Weights()
    f = lib.gnca_rollout_trace_metrics_f32
    a = _args(6, [2, 6], keep)
    big = 1 << 40
    assert f(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), None, 4096, 8192, 12288, big, None) == -1
    assert f(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), ctypes.byref(_met()), None, None, None, 0, None) == -1
    assert f(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), ctypes.byref(_met()), 4096, 4096, 12288, big, None) == -1
    # a target without an output, an output without a target, a negative stride
    for m in (_met(out=None), _met(target=None), _met(tbs=-4)):
        assert f(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), ctypes.byref(m), 4096, 8192, 12288, big, None) == -1
    # frames may be missing here, unlike in gnca_rollout_trace_f32: the call gets as far as the workspace check
    assert f(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), ctypes.byref(_met()), 4096, 8192, 12288, 16, None) == -3
    assert lib.gnca_rollout_trace_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), 4096, 8192, 12288, big, None) == -1


# ---- Python: validation before the library is touched ----
def _no_load(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")
    monkeypatch.setattr(L, "load", no_load)


def test_image_metrics_validates_before_loading_the_library(monkeypatch):
    from graph_neural_cellular_automata_amd.metrics import ImageMetrics, image_metrics
    _no_load(monkeypatch)
    t = torch.zeros(4, 8, 8)
    for pred, target in ((torch.zeros(2, 3, 8, 8), t),              # fewer than 4 channels
                         (torch.zeros(4, 8, 8), t),                 # no batch dimension
                         (torch.zeros(1, 2, 2, 4, 8, 8), t),        # too many
                         (torch.zeros(2, 4, 8, 8), torch.zeros(4, 8, 9)),
                         (torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8)),
                         (torch.zeros(2, 4, 8, 8), torch.zeros(3, 4, 8, 8)),      # neither 1 nor B
                         (torch.zeros(3, 2, 16, 8, 8), torch.zeros(3, 4, 8, 8)),  # [R,B,...]: B is 2, not R
                         (torch.zeros(2, 4, 8, 8), torch.zeros(1, 1, 4, 8, 8)),
                         (torch.zeros(0, 4, 8, 8), t),
                         (torch.zeros(2, 4, 8, 8), None)):
        with pytest.raises(ValueError):
            image_metrics(pred, target)
    assert ImageMetrics._fields == ("mse", "pixel_perfect", "psnr", "ssim")
    m = ImageMetrics(torch.arange(24.).reshape(2, 3, 4))
    assert m.stacked.shape == (2, 3, 4) and m.ssim.shape == (2, 3)
    assert torch.equal(m.psnr, m.stacked[..., 2]) and m.mse.data_ptr() == m.stacked.data_ptr()
    assert tuple(x.shape for x in m) == ((2, 3),) * 4


def test_module_trace_validates_target_before_loading_the_library(monkeypatch):
    """A wrong ``target`` / ``frames`` is a ValueError raised before the offsets are drawn and before
    the library is touched."""
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    _no_load(monkeypatch)
    g, c = NeuralCAGraph(16), NeuralCA(16)
    x = torch.zeros(2, 16, 8, 8)
    random.seed(4)
    st = random.getstate()
    for model in (g, c):
        for kw in (dict(target=torch.zeros(4, 8, 9)), dict(target=torch.zeros(3, 8, 8)),
                   dict(target=torch.zeros(3, 4, 8, 8)), dict(target=torch.zeros(16, 8, 8)),
                   dict(target="t"), dict(frames=None), dict(frames=1),
                   dict(target=torch.zeros(4, 8, 8), record=[7])):
            with pytest.raises(ValueError):
                model.trace(x, 6, **kw)
            assert random.getstate() == st


def test_trace_result_carries_metrics():
    from graph_neural_cellular_automata_amd.modules._stepper import TraceResult
    from graph_neural_cellular_automata_amd.metrics import ImageMetrics
    r = TraceResult(torch.zeros(1), None, [2], None, ImageMetrics(torch.zeros(1, 3, 4)))
    assert r.frames is None and r.metrics.ssim.shape == (1, 3) and "metrics=(1, 3, 4)" in repr(r)
    assert TraceResult(torch.zeros(1), torch.zeros(1, 1), [2], None).metrics is None


# ---- the oracle against a direct restatement ----
def _pair(N, H, W, seed):
    rng = np.random.default_rng(seed)
    target = rng.random((N, 4, H, W), dtype=np.float32)
    target[:, :3] *= target[:, 3:4]
    pred = rng.random((N, 6, H, W), dtype=np.float32) * 1.3 - 0.1   # some values outside [0, 1]
    return pred, target


@pytest.mark.parametrize("H,W", [(7, 7), (9, 13), (40, 40), (72, 72)])
def test_oracle_filter_path_equals_valid_windows(H, W):
    pred, target = _pair(1, H, W, 7)
    a = MR.image_metrics(pred, target)
    b = MR.image_metrics(pred, target, ssim=MR.ssim_windows)
    assert np.isfinite(a).all()
    # both are float64 throughout; the filter keeps running sums along each axis, so its window
    # moments carry up to ~max(H, W) roundings (72 * 1.1e-16 = 8e-15), which the variances of this
    # random data (~0.1, against C2 = 9e-4) do not amplify beyond 1e-12
    assert abs(a[0, 3] - b[0, 3]) <= 1e-12, (a[0, 3], b[0, 3])
    assert np.array_equal(a[:, :3], b[:, :3])


def test_oracle_definitions():
    pred, target = _pair(2, 9, 13, 3)
    m = MR.image_metrics(pred, target)
    P = MR.premultiply(pred)
    assert P.dtype == np.float32 and np.array_equal(P[:, 3], pred[:, 3])
    assert np.array_equal(P[:, 1], pred[:, 1] * pred[:, 3])
    assert m[0, 0] == ((P[0].astype(np.float64) - target[0]) ** 2).mean()
    # equal images: ssim 1, psnr +inf, mse 0, every cell pixel-perfect
    t1 = target.copy()
    t1[:, 3] = 1          # alpha 1: P == pred
    eq = MR.image_metrics(t1, t1)
    assert np.array_equal(eq[:, 0], [0, 0]) and np.array_equal(eq[:, 1], [1, 1])
    assert np.isinf(eq[:, 2]).all() and np.abs(eq[:, 3] - 1).max() <= 1e-15
    # too small for a window: NaN ssim only
    small = MR.image_metrics(*_pair(1, 6, 9, 1))
    assert np.isnan(small[0, 3]) and np.isfinite(small[0, :3]).all()
