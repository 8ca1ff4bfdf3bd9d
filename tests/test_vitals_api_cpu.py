"""CPU-side checks of the state-vitals ABI (gnca_state_vitals / gnca_rollout_trace_vitals): the ctypes
mirror of gnca_trace_vitals matches the header, the library exports the new symbols, the host-only size
functions behave, bad arguments are rejected before any launch, ``state_vitals`` and
``trace(vitals=...)`` validate before the library is touched and before ``random`` is consumed, and the
float64 oracle (tests/vitals_ref.py) gives the closed forms of simple states.  No GPU needed."""
import ctypes
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import vitals_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnca_state_vitals_workspace_bytes", "gnca_state_vitals",
               "gnca_rollout_trace_vitals_workspace_bytes", "gnca_rollout_trace_vitals")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_trace_vitals_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.TraceVitals._fields_]
    assert fields == ["alpha_thr", "out"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_trace_vitals));',
             'printf("args %zu\\n", sizeof(gnca_trace_args));',
             'printf("metrics %zu\\n", sizeof(gnca_trace_metrics));',
             'printf("nfields %d\\n", GNCA_VITALS_FIELDS);',
             'printf("band %d\\n", GNCA_VITALS_BAND_ROWS);',
             'printf("cols %d\\n", GNCA_VITALS_TILE_COLS);',
             'printf("abi %d\\n", GNCA_ABI_VERSION);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_trace_vitals, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.TraceVitals)
    assert int(got["args"]) == ctypes.sizeof(L.TraceArgs)          # the existing structs are unchanged
    assert int(got["metrics"]) == ctypes.sizeof(L.TraceMetrics)
    assert int(got["nfields"]) == len(L.VITALS_FIELDS) == 13
    assert int(got["band"]) == L.VITALS_BAND_ROWS
    assert int(got["cols"]) == L.VITALS_TILE_COLS
    assert int(got["abi"]) == L.ABI_VERSION == 5
    for f in fields:
        assert int(got[f]) == getattr(L.TraceVitals, f).offset, f
    assert L.VITALS_FIELDS == VR.FIELDS


def test_exports_new_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTS
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert hasattr(lib, n)
    assert lib.gnca_abi_version() == 5


def test_state_vitals_workspace_bytes_host_only(lib):
    size = lib.gnca_state_vitals_workspace_bytes
    for bad in ((0, 16, 8, 8), (1, 3, 8, 8), (1, 16, 0, 8), (1, 16, 8, 0), (-1, 16, 8, 8), (1, 0, 8, 8),
                (1, 16, -2, 8)):
        assert size(*bad) == 0, bad
    assert size(1, 4, 1, 1) > 0 and size(1, 4, 1, 1) % 8 == 0
    assert size(8, 16, 72, 72) == 8 * size(1, 16, 72, 72)
    assert size(1, 4, 72, 72) == size(1, 32, 72, 72)      # the tiles depend on (H, W) alone
    hs = [1, 7, 8, 9, 16, 17, 72, 73, 200, 4096]
    sizes = [size(1, 16, h, 72) for h in hs]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]   # monotone in H
    assert size(1, 16, 72, 4096) > size(1, 16, 72, 72)


def test_state_vitals_rejects_bad_args_without_touching_gpu(lib):
    f = lib.gnca_state_vitals
    big = 1 << 40
    x, out, ws = 4096, 8192, 16384
    st = 16 * 64
    assert f(0, 16, 8, 8, x, st, 0.1, out, ws, big, None) == -1
    assert f(2, 0, 8, 8, x, st, 0.1, out, ws, big, None) == -1
    assert f(2, 3, 8, 8, x, st, 0.1, out, ws, big, None) == -1
    assert f(2, 16, 0, 8, x, st, 0.1, out, ws, big, None) == -1
    assert f(2, 16, 8, -1, x, st, 0.1, out, ws, big, None) == -1
    assert f(2, 16, 8, 8, None, st, 0.1, out, ws, big, None) == -1
    assert f(2, 16, 8, 8, x, st, 0.1, None, ws, big, None) == -1
    assert f(2, 16, 8, 8, x, -1, 0.1, out, ws, big, None) == -1
    need = lib.gnca_state_vitals_workspace_bytes(2, 16, 8, 8)
    assert need > 0
    assert f(2, 16, 8, 8, x, st, 0.1, out, ws, need - 1, None) == -3
    assert f(2, 16, 8, 8, x, st, 0.1, out, None, big, None) == -3
    assert f(2, 16, 8, 8, x, st, 0.1, out, None, 0, None) == -3


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


def _vit(out=8192, thr=0.1):
    v = L.TraceVitals()
    v.alpha_thr, v.out = thr, out
    return v


def test_trace_vitals_workspace_bytes_host_only(lib):
    keep = []
    d = _desc()
    a = _args(6, [2, 6], keep)
    m = L.TraceMetrics()
    m.target, m.target_bstride, m.out = 4096, 0, 8192
    o = L.GraphDiagOut()
    size = lib.gnca_rollout_trace_vitals_workspace_bytes
    vit = lib.gnca_state_vitals_workspace_bytes(4, 16, 72, 72)
    plain = lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), ctypes.byref(a))
    assert plain + vit <= size(ctypes.byref(d), ctypes.byref(a), None, None) < plain + vit + 256
    withm = lib.gnca_rollout_trace_metrics_workspace_bytes(ctypes.byref(d), ctypes.byref(a), ctypes.byref(m))
    assert withm + vit <= size(ctypes.byref(d), ctypes.byref(a), ctypes.byref(m), None) < withm + vit + 256
    withd = lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(d), ctypes.byref(a), ctypes.byref(m))
    assert withd + vit <= size(ctypes.byref(d), ctypes.byref(a), ctypes.byref(m), ctypes.byref(o)) < withd + vit + 256
    assert size(None, ctypes.byref(a), None, None) == 0
    assert size(ctypes.byref(d), None, None, None) == 0
    assert size(ctypes.byref(d), ctypes.byref(_args(6, [6, 2], keep)), None, None) == 0
    # the sizes of the existing entry points do not move
    assert lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(d), ctypes.byref(a), None) >= plain


def test_trace_vitals_rejects_bad_args_without_touching_gpu(lib):
    keep = []
    d, w = _desc(), L.Weights()
    f = lib.gnca_rollout_trace_vitals
    a = _args(6, [2, 6], keep)
    big = 1 << 40
    ok = (ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), None, None)
    assert f(*ok, None, 4096, 8192, 12288, big, None) == -1                      # no vitals
    assert f(*ok, ctypes.byref(_vit(out=None)), 4096, 8192, 12288, big, None) == -1   # records without an output
    assert f(*ok, ctypes.byref(_vit()), None, 8192, 12288, big, None) == -1
    assert f(*ok, ctypes.byref(_vit()), 4096, 4096, 12288, big, None) == -1      # x_final aliases x
    assert f(ctypes.byref(d), ctypes.byref(w), None, None, None, ctypes.byref(_vit()), 4096, 8192, 12288, big,
             None) == -1
    bad = _args(6, [6, 2], keep)
    assert f(ctypes.byref(d), ctypes.byref(w), ctypes.byref(bad), None, None, ctypes.byref(_vit()), 4096, 8192,
             12288, big, None) == -1
    # frames may be missing (vitals without frames): the call gets as far as the workspace check
    assert f(*ok, ctypes.byref(_vit()), 4096, 8192, 12288, 16, None) == -3
    assert f(*ok, ctypes.byref(_vit()), 4096, 8192, None, big, None) == -3
    need = lib.gnca_rollout_trace_vitals_workspace_bytes(ctypes.byref(d), ctypes.byref(a), None, None)
    assert f(*ok, ctypes.byref(_vit()), 4096, 8192, 12288, need - 1, None) == -3


# ---- Python: validation before the library is touched ----
def _no_load(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")
    monkeypatch.setattr(L, "load", no_load)


def test_state_vitals_validates_before_loading_the_library(monkeypatch):
    import graph_neural_cellular_automata_amd as pkg
    from graph_neural_cellular_automata_amd.vitals import StateVitals, state_vitals
    assert pkg.state_vitals is state_vitals and pkg.StateVitals is StateVitals
    assert "state_vitals" in pkg.__all__ and "StateVitals" in pkg.__all__
    _no_load(monkeypatch)
    ok = torch.zeros(2, 16, 8, 8)
    for x, kw in ((torch.zeros(2, 3, 8, 8), {}),                 # fewer than 4 channels
                  (torch.zeros(16, 8, 8), {}),                   # no batch dimension
                  (torch.zeros(1, 2, 2, 16, 8, 8), {}),          # too many
                  (torch.zeros(0, 16, 8, 8), {}),
                  (torch.zeros(2, 16, 8, 0), {}),
                  ("x", {}),
                  (ok, dict(alpha_thr=float("nan"))),
                  (ok, dict(alpha_thr=float("inf"))),
                  (ok, dict(alpha_thr=None)),
                  (ok, dict(alpha_thr="0.1")),
                  (ok, dict(alpha_thr=True))):
        with pytest.raises(ValueError):
            state_vitals(x, **kw)
    # no CPU path: a RuntimeError, as image_metrics (and still before the library is loaded)
    with pytest.raises(RuntimeError):
        state_vitals(ok)
    assert StateVitals._fields == VR.FIELDS
    v = StateVitals(torch.arange(78.0, dtype=torch.float64).reshape(2, 3, 13))
    assert v.stacked.shape == (2, 3, 13) and v.hidden_rms.shape == (2, 3)
    assert torch.equal(v.nonfinite, v.stacked[..., 11]) and v.alive.data_ptr() == v.stacked.data_ptr()
    assert tuple(t.shape for t in v) == ((2, 3),) * 13


def test_module_trace_validates_vitals_before_loading_the_library(monkeypatch):
    """A wrong ``vitals`` is a ValueError raised before the offsets are drawn and before the library is
    touched; so is any other bad argument of a call that asks for vitals."""
    from graph_neural_cellular_automata_amd import DamagePolicy, NeuralCA, NeuralCAGraph, regrow_trace
    _no_load(monkeypatch)
    g, c = NeuralCAGraph(16), NeuralCA(16)
    x = torch.zeros(2, 16, 8, 8)
    random.seed(4)
    st = random.getstate()
    for model in (g, c):
        for kw in (dict(vitals=None), dict(vitals="yes"), dict(vitals=float("nan")), dict(vitals=float("-inf")),
                   dict(vitals=[0.1]), dict(vitals=True, record=[7]), dict(vitals=0.2, frames=None),
                   dict(vitals=True, channels=17), dict(vitals=True, target=torch.zeros(4, 8, 9))):
            with pytest.raises(ValueError):
                model.trace(x, 6, **kw)
            assert random.getstate() == st
        with pytest.raises(ValueError):      # regrow_trace passes it through
            regrow_trace(model, x, 6, DamagePolicy({}, 3), 2, vitals="yes")
        assert random.getstate() == st


def test_trace_result_carries_vitals():
    from graph_neural_cellular_automata_amd.modules._stepper import TraceResult
    from graph_neural_cellular_automata_amd.vitals import StateVitals
    r = TraceResult(torch.zeros(1), None, [2], None, vitals=StateVitals(torch.zeros(1, 3, 13, dtype=torch.float64)))
    assert r.frames is None and r.vitals.alive.shape == (1, 3) and "vitals=(1, 3, 13)" in repr(r)
    assert TraceResult(torch.zeros(1), torch.zeros(1, 1), [2], None).vitals is None
    assert "vitals" not in repr(TraceResult(torch.zeros(1), torch.zeros(1, 1), [2], None))


# ---- the oracle against closed forms ----
def test_oracle_all_zero_state():
    v = VR.state_vitals(np.zeros((2, 6, 5, 7), np.float32), 0.1)
    assert v.shape == (2, 13)
    for b in range(2):
        assert np.array_equal(v[b, :4], [0, 0, 0, 0])
        assert np.isnan(v[b, 4]) and np.isnan(v[b, 5])
        assert np.array_equal(v[b, 6:], [-1, -1, -1, -1, 0, 0, 0])


@pytest.mark.parametrize("H,W,cy,cx,alive", [(9, 13, 4, 6, 9), (9, 13, 0, 0, 4), (9, 13, 8, 12, 4),
                                            (9, 13, 0, 5, 6), (1, 1, 0, 0, 1)])
def test_oracle_one_seed_cell(H, W, cy, cx, alive):
    x = np.zeros((1, 16, H, W), np.float32)
    x[0, 3:, cy, cx] = 1.0                       # the seed: alpha and hidden channels 1
    v = VR.state_vitals(x, 0.1)[0]
    assert v[0] == alive and v[1] == 1 and v[2] == 1 and v[3] == 1
    assert v[4] == cy and v[5] == cx
    assert np.array_equal(v[6:10], [cy, cy, cx, cx])
    assert v[10] == 1 and v[11] == 0
    assert v[12] == math.sqrt(12.0 / (12.0 * H * W))


def test_oracle_threshold_is_strict_and_clip_and_nonfinite():
    thr = 0.125
    x = np.zeros((1, 6, 4, 4), np.float32)
    x[0, 3] = thr                                # a == alpha_thr: neither mature nor alive
    v = VR.state_vitals(x, thr)[0]
    assert v[0] == 0 and v[1] == 0 and np.array_equal(v[6:10], [-1] * 4)
    assert v[2] == 16 * thr and v[3] == 16 * thr
    x[0, 3, 1, 2] = np.nextafter(np.float32(thr), np.float32(1))
    v = VR.state_vitals(x, thr)[0]
    assert v[0] == 9 and v[1] == 1 and np.array_equal(v[6:10], [1, 1, 2, 2])
    # clip: alpha 3 counts 1 towards the mass, alpha -2 counts 0; alpha_sum keeps both
    y = np.zeros((1, 6, 4, 4), np.float32)
    y[0, 3, 0, 0], y[0, 3, 3, 3] = 3.0, -2.0
    v = VR.state_vitals(y, thr)[0]
    assert v[2] == 1.0 and v[3] == 1.0 and v[4] == 0 and v[5] == 0 and v[10] == 3.0
    # non-finite hidden values: counted, left out of max_abs and of the rms; the alpha fields unmoved
    z = y.copy()
    z[0, 4, 0, 0], z[0, 5, 1, 1], z[0, 5, 2, 2], z[0, 4, 3, 3] = np.nan, np.inf, -np.inf, 0.5
    w = VR.state_vitals(z, thr)[0]
    assert w[11] == 3 and w[10] == 3.0 and w[12] == math.sqrt(0.25 / 32.0)
    assert np.array_equal(w[:10], v[:10])
    # C = 4: no hidden channels, rms 0
    assert VR.state_vitals(y[:, :4], thr)[0, 12] == 0.0
