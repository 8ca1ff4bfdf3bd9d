"""CPU-side checks of the graph-diagnostics ABI (gnca_graph_diag / gnca_rollout_trace_diag): the ctypes
mirror of gnca_graph_diag_out matches the header, the library exports the four symbols, the ABI version
stays 5, the host-only size functions behave, bad arguments are rejected before any launch, and the
Python entry points validate their arguments before anything is drawn.  No GPU needed."""
import ctypes
import os
import random
import re
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnca_graph_diag_workspace_bytes", "gnca_graph_diag",
               "gnca_rollout_trace_diag_workspace_bytes", "gnca_rollout_trace_diag")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_diag_out_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.GraphDiagOut._fields_]
    assert tuple(fields) == L.DIAG_FIELDS and len(fields) == 8
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_graph_diag_out));',
             'printf("args %zu\\n", sizeof(gnca_trace_args));',
             'printf("metrics %zu\\n", sizeof(gnca_trace_metrics));',
             'printf("abi %d\\n", GNCA_ABI_VERSION);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_graph_diag_out, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.GraphDiagOut)
    for f in fields:
        assert int(got[f]) == getattr(L.GraphDiagOut, f).offset, f
    # additions only: the version and the trace structs are what they were
    assert int(got["abi"]) == 5 == L.ABI_VERSION
    assert int(got["args"]) == ctypes.sizeof(L.TraceArgs) and int(got["metrics"]) == ctypes.sizeof(L.TraceMetrics)


def test_exports_new_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTS and not n.endswith("_f32")
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert hasattr(lib, n)
    assert lib.gnca_abi_version() == 5


R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]


def _desc(**kw):
    base = dict(B=4, C=16, H=72, W=72, hidden=128, d_model=16, offsets=R4[:8],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY,
                update_gain=0.05, alpha_thr=0.12, message_gain=0.25, fire_rate=0.5, fire_mode=L.FIRE_HASH)
    base.update(kw)
    return S.make_desc(**base)


def _args(steps, record, channels=4, keep=None):
    a = L.TraceArgs()
    a.steps, a.num_records, a.frame_channels = steps, len(record), channels
    rec = (ctypes.c_int32 * max(1, len(record)))(*record)
    keep.append(rec)
    a.record = ctypes.cast(rec, ctypes.c_void_p)
    return a


def test_diag_workspace_bytes_host_only(lib):
    d = _desc()
    n = lib.gnca_graph_diag_workspace_bytes(ctypes.byref(d))
    plane = 4 * 72 * 72
    # the attention op's workspace, the three masked group planes and the src bytes
    assert n >= lib.gnca_attention_workspace_bytes(ctypes.byref(d)) + 3 * plane * 4 + plane
    zp = lib.gnca_graph_diag_workspace_bytes(ctypes.byref(_desc(flags=L.GRAPH | L.ZERO_PAD_SHIFT)))
    assert zp >= n + 4 * 16 * 72 * 8       # + K0's fp64 row sums
    assert lib.gnca_graph_diag_workspace_bytes(ctypes.byref(_desc(hidden=1))) == n
    assert lib.gnca_graph_diag_workspace_bytes(ctypes.byref(_desc(offsets=[]))) > 0   # k = 0
    assert lib.gnca_graph_diag_workspace_bytes(ctypes.byref(_desc(flags=0))) > 0      # graph off
    for bad in (dict(C=3), dict(C=36), dict(B=0), dict(H=0), dict(W=0)):
        assert lib.gnca_graph_diag_workspace_bytes(ctypes.byref(_desc(**bad))) == 0
    assert lib.gnca_graph_diag_workspace_bytes(None) == 0


def test_trace_diag_workspace_bytes_host_only(lib):
    keep = []
    d = _desc()
    a = _args(6, [2, 6], keep=keep)
    m = L.TraceMetrics()
    plain = lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), ctypes.byref(a))
    n = lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(d), ctypes.byref(a), None)
    assert n >= plain + lib.gnca_graph_diag_workspace_bytes(ctypes.byref(d)) - 256
    withm = lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(d), ctypes.byref(a), ctypes.byref(m))
    assert withm >= n
    size = lambda dd, aa: lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(dd), ctypes.byref(aa), None)
    assert size(d, _args(6, [], keep=keep)) > 0 and size(d, _args(0, [], keep=keep)) > 0
    assert size(d, _args(6, [7], keep=keep)) == 0 and size(d, _args(6, [4, 2], keep=keep)) == 0
    assert size(d, _args(6, [2], channels=17, keep=keep)) == 0
    assert size(_desc(C=3), a) == 0 and size(_desc(C=36), a) == 0
    assert lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(d), None, None) == 0
    assert lib.gnca_rollout_trace_diag_workspace_bytes(None, ctypes.byref(a), None) == 0


def _out(**kw):
    o = L.GraphDiagOut()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_rejects_bad_args_without_touching_gpu(lib):
    """Every rejection happens before a launch: the pointers are made-up addresses."""
    keep = []
    d, w, o = _desc(), L.Weights(), _out(raw=16384, magnitude=20480)
    big = 1 << 40
    fn = lib.gnca_graph_diag
    assert fn(ctypes.byref(d), ctypes.byref(w), None, ctypes.byref(o), 12288, big, None) == -1      # x
    assert fn(ctypes.byref(d), ctypes.byref(w), 4096, None, 12288, big, None) == -1                 # out
    assert fn(None, ctypes.byref(w), 4096, ctypes.byref(o), 12288, big, None) == -1                 # desc
    assert fn(ctypes.byref(d), None, 4096, ctypes.byref(o), 12288, big, None) == -1                 # weights
    assert fn(ctypes.byref(_desc(C=36)), ctypes.byref(w), 4096, ctypes.byref(o), 12288, big, None) == -2
    assert fn(ctypes.byref(_desc(C=3)), ctypes.byref(w), 4096, ctypes.byref(o), 12288, big, None) == -1
    # null weight pointers with the graph on are rejected before the workspace check or any launch
    assert fn(ctypes.byref(d), ctypes.byref(w), 4096, ctypes.byref(o), 12288, big, None) == -1
    w.wm, w.bm = 24576, 28672
    need = lib.gnca_graph_diag_workspace_bytes(ctypes.byref(d))
    assert fn(ctypes.byref(d), ctypes.byref(w), 4096, ctypes.byref(o), 12288, need - 1, None) == -3
    assert fn(ctypes.byref(d), ctypes.byref(w), 4096, ctypes.byref(o), None, big, None) == -3
    # the zero-padded shift also needs the query / key weights
    dz = _desc(flags=L.GRAPH | L.ZERO_PAD_SHIFT)
    assert fn(ctypes.byref(dz), ctypes.byref(w), 4096, ctypes.byref(o), 12288, big, None) == -1
    # nothing requested: nothing is launched (the arguments are still checked)
    assert fn(ctypes.byref(d), ctypes.byref(w), 4096, ctypes.byref(_out()), 12288, big, None) == 0
    assert fn(ctypes.byref(d), ctypes.byref(w), 4096, ctypes.byref(_out()), None, 0, None) == -3

    tr = lib.gnca_rollout_trace_diag
    a = _args(6, [2, 6], keep=keep)
    a.frames = 32768
    args = lambda **k: [ctypes.byref(k.get("d", d)), ctypes.byref(w), k.get("a", ctypes.byref(a)), None,
                        k.get("o", ctypes.byref(o)), k.get("x", 4096), k.get("xf", 8192), k.get("ws", 12288),
                        k.get("n", big), None]
    assert tr(*args(x=None)) == -1 and tr(*args(xf=None)) == -1 and tr(*args(xf=4096)) == -1
    assert tr(*args(o=None)) == -1 and tr(*args(a=None)) == -1
    assert tr(*args(d=_desc(C=36))) == -2
    bad = _args(6, [6, 2], keep=keep)
    bad.frames = 32768
    assert tr(*args(a=ctypes.byref(bad))) == -1
    assert tr(*args(a=ctypes.byref(a))) == -1            # no offsets for a graph rollout
    flat = [v for _ in range(6) for pr in R4[:8] for v in pr]
    arr = (ctypes.c_int8 * len(flat))(*flat)
    a.offsets = ctypes.cast(arr, ctypes.c_void_p)
    need = lib.gnca_rollout_trace_diag_workspace_bytes(ctypes.byref(d), ctypes.byref(a), None)
    assert need > 0
    assert tr(*args(n=need - 1)) == -3 and tr(*args(ws=None)) == -3


# ---- the Python entry points ----
def test_trace_validates_diagnostics_before_drawing(monkeypatch):
    """``trace(diagnostics=...)`` on a CPU tensor: the argument errors are ValueErrors raised before the
    library is touched and before any offset is drawn."""
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(L, "load", no_load)
    g, c = NeuralCAGraph(16), NeuralCA(16)
    x = torch.zeros(1, 16, 8, 8)
    random.seed(4)
    st = random.getstate()
    for model, kw in ((c, dict(diagnostics=True)), (c, dict(per_offset=True)),
                      (g, dict(diagnostics=1)), (g, dict(diagnostics="yes")),
                      (g, dict(diagnostics=True, per_offset=1)), (g, dict(per_offset=True)),
                      (g, dict(diagnostics=True, record=[7])), (g, dict(diagnostics=True, channels=17)),
                      (g, dict(diagnostics=True, every=0))):
        with pytest.raises(ValueError):
            model.trace(x, 6, **kw)
        assert random.getstate() == st, kw


def test_trace_result_keeps_positional_construction():
    from graph_neural_cellular_automata_amd.modules._stepper import TraceResult
    r = TraceResult(1, 2, [3], 4)
    assert (r.x_final, r.frames, r.steps, r.attention, r.metrics, r.diagnostics) == (1, 2, [3], 4, None, None)
    r = TraceResult(1, 2, [3], 4, 5)
    assert r.metrics == 5 and r.diagnostics is None
    assert TraceResult(1, 2, [3], 4, 5, 6).diagnostics == 6
    assert TraceResult.__slots__[-1] == "diagnostics"


def test_diagnostics_validates_before_drawing(monkeypatch):
    from graph_neural_cellular_automata_amd.modules.graph_augmentation import GraphAugmentation

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(L, "load", no_load)
    g = GraphAugmentation(16)
    x = torch.zeros(1, 16, 8, 8)
    random.seed(9)
    st = random.getstate()
    for args, kw in (((x,), dict(per_offset=1)), ((x,), dict(per_offset=None)),
                     ((torch.zeros(1, 12, 8, 8),), {}), ((torch.zeros(16, 8, 8),), {}),
                     ((x, 3), {}), ((x, [(1, 2, 3)]), {}), ((x, [(2.0, 3)]), {}), ((x, [(True, 3)]), {}),
                     ((x, [(200, 0)]), {}), ((x, [(2, 0)] * 129), {}), ((x, [5]), {})):
        with pytest.raises(ValueError):
            g.diagnostics(*args, **kw)
        assert random.getstate() == st, (args[1:], kw)
    # a valid call on a CPU tensor stops at the device check (there is no CPU path), still without a draw
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        g.diagnostics(x)
    assert random.getstate() == st


def test_graph_diagnostics_fields():
    d = S.GraphDiagnostics([(2, 3)], raw=1, weights=2)
    assert d.raw == 1 and d.weights == 2 and d.per_offset is None and d.offsets == [(2, 3)]
    assert set(S.GraphDiagnostics.__slots__) == set(L.DIAG_FIELDS) | {"offsets"}
    assert "raw=" in repr(S.GraphDiagnostics())
