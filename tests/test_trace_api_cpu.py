"""CPU-side checks of the trace ABI (gnca_attention_f32 / gnca_rollout_trace_f32): the ctypes mirror
of gnca_trace_args matches the header, the library exports the new symbols, the host-only size
functions behave, bad arguments are rejected before any launch, and the pure-Python trace helper
validates its arguments and expands ``every`` into record points.  No GPU needed."""
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
NEW_SYMBOLS = ("gnca_attention_workspace_bytes", "gnca_attention_f32",
               "gnca_rollout_trace_workspace_bytes", "gnca_rollout_trace_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_trace_args_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.TraceArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_trace_args));',
             'printf("abi %d\\n", GNCA_ABI_VERSION);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_trace_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.TraceArgs)
    assert int(got["abi"]) == L.ABI_VERSION
    for f in fields:
        assert int(got[f]) == getattr(L.TraceArgs, f).offset, f


def test_exports_new_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTS
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert hasattr(lib, n)


R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]


def _desc(**kw):
    base = dict(B=4, C=16, H=72, W=72, hidden=128, d_model=16, offsets=R4[:8],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY,
                update_gain=0.05, alpha_thr=0.12, message_gain=0.25, fire_rate=0.5, fire_mode=L.FIRE_HASH)
    base.update(kw)
    return S.make_desc(**base)


def _args(steps, record, channels=4, attn=False, keep=None):
    a = L.TraceArgs()
    a.steps, a.num_records, a.frame_channels = steps, len(record), channels
    rec = (ctypes.c_int32 * max(1, len(record)))(*record)
    keep.append(rec)
    a.record = ctypes.cast(rec, ctypes.c_void_p)
    a.attn = 4096 if attn else None   # only its presence is read on the host
    return a


def test_attention_workspace_bytes_host_only(lib):
    n = lib.gnca_attention_workspace_bytes(ctypes.byref(_desc()))
    assert n >= 4 * 72 * 72 * 4            # the S plane at least
    zp = lib.gnca_attention_workspace_bytes(ctypes.byref(_desc(flags=L.GRAPH | L.ZERO_PAD_SHIFT)))
    assert zp >= n + 4 * 16 * 72 * 8       # + K0's fp64 row sums
    # every field but the shape, the offsets and the graph flags is ignored: hidden = 1 is fine
    assert lib.gnca_attention_workspace_bytes(ctypes.byref(_desc(hidden=1))) == n
    assert lib.gnca_attention_workspace_bytes(ctypes.byref(_desc(offsets=[]))) > 0   # k = 0: zeros
    for bad in (dict(C=3), dict(C=36), dict(B=0), dict(H=0), dict(W=0)):
        assert lib.gnca_attention_workspace_bytes(ctypes.byref(_desc(**bad))) == 0
    assert lib.gnca_attention_workspace_bytes(None) == 0


def test_trace_workspace_bytes_host_only(lib):
    keep = []
    d = _desc()
    state = 4 * 16 * 72 * 72 * 4
    plain = lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), ctypes.byref(_args(6, [2, 6], keep=keep)))
    assert plain >= 3 * state + lib.gnca_workspace_bytes(ctypes.byref(d))
    maps = lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), ctypes.byref(_args(6, [2, 6], attn=True, keep=keep)))
    assert maps >= plain + lib.gnca_attention_workspace_bytes(ctypes.byref(d)) - 256
    size = lambda *a, **k: lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), ctypes.byref(_args(*a, keep=keep, **k)))
    assert size(6, []) > 0 and size(0, []) > 0
    assert size(6, [0]) == 0 and size(6, [7]) == 0           # out of 1..T
    assert size(6, [3, 3]) == 0 and size(6, [4, 2]) == 0     # not strictly increasing
    assert size(6, [2], channels=0) == 0 and size(6, [2], channels=17) == 0
    assert size(-1, []) == 0
    assert lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(_desc(C=3)), ctypes.byref(_args(6, [2], keep=keep))) == 0
    assert lib.gnca_rollout_trace_workspace_bytes(ctypes.byref(d), None) == 0
    assert lib.gnca_rollout_trace_workspace_bytes(None, ctypes.byref(_args(6, [2], keep=keep))) == 0


def test_rejects_bad_args_without_touching_gpu(lib):
    keep = []
    d, w = _desc(), L.Weights()
    assert lib.gnca_attention_f32(ctypes.byref(d), ctypes.byref(w), None, None, None, 0, None) == -1
    assert lib.gnca_attention_f32(None, ctypes.byref(w), 4096, 8192, 12288, 1 << 40, None) == -1
    assert lib.gnca_attention_f32(ctypes.byref(_desc(C=36)), ctypes.byref(w), 4096, 8192, 12288, 1 << 40, None) == -2
    # null weights with the graph on are rejected before the workspace check or any launch
    assert lib.gnca_attention_f32(ctypes.byref(d), ctypes.byref(w), 4096, 8192, 12288, 1 << 40, None) == -1
    a = _args(6, [2, 6], keep=keep)
    assert lib.gnca_rollout_trace_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), None, None, None, 0, None) == -1
    assert lib.gnca_rollout_trace_f32(ctypes.byref(d), ctypes.byref(w), None, 4096, 8192, 12288, 1 << 40, None) == -1
    # x_final aliasing x, a bad record list, missing frames: invalid with every pointer set
    assert lib.gnca_rollout_trace_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), 4096, 4096, 12288, 1 << 40, None) == -1
    bad = _args(6, [6, 2], keep=keep)
    bad.frames = 16384
    assert lib.gnca_rollout_trace_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(bad), 4096, 8192, 12288, 1 << 40, None) == -1
    assert lib.gnca_rollout_trace_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(a), 4096, 8192, 12288, 1 << 40, None) == -1


# ---- the pure-Python helpers ----
@pytest.mark.parametrize("steps,every,want", [
    (7, 1, [1, 2, 3, 4, 5, 6, 7]), (7, 3, [3, 6, 7]), (6, 3, [3, 6]), (64, 16, [16, 32, 48, 64]),
    (3, 5, [3]), (0, 1, []), (0, 4, []), (1, 1, [1]),
])
def test_every_expands_to_record(steps, every, want):
    assert S.expand_record(steps, every) == want


def test_record_is_kept_as_given():
    assert S.expand_record(7, record=[1, 4, 7]) == [1, 4, 7]
    assert S.expand_record(7, record=(2,)) == [2]
    assert S.expand_record(7, record=[]) == []


def _build(**kw):
    base = dict(steps=6, B=2, C=16, H=8, W=8, device="cpu", message_gain=0.25, offsets=[R4[:2]] * 6)
    base.update(kw)
    return S.build_trace(**base)


def test_trace_plan_defaults():
    p = _build()
    assert p.record == [1, 2, 3, 4, 5, 6] and p.channels == 4 and p.first_step == 0 and not p.attention
    assert p.schedule.uniform and p.schedule.k == 2 and p.schedule.fire_mode == L.FIRE_NONE
    p = _build(every=4, channels=16, return_attention=True, fire_rate=0.5, seed=3, first_step=9, sample_base=5)
    assert p.record == [4, 6] and p.channels == 16 and p.first_step == 9 and p.attention
    assert p.schedule.fire_mode == L.FIRE_HASH and p.schedule.seed == 3 and p.schedule.sample_base == 5
    # a per-step list with one value is the uniform schedule
    assert _build(fire_rate=[0.5] * 6, seed=1, message_gain=[0.1] * 6).schedule.uniform
    # the classic model: no gain, no offsets
    assert _build(message_gain=None, offsets=None).schedule.k == 0


@pytest.mark.parametrize("bad", [
    dict(fire_rate=[0.5, 0.5, 0.5, 0.5, 0.5, 1.0], seed=1),       # per-step rates that differ
    dict(message_gain=[0.25, 0.25, 0.0, 0.25, 0.25, 0.25]),       # per-step gains that differ
    dict(fire_rate=[0.5] * 5, seed=1),                            # wrong length
    dict(record=[4, 2]), dict(record=[2, 2]),                     # unsorted / repeated
    dict(record=[0]), dict(record=[7]), dict(record=[-1, 3]),     # out of 1..steps
    dict(record=[1.5]), dict(record=[True]), dict(record=3),
    dict(record=[2], every=2),                                    # both
    dict(every=0), dict(every=-2), dict(every=1.5), dict(every=True),
    dict(channels=17), dict(channels=0), dict(channels=4.0),      # channels > C, < 1, not an int
    dict(first_step=-1), dict(first_step=1.5),
    dict(steps=-1), dict(steps=2.5),
    dict(return_attention=True, message_gain=None, offsets=None),  # no graph term, no map
    dict(offsets=[R4[:2]] * 5),                                   # (build_schedule's own checks still hold)
    dict(fire_rate=0.5, seed="s"),
])
def test_trace_rejects_malformed(bad):
    with pytest.raises(ValueError):
        _build(**bad)


def test_rejected_trace_draws_nothing():
    """A bad call raises before the offsets are drawn: Python's ``random`` stays where it was."""
    from graph_neural_cellular_automata_amd.modules.graph_augmentation import GraphAugmentation
    graph = GraphAugmentation(16)
    random.seed(4)
    st = random.getstate()
    for bad in (dict(record=[9]), dict(channels=32), dict(fire_rate=[0.5, 1.0] * 3, seed=1)):
        with pytest.raises(ValueError):
            _build(offsets=None, sample_offsets=graph.sample_offsets, **bad)
        assert random.getstate() == st


@pytest.mark.parametrize("T", [0, 1, 5])
def test_trace_draws_offsets_like_rollout(T):
    """offsets=None: one graph.sample_offsets() per step in step order, as rollout() draws them."""
    from graph_neural_cellular_automata_amd.modules.graph_augmentation import GraphAugmentation
    graph = GraphAugmentation(16)
    random.seed(11)
    manual = [random.sample(graph.offsets, 8) for _ in range(T)]
    after = random.random()
    random.seed(11)
    p = _build(steps=T, offsets=None, sample_offsets=graph.sample_offsets)
    assert random.random() == after
    assert (p.schedule.offsets or []) == manual


def test_module_trace_validates_before_loading_the_library(monkeypatch):
    """NeuralCAGraph.trace / NeuralCA.trace on a CPU tensor: the argument errors are ValueErrors raised
    before the library is touched (L.load is never reached)."""
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(L, "load", no_load)
    g, c = NeuralCAGraph(16), NeuralCA(16)
    x = torch.zeros(1, 16, 8, 8)
    for model, kw in ((g, dict(channels=17)), (g, dict(record=[3, 2])), (g, dict(record=[7])),
                      (g, dict(fire_rate=[0.5] * 5 + [1.0], seed=1)), (g, dict(message_gain=[0.1] * 5 + [0.2])),
                      (c, dict(return_attention=True)), (c, dict(channels=17)), (c, dict(message_gain=0.5)),
                      (c, dict(offsets=[R4[:2]] * 6))):
        with pytest.raises(ValueError):
            model.trace(x, 6, **kw)
