"""CPU-side checks of the whole-rollout ABI (gnca_rollout_fwd_f32 / gnca_rollout_bwd_f32): the
ctypes mirror of gnca_rollout_sched matches the header, the host-only size functions behave, bad
arguments are rejected before any launch, and the pure-Python schedule helper validates its
arguments and consumes Python's ``random`` as ``steps`` forward calls do.  No GPU needed."""
import ctypes
import os
import random
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_sched_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.RolloutSched._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_rollout_sched));',
             'printf("recompute %u\\n", GNCA_SCHED_RECOMPUTE);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_rollout_sched, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.RolloutSched)
    assert int(got["recompute"]) == L.SCHED_RECOMPUTE
    for f in fields:
        assert int(got[f]) == getattr(L.RolloutSched, f).offset, f


R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]


def _desc(**kw):
    base = dict(B=4, C=16, H=72, W=72, hidden=128, d_model=16, offsets=R4[:8],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY,
                update_gain=0.05, alpha_thr=0.12, message_gain=0.25, fire_rate=0.5, fire_mode=L.FIRE_HASH)
    base.update(kw)
    return S.make_desc(**base)


def _sched(steps, k=8, flags=0, keep=None):
    s = L.RolloutSched()
    s.steps, s.flags = steps, flags
    if steps > 0 and k > 0:
        flat = [v for t in range(steps) for o in R4[t:t + k] for v in o]
        arr = (ctypes.c_int8 * len(flat))(*flat)
        keep.append(arr)
        s.offsets = ctypes.cast(arr, ctypes.c_void_p)
    return s


def test_tape_bytes_host_only(lib):
    keep = []
    d = _desc()
    n = 4 * 16 * 72 * 72 * 4
    sizes = {}
    for T in (1, 3, 6):
        s = _sched(T, keep=keep)
        sizes[T] = lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(s))
        assert sizes[T] >= T * n
        r = _sched(T, flags=L.SCHED_RECOMPUTE, keep=keep)
        lean = lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(r))
        assert T * n <= lean < sizes[T]
    assert sizes[1] < sizes[3] < sizes[6]
    s = _sched(3, keep=keep)
    for bad in (dict(C=3), dict(C=36), dict(hidden=512), dict(B=0)):
        assert lib.gnca_rollout_tape_bytes(ctypes.byref(_desc(**bad)), ctypes.byref(s)) == 0
    neg = _sched(3, keep=keep)
    neg.steps = -1
    assert lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(neg)) == 0
    assert lib.gnca_rollout_tape_bytes(ctypes.byref(d), None) == 0
    assert lib.gnca_rollout_tape_bytes(None, ctypes.byref(s)) == 0


def test_workspace_bytes_host_only(lib):
    keep = []
    d = _desc()
    s = _sched(4, keep=keep)
    assert lib.gnca_rollout_bwd_workspace_bytes(ctypes.byref(d), ctypes.byref(s)) >= \
        lib.gnca_bwd_workspace_bytes(ctypes.byref(d))
    # the forward's: the masks, one step workspace and the two states of the no-tape form
    assert lib.gnca_rollout_fwd_workspace_bytes(ctypes.byref(d), ctypes.byref(s)) >= \
        lib.gnca_workspace_bytes(ctypes.byref(d)) + 2 * 4 * 16 * 72 * 72 * 4
    assert lib.gnca_rollout_bwd_workspace_bytes(ctypes.byref(_desc(C=3)), ctypes.byref(s)) == 0
    assert lib.gnca_rollout_fwd_workspace_bytes(ctypes.byref(_desc(C=3)), ctypes.byref(s)) == 0


def test_rejects_bad_args_without_touching_gpu(lib):
    keep = []
    d, w, g = _desc(), L.Weights(), L.Grads()
    s = _sched(3, keep=keep)
    fwd = lambda sched: lib.gnca_rollout_fwd_f32(ctypes.byref(d), ctypes.byref(w), sched, None, None, None, 0,
                                                 None, 0, None)
    bwd = lambda sched: lib.gnca_rollout_bwd_f32(ctypes.byref(d), ctypes.byref(w), sched, None, 0, None, None,
                                                 ctypes.byref(g), None, 0, None)
    assert fwd(ctypes.byref(s)) == -1 and bwd(ctypes.byref(s)) == -1
    assert fwd(None) == -1 and bwd(None) == -1
    neg = _sched(3, keep=keep)
    neg.steps = -1
    # steps < 0 is invalid even with every pointer set (addresses never dereferenced: no launch is reached)
    p = 4096
    assert lib.gnca_rollout_fwd_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(neg), p, 2 * p, 3 * p, 1 << 40,
                                    4 * p, 1 << 40, None) == -1
    assert lib.gnca_rollout_bwd_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(neg), 3 * p, 1 << 40, p, 2 * p,
                                    ctypes.byref(g), 4 * p, 1 << 40, None) == -1


# ---- the schedule helper ----
def _build(**kw):
    base = dict(steps=3, B=2, H=8, W=8, device="cpu", message_gain=0.25)
    base.update(kw)
    return S.build_schedule(**base)


def test_schedule_defaults():
    s = _build(offsets=[R4[:2], R4[2:4], R4[4:6]])
    assert (s.steps, s.full_steps, s.k, s.fire_mode, s.recompute) == (3, 0, 2, L.FIRE_NONE, False)
    assert s.fire_rates == [1.0] * 3 and s.gains == [0.25] * 3 and s.uniform
    s = _build(fire_rate=[1.0, 0.5, 0.5], seed=7, min_steps=9, message_gain=[0.25, 0.0, 0.25])
    assert s.fire_mode == L.FIRE_HASH and s.seed == 7 and s.full_steps == 3 and not s.uniform
    assert _build(nsteps=torch.zeros(2, dtype=torch.int32)).uniform is False
    assert _build(fire=torch.zeros(3, 2, 1, 8, 8, dtype=torch.bool)).fire_mode == L.FIRE_MASK_U8
    assert _build(fire=torch.zeros(3, 2, 1, 8, 8)).fire_mode == L.FIRE_RAND_F32
    assert _build(steps=0).fire_rates == []


def test_schedule_seed_from_torch_generator():
    torch.manual_seed(5)
    a = _build(fire_rate=0.5).seed
    torch.manual_seed(5)
    assert _build(fire_rate=0.5).seed == a
    st = torch.get_rng_state()
    _build(fire_rate=1.0)   # no mask, no draw
    assert torch.equal(torch.get_rng_state(), st)


@pytest.mark.parametrize("bad", [
    dict(steps=-1), dict(steps=2.0), dict(steps=True), dict(min_steps=-1), dict(min_steps=1.5),
    dict(fire_rate=[0.5, 0.5]), dict(fire_rate="x"), dict(message_gain=[0.1] * 4),
    dict(offsets=[R4[:2], R4[:2]]),                       # 2 entries for 3 steps
    dict(offsets=[R4[:2], R4[:3], R4[:2]]),               # ragged
    dict(offsets=[[(0, 128)]] * 3), dict(offsets=[[(-200, 0)]] * 3), dict(offsets=[[(1.5, 0)]] * 3),
    dict(offsets=[[(1, 2, 3)]] * 3),
    dict(offsets=[R4[:1] * 129] * 3),                     # more than GNCA_MAX_OFFSETS
    dict(offsets=[R4[:2]] * 3, message_gain=None),        # offsets without the graph term
    dict(nsteps=[3, 3]), dict(nsteps=torch.zeros(2, dtype=torch.int64)),
    dict(nsteps=torch.zeros(3, dtype=torch.int32)), dict(nsteps=torch.zeros(2, 1, dtype=torch.int32)),
    dict(nsteps=torch.zeros(2, dtype=torch.int32, device="meta")),
    dict(fire=torch.zeros(2, 2, 1, 8, 8)), dict(fire=torch.zeros(3, 2, 8, 8)),
    dict(fire=torch.zeros(3, 2, 1, 8, 8, dtype=torch.float64)),
    dict(fire=torch.zeros(3, 2, 1, 8, 8, device="meta")), dict(fire=[[0.5]]),
    dict(fire_rate=0.5, seed=1.5), dict(fire_rate=0.5, seed="s"),
])
def test_schedule_rejects_malformed(bad):
    with pytest.raises(ValueError):
        _build(**bad)


@pytest.mark.parametrize("T", [0, 1, 5])
def test_schedule_draws_offsets_like_forward(T):
    """offsets=None: one graph.sample_offsets() per step in step order, i.e. Python's ``random`` is
    left where T manual random.sample(graph.offsets, k) draws leave it (message-off steps too)."""
    from graph_neural_cellular_automata_amd.modules.graph_augmentation import GraphAugmentation
    graph = GraphAugmentation(16)
    random.seed(11)
    manual = [random.sample(graph.offsets, 8) for _ in range(T)]
    after = random.random()
    random.seed(11)
    s = _build(steps=T, message_gain=[0.0] * T, sample_offsets=graph.sample_offsets)
    assert random.random() == after
    assert (s.offsets or []) == manual and s.k == (8 if T else 0)
