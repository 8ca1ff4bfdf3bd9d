"""CPU-side checks of checkpointed BPTT (GNCA_SCHED_CHECKPOINT): the new field sits in the schedule's old
padding, the tape is the anchors alone, the memory really is bounded, bad schedules and taps are
rejected before any launch, the Python layer validates ``checkpoint_every`` before anything is drawn, and
``rollout_memory`` is the three host-only size queries.  No GPU needed."""
import ctypes
import math
import os
import random
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a non-null pointer that is never dereferenced: every call below returns before a launch
R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _desc(**kw):
    base = dict(B=4, C=16, H=72, W=72, hidden=128, d_model=16, offsets=R4[:8],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY,
                update_gain=0.05, alpha_thr=0.12, message_gain=0.25, fire_rate=0.5, fire_mode=L.FIRE_HASH)
    base.update(kw)
    return S.make_desc(**base)


def _sched(steps, keep, flags=0, every=0, k=8):
    s = L.RolloutSched()
    s.steps, s.flags, s.ckpt_every = steps, flags, every
    if steps > 0 and k > 0:
        flat = [v for t in range(steps) for o in R4[t % 8:t % 8 + k] for v in o]
        arr = (ctypes.c_int8 * len(flat))(*flat)
        keep.append(arr)
        s.offsets = ctypes.cast(arr, ctypes.c_void_p)
    return s


def _sizes(lib, d, s):
    return tuple(fn(ctypes.byref(d), ctypes.byref(s)) for fn in (
        lib.gnca_rollout_tape_bytes, lib.gnca_rollout_fwd_workspace_bytes, lib.gnca_rollout_bwd_workspace_bytes))


def _align256(n):
    return (n + 255) & ~255


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_struct_probe(lib, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_rollout_sched));',
             'printf("ckpt_every %zu\\n", offsetof(gnca_rollout_sched, ckpt_every));',
             'printf("flags %zu\\n", offsetof(gnca_rollout_sched, flags));',
             'printf("offsets %zu\\n", offsetof(gnca_rollout_sched, offsets));',
             'printf("checkpoint %u\\n", GNCA_SCHED_CHECKPOINT);',
             'printf("recompute %u\\n", GNCA_SCHED_RECOMPUTE);',
             'printf("version %d\\n", GNCA_ABI_VERSION);', 'return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (l.split() for l in
                                  subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())}
    assert got["ckpt_every"] == 12 == L.RolloutSched.ckpt_every.offset
    assert got["flags"] == 8 and got["offsets"] == 16 == L.RolloutSched.offsets.offset
    assert got["size"] == ctypes.sizeof(L.RolloutSched) == 56     # (what it was before the field)
    assert got["checkpoint"] == L.SCHED_CHECKPOINT == 2 and got["recompute"] == L.SCHED_RECOMPUTE == 1
    assert got["version"] == L.ABI_VERSION == lib.gnca_abi_version() == 5
    assert "gnca_rollout_fwd_taps" in L.EXPORTS and len(lib.gnca_rollout_fwd_taps.argtypes) == 12


@pytest.mark.parametrize("flags", [0, L.SCHED_RECOMPUTE], ids=["tape", "recompute"])
def test_tape_is_the_anchors(lib, flags):
    keep = []
    d = _desc()
    state = _align256(4 * 16 * 72 * 72 * 4)
    for T in (1, 5, 6, 7, 12):
        for k in (1, 2, 3, 6, 7, 100):
            s = _sched(T, keep, flags | L.SCHED_CHECKPOINT, k)
            assert lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(s)) == math.ceil(T / k) * state, (T, k)
    odd = _desc(B=3, C=5, H=11, W=13, hidden=64, offsets=[], flags=L.USE_GROUPNORM)   # a state that needs the padding
    s = _sched(7, keep, flags | L.SCHED_CHECKPOINT, 3, k=0)
    assert lib.gnca_rollout_tape_bytes(ctypes.byref(odd), ctypes.byref(s)) == 3 * _align256(3 * 5 * 11 * 13 * 4)
    assert lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(_sched(0, keep, L.SCHED_CHECKPOINT, 3))) == 0


def test_flag_handling(lib):
    keep = []
    d, w, g = _desc(), L.Weights(), L.Grads()
    p = 4096
    for every in (0, -1):
        s = _sched(6, keep, L.SCHED_CHECKPOINT, every)
        assert _sizes(lib, d, s) == (0, 0, 0)
        assert lib.gnca_rollout_fwd_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(s), p, 2 * p, 3 * p, 1 << 40,
                                        4 * p, 1 << 40, None) == -1
        assert lib.gnca_rollout_bwd_f32(ctypes.byref(d), ctypes.byref(w), ctypes.byref(s), 3 * p, 1 << 40, p, 2 * p,
                                        ctypes.byref(g), 4 * p, 1 << 40, None) == -1
    # the field is read only with the flag: whatever it holds, a schedule without the flag is today's
    for flags in (0, L.SCHED_RECOMPUTE):
        plain = _sizes(lib, d, _sched(6, keep, flags))
        assert all(plain)
        for every in (3, -7, 0x7FFFFFFF):
            assert _sizes(lib, d, _sched(6, keep, flags, every)) == plain


@pytest.mark.parametrize("B", [4, 1024])
@pytest.mark.parametrize("flags", [0, L.SCHED_RECOMPUTE], ids=["tape", "recompute"])
def test_memory_is_bounded(lib, B, flags):
    """What the backward keeps alive beyond the plain schedule's workspace: the anchors, the segment's
    states (and workspaces) and at most two extra slots."""
    keep = []
    d = _desc(B=B)
    for T, k, frac in ((36, 6, 2), (400, 20, 4)):
        tape0, fwd0, bwd0 = _sizes(lib, d, _sched(T, keep, flags))
        tape1, fwd1, bwd1 = _sizes(lib, d, _sched(T, keep, flags | L.SCHED_CHECKPOINT, k))
        assert fwd1 == fwd0                      # the forward's workspace does not grow
        assert tape1 + bwd1 - bwd0 < tape0 // frac, (T, k, tape1, bwd1 - bwd0, tape0)
        # the documented formula: (m-1) states and (m-1) (or one) forward workspaces
        state = _align256(B * 16 * 72 * 72 * 4)
        slot = tape0 // T
        fwd_ws = slot - state if not flags else None
        if fwd_ws is not None:
            assert bwd1 - bwd0 == (k - 1) * (state + fwd_ws)
        else:
            full_slot = _sizes(lib, d, _sched(T, keep, 0))[0] // T
            assert bwd1 - bwd0 == (k - 1) * state + (full_slot - state)
    # k >= T: m = T;  k = 1: no segment area at all
    tape0, _, bwd0 = _sizes(lib, d, _sched(5, keep, flags))
    assert _sizes(lib, d, _sched(5, keep, flags | L.SCHED_CHECKPOINT, 100)) == \
        _sizes(lib, d, _sched(5, keep, flags | L.SCHED_CHECKPOINT, 5))
    assert _sizes(lib, d, _sched(5, keep, flags | L.SCHED_CHECKPOINT, 1))[2] == bwd0


# ---------------------------------------------------------------------------------------------
# Taps
# ---------------------------------------------------------------------------------------------
def _taps(steps, keep, kind=L.TAP_PREMULT, n=None, target=FAKE, geometry=(4, 72, 72)):
    t = L.RolloutTaps()
    t.n = len(steps) if n is None else n
    if steps is not None:
        arr = (ctypes.c_int32 * max(len(steps), 1))(*steps)
        keep.append(arr)
        t.steps = ctypes.cast(arr, ctypes.c_void_p)
    t.kind = kind
    t.masked.B, t.masked.H, t.masked.W = geometry
    t.target = target
    return t


def test_tap_loss_refuses_a_checkpointed_tape(lib):
    keep = []
    d = _desc()
    t = _taps([2, 4, 6], keep)
    for k in (1, 2, 6):
        s = _sched(6, keep, L.SCHED_CHECKPOINT, k)
        assert lib.gnca_rollout_tap_loss(ctypes.byref(d), ctypes.byref(s), ctypes.byref(t), FAKE, 1 << 40, FAKE, FAKE,
                                         FAKE) == -1


BAD_TAPS = {
    "null-steps": dict(steps=None, n=2),
    "null-target": dict(steps=[2, 4], target=None),
    "n-zero": dict(steps=[2], n=0),
    "n-negative": dict(steps=[2], n=-1),
    "not-increasing": dict(steps=[2, 2]),
    "decreasing": dict(steps=[4, 2]),
    "step-zero": dict(steps=[0, 2]),
    "past-T": dict(steps=[2, 7]),
    "unknown-kind": dict(steps=[2], kind=2),
    "premult-B": dict(steps=[2], geometry=(5, 72, 72)),
    "masked-H": dict(steps=[2], kind=L.TAP_MASKED, geometry=(4, 71, 72)),
    "masked-W": dict(steps=[2], kind=L.TAP_MASKED, geometry=(4, 72, 16)),
}


@pytest.mark.parametrize("every", [None, 2], ids=["plain", "checkpointed"])
@pytest.mark.parametrize("case", list(BAD_TAPS))
def test_fwd_taps_rejects_bad_taps_before_any_launch(lib, case, every):
    keep = []
    d, w = _desc(), L.Weights()
    s = _sched(6, keep) if every is None else _sched(6, keep, L.SCHED_CHECKPOINT, every)
    t = _taps(keep=keep, **BAD_TAPS[case])
    assert lib.gnca_rollout_fwd_taps(ctypes.byref(d), ctypes.byref(w), ctypes.byref(s), ctypes.byref(t), FAKE,
                                     FAKE + 64, FAKE, 1 << 40, FAKE, FAKE, FAKE, 1 << 40) == -1


def test_fwd_taps_rejects_null_arguments(lib):
    keep = []
    d, w = _desc(), L.Weights()
    s = _sched(6, keep, L.SCHED_CHECKPOINT, 2)
    t, m = _taps([2, 4, 6], keep), _taps([2, 4, 6], keep, kind=L.TAP_MASKED)
    ft = lambda taps, x=FAKE, out=FAKE + 64, losses=FAKE, alive=FAKE, sched=s: lib.gnca_rollout_fwd_taps(
        ctypes.byref(d), ctypes.byref(w), ctypes.byref(sched), taps, x, out, FAKE, 1 << 40, losses, alive, FAKE,
        1 << 40)
    assert ft(None) == -1
    assert ft(ctypes.byref(t), losses=None) == -1
    assert ft(ctypes.byref(m), alive=None) == -1
    assert ft(ctypes.byref(t), x=None) == -1 and ft(ctypes.byref(t), out=None) == -1
    assert ft(ctypes.byref(t), x=FAKE, out=FAKE) == -1                      # x_final aliases x
    assert ft(ctypes.byref(t), sched=_sched(6, keep, L.SCHED_CHECKPOINT, 0)) == -1


# ---------------------------------------------------------------------------------------------
# The Python layer
# ---------------------------------------------------------------------------------------------
def _models():
    torch.manual_seed(0)
    return NeuralCA(16, 32), NeuralCAGraph(16, 32, graph_attention_radius=2, graph_num_neighbors=4)


X = torch.rand(3, 16, 12, 12)
TGT = torch.rand(4, 12, 12)


@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", boom)


@pytest.mark.parametrize("graph", [False, True], ids=["classic", "graph"])
@pytest.mark.parametrize("bad", [0, -3, 2.5, True, "sqrt"], ids=repr)
def test_bad_checkpoint_every_raises_before_anything_is_drawn(no_library, graph, bad):
    model = _models()[graph]
    random.seed(5)
    before = random.getstate()
    tbefore = torch.get_rng_state()
    with pytest.raises(ValueError, match="checkpoint_every"):
        model.rollout(X, 6, fire_rate=0.5, checkpoint_every=bad)
    with pytest.raises(ValueError, match="checkpoint_every"):
        model.rollout_objective(X, 6, TGT, fire_rate=0.5, checkpoint_every=bad)
    with pytest.raises(ValueError, match="checkpoint_every"):
        model.rollout_memory(X, 6, fire_rate=0.5, checkpoint_every=bad)
    with pytest.raises(ValueError, match="checkpoint_every"):
        S.build_schedule(steps=6, B=3, H=12, W=12, device="cpu", checkpoint_every=bad,
                         message_gain=0.5 if graph else None,
                         sample_offsets=model.graph.sample_offsets if graph else None)
    assert random.getstate() == before, "offsets were drawn on a bad call"
    assert torch.equal(torch.get_rng_state(), tbefore), "a seed was drawn on a bad call"


def test_auto_is_the_ceiling_of_the_square_root():
    for T in (0, 1, 2, 3, 4, 5, 9, 10, 16, 17, 48, 72, 80, 99, 100, 101, 200, 399, 400, 401):
        s = S.build_schedule(steps=T, B=2, H=8, W=8, device="cpu", checkpoint_every="auto")
        assert s.checkpoint_every == max(math.ceil(math.sqrt(T)), 1), T
        assert (s.checkpoint_every - 1) ** 2 < max(T, 1) <= s.checkpoint_every ** 2
    assert S.build_schedule(steps=6, B=2, H=8, W=8, device="cpu").checkpoint_every is None
    assert S.build_schedule(steps=6, B=2, H=8, W=8, device="cpu", checkpoint_every=9).checkpoint_every == 9


def test_rollout_call_sets_the_flag_and_the_field():
    d = _desc(B=2, H=8, W=8, offsets=[])
    mk = lambda **kw: S.RolloutCall(d, S.build_schedule(steps=6, B=2, H=8, W=8, device="cpu", **kw)).c
    c = mk()
    assert c.flags == 0 and c.ckpt_every == 0
    c = mk(checkpoint_every=4)
    assert c.flags == L.SCHED_CHECKPOINT and c.ckpt_every == 4
    c = mk(checkpoint_every="auto", recompute=True)
    assert c.flags == L.SCHED_CHECKPOINT | L.SCHED_RECOMPUTE and c.ckpt_every == 3


def test_signatures_carry_the_keyword():
    import inspect
    for cls in (NeuralCA, NeuralCAGraph):
        ro = inspect.signature(cls.rollout).parameters
        for name in ("rollout", "rollout_objective", "rollout_memory"):
            p = inspect.signature(getattr(cls, name)).parameters["checkpoint_every"]
            assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
        mem = inspect.signature(cls.rollout_memory).parameters
        assert list(mem)[:3] == ["self", "x_or_shape", "steps"]
        for name, p in list(ro.items())[3:]:
            assert name in mem and mem[name].default == p.default, (cls.__name__, name)


@pytest.mark.parametrize("graph", [False, True], ids=["classic", "graph"])
def test_rollout_memory_is_the_three_queries(lib, graph):
    model = _models()[graph]
    T = 7
    offs = [R4[t:t + 4] for t in range(T)]
    nst = torch.tensor([7, 4, 5], dtype=torch.int32)
    for kw in (dict(), dict(recompute=True), dict(checkpoint_every=3), dict(checkpoint_every="auto", recompute=True),
               dict(checkpoint_every=2, nsteps=nst, min_steps=2)):
        extra = dict(offsets=offs) if graph else {}
        random.seed(3)
        torch.manual_seed(3)
        before, tbefore = random.getstate(), torch.get_rng_state()
        got = model.rollout_memory(X, T, fire_rate=0.5, **extra, **kw)
        same = model.rollout_memory((3, 16, 12, 12), T, fire_rate=0.5, **extra, **kw)
        assert random.getstate() == before and torch.equal(torch.get_rng_state(), tbefore)
        # the raw queries on a schedule built by hand
        d = S.make_desc(B=3, C=16, H=12, W=12, hidden=32, d_model=16 if graph else 1, offsets=offs[0] if graph else [],
                        flags=(L.USE_GROUPNORM | model.graph.flags(False) | L.HIDDEN_ONLY) if graph else L.USE_GROUPNORM,
                        update_gain=model.update_gain, alpha_thr=model.alpha_thr,
                        message_gain=model.message_gain if graph else 0.0, fire_rate=0.5, fire_mode=L.FIRE_HASH)
        s = L.RolloutSched()
        s.steps, s.full_steps = T, kw.get("min_steps", 0)
        s.flags = (L.SCHED_RECOMPUTE if kw.get("recompute") else 0)
        every = kw.get("checkpoint_every")
        if every is not None:
            s.flags |= L.SCHED_CHECKPOINT
            s.ckpt_every = 3 if every == "auto" else every
        keep = []
        if graph:
            flat = [v for o in offs for pair in o for v in pair]
            arr = (ctypes.c_int8 * len(flat))(*flat)
            keep.append(arr)
            s.offsets = ctypes.cast(arr, ctypes.c_void_p)
        if "nsteps" in kw:
            s.nsteps = FAKE   # (a device pointer: the size queries never read it)
        raw = _sizes(lib, d, s)
        assert all(raw)
        assert got == same == dict(zip(("tape", "forward_workspace", "backward_workspace"), raw)), kw
    # offsets=None draws as rollout() would, then puts Python's random back
    if graph:
        random.seed(9)
        before = random.getstate()
        r = model.rollout_memory(X, T, checkpoint_every="auto")
        assert random.getstate() == before and r["tape"] == 3 * _align256(3 * 16 * 12 * 12 * 4)
