"""The tangent's ABI, refusals and host-only size queries, without a GPU: the struct layout against a C
probe, the export list, what the two C entry points refuse before any launch (a fake non-null pointer
is never dereferenced), the workspace sizes, and every ValueError of the Python layer, which fires
before anything is drawn from Python's ``random`` or torch's generator.
"""
import ctypes
import os
import random
import re
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph, TangentResult
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import shape_class_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a non-null pointer that is never dereferenced: every call below returns before a launch
R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


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


def _sched(steps, keep, flags=0, k=8):
    s = L.RolloutSched()
    s.steps, s.flags, s.ckpt_every = steps, flags, 2
    if steps > 0 and k > 0:
        flat = [v for t in range(steps) for o in R4[t % 8:t % 8 + k] for v in o]
        arr = (ctypes.c_int8 * len(flat))(*flat)
        keep.append(arr)
        s.offsets = ctypes.cast(arr, ctypes.c_void_p)
    return s


def _args(record, keep, flags=0, log_norm=FAKE):
    a = L.TangentArgs()
    a.num_records = len(record)
    if record:
        arr = (ctypes.c_int32 * len(record))(*record)
        keep.append(arr)
        a.record = ctypes.cast(arr, ctypes.c_void_p)
    a.flags = flags
    a.log_norm = log_norm
    return a


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_struct_probe(lib, tmp_path):
    fields = ("num_records", "record", "flags", "log_norm", "stream")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_tangent_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(gnca_tangent_args, {f}));' for f in fields]
    lines += ['printf("renorm %u\\n", GNCA_TANGENT_RENORM);', 'printf("version %d\\n", GNCA_ABI_VERSION);',
              'return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (l.split() for l in
                                  subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())}
    assert got["size"] == ctypes.sizeof(L.TangentArgs)
    for f in fields:
        assert got[f] == getattr(L.TangentArgs, f).offset, f
    assert got["renorm"] == L.TANGENT_RENORM == 1
    assert got["version"] == L.ABI_VERSION == 5 == lib.gnca_abi_version()


def test_exports_and_names(lib):
    new = ("gnca_step_tangent_workspace_bytes", "gnca_step_tangent", "gnca_rollout_tangent_workspace_bytes",
           "gnca_rollout_tangent")
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(gnca_\w+)\s*\(", src, re.M))
    assert declared == set(L.EXPORTS)
    for n in new:
        assert n in L.EXPORTS and n in declared and hasattr(lib, n) and not n.endswith("_f32")
    for n, params in re.findall(r"^int (gnca_\w*tangent\w*)\(([^;]*)\);", src, re.M):
        assert not re.search(r"\bvoid\s*\*\s*stream\b", params), n


# ---------------------------------------------------------------------------------------------
# What the C entry points refuse, before any launch
# ---------------------------------------------------------------------------------------------
def _step(lib, d, x=FAKE, v=FAKE, xo=FAKE + 0x100, vo=FAKE + 0x200, w=None, ws=None, n=0):
    w = L.Weights() if w is None else w
    return lib.gnca_step_tangent(ctypes.byref(d), ctypes.byref(w), x, None, None, v, xo, vo, ws, n, None)


def test_step_refusals(lib):
    d = _desc()
    assert lib.gnca_step_tangent_workspace_bytes(ctypes.byref(d)) > 0
    assert _step(lib, d) == WORKSPACE                       # everything else is in order: no workspace
    for kw in (dict(x=None), dict(v=None), dict(xo=None), dict(vo=None)):
        assert _step(lib, d, **kw) == INVALID, kw
    assert lib.gnca_step_tangent(None, ctypes.byref(L.Weights()), FAKE, None, None, FAKE, FAKE + 1, FAKE + 2, None, 0,
                                 None) == INVALID
    assert lib.gnca_step_tangent(ctypes.byref(d), None, FAKE, None, None, FAKE, FAKE + 1, FAKE + 2, None, 0,
                                 None) == INVALID
    # aliasing between x / v and the outputs
    for kw in (dict(xo=FAKE), dict(vo=FAKE), dict(v=FAKE + 0x40, xo=FAKE + 0x40), dict(v=FAKE + 0x40, vo=FAKE + 0x40),
               dict(xo=FAKE + 0x80, vo=FAKE + 0x80)):
        assert _step(lib, d, **kw) == INVALID, kw
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _step(lib, zp) == UNSUPPORTED and lib.gnca_step_tangent_workspace_bytes(ctypes.byref(zp)) == 0
    # the zero-padded flag without a graph step with offsets changes nothing: that step has no shift
    for ok in (_desc(flags=(d.flags | L.ZERO_PAD_SHIFT) & ~L.GRAPH, offsets=[]), _desc(flags=d.flags | L.ZERO_PAD_SHIFT, offsets=[])):
        assert lib.gnca_step_tangent_workspace_bytes(ctypes.byref(ok)) > 0 and _step(lib, ok) == WORKSPACE
    neg = _desc(alpha_thr=-0.1)        # a negative threshold is served, as by the forward and the backward
    assert _step(lib, neg) == WORKSPACE and lib.gnca_step_tangent_workspace_bytes(ctypes.byref(neg)) > 0


@pytest.mark.parametrize("C,hidden", SC.UNSUPPORTED)
def test_unsupported_shapes(lib, C, hidden):
    d = SC.bare_desc(C, hidden)
    assert lib.gnca_step_tangent_workspace_bytes(ctypes.byref(d)) == 0
    assert _step(lib, d) == UNSUPPORTED
    keep = []
    s, a = _sched(2, keep, k=2), _args([], keep)
    assert lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(a)) == 0


def test_every_supported_class_has_a_size(lib):
    for name in SC.IDS:
        d = SC.desc(name)
        n = lib.gnca_step_tangent_workspace_bytes(ctypes.byref(d))
        assert (n == 0) == bool(SC.CASES[name]["zp"] and SC.CASES[name]["graph"]), name


def _roll(lib, d, s, a, x=FAKE, v=FAKE, xf=FAKE + 0x100, vf=FAKE + 0x200, ws=None, n=0):
    return lib.gnca_rollout_tangent(ctypes.byref(d), ctypes.byref(L.Weights()), ctypes.byref(s), ctypes.byref(a),
                                    x, v, xf, vf, ws, n)


def test_rollout_refusals(lib):
    keep = []
    d = _desc()
    s, a = _sched(6, keep), _args([2, 6], keep)
    size = lambda d_, s_, a_: lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d_), ctypes.byref(s_),  # noqa: E731
                                                                       ctypes.byref(a_))
    assert size(d, s, a) > 0 and _roll(lib, d, s, a) == WORKSPACE
    for kw in (dict(x=None), dict(v=None), dict(xf=None), dict(vf=None), dict(xf=FAKE), dict(vf=FAKE),
               dict(v=FAKE + 8, xf=FAKE + 8), dict(v=FAKE + 8, vf=FAKE + 8), dict(xf=FAKE + 16, vf=FAKE + 16)):
        assert _roll(lib, d, s, a, **kw) == INVALID, kw
    for fl in (L.SCHED_RECOMPUTE, L.SCHED_CHECKPOINT, L.SCHED_RECOMPUTE | L.SCHED_CHECKPOINT):   # there is no tape
        bad = _sched(6, keep, flags=fl)
        assert _roll(lib, d, bad, a) == INVALID and size(d, bad, a) == 0, fl
    for rec in ([0], [7], [2, 2], [3, 2], [-1]):                      # a malformed record list
        bad = _args(rec, keep)
        assert _roll(lib, d, s, bad) == INVALID and size(d, s, bad) == 0, rec
    null_rec = _args([2], keep)
    null_rec.record = None
    assert _roll(lib, d, s, null_rec) == INVALID
    assert _roll(lib, d, s, _args([2], keep, log_norm=None)) == INVALID
    assert _roll(lib, d, s, _args([2], keep, flags=2)) == INVALID    # an unknown flag
    assert _roll(lib, d, s, _args([], keep, log_norm=None)) == WORKSPACE
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _roll(lib, zp, s, a) == UNSUPPORTED and size(zp, s, a) == 0


def test_rollout_workspace_does_not_grow_with_steps(lib):
    """T = 8 against T = 4096: the difference is the [T][B] mask bytes (256-byte aligned), nothing else."""
    keep = []
    d = _desc()
    a = _args([], keep)
    n8 = lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(8, keep)), ctypes.byref(a))
    n4096 = lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(4096, keep)), ctypes.byref(a))
    al = lambda n: (n + 255) & ~255                                   # noqa: E731
    assert n8 > 0 and n4096 - n8 == al(4096 * d.B) - al(8 * d.B)
    state = al(d.B * d.C * d.H * d.W * 4)
    step = lib.gnca_step_tangent_workspace_bytes(ctypes.byref(d))
    assert n8 >= al(8 * d.B) + step + 4 * state and n8 - (al(8 * d.B) + step + 4 * state) < 64 * 1024
    # records change nothing either: the norm buffers are there anyway
    assert lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(8, keep)),
                                                    ctypes.byref(_args([1, 8], keep))) == n8


# ---------------------------------------------------------------------------------------------
# The Python layer: every ValueError, before anything is drawn
# ---------------------------------------------------------------------------------------------
def _graph(zp=False, thr=0.1):
    torch.manual_seed(0)
    return NeuralCAGraph(8, 32, alpha_thr=thr, graph_attention_radius=2, graph_num_neighbors=4,
                         graph_zero_padded_shift=zp)


def _raises_untouched(fn):
    random.seed(5)
    torch.manual_seed(5)
    py, tc = random.getstate(), torch.get_rng_state()
    with pytest.raises(ValueError) as e:
        fn()
    assert random.getstate() == py and torch.equal(torch.get_rng_state(), tc), "a refused call drew something"
    return str(e.value)


def test_python_refusals():
    m, c = _graph(), NeuralCA(8, 32)
    x, v = torch.rand(2, 8, 6, 6), torch.rand(2, 8, 6, 6)
    offs = [(2, 0), (0, 2), (-2, 0), (0, -2)]
    f56, f66d, f1 = torch.rand(2, 1, 5, 6), torch.rand(2, 1, 6, 6).double(), torch.rand(1, 1, 6, 6)   # (drawn here)
    for fn in (
        lambda: m.tangent_step(x, v[:1]),                                  # shapes differ
        lambda: m.tangent_step(x[0], v[0]),                                # not [B,C,H,W]
        lambda: m.tangent_step(x[:, :4], v[:, :4]),                        # channel count
        lambda: m.tangent_step(x, v.double()),                             # dtype
        lambda: m.tangent_step(x, v, "half"),
        lambda: m.tangent_step(x, v, offsets=[(1, 2, 3)]),
        lambda: m.tangent_step(x, v, offsets=[(300, 0)]),
        lambda: m.tangent_step(x, v, offsets=5),
        lambda: m.tangent_step(x, v, fire=f56),
        lambda: m.tangent_step(x, v, fire=f66d),
        lambda: m.tangent_step(x, v, active=torch.ones(3, dtype=torch.bool)),
        lambda: m.tangent_step(x, v, active=torch.ones(2)),
        lambda: c.tangent_step(x, v, fire=f1),
        lambda: m.rollout_tangent(x, v, -1),
        lambda: m.rollout_tangent(x, v, 2.0),
        lambda: m.rollout_tangent(x, v[:1], 2),
        lambda: m.rollout_tangent(x, v, 4, record=[0]),
        lambda: m.rollout_tangent(x, v, 4, record=[5]),
        lambda: m.rollout_tangent(x, v, 4, record=[2, 2]),
        lambda: m.rollout_tangent(x, v, 4, record=[1.5]),
        lambda: m.rollout_tangent(x, v, 4, every=0),
        lambda: m.rollout_tangent(x, v, 4, every=2, record=[2]),
        lambda: m.rollout_tangent(x, v, 4, renormalize=1),
        lambda: c.rollout_tangent(x, v, 4, every="2"),
    ):
        _raises_untouched(fn)
    # schedule errors are build_schedule's (after the device check for a CPU state they cannot be reached
    # here); the pure-Python builder raises them on its own
    for kw in (dict(fire_rate=[0.5]), dict(message_gain=[0.1] * 3), dict(offsets=[offs] * 3), dict(seed="s", fire_rate=0.5),
               dict(nsteps=torch.zeros(3, dtype=torch.int32)), dict(min_steps=-1)):
        base = dict(steps=4, B=2, H=6, W=6, device="cpu", message_gain=0.5)
        base.update(kw)
        with pytest.raises(ValueError):
            S.build_schedule(**base)


def test_zero_padded_shift_is_refused_and_nothing_else():
    x, v = torch.rand(2, 8, 6, 6), torch.rand(2, 8, 6, 6)
    zp = _graph(zp=True)
    for fn in (lambda: zp.tangent_step(x, v), lambda: zp.rollout_tangent(x, v, 3)):
        msg = _raises_untouched(fn)
        assert "zero-padded shift" in msg and "graph_zero_padded_shift=False" in msg
    # a valid call on a CPU state reaches the device check (there is no CPU path), a negative threshold included
    for m in (_graph(), _graph(thr=-0.1)):
        with pytest.raises(RuntimeError):
            m.tangent_step(x, v)


def test_allocation_sites_and_result_type():
    src = open(os.path.join(ROOT, "graph_neural_cellular_automata_amd", "step.py")).read()
    body = src[src.index("def step_tangent"):]
    assert "torch.empty" in body and ".new_empty" not in body and ".new_zeros" not in body and "torch.zeros" not in body
    r = TangentResult(1, 2, [3], 4)
    assert (r.x_final, r.v_final, r.steps, r.log_norm) == (1, 2, [3], 4)
