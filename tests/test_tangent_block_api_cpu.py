"""The tangent block's ABI, refusals and host-only size queries, without a GPU: the struct layout against
a C probe, the export list and the naming rules, what the four C entry points (gnca_tangent_qr,
gnca_rollout_tangent_block and their workspace queries) refuse before any launch (a fake non-null
pointer is never dereferenced), the workspace sizes, and every ValueError of the Python layer, which
fires before anything is drawn from Python's ``random`` or torch's generators.
"""
import ctypes
import os
import random
import re
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import (NeuralCA, NeuralCAGraph, TangentBlockResult, TangentQR,
                                                orthonormalize_tangents)
from graph_neural_cellular_automata_amd import _lib as L
from tests import shape_class_cases as SC
from tests.test_tangent_api_cpu import FAKE, INVALID, ROOT, UNSUPPORTED, WORKSPACE, _desc, _sched

NEW = ("gnca_tangent_qr_workspace_bytes", "gnca_tangent_qr", "gnca_rollout_tangent_block_workspace_bytes",
       "gnca_rollout_tangent_block")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _args(record, keep, K=3, flags=L.TBLOCK_ORTHO, log_r=FAKE):
    a = L.TangentBlockArgs()
    a.num_dirs = K
    a.num_records = len(record)
    if record:
        arr = (ctypes.c_int32 * len(record))(*record)
        keep.append(arr)
        a.record = ctypes.cast(arr, ctypes.c_void_p)
    a.flags = flags
    a.log_r = log_r
    return a


def _al(n):
    return (n + 255) & ~255


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_struct_probe(lib, tmp_path):
    fields = ("num_dirs", "num_records", "record", "flags", "log_r", "stream")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_tangent_block_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(gnca_tangent_block_args, {f}));' for f in fields]
    lines += ['printf("ortho %u\\n", GNCA_TBLOCK_ORTHO);', 'printf("maxdirs %d\\n", GNCA_TANGENT_MAX_DIRS);',
              'printf("chunk %d\\n", GNCA_TANGENT_QR_CHUNK);', 'printf("version %d\\n", GNCA_ABI_VERSION);',
              'return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (l.split() for l in
                                  subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())}
    assert got["size"] == ctypes.sizeof(L.TangentBlockArgs)
    for f in fields:
        assert got[f] == getattr(L.TangentBlockArgs, f).offset, f
    assert got["ortho"] == L.TBLOCK_ORTHO == 1
    assert got["maxdirs"] == L.TANGENT_MAX_DIRS == 16 and got["chunk"] == L.TANGENT_QR_CHUNK
    assert got["version"] == L.ABI_VERSION == 5 == lib.gnca_abi_version()      # additions only


def test_exports_and_names(lib):
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(gnca_\w+)\s*\(", src, re.M))
    assert declared == set(L.EXPORTS)
    for n in NEW:
        assert n in L.EXPORTS and n in declared and hasattr(lib, n) and not n.endswith("_f32")
    decls = dict(re.findall(r"^int (gnca_\w*tangent\w*)\(([^;]*)\);", src, re.M))
    assert {"gnca_tangent_qr", "gnca_rollout_tangent_block"} <= set(decls)
    for n, params in decls.items():
        assert not re.search(r"\bvoid\s*\*\s*stream\b", params), n
    assert re.search(r"\bvoid\s*\*\s*hip_stream\b", decls["gnca_tangent_qr"])
    assert "stream" not in decls["gnca_rollout_tangent_block"]                  # it travels in the args struct


# ---------------------------------------------------------------------------------------------
# gnca_tangent_qr: refusals and sizes
# ---------------------------------------------------------------------------------------------
def _qr(lib, K=3, B=2, n=140, v=FAKE, r=FAKE + 0x100, ld=FAKE + 0x200, ws=None, nb=0):
    return lib.gnca_tangent_qr(K, B, n, v, r, ld, ws, nb, None)


def test_qr_refusals_and_sizes(lib):
    size = lib.gnca_tangent_qr_workspace_bytes
    assert size(3, 2, 140) > 0 and _qr(lib) == WORKSPACE          # everything else is in order: no workspace
    assert _qr(lib, r=None, ld=None) == WORKSPACE                  # both outputs are optional
    assert _qr(lib, ws=FAKE, nb=size(3, 2, 140) - 1) == WORKSPACE
    for kw in (dict(K=0), dict(K=17), dict(K=-1), dict(B=0), dict(n=0), dict(n=-5), dict(v=None)):
        assert _qr(lib, **kw) == INVALID, kw
    for K, B, n in ((0, 2, 140), (17, 2, 140), (3, 0, 140), (3, 2, 0)):
        assert size(K, B, n) == 0, (K, B, n)
    assert size(1, 1, 1) > 0 and size(16, 1, 3) > 0                # K > n is served
    # [Gram partials: room for 16 directions' 136 pairs per (sample, chunk) | Rinv [B][16][16]]
    for B, n in ((2, 140), (3, 4096), (3, 4097), (128, 16 * 72 * 72)):
        nchunk = -(-n // L.TANGENT_QR_CHUNK)
        want = _al(B * nchunk * 136 * 8) + _al(B * 256 * 8)
        assert {size(K, B, n) for K in (1, 3, 16)} == {want}, (B, n)
    assert size(3, 2, 1 << 33) > 0                                  # a 64-bit element count
    assert size(3, 1 << 30, 1 << 20) == 0                           # more workgroups than a grid holds


# ---------------------------------------------------------------------------------------------
# gnca_rollout_tangent_block: refusals and sizes
# ---------------------------------------------------------------------------------------------
def _roll(lib, d, s, a, x=FAKE, v=FAKE + 0x40, xf=FAKE + 0x100, vf=FAKE + 0x200, ws=None, n=0):
    return lib.gnca_rollout_tangent_block(ctypes.byref(d), ctypes.byref(L.Weights()), ctypes.byref(s), ctypes.byref(a),
                                          x, v, xf, vf, ws, n)


def _size(lib, d, s, a):
    return lib.gnca_rollout_tangent_block_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(a))


def test_rollout_refusals(lib):
    keep = []
    d = _desc()
    s, a = _sched(6, keep), _args([2, 6], keep)
    assert _size(lib, d, s, a) > 0 and _roll(lib, d, s, a) == WORKSPACE
    assert _roll(lib, d, s, a, ws=FAKE + 0x1000, n=_size(lib, d, s, a) - 1) == WORKSPACE
    for kw in (dict(x=None), dict(v=None), dict(xf=None), dict(vf=None), dict(xf=FAKE), dict(vf=FAKE),
               dict(v=FAKE + 8, xf=FAKE + 8), dict(v=FAKE + 8, vf=FAKE + 8), dict(xf=FAKE + 16, vf=FAKE + 16)):
        assert _roll(lib, d, s, a, **kw) == INVALID, kw
    w = L.Weights()
    assert lib.gnca_rollout_tangent_block(None, ctypes.byref(w), ctypes.byref(s), ctypes.byref(a), FAKE, FAKE + 8,
                                          FAKE + 16, FAKE + 24, None, 0) == INVALID
    assert lib.gnca_rollout_tangent_block(ctypes.byref(d), None, ctypes.byref(s), ctypes.byref(a), FAKE, FAKE + 8,
                                          FAKE + 16, FAKE + 24, None, 0) == INVALID
    assert lib.gnca_rollout_tangent_block(ctypes.byref(d), ctypes.byref(w), None, ctypes.byref(a), FAKE, FAKE + 8,
                                          FAKE + 16, FAKE + 24, None, 0) == INVALID
    assert lib.gnca_rollout_tangent_block(ctypes.byref(d), ctypes.byref(w), ctypes.byref(s), None, FAKE, FAKE + 8,
                                          FAKE + 16, FAKE + 24, None, 0) == INVALID
    for K in (0, 17, -3):                                              # the number of directions
        bad = _args([2, 6], keep, K=K)
        assert _roll(lib, d, s, bad) == INVALID and _size(lib, d, s, bad) == 0, K
    for K in (1, 16):
        ok = _args([2, 6], keep, K=K)
        assert _roll(lib, d, s, ok) == WORKSPACE and _size(lib, d, s, ok) > 0, K
    for fl in (L.SCHED_RECOMPUTE, L.SCHED_CHECKPOINT, L.SCHED_RECOMPUTE | L.SCHED_CHECKPOINT):   # there is no tape
        bad = _sched(6, keep, flags=fl)
        assert _roll(lib, d, bad, a) == INVALID and _size(lib, d, bad, a) == 0, fl
    for rec in ([0], [7], [2, 2], [3, 2], [-1]):                      # a malformed record list
        bad = _args(rec, keep)
        assert _roll(lib, d, s, bad) == INVALID and _size(lib, d, s, bad) == 0, rec
    null_rec = _args([2], keep)
    null_rec.record = None
    assert _roll(lib, d, s, null_rec) == INVALID and _size(lib, d, s, null_rec) == 0
    assert _roll(lib, d, s, _args([2], keep, log_r=None)) == INVALID
    for fl in (2, 3, 1 << 31):                                         # an unknown flag
        bad = _args([2], keep, flags=fl)
        assert _roll(lib, d, s, bad) == INVALID and _size(lib, d, s, bad) == 0, fl
    assert _roll(lib, d, s, _args([2], keep, flags=0)) == WORKSPACE    # without ORTHO
    assert _roll(lib, d, s, _args([], keep, log_r=None)) == WORKSPACE
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _roll(lib, zp, s, a) == UNSUPPORTED and _size(lib, zp, s, a) == 0
    # the zero-padded flag without a graph step with offsets changes nothing: that step has no shift
    plain = _desc(flags=(d.flags | L.ZERO_PAD_SHIFT) & ~L.GRAPH, offsets=[])
    s0 = _sched(6, keep, k=0)
    assert _size(lib, plain, s0, a) > 0 and _roll(lib, plain, s0, a) == WORKSPACE
    mask = _desc(fire_mode=L.FIRE_MASK_U8)                              # a fire stack is needed and absent
    assert _roll(lib, mask, s, a, ws=FAKE + 0x1000, n=1 << 40) == INVALID


@pytest.mark.parametrize("C,hidden", SC.UNSUPPORTED)
def test_support_set_boundary(lib, C, hidden):
    d = SC.bare_desc(C, hidden)
    keep = []
    s, a = _sched(2, keep, k=2), _args([], keep)
    assert _size(lib, d, s, a) == 0 and _roll(lib, d, s, a) == UNSUPPORTED


def test_every_supported_class_has_a_size(lib):
    keep = []
    for name in SC.IDS:
        d = SC.desc(name)
        s, a = _sched(2, keep, k=d.num_offsets), _args([1], keep)
        n = _size(lib, d, s, a)
        assert (n == 0) == bool(SC.CASES[name]["zp"] and SC.CASES[name]["graph"]), name


def test_rollout_workspace(lib):
    """T = 8 against T = 4096: the difference is the [T][B] mask bytes (256-byte aligned), nothing else; and the
    size is linear in K: masks, one step workspace, two states, 2 K tangents and what does not depend on K."""
    keep = []
    d = _desc()
    sizes = {}
    for K in (1, 2, 3, 8, 16):
        a = _args([], keep, K=K)
        n8 = _size(lib, d, _sched(8, keep), a)
        n4096 = _size(lib, d, _sched(4096, keep), a)
        assert n8 > 0 and n4096 - n8 == _al(4096 * d.B) - _al(8 * d.B), K
        assert _size(lib, d, _sched(8, keep), _args([1, 8], keep, K=K)) == n8      # records change nothing
        assert _size(lib, d, _sched(8, keep), _args([1, 8], keep, K=K, flags=0)) == n8
        sizes[K] = n8
    state = _al(d.B * d.C * d.H * d.W * 4)
    assert state == d.B * d.C * d.H * d.W * 4                          # (so that K tangents are K states)
    for K in (2, 3, 8, 16):
        assert sizes[K] - sizes[1] == (K - 1) * 2 * state, K
    step = lib.gnca_step_tangent_workspace_bytes(ctypes.byref(d))
    fixed = sizes[1] - (_al(8 * d.B) + step + 2 * state + 2 * state)
    n = d.C * d.H * d.W
    qr = lib.gnca_tangent_qr_workspace_bytes(1, d.B, n)
    assert qr <= fixed < qr + 64 * 1024                                # the QR's, the norm partials, scale, carry
    # one direction more than gnca_rollout_tangent's own workspace costs the QR's buffers alone
    single = lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(8, keep)),
                                                      ctypes.byref(L.TangentArgs()))
    assert 0 < sizes[1] - single <= qr + 64 * 1024


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
    cuda = torch.cuda.is_available()
    py, tc = random.getstate(), torch.get_rng_state()
    cu = torch.cuda.get_rng_state() if cuda else None
    with pytest.raises(ValueError) as e:
        fn()
    assert random.getstate() == py and torch.equal(torch.get_rng_state(), tc), "a refused call drew something"
    assert not cuda or torch.equal(torch.cuda.get_rng_state(), cu), "a refused call drew from the GPU's generator"
    return str(e.value)


def test_python_refusals():
    m, c = _graph(), NeuralCA(8, 32)
    x, V = torch.rand(2, 8, 6, 6), torch.rand(3, 2, 8, 6, 6)
    V17, Q17, Q0b, Q0n = torch.rand(17, 2, 8, 6, 6), torch.rand(17, 2, 5), torch.rand(3, 0, 5), torch.rand(3, 2, 0)
    for fn in (
        lambda: m.rollout_tangent_block(x, V[0], 2),                               # not [K,B,C,H,W]
        lambda: m.rollout_tangent_block(x, V[:0], 2),                              # K = 0
        lambda: m.rollout_tangent_block(x, V17, 2),                                # K = 17
        lambda: m.rollout_tangent_block(x, V[:, :1], 2),                           # another batch
        lambda: m.rollout_tangent_block(x, V[:, :, :4], 2),                        # another channel count
        lambda: m.rollout_tangent_block(x[:, :4], V[:, :, :4], 2),                 # not the model's channels
        lambda: m.rollout_tangent_block(x[0], V, 2),
        lambda: m.rollout_tangent_block(x, V.double(), 2),
        lambda: m.rollout_tangent_block(x, [V[0], V[1]], 2),
        lambda: m.rollout_tangent_block(x, V, -1),
        lambda: m.rollout_tangent_block(x, V, 2.0),
        lambda: m.rollout_tangent_block(x, V, True),
        lambda: m.rollout_tangent_block(x, V, 4, record=[0]),
        lambda: m.rollout_tangent_block(x, V, 4, record=[5]),
        lambda: m.rollout_tangent_block(x, V, 4, record=[2, 2]),
        lambda: m.rollout_tangent_block(x, V, 4, record=[1.5]),
        lambda: m.rollout_tangent_block(x, V, 4, every=0),
        lambda: m.rollout_tangent_block(x, V, 4, every=2, record=[2]),
        lambda: m.rollout_tangent_block(x, V, 4, orthonormalize=1),
        lambda: c.rollout_tangent_block(x, V, 4, every="2"),
        lambda: c.rollout_tangent_block(x, V, 4, orthonormalize=None),
        lambda: orthonormalize_tangents(V[0, 0, 0]),                               # fewer than three dimensions
        lambda: orthonormalize_tangents(V[:0]),
        lambda: orthonormalize_tangents(Q17),
        lambda: orthonormalize_tangents(Q0b),
        lambda: orthonormalize_tangents(Q0n),
        lambda: orthonormalize_tangents(V.double()),
        lambda: orthonormalize_tangents(V.numpy()),
        lambda: orthonormalize_tangents(V, inplace=1),
    ):
        _raises_untouched(fn)


def test_zero_padded_shift_is_refused_and_nothing_else():
    x, V = torch.rand(2, 8, 6, 6), torch.rand(3, 2, 8, 6, 6)
    zp = _graph(zp=True)
    msg = _raises_untouched(lambda: zp.rollout_tangent_block(x, V, 3))
    assert "zero-padded shift" in msg and "graph_zero_padded_shift=False" in msg
    # a valid call on a CPU state reaches the device check (there is no CPU path), a negative threshold included
    for m in (_graph(), _graph(thr=-0.1), NeuralCA(8, 32)):
        with pytest.raises(RuntimeError):
            m.rollout_tangent_block(x, V, 3, every=1)
    with pytest.raises(RuntimeError):
        orthonormalize_tangents(V)


def test_allocation_sites_and_result_types():
    pkg = os.path.join(ROOT, "graph_neural_cellular_automata_amd")
    src = open(os.path.join(pkg, "step.py")).read()
    body = src[src.index("def tangent_qr"):]
    assert "def rollout_tangent_block" in body
    assert "torch.empty" in body and ".new_empty" not in body and ".new_zeros" not in body and "torch.zeros" not in body
    lya = open(os.path.join(pkg, "lyapunov.py")).read()
    assert "torch.empty_like" in lya and not re.search(r"from torch import .*\bempty", lya)
    assert ".new_empty" not in lya and ".new_zeros" not in lya and "torch.zeros" not in lya and ".clone(" not in lya
    r = TangentBlockResult(1, 2, [3, 6], torch.tensor([[[1.0, 2.0]], [[3.0, -6.0]]], dtype=torch.float64))
    assert (r.x_final, r.v_final, r.steps) == (1, 2, [3, 6])
    assert torch.equal(r.exponents(), torch.tensor([[0.5, -1.0]], dtype=torch.float64))
    with pytest.raises(ValueError):
        TangentBlockResult(1, 2, [], torch.empty(0, 1, 2, dtype=torch.float64)).exponents()
    doc = TangentBlockResult.exponents.__doc__
    assert "finite-time" in doc and "nsteps" in doc and "caller" in doc
    q = TangentQR(1, 2, 3)
    assert (q.q, q.r, q.log_diag) == (1, 2, 3)
