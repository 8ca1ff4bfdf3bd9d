"""CPU-side checks of rollout_objective(): the ctypes mirror of gnca_rollout_taps matches the header,
the two entry points are exported and reject bad arguments before any launch, the Python layer
validates taps, target and keywords before any library call (and before any offset is drawn), and
the header gates that read include/gnca.h still see what they expect.  No GPU needed."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnca.h")
NEW = ("gnca_rollout_tap_loss", "gnca_rollout_bwd_taps")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_taps_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.RolloutTaps._fields_]
    inner = [f for f, _ in L.MaskedLossDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_rollout_taps));',
             'printf("premult %d\\n", GNCA_TAP_PREMULT);', 'printf("masked_kind %d\\n", GNCA_TAP_MASKED);',
             'printf("chunk %d\\n", GNCA_TAP_CHUNK);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_rollout_taps, {f}));')
    for f in inner:
        lines.append(f'printf("masked.{f} %zu\\n", offsetof(gnca_rollout_taps, masked.{f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.RolloutTaps)
    assert (int(got["premult"]), int(got["masked_kind"])) == (L.TAP_PREMULT, L.TAP_MASKED) == (0, 1)
    assert int(got["chunk"]) == L.TAP_CHUNK
    for f in fields:
        assert int(got[f]) == getattr(L.RolloutTaps, f).offset, f
    for f in inner:
        assert int(got[f"masked.{f}"]) == L.RolloutTaps.masked.offset + getattr(L.MaskedLossDesc, f).offset, f


def test_new_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW:
        assert n in L.EXPORTS
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert getattr(lib, n).restype is ctypes.c_int
    assert len(lib.gnca_rollout_tap_loss.argtypes) == 8 and len(lib.gnca_rollout_bwd_taps.argtypes) == 14
    assert lib.gnca_abi_version() == L.ABI_VERSION


def test_header_gates_still_pass():
    """The three gates that read the header: every declaration is in EXPORTS; the new entry points carry
    the stream in the descriptor (no ``void* stream`` parameter) and no ``_f32`` suffix."""
    from tests import test_abi_cpu, test_poison_cpu, test_streams_cpu
    assert set(test_abi_cpu.declared_functions()) == set(L.EXPORTS)
    for n in NEW:
        assert n in test_abi_cpu.declared_functions()
        assert n not in test_streams_cpu._entry_points()
        assert n not in test_poison_cpu._entry_points()
    test_streams_cpu.test_every_stream_taking_entry_point_is_covered_or_excluded_with_a_reason()
    test_poison_cpu.test_every_entry_point_is_covered_or_excluded_with_a_reason()
    src = open(HEADER).read()
    struct = re.search(r"typedef struct gnca_rollout_taps \{(.*?)\} gnca_rollout_taps;", src, re.S).group(1)
    assert re.search(r"\bvoid\s*\*\s*stream\b", struct)


R2 = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if max(abs(dy), abs(dx)) > 1]
FAKE = 0x1000      # a non-null pointer that is never dereferenced: every call below returns before a launch


def _desc(**kw):
    base = dict(B=3, C=16, H=32, W=32, hidden=64, d_model=16, offsets=R2[:4],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY, update_gain=0.05, alpha_thr=0.12,
                message_gain=0.25, fire_rate=1.0, fire_mode=L.FIRE_NONE)
    base.update(kw)
    return S.make_desc(**base)


def _sched(T, keep):
    s = L.RolloutSched()
    s.steps = T
    flat = [v for t in range(T) for o in R2[t:t + 4] for v in o]
    arr = (ctypes.c_int8 * len(flat))(*flat)
    keep.append(arr)
    s.offsets = ctypes.cast(arr, ctypes.c_void_p)
    return s


def _taps(steps, keep, kind=L.TAP_PREMULT, n=None, target=FAKE, geometry=(3, 32, 32)):
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
    "premult-B": dict(steps=[2], geometry=(4, 32, 32)),
    "premult-H": dict(steps=[2], geometry=(3, 16, 32)),
    "premult-W": dict(steps=[2], geometry=(3, 32, 0)),
    "masked-B": dict(steps=[2], kind=L.TAP_MASKED, geometry=(4, 32, 32)),
    "masked-H": dict(steps=[2], kind=L.TAP_MASKED, geometry=(3, 31, 32)),
    "masked-W": dict(steps=[2], kind=L.TAP_MASKED, geometry=(3, 32, 16)),
}


@pytest.mark.parametrize("case", list(BAD_TAPS))
def test_entry_points_reject_bad_taps_before_any_launch(lib, case):
    keep = []
    d, s, w, g = _desc(), _sched(6, keep), L.Weights(), L.Grads()
    t = _taps(keep=keep, **BAD_TAPS[case])
    rc = lib.gnca_rollout_tap_loss(ctypes.byref(d), ctypes.byref(s), ctypes.byref(t), FAKE, 1 << 40, FAKE, FAKE, FAKE)
    assert rc == -1
    rc = lib.gnca_rollout_bwd_taps(ctypes.byref(d), ctypes.byref(w), ctypes.byref(s), ctypes.byref(t), FAKE, 1 << 40,
                                   FAKE, FAKE, FAKE, FAKE, FAKE + 64, ctypes.byref(g), FAKE, 1 << 40)
    assert rc == -1


def test_entry_points_reject_null_and_aliased_arguments(lib):
    keep = []
    d, s, w, g = _desc(), _sched(6, keep), L.Weights(), L.Grads()
    t = _taps([2, 4, 6], keep)
    tl = lambda taps, x_final=FAKE, losses=FAKE, alive=FAKE: lib.gnca_rollout_tap_loss(
        ctypes.byref(d), ctypes.byref(s), taps, FAKE, 1 << 40, x_final, losses, alive)
    assert tl(None) == -1 and tl(ctypes.byref(t), x_final=None) == -1 and tl(ctypes.byref(t), losses=None) == -1
    m = _taps([2, 4, 6], keep, kind=L.TAP_MASKED)
    assert tl(ctypes.byref(m), alive=None) == -1
    bt = lambda taps, gy=FAKE, gl=FAKE, gx=FAKE + 64, alive=FAKE: lib.gnca_rollout_bwd_taps(
        ctypes.byref(d), ctypes.byref(w), ctypes.byref(s), taps, FAKE, 1 << 40, FAKE, gy, gl, alive, gx,
        ctypes.byref(g), FAKE, 1 << 40)
    assert bt(None) == -1
    assert bt(ctypes.byref(t), gy=None, gl=None) == -1          # nothing to back-propagate
    assert bt(ctypes.byref(t), gy=FAKE, gx=FAKE) == -1          # gx aliases gy
    assert bt(ctypes.byref(t), gx=None) == -1
    assert bt(ctypes.byref(m), alive=None) == -1


# ---------------------------------------------------------------------------------------------
# The Python layer: validation before any library call
# ---------------------------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", boom)
    monkeypatch.setattr(S.RolloutCall, "forward", boom)


def _models():
    torch.manual_seed(0)
    return NeuralCA(16, 32), NeuralCAGraph(16, 32, graph_attention_radius=2, graph_num_neighbors=4)


X = torch.rand(3, 16, 12, 12)
TGT = torch.rand(4, 12, 12)

BAD_CALLS = {
    "every-and-record": dict(every=2, record=[2, 4]),
    "every-zero": dict(every=0),
    "every-bool": dict(every=True),
    "record-not-increasing": dict(record=[4, 2]),
    "record-repeats": dict(record=[2, 2]),
    "record-zero": dict(record=[0, 3]),
    "record-past-steps": dict(record=[2, 7]),
    "record-float": dict(record=[2.0]),
    "record-empty": dict(record=[]),
    "record-not-a-sequence": dict(record=3),
    "loss-unknown": dict(loss="stability"),
    "alpha-thr-nan": dict(loss="masked", alpha_thr=float("nan")),
    "lam-area-str": dict(loss="masked", lam_area="1e-5"),
    "lam-bg-alpha-inf": dict(loss="masked", lam_bg_alpha=float("inf")),
    "lam-bg-rgb-bool": dict(loss="masked", lam_bg_rgb=True),
}
# (the schedule's own checks are rollout()'s, behind the same refusal of a CPU state: they are run with the
#  state on the device in tests/test_gpu_rollout_objective.py)


@pytest.mark.parametrize("graph", [False, True], ids=["classic", "graph"])
@pytest.mark.parametrize("case", list(BAD_CALLS))
def test_bad_arguments_raise_before_any_library_call(no_library, graph, case):
    model = _models()[graph]
    random.seed(5)
    before = random.getstate()
    with pytest.raises(ValueError):
        model.rollout_objective(X, 6, TGT, **BAD_CALLS[case])
    assert random.getstate() == before, "offsets were drawn on a bad call"


@pytest.mark.parametrize("target", [torch.rand(3, 12, 12), torch.rand(2, 4, 12, 12), torch.rand(4, 12, 11),
                                    torch.rand(1, 1, 4, 12, 12), "target", None],
                         ids=["3ch", "B2", "W11", "5d", "str", "none"])
def test_bad_targets_raise_before_any_library_call(no_library, target):
    for model in _models():
        with pytest.raises(ValueError):
            model.rollout_objective(X, 6, target)


@pytest.mark.parametrize("steps", [0, -1, 2.0, True, None])
def test_bad_steps_raise_before_any_library_call(no_library, steps):
    for model in _models():
        with pytest.raises(ValueError):
            model.rollout_objective(X, steps, TGT)


def test_bad_state_and_graph_keywords(no_library):
    classic, graph = _models()
    with pytest.raises(ValueError):
        classic.rollout_objective(torch.rand(3, 12, 12, 12), 6, TGT)        # 12 channels, the model has 16
    with pytest.raises(ValueError):
        classic.rollout_objective(torch.rand(16, 12, 12), 6, TGT)
    with pytest.raises(TypeError):
        classic.rollout_objective(X, 6, TGT, message_gain=0.5)              # no graph term: no such keyword
    with pytest.raises(TypeError):
        classic.rollout_objective(X, 6, TGT, offsets=[[]] * 6)
    # a CPU or wrongly typed state is refused as every op of the package refuses it, before the schedule
    # is built (no offsets are drawn) and before the library
    random.seed(5)
    before = random.getstate()
    with pytest.raises(RuntimeError, match="There is no CPU path"):
        graph.rollout_objective(X, 6, TGT, every=2)
    with pytest.raises(RuntimeError, match="There is no CPU path"):
        graph.rollout_objective(X, 6, TGT, offsets=[[(2, 0)]] * 5)
    assert random.getstate() == before, "offsets were drawn for a state the call refuses"


def test_signature_carries_every_keyword_of_rollout():
    for cls in (NeuralCA, NeuralCAGraph):
        ro = inspect.signature(cls.rollout).parameters
        ob = inspect.signature(cls.rollout_objective).parameters
        assert list(ob)[:4] == ["self", "x", "steps", "target"]
        for name, p in ro.items():
            assert name in ob and ob[name].default == p.default and ob[name].kind == p.kind, (cls.__name__, name)
        for name, default in dict(every=1, record=None, loss="premult", alpha_thr=0.2, lam_area=5e-5,
                                  lam_bg_alpha=0.0, lam_bg_rgb=0.0).items():
            assert ob[name].default == default and ob[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert "no_grad" in cls.rollout_objective.__doc__ and "trace(" in cls.rollout_objective.__doc__


def test_taps_struct_is_built_from_the_validated_record():
    d = _desc()
    tgt = torch.rand(1, 4, 32, 32)
    t = S.RolloutTaps(d, [2, 4, 6], "masked", (0.2, 5e-5, 1e-3, 2e-4), tgt)
    assert (t.c.n, t.c.kind, t.c.target_bstride, t.c.target) == (3, L.TAP_MASKED, 0, tgt.data_ptr())
    assert list((ctypes.c_int32 * 3).from_address(t.c.steps)) == [2, 4, 6]
    assert (t.c.masked.B, t.c.masked.H, t.c.masked.W) == (3, 32, 32)
    assert t.c.masked.alpha_thr == pytest.approx(0.2) and t.c.masked.lam_bg_rgb == pytest.approx(2e-4)
    per = torch.rand(3, 4, 32, 32)
    assert S.RolloutTaps(d, [6], "premult", None, per).c.target_bstride == 4 * 32 * 32
    with pytest.raises(ValueError):
        S.RolloutTaps(d, [], "premult", None, tgt)
