"""The Gauss-Newton product's ABI, refusals and Python layer, without a GPU: the export list and the naming rules,
what the three C entry points refuse before any launch (a fake non-null pointer is never dereferenced), the
workspace size (flat in T apart from the masks, flat in the number of taps), the tape size (the forward's own), and
every ValueError of the Python calls with the RNG states untouched.
"""
import ctypes
import os
import random
import re
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import GaussNewtonProduct, NeuralCA, NeuralCAGraph, cg_solve, loss_curvature
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a non-null pointer that is never dereferenced: every call below returns before a launch
R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NEW = ("gnca_loss_curvature", "gnca_rollout_gn_fwd_workspace_bytes", "gnca_rollout_gn_fwd", "gnca_rollout_gn_bwd")
DIR_FIELDS = ("w1", "b1", "w2", "gn_weight", "gn_bias", "wm", "bm")
RC, CK = L.SCHED_RECOMPUTE, L.SCHED_CHECKPOINT


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_exports_and_naming_rules(lib):
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(gnca_\w+)\s*\(", src, re.M))
    assert declared == set(L.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW:
        assert n in L.EXPORTS and n in declared and hasattr(lib, n) and not n.endswith("_f32")
        assert re.search(rf"\bT {n}$", out, re.M), n
    decls = dict(re.findall(r"^int (gnca_\w+)\(([^;]*)\);", src, re.M))
    for n in NEW:
        if n in decls:
            assert not re.search(r"\bvoid\s*\*\s*stream\b", decls[n]), n
    assert "void* hip_stream" in decls["gnca_loss_curvature"]
    assert "stream" not in decls["gnca_rollout_gn_fwd"] and "stream" not in decls["gnca_rollout_gn_bwd"]
    assert lib.gnca_rollout_gn_fwd_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.gnca_rollout_gn_fwd.argtypes) == 17 and len(lib.gnca_rollout_gn_bwd.argtypes) == 12
    assert len(lib.gnca_loss_curvature.argtypes) == 14
    assert lib.gnca_abi_version() == L.ABI_VERSION == 5          # additions only
    import graph_neural_cellular_automata_amd as G
    for name in ("GaussNewtonProduct", "cg_solve", "loss_curvature"):
        assert name in G.__all__
    for cls in (NeuralCA, NeuralCAGraph):
        assert callable(cls.rollout_gauss_newton) and callable(cls.gauss_newton_memory)


def test_header_gates_still_pass():
    """The gates of the existing suite that read include/gnca.h, on the header with the new declarations."""
    from tests import test_abi_cpu, test_param_tangent_api_cpu, test_streams_cpu, test_tangent_api_cpu
    lib_ = L.load()
    test_abi_cpu.test_exports_every_declared_symbol(lib_)
    test_param_tangent_api_cpu.test_exports_names_and_abi(lib_)
    test_tangent_api_cpu.test_exports_and_names(lib_)
    test_streams_cpu.test_every_stream_taking_entry_point_is_covered_or_excluded_with_a_reason()
    assert not set(NEW) & set(test_streams_cpu._entry_points())


# ---------------------------------------------------------------------------------------------
# What the C entry points refuse, before any launch
# ---------------------------------------------------------------------------------------------
def _desc(**kw):
    base = dict(B=4, C=16, H=72, W=72, hidden=128, d_model=16, offsets=R4[:8],
                flags=L.GRAPH | L.USE_GROUPNORM | L.ALIVE_TO_ALIVE | L.HIDDEN_ONLY,
                update_gain=0.05, alpha_thr=0.12, message_gain=0.25, fire_rate=0.5, fire_mode=L.FIRE_HASH)
    base.update(kw)
    return S.make_desc(**base)


def _sched(steps, keep, flags=RC, k=8, every=2):
    s = L.RolloutSched()
    s.steps, s.flags, s.ckpt_every = steps, flags, every
    if steps > 0 and k > 0:
        flat = [v for t in range(steps) for o in R4[t % 8:t % 8 + k] for v in o]
        arr = (ctypes.c_int8 * len(flat))(*flat)
        keep.append(arr)
        s.offsets = ctypes.cast(arr, ctypes.c_void_p)
    return s


def _taps(steps, keep, kind=L.TAP_PREMULT, n=None, target=FAKE + 0x900, geometry=(4, 72, 72)):
    t = L.RolloutTaps()
    t.n = len(steps) if n is None else n
    if steps is not None and len(steps):
        arr = (ctypes.c_int32 * len(steps))(*steps)
        keep.append(arr)
        t.steps = ctypes.cast(arr, ctypes.c_void_p)
    t.kind = kind
    t.masked.B, t.masked.H, t.masked.W = geometry
    t.target = target
    return t


def _fwd(lib, d, s, t, dw="zero", x=FAKE, v=FAKE + 0x40, xf=FAKE + 0x100, tape=FAKE + 0x200, tape_n=None,
         fields=FAKE + 0x300, losses=FAKE + 0x400, dl=FAKE + 0x500, quad=FAKE + 0x600, alive=FAKE + 0x700, ws=None, n=0):
    w = L.Weights() if isinstance(dw, str) else dw
    if tape_n is None:
        tape_n = lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(s))
    return lib.gnca_rollout_gn_fwd(ctypes.byref(d), ctypes.byref(L.Weights()), None if w is None else ctypes.byref(w),
                                   ctypes.byref(s), ctypes.byref(t), x, v, xf, tape, tape_n, fields, losses, dl, quad,
                                   alive, ws, n)


def test_forward_refusals(lib):
    keep = []
    d = _desc()
    s, t = _sched(6, keep), _taps([2, 6], keep)
    size = lib.gnca_rollout_gn_fwd_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(t))
    assert size > 0 and _fwd(lib, d, s, t) == WORKSPACE             # everything else is in order: no workspace
    assert _fwd(lib, d, s, t, ws=FAKE + 0x1000, n=size - 1) == WORKSPACE
    for kw in (dict(v=None), dict(dw=None), dict(alive=None)):    # the optional arguments
        assert _fwd(lib, d, s, t, **kw) == WORKSPACE, kw
    assert _fwd(lib, d, s, t, v=None, dw=None) == INVALID
    for kw in (dict(x=None), dict(xf=None), dict(tape=None), dict(fields=None), dict(losses=None), dict(dl=None),
               dict(quad=None)):
        assert _fwd(lib, d, s, t, **kw) == INVALID, kw
    # aliasing: an input that is an output, two outputs at one address, a direction tensor that is an output
    outs = ("xf", "tape", "fields", "losses", "dl", "quad", "alive")
    for o in outs:
        assert _fwd(lib, d, s, t, **{o: FAKE}) == INVALID, o                  # x
        assert _fwd(lib, d, s, t, **{o: FAKE + 0x40}) == INVALID, o           # v
    for i, a in enumerate(outs):
        for b in outs[i + 1:]:
            assert _fwd(lib, d, s, t, **{a: FAKE + 0x800, b: FAKE + 0x800}) == INVALID, (a, b)
    for f in DIR_FIELDS:
        for addr in (FAKE + 0x100, FAKE + 0x200, FAKE + 0x300, FAKE + 0x400, FAKE + 0x500, FAKE + 0x600, FAKE + 0x700):
            w = L.Weights()
            setattr(w, f, addr)
            assert _fwd(lib, d, s, t, dw=w) == INVALID, (f, addr)
    # the tape holds states only: a schedule without RECOMPUTE is refused, with CHECKPOINT beside it accepted
    for fl in (0, CK):
        bad = _sched(6, keep, flags=fl)
        assert _fwd(lib, d, bad, t, tape_n=1 << 40) == INVALID, fl
        assert lib.gnca_rollout_gn_fwd_workspace_bytes(ctypes.byref(d), ctypes.byref(bad), ctypes.byref(t)) == 0
    ck = _sched(6, keep, flags=RC | CK)
    assert lib.gnca_rollout_gn_fwd_workspace_bytes(ctypes.byref(d), ctypes.byref(ck), ctypes.byref(t)) > size
    assert _fwd(lib, d, ck, t) == WORKSPACE
    assert _fwd(lib, d, _sched(6, keep, flags=RC | CK, every=0), t) == INVALID
    # a short tape
    need = lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(s))
    assert need == 6 * d.B * d.C * d.H * d.W * 4
    assert _fwd(lib, d, s, t, tape_n=need - 1, ws=FAKE + 0x1000, n=size) == WORKSPACE
    # what gnca_rollout_fwd_taps refuses about a tap list
    for steps in ([0], [7], [2, 2], [3, 2], [-1]):
        assert _fwd(lib, d, s, _taps(steps, keep)) == INVALID, steps
    assert _fwd(lib, d, s, _taps([], keep, n=0)) == INVALID
    assert _fwd(lib, d, s, _taps(None, keep, n=1)) == INVALID
    assert _fwd(lib, d, s, _taps([2], keep, target=None)) == INVALID
    assert _fwd(lib, d, s, _taps([2], keep, kind=2)) == INVALID
    for geo in ((3, 72, 72), (4, 71, 72), (4, 72, 71)):
        assert _fwd(lib, d, s, _taps([2], keep, geometry=geo)) == INVALID, geo
    masked = _taps([2, 6], keep, kind=L.TAP_MASKED)
    assert _fwd(lib, d, s, masked) == WORKSPACE and _fwd(lib, d, s, masked, alive=None) == INVALID
    # the zero-padded shift stays refused: unsupported, workspace size 0
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _fwd(lib, zp, s, t) == UNSUPPORTED
    assert lib.gnca_rollout_gn_fwd_workspace_bytes(ctypes.byref(zp), ctypes.byref(s), ctypes.byref(t)) == 0
    assert _fwd(lib, _desc(C=40), _sched(6, keep), t, tape_n=1 << 40) == UNSUPPORTED      # outside the support set


def test_tape_size_is_the_forwards_own(lib):
    """A fire mode without sched->fire is refused AFTER the tape and workspace checks: with it, INVALID says that
    the sizes passed, WORKSPACE that one did not."""
    keep = []
    d = _desc(fire_mode=L.FIRE_MASK_U8)
    t = _taps([2, 7], keep)
    for fl, every in ((RC, 2), (RC | CK, 3), (RC | CK, 1), (RC | CK, 7), (RC | CK, 50)):
        s = _sched(7, keep, flags=fl, every=every)
        need = lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(s))
        size = lib.gnca_rollout_gn_fwd_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(t))
        assert need > 0 and size > 0
        assert _fwd(lib, d, s, t, tape_n=need, ws=FAKE + 0x1000, n=size) == INVALID, (fl, every)
        assert _fwd(lib, d, s, t, tape_n=need - 1, ws=FAKE + 0x1000, n=size) == WORKSPACE, (fl, every)
        # the backward reads that tape with its own, unchanged workspace
        bsize = lib.gnca_rollout_bwd_workspace_bytes(ctypes.byref(d), ctypes.byref(s))
        assert _bwd(lib, d, s, t, tape_n=need, ws=FAKE + 0x1000, n=bsize) == INVALID, (fl, every)
        assert _bwd(lib, d, s, t, tape_n=need - 1, ws=FAKE + 0x1000, n=bsize) == WORKSPACE, (fl, every)
        assert _bwd(lib, d, s, t, tape_n=need, ws=FAKE + 0x1000, n=bsize - 1) == WORKSPACE, (fl, every)


def test_workspace_is_flat_in_T_and_in_the_taps(lib):
    keep = []
    d = _desc()
    size = lambda T, taps, fl=RC, every=2: lib.gnca_rollout_gn_fwd_workspace_bytes(   # noqa: E731
        ctypes.byref(d), ctypes.byref(_sched(T, keep, flags=fl, every=every)), ctypes.byref(_taps(taps, keep)))
    align = lambda n: (n + 255) // 256 * 256                                          # noqa: E731
    a, b = size(8, [8]), size(4096, [4096])
    assert a > 0 and b - a == align(4096 * d.B) - align(8 * d.B)                      # the [T][B] masks alone
    assert size(4096, list(range(1, 4097))) == b and size(8, [1, 2, 3, 4, 5, 6, 7, 8]) == a
    n = d.B * d.C * d.H * d.W * 4
    assert size(8, [8], RC | CK) - a == 2 * n                                         # the two ping-pong states
    assert size(8, [8], RC | CK, 2) == size(8, [8], RC | CK, 5)
    obj = lib.gnca_rollout_objective_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(8, keep, flags=0)),
                                                             ctypes.byref(_taps([8], keep)), 1)
    assert a == obj - 2 * n                                                           # the states go to the tape


def _bwd(lib, d, s, t, tape=FAKE + 0x200, tape_n=None, fields=FAKE + 0x300, scale="ones", gx=FAKE + 0x800, ws=None,
         n=0):
    if tape_n is None:
        tape_n = lib.gnca_rollout_tape_bytes(ctypes.byref(d), ctypes.byref(s))
    sc = (ctypes.c_float * max(1, t.n))(*([1.0] * max(1, t.n))) if isinstance(scale, str) else scale
    return lib.gnca_rollout_gn_bwd(ctypes.byref(d), ctypes.byref(L.Weights()), ctypes.byref(s), ctypes.byref(t), tape,
                                   tape_n, fields, sc, gx, ctypes.byref(L.Grads()), ws, n)


def test_backward_refusals(lib):
    keep = []
    d = _desc()
    s, t = _sched(6, keep), _taps([2, 6], keep)
    assert _bwd(lib, d, s, t) == WORKSPACE
    for kw in (dict(fields=None), dict(scale=None), dict(gx=None), dict(tape=None), dict(gx=FAKE + 0x300)):
        assert _bwd(lib, d, s, t, **kw) == INVALID, kw
    for fl in (0, CK):
        assert _bwd(lib, d, _sched(6, keep, flags=fl), t, tape_n=1 << 40) == INVALID, fl
    for steps in ([0], [7], [2, 2]):
        assert _bwd(lib, d, s, _taps(steps, keep)) == INVALID, steps
    assert _bwd(lib, d, s, _taps([2], keep, target=None)) == INVALID


def _curv(lib, kind=L.TAP_PREMULT, d="ok", pred=FAKE, pbs=4, v=FAKE + 0x100, vbs=4, target=FAKE + 0x200, tbs=0,
          losses=FAKE + 0x300, dl=FAKE + 0x400, quad=FAKE + 0x500, field=FAKE + 0x600, fbs=4):
    if isinstance(d, str):
        d = L.MaskedLossDesc()
        d.B, d.H, d.W = 2, 8, 8
    return lib.gnca_loss_curvature(kind, None if d is None else ctypes.byref(d), pred, pbs, v, vbs, target, tbs, losses,
                                   dl, quad, field, fbs, None)


def test_loss_curvature_refusals(lib):
    for kw in (dict(kind=2), dict(kind=-1), dict(d=None), dict(pred=None), dict(v=None), dict(target=None),
               dict(quad=None), dict(field=None), dict(pbs=-1), dict(vbs=-1), dict(tbs=-1), dict(fbs=-1)):
        assert _curv(lib, **kw) == INVALID, kw
    for geo in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        d = L.MaskedLossDesc()
        d.B, d.H, d.W = geo
        assert _curv(lib, d=d) == INVALID, geo


# ---------------------------------------------------------------------------------------------
# The Python layer
# ---------------------------------------------------------------------------------------------
def _graph_model(zero_pad=False):
    torch.manual_seed(0)
    return NeuralCAGraph(8, 16, graph_attention_radius=2, graph_num_neighbors=4, graph_zero_padded_shift=zero_pad).eval()


def _states():
    return random.getstate(), torch.get_rng_state()


def test_every_bad_argument_is_a_value_error_and_draws_nothing():
    m = _graph_model()
    x, tgt = torch.rand(2, 8, 6, 6), torch.rand(4, 6, 6)
    v = torch.randn(2, 8, 6, 6)
    dp = m.param_direction(1.0)
    good = dict(v=v, dparams=dp)
    classic = NeuralCA(8, 16).eval()
    bad = [
        dict(kw=dict()),                                                  # neither v nor dparams
        dict(kw=dict(v=v[0])), dict(kw=dict(v=torch.randn(2, 8, 6, 5))), dict(kw=dict(v=v.double())),
        dict(kw=dict(v="no")), dict(kw=dict(v=v.unsqueeze(0))),
        dict(kw=dict(dparams=[dp])), dict(kw=dict(dparams="no")),         # one direction per call: a dict
        dict(kw=dict(dparams={"nope": torch.zeros(1)})),
        dict(kw=dict(dparams={"update_net.0.bias": torch.zeros(3)})),
        dict(kw=dict(dparams={"perception.conv.weight": torch.zeros(1)})),
        dict(kw=dict(good, loss="l2")), dict(kw=dict(good, loss="masked", alpha_thr=float("nan"))),
        dict(kw=dict(good, loss="masked", lam_area="x")),
        dict(kw=good, steps=0), dict(kw=good, steps=True), dict(kw=good, steps=2.0),
        dict(kw=dict(good, every=0)), dict(kw=dict(good, record=[0])), dict(kw=dict(good, record=[5])),
        dict(kw=dict(good, record=[2, 2])), dict(kw=dict(good, record=[])),
        dict(kw=dict(good, tap_weights=[1.0])), dict(kw=dict(good, tap_weights=torch.ones(4))),
        dict(kw=dict(good, tap_weights=[1.0, "x", 1.0, 1.0])), dict(kw=dict(good, tap_weights=2.0)),
        dict(kw=dict(good, checkpoint_every=0)), dict(kw=dict(good, checkpoint_every="no")),
        dict(kw=good, target=torch.rand(4, 6, 5)), dict(kw=good, target=torch.rand(3, 4, 6, 6)), dict(kw=good, target="t"),
        dict(kw=good, x=torch.rand(2, 7, 6, 6)), dict(kw=good, x=torch.rand(8, 6, 6)), dict(kw=good, x=None),
    ]
    before = _states()
    for case in bad:
        with pytest.raises(ValueError):
            m.rollout_gauss_newton(case.get("x", x), case.get("steps", 4), case.get("target", tgt), **case["kw"])
        after = _states()
        assert after[0] == before[0] and torch.equal(after[1], before[1]), case
    with pytest.raises(ValueError):
        classic.rollout_gauss_newton(x, 4, tgt)
    with pytest.raises(TypeError):
        classic.rollout_gauss_newton(x, 4, tgt, v=v, offsets=[])           # no graph keywords on the classic model
    after = _states()
    assert after[0] == before[0] and torch.equal(after[1], before[1])


def test_the_zero_padded_model_is_refused_with_the_existing_message():
    m = _graph_model(zero_pad=True)
    x, tgt = torch.rand(2, 8, 6, 6), torch.rand(4, 6, 6)
    before = _states()
    with pytest.raises(ValueError) as e:
        m.rollout_gauss_newton(x, 4, tgt, dparams=m.param_direction(1.0))
    assert str(e.value) == S.ZERO_PAD_TANGENT
    with pytest.raises(ValueError) as e:
        m.gauss_newton_memory((2, 8, 6, 6), 4)
    assert str(e.value) == S.ZERO_PAD_TANGENT
    after = _states()
    assert after[0] == before[0] and torch.equal(after[1], before[1])


def test_memory_is_a_host_only_query(lib):
    m = _graph_model()
    before = _states()
    plain = m.gauss_newton_memory((3, 8, 24, 24), 12, every=4, fire_rate=0.5)
    ck = m.gauss_newton_memory(torch.empty(3, 8, 24, 24), 12, every=4, fire_rate=0.5, checkpoint_every=4)
    after = _states()
    assert after[0] == before[0] and torch.equal(after[1], before[1])
    n = 3 * 8 * 24 * 24 * 4
    assert plain["tape"] == 12 * n and ck["tape"] == 3 * n                   # n is a multiple of 256 here
    assert plain["fields"] == ck["fields"] == 3 * 3 * 4 * 24 * 24 * 4
    assert ck["forward_workspace"] - plain["forward_workspace"] == 2 * n
    assert plain["tape"] == m.rollout_memory((3, 8, 24, 24), 12, fire_rate=0.5, recompute=True)["tape"]
    assert plain["backward_workspace"] == m.rollout_memory((3, 8, 24, 24), 12, fire_rate=0.5,
                                                           recompute=True)["backward_workspace"]
    for kw in (dict(steps=0), dict(every=0), dict(record=[13])):
        a = dict(steps=12)
        a.update(kw)
        with pytest.raises(ValueError):
            m.gauss_newton_memory((3, 8, 24, 24), a.pop("steps"), **a)
    with pytest.raises(ValueError):
        m.gauss_newton_memory((3, 7, 24, 24), 12)


def test_result_type_and_flat_order():
    m = _graph_model()
    prod = {n: torch.full_like(p, float(i)) for i, (n, p) in enumerate(m.named_parameters()) if n in S.DIRECTION_FIELDS}
    r = GaussNewtonProduct(1, 2, 3, 4, [2, 4], prod, 5, 6)
    assert (r.x_final, r.losses, r.dlosses, r.quad, r.steps, r.gx, r.energy) == (1, 2, 3, 4, [2, 4], 5, 6)
    assert "steps=[2, 4]" in repr(r)
    from graph_neural_cellular_automata_amd import ParamDirections
    d = ParamDirections(m, 1)
    flat = r.product_flat()
    assert tuple(flat.shape) == (d.P,)
    for n, p, o in zip(d.names, d.params, d.offsets):
        assert torch.equal(flat[o:o + p.numel()], prod[n].reshape(-1)), n


def test_python_value_errors_of_the_loss_and_the_solver():
    pred, tgt, v = torch.rand(2, 4, 6, 6), torch.rand(4, 6, 6), torch.randn(2, 4, 6, 6)
    for kw in (dict(loss="l2"), dict(v=v[0]), dict(v=v[:1]), dict(v=v.double()), dict(pred=pred[:, :3]),
               dict(target=torch.rand(4, 6, 5)), dict(loss="masked", lam_bg_rgb=float("inf"))):
        a = dict(pred=pred, v=v, target=tgt, loss="premult")
        a.update(kw)
        with pytest.raises(ValueError):
            loss_curvature(a.pop("pred"), a.pop("v"), a.pop("target"), **a)
    with pytest.raises(RuntimeError):
        loss_curvature(pred, v, tgt)                                         # no CPU path
    b = torch.ones(3)
    for args, kw in (((lambda p: p, b.reshape(1, 3), 2), {}), ((lambda p: p, b, 0), {}), ((lambda p: p, b, True), {}),
                     ((lambda p: p, b, 2), dict(damping=-1.0)), ((lambda p: p, b, 2), dict(damping="x")),
                     (("f", b, 2), {}), ((lambda p: p[:2], b, 2), {}), ((lambda p: p, torch.ones(3, dtype=torch.int32), 2), {})):
        with pytest.raises(ValueError):
            cg_solve(*args, **kw)
