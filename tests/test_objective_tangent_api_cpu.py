"""The forward-mode objective's ABI, refusals and Python layer, without a GPU: the descriptor of gnca_forward_grad
against its ctypes mirror, the export list and the naming rules, what the three C entry points refuse before any
launch (a fake non-null pointer is never dereferenced), the workspace size (flat in T apart from the masks, flat in
the number of taps), every ValueError of the Python calls with the RNG states untouched, and the layout of
ParamDirections.
"""
import ctypes
import os
import random
import re
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph, ObjectiveTangent, ParamDirections
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import forward_gradient_, loss_tangent
from graph_neural_cellular_automata_amd import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a non-null pointer that is never dereferenced: every call below returns before a launch
R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NEW = ("gnca_loss_tangent", "gnca_rollout_objective_tangent_workspace_bytes", "gnca_rollout_objective_tangent",
       "gnca_forward_grad")
DIR_FIELDS = ("w1", "b1", "w2", "gn_weight", "gn_bias", "wm", "bm")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_forward_grad_desc_matches_the_header(tmp_path):
    structs = [("gnca_forward_grad_tensor", L.ForwardGradTensor), ("gnca_forward_grad_desc", L.ForwardGradDesc)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){']
    for cname, mirror in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("acc %u\\n", GNCA_FGRAD_ACCUMULATE);')
    lines.append('printf("dirs %d\\n", GNCA_LOSS_TANGENT_DIRS);')
    lines.append('printf("abi %d\\n", GNCA_ABI_VERSION);')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for cname, mirror in structs:
        assert int(got[cname][0]) == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert int(got[f"{cname}.{f}"][0]) == getattr(mirror, f).offset, (cname, f)
    assert ctypes.sizeof(L.ForwardGradDesc) < 4096          # the descriptor travels as a kernel argument
    assert int(got["acc"][0]) == L.FGRAD_ACCUMULATE and int(got["dirs"][0]) == L.LOSS_TANGENT_DIRS
    assert int(got["abi"][0]) == L.ABI_VERSION == 5          # additions only


def test_exports_and_naming_rules(lib):
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(gnca_\w+)\s*\(", src, re.M))
    assert declared == set(L.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW:
        assert n in L.EXPORTS and n in declared and hasattr(lib, n) and not n.endswith("_f32")
        assert re.search(rf"\bT {n}$", out, re.M), n
        assert not re.fullmatch(r"gnca_\w*tangent\w*_params", n)
    decls = dict(re.findall(r"^int (gnca_\w+)\(([^;]*)\);", src, re.M))
    for n in NEW:
        if n in decls:
            assert not re.search(r"\bvoid\s*\*\s*stream\b", decls[n]), n
    assert "void* hip_stream" in decls["gnca_loss_tangent"] and "void* hip_stream" in decls["gnca_forward_grad"]
    assert "stream" not in decls["gnca_rollout_objective_tangent"]       # it travels in gnca_rollout_taps
    assert lib.gnca_rollout_objective_tangent_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.gnca_rollout_objective_tangent.argtypes) == 15 and len(lib.gnca_loss_tangent.argtypes) == 13


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


def _sched(steps, keep, flags=0, k=8):
    s = L.RolloutSched()
    s.steps, s.flags, s.ckpt_every = steps, flags, 2
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


def _obj(lib, d, s, t, K=3, dw="zero", x=FAKE, v=FAKE + 0x40, xf=FAKE + 0x100, vf=FAKE + 0x200, losses=FAKE + 0x300,
         dl=FAKE + 0x400, alive=FAKE + 0x500, ws=None, n=0):
    arr = (L.Weights * max(1, min(K, L.TANGENT_MAX_DIRS)))() if isinstance(dw, str) else dw
    return lib.gnca_rollout_objective_tangent(ctypes.byref(d), ctypes.byref(L.Weights()), arr, ctypes.byref(s),
                                              ctypes.byref(t), K, x, v, xf, vf, losses, dl, alive, ws, n)


def test_rollout_refusals(lib):
    keep = []
    d = _desc()
    s, t = _sched(6, keep), _taps([2, 6], keep)
    size = lib.gnca_rollout_objective_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(t), 3)
    assert size > 0 and _obj(lib, d, s, t) == WORKSPACE           # everything else is in order: no workspace
    assert _obj(lib, d, s, t, ws=FAKE + 0x1000, n=size - 1) == WORKSPACE
    # the optional arguments: no v with a direction, no direction with a v, no v_final, no alive_count (premult)
    for kw in (dict(v=None), dict(dw=None), dict(vf=None), dict(alive=None)):
        assert _obj(lib, d, s, t, **kw) == WORKSPACE, kw
    assert _obj(lib, d, s, t, v=None, dw=None) == INVALID
    for kw in (dict(x=None), dict(xf=None), dict(losses=None), dict(dl=None)):
        assert _obj(lib, d, s, t, **kw) == INVALID, kw
    for K in (0, -1, 17):
        assert _obj(lib, d, s, t, K=K) == INVALID, K
        assert lib.gnca_rollout_objective_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(t),
                                                                  K) == 0
    # aliasing: an input that is an output, two outputs at one address, a direction tensor that is an output
    outs = ("xf", "vf", "losses", "dl", "alive")
    for o in outs:
        assert _obj(lib, d, s, t, **{o: FAKE}) == INVALID, o                  # x
        assert _obj(lib, d, s, t, **{o: FAKE + 0x40}) == INVALID, o           # v
    for i, a in enumerate(outs):
        for b in outs[i + 1:]:
            assert _obj(lib, d, s, t, **{a: FAKE + 0x700, b: FAKE + 0x700}) == INVALID, (a, b)
    for j in range(3):
        for f in DIR_FIELDS:
            for addr in (FAKE + 0x100, FAKE + 0x200, FAKE + 0x300, FAKE + 0x400):
                arr = (L.Weights * 3)()
                setattr(arr[j], f, addr)
                assert _obj(lib, d, s, t, dw=arr) == INVALID, (j, f, addr)
    for fl in (L.SCHED_RECOMPUTE, L.SCHED_CHECKPOINT, L.SCHED_RECOMPUTE | L.SCHED_CHECKPOINT):   # there is no tape
        assert _obj(lib, d, _sched(6, keep, flags=fl), t) == INVALID, fl
        assert lib.gnca_rollout_objective_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(6, keep, flags=fl)),
                                                                  ctypes.byref(t), 3) == 0
    # what gnca_rollout_fwd_taps refuses about a tap list
    for steps in ([0], [7], [2, 2], [3, 2], [-1]):
        assert _obj(lib, d, s, _taps(steps, keep)) == INVALID, steps
    assert _obj(lib, d, s, _taps([], keep, n=0)) == INVALID
    assert _obj(lib, d, s, _taps([2], keep, n=-1)) == INVALID
    assert _obj(lib, d, s, _taps(None, keep, n=1)) == INVALID                 # a null step list
    assert _obj(lib, d, s, _taps([2], keep, target=None)) == INVALID
    assert _obj(lib, d, s, _taps([2], keep, kind=2)) == INVALID
    for geo in ((3, 72, 72), (4, 71, 72), (4, 72, 71)):
        assert _obj(lib, d, s, _taps([2], keep, geometry=geo)) == INVALID, geo
    masked = _taps([2, 6], keep, kind=L.TAP_MASKED)
    assert _obj(lib, d, s, masked) == WORKSPACE and _obj(lib, d, s, masked, alive=None) == INVALID
    # the zero-padded shift stays refused: unsupported, workspace size 0
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _obj(lib, zp, s, t) == UNSUPPORTED
    assert lib.gnca_rollout_objective_tangent_workspace_bytes(ctypes.byref(zp), ctypes.byref(s), ctypes.byref(t), 3) == 0
    assert _obj(lib, _desc(C=40), _sched(6, keep), t) == UNSUPPORTED            # outside the support set
    mask_fire = _desc(fire_mode=L.FIRE_MASK_U8)
    assert _obj(lib, mask_fire, s, t, ws=FAKE + 0x1000, n=size) == INVALID      # a fire mode without sched->fire


def test_workspace_is_flat_in_T_and_in_the_taps(lib):
    keep = []
    d = _desc()
    size = lambda T, taps, K=8: lib.gnca_rollout_objective_tangent_workspace_bytes(   # noqa: E731
        ctypes.byref(d), ctypes.byref(_sched(T, keep)), ctypes.byref(_taps(taps, keep)), K)
    align = lambda n: (n + 255) // 256 * 256                                          # noqa: E731
    a, b = size(8, [8]), size(4096, [4096])
    assert a > 0 and b - a == align(4096 * d.B) - align(8 * d.B)                      # the [T][B] masks alone
    assert size(4096, list(range(1, 4097))) == b and size(8, [1, 2, 3, 4, 5, 6, 7, 8]) == a
    n = d.B * d.C * d.H * d.W * 4
    assert size(8, [8], 16) - size(8, [8], 8) == 2 * 8 * n                            # linear in K: two blocks
    blk = L.TangentBlockArgs()
    blk.num_dirs = 8
    assert a < lib.gnca_rollout_tangent_block_workspace_bytes(ctypes.byref(d), ctypes.byref(_sched(8, keep)),
                                                              ctypes.byref(blk))      # no QR area, no norm partials


def _loss(lib, kind=L.TAP_PREMULT, d="ok", K=3, pred=FAKE, pbs=4, v=FAKE + 0x100, vds=16, vbs=4, target=FAKE + 0x200,
          tbs=0, losses=FAKE + 0x300, dl=FAKE + 0x400):
    if isinstance(d, str):
        d = L.MaskedLossDesc()
        d.B, d.H, d.W = 2, 8, 8
    return lib.gnca_loss_tangent(kind, None if d is None else ctypes.byref(d), K, pred, pbs, v, vds, vbs, target, tbs,
                                 losses, dl, None)


def test_loss_tangent_refusals(lib):
    for kw in (dict(kind=2), dict(kind=-1), dict(d=None), dict(K=0), dict(K=-3), dict(pred=None), dict(v=None),
               dict(target=None), dict(dl=None), dict(pbs=-1), dict(vds=-1), dict(vbs=-1), dict(tbs=-1)):
        assert _loss(lib, **kw) == INVALID, kw
    for geo in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        d = L.MaskedLossDesc()
        d.B, d.H, d.W = geo
        assert _loss(lib, d=d) == INVALID, geo


def _fg(**kw):
    d = L.ForwardGradDesc()
    d.K, d.R, d.B = 3, 2, 4
    d.dlosses, d.coef, d.scale = FAKE, FAKE + 0x100, 1.0
    d.num_tensors = 1
    d.t[0].g, d.t[0].dir, d.t[0].dir_stride, d.t[0].numel = FAKE + 0x200, FAKE + 0x300, 10, 10
    for k, v in kw.items():
        if k.startswith("t_"):
            setattr(d.t[0], k[2:], v)
        else:
            setattr(d, k, v)
    return d


def test_forward_grad_refusals(lib):
    assert lib.gnca_forward_grad(None, None) == INVALID
    for kw in (dict(K=0), dict(R=0), dict(B=0), dict(dlosses=None), dict(coef=None), dict(num_tensors=-1),
               dict(num_tensors=L.OPTIM_MAX_TENSORS + 1), dict(flags=2), dict(dlosses=FAKE + 4), dict(coef=FAKE + 4),
               dict(t_g=None), dict(t_dir=None), dict(t_numel=-1), dict(t_dir_stride=-1)):
        assert lib.gnca_forward_grad(ctypes.byref(_fg(**kw)), None) == INVALID, kw


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
    V = torch.randn(3, 2, 8, 6, 6)
    dp = m.param_direction(1.0)
    good = dict(V=V, dparams=[dp, dp, dp])
    classic = NeuralCA(8, 16).eval()
    bad = [
        dict(kw=dict()),                                                  # neither V nor dparams
        dict(kw=dict(V=V[0])), dict(kw=dict(V=torch.randn(17, 2, 8, 6, 6))), dict(kw=dict(V=torch.randn(3, 2, 8, 6, 5))),
        dict(kw=dict(V=V.double())), dict(kw=dict(V="no")),
        dict(kw=dict(dparams=[])), dict(kw=dict(dparams=[dp] * 17)), dict(kw=dict(dparams="no")),
        dict(kw=dict(V=V, dparams=[dp, dp])),                             # K mismatch
        dict(kw=dict(dparams=[{"nope": torch.zeros(1)}])),
        dict(kw=dict(dparams=[{"update_net.0.bias": torch.zeros(3)}])),
        dict(kw=dict(dparams=[{"perception.conv.weight": torch.zeros(1)}])),
        dict(kw=dict(good, loss="l2")), dict(kw=dict(good, loss="masked", alpha_thr=float("nan"))),
        dict(kw=dict(good, loss="masked", lam_area="x")),
        dict(kw=good, steps=0), dict(kw=good, steps=True), dict(kw=good, steps=2.0),
        dict(kw=dict(good, every=0)), dict(kw=dict(good, record=[0])), dict(kw=dict(good, record=[5])),
        dict(kw=dict(good, record=[2, 2])), dict(kw=dict(good, record=[])),
        dict(kw=dict(good, return_tangents=1)),
        dict(kw=good, target=torch.rand(4, 6, 5)), dict(kw=good, target=torch.rand(3, 4, 6, 6)), dict(kw=good, target="t"),
        dict(kw=good, x=torch.rand(2, 7, 6, 6)), dict(kw=good, x=torch.rand(8, 6, 6)), dict(kw=good, x=None),
    ]
    before = _states()
    for case in bad:
        with pytest.raises(ValueError):
            m.rollout_objective_tangent(case.get("x", x), case.get("steps", 4), case.get("target", tgt), **case["kw"])
        after = _states()
        assert after[0] == before[0] and torch.equal(after[1], before[1]), case
    with pytest.raises(ValueError):
        classic.rollout_objective_tangent(x, 4, tgt)
    with pytest.raises(TypeError):
        classic.rollout_objective_tangent(x, 4, tgt, V=V, offsets=[])      # no graph keywords on the classic model
    after = _states()
    assert after[0] == before[0] and torch.equal(after[1], before[1])


def test_the_zero_padded_model_is_refused_with_the_existing_message():
    m = _graph_model(zero_pad=True)
    x, tgt = torch.rand(2, 8, 6, 6), torch.rand(4, 6, 6)
    before = _states()
    with pytest.raises(ValueError) as e:
        m.rollout_objective_tangent(x, 4, tgt, dparams=m.param_direction(1.0))
    assert str(e.value) == S.ZERO_PAD_TANGENT
    after = _states()
    assert after[0] == before[0] and torch.equal(after[1], before[1])


def test_result_type():
    r = ObjectiveTangent(1, 2, torch.zeros(2, 3, 4, dtype=torch.float64), [2, 4])
    assert (r.x_final, r.losses, r.steps, r.v_final) == (1, 2, [2, 4], None) and "dlosses=(2, 3, 4)" in repr(r)


def test_param_directions_layout():
    for m in (_graph_model(), NeuralCA(8, 16).eval(), NeuralCA(8, 16, use_groupnorm=False).eval()):
        params = dict(m.named_parameters())
        d = ParamDirections(m, 3, seed=5)
        assert d.names == [n for n in S.DIRECTION_FIELDS if n in params]
        assert set(d.names) == set(S.DIRECTION_FIELDS) & set(params)
        assert d.P == sum(params[n].numel() for n in d.names) and tuple(d.flat.shape) == (3, d.P)
        assert d.flat.dtype == torch.float32 and d.flat.is_contiguous() and not d.flat.any()
        dicts = d.dicts()
        assert len(dicts) == 3
        o = 0
        for n in d.names:
            for k in range(3):
                v = dicts[k][n]
                assert tuple(v.shape) == tuple(params[n].shape) and v.is_contiguous()
                assert v.data_ptr() == d.flat.data_ptr() + 4 * (k * d.P + o)        # a view of the buffer
            o += params[n].numel()
        d.fill_(2.0)
        assert all(bool((t == 2.0).all()) for dd in dicts for t in dd.values())
        d.normal_()
        a = d.flat.clone()
        assert ParamDirections(m, 3, seed=5).normal_().flat.equal(a) and a.std() > 0.5
        assert set(dicts[0]) == set(d.names)
        from graph_neural_cellular_automata_amd.modules import _stepper as M
        assert set(M._check_dparams(m, dicts[0])) == {S.DIRECTION_FIELDS[n] for n in d.names}   # accepted as dparams
    for K in (0, 17, True, 2.0):
        with pytest.raises(ValueError):
            ParamDirections(_graph_model(), K)


def test_loss_tangent_and_forward_gradient_value_errors():
    pred, tgt, V = torch.rand(2, 4, 6, 6), torch.rand(4, 6, 6), torch.randn(3, 2, 4, 6, 6)
    for kw in (dict(loss="l2"), dict(V=V[0]), dict(V=V[:, :1]), dict(V=V.double()), dict(pred=pred[:, :3]),
               dict(target=torch.rand(4, 6, 5)), dict(loss="masked", lam_bg_rgb=float("inf"))):
        a = dict(pred=pred, V=V, target=tgt, loss="premult")
        a.update(kw)
        with pytest.raises(ValueError):
            loss_tangent(a.pop("pred"), a.pop("V"), a.pop("target"), **a)
    m = _graph_model()
    d = ParamDirections(m, 3)
    dl = torch.zeros(2, 3, 4, dtype=torch.float64)
    for args, kw in (((m, dl.float(), d), {}), ((m, dl[:, :2], d), {}), ((m, dl, "d"), {}), ((m, dl[0, 0], d), {}),
                     ((_graph_model(), dl, d), {}), ((m, dl, d), dict(accumulate=1)),
                     ((m, dl, d), dict(tap_weights=[1.0])), ((m, dl, d), dict(scale="x"))):
        with pytest.raises(ValueError):
            forward_gradient_(*args, **kw)
    assert all(p.grad is None for p in m.parameters())
