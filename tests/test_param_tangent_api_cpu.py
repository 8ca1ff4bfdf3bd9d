"""The weight-direction tangent's ABI, refusals and Python layer, without a GPU: the export list and the naming
rules, what the three ``_params`` entry points refuse before any launch (a fake non-null pointer is never
dereferenced), the workspace sizes (the twins'), and every ValueError of ``dparams=``, which fires before
anything is drawn from Python's ``random`` or torch's generator.
"""
import ctypes
import inspect
import os
import random
import re

import pytest
import torch

from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import shape_class_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a non-null pointer that is never dereferenced: every call below returns before a launch
R4 = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if max(abs(dy), abs(dx)) > 1]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NEW = ("gnca_step_tangent_params", "gnca_rollout_tangent_params", "gnca_rollout_tangent_block_params")
DIR_FIELDS = ("w1", "b1", "w2", "gn_weight", "gn_bias", "wm", "bm")


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


def _bargs(K, record, keep, flags=0, log_r=FAKE):
    a = L.TangentBlockArgs()
    a.num_dirs, a.num_records = K, len(record)
    if record:
        arr = (ctypes.c_int32 * len(record))(*record)
        keep.append(arr)
        a.record = ctypes.cast(arr, ctypes.c_void_p)
    a.flags = flags
    a.log_r = log_r
    return a


def _dw(**fields):
    w = L.Weights()
    for k, v in fields.items():
        setattr(w, k, v)
    return w


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_exports_names_and_abi(lib):
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(gnca_\w+)\s*\(", src, re.M))
    assert declared == set(L.EXPORTS)
    for n in NEW:
        assert n in L.EXPORTS and n in declared and hasattr(lib, n) and not n.endswith("_f32")
        assert getattr(lib, n).argtypes is not None and getattr(lib, n).restype is ctypes.c_int
    assert L.ABI_VERSION == 5 == lib.gnca_abi_version()                      # additions only
    assert int(re.search(r"#define\s+GNCA_ABI_VERSION\s+(\d+)", src).group(1)) == 5
    decl = {n: re.sub(r"/\*.*?\*/", "", p) for n, p in re.findall(r"^int (gnca_\w*tangent\w*_params)\(([^;]*)\);", src, re.M | re.S)}
    assert set(decl) == set(NEW)
    for n, params in decl.items():
        assert not re.search(r"\bvoid\s*\*\s*stream\b", params), n            # hip_stream, or in the args struct
        assert re.search(r"const gnca_weights\*\s*w,\s*const gnca_weights\*\s*dw\b", params), n
    # the stream follows each twin: the step names it, the rollouts carry it in their args
    assert "void* hip_stream" in decl["gnca_step_tangent_params"]
    assert "hip_stream" not in decl["gnca_rollout_tangent_params"] + decl["gnca_rollout_tangent_block_params"]
    assert not any(n.endswith("_params_workspace_bytes") for n in declared)  # the twins' size functions serve
    # argument counts: the twin's plus the direction
    assert len(lib.gnca_step_tangent_params.argtypes) == len(lib.gnca_step_tangent.argtypes) + 1
    assert len(lib.gnca_rollout_tangent_params.argtypes) == len(lib.gnca_rollout_tangent.argtypes) + 1
    assert len(lib.gnca_rollout_tangent_block_params.argtypes) == len(lib.gnca_rollout_tangent_block.argtypes) + 1


# ---------------------------------------------------------------------------------------------
# What the C entry points refuse, before any launch
# ---------------------------------------------------------------------------------------------
def _step(lib, d, dw="zero", x=FAKE, v=FAKE, xo=FAKE + 0x100, vo=FAKE + 0x200, ws=None, n=0):
    dw = L.Weights() if isinstance(dw, str) else dw
    return lib.gnca_step_tangent_params(ctypes.byref(d), ctypes.byref(L.Weights()),
                                        None if dw is None else ctypes.byref(dw), x, None, None, v, xo, vo, ws, n,
                                        None)


def test_step_refusals(lib):
    d = _desc()
    assert _step(lib, d) == WORKSPACE                       # everything else is in order: no workspace
    assert _step(lib, d, dw=_dw(**{f: FAKE + 0x300 + 8 * i for i, f in enumerate(DIR_FIELDS)})) == WORKSPACE
    assert _step(lib, d, dw=None) == INVALID                # a null direction
    for kw in (dict(x=None), dict(v=None), dict(xo=None), dict(vo=None)):
        assert _step(lib, d, **kw) == INVALID, kw
    for kw in (dict(xo=FAKE), dict(vo=FAKE), dict(v=FAKE + 0x40, xo=FAKE + 0x40), dict(v=FAKE + 0x40, vo=FAKE + 0x40),
               dict(xo=FAKE + 0x80, vo=FAKE + 0x80)):
        assert _step(lib, d, **kw) == INVALID, kw
    for f in DIR_FIELDS:                                     # a direction tensor that is one of the outputs
        assert _step(lib, d, dw=_dw(**{f: FAKE + 0x100})) == INVALID, f
        assert _step(lib, d, dw=_dw(**{f: FAKE + 0x200})) == INVALID, f
    # the fields that are not read may hold anything, an output's address included
    assert _step(lib, d, dw=_dw(perception=FAKE + 0x100, wq=FAKE + 0x200, bq=FAKE + 0x100, wk=FAKE + 0x100,
                                bk=FAKE + 0x100, scaling=FAKE + 0x200)) == WORKSPACE
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _step(lib, zp) == UNSUPPORTED
    for ok in (_desc(flags=(d.flags | L.ZERO_PAD_SHIFT) & ~L.GRAPH, offsets=[]), _desc(flags=d.flags | L.ZERO_PAD_SHIFT, offsets=[])):
        assert _step(lib, ok) == WORKSPACE
    assert _step(lib, _desc(alpha_thr=-0.1)) == WORKSPACE


@pytest.mark.parametrize("C,hidden", SC.UNSUPPORTED)
def test_unsupported_shapes(lib, C, hidden):
    d = SC.bare_desc(C, hidden)
    assert _step(lib, d) == UNSUPPORTED
    keep = []
    s = _sched(2, keep, k=2)
    assert _roll(lib, d, s, _args([], keep)) == UNSUPPORTED
    assert _block(lib, d, s, _bargs(2, [], keep)) == UNSUPPORTED


def test_every_supported_class_is_served(lib):
    """No class of the support set is refused for LDS reasons: the hidden > 128 classes and p31 reach the
    workspace check like every other torus class, with the twin's workspace size."""
    seen = set()
    for name in SC.IDS:
        d = SC.desc(name)
        n = lib.gnca_step_tangent_workspace_bytes(ctypes.byref(d))
        if SC.CASES[name]["zp"] and SC.CASES[name]["graph"]:
            assert n == 0 and _step(lib, d) == UNSUPPORTED, name
            continue
        assert n > 0 and _step(lib, d) == WORKSPACE, name
        assert _step(lib, d, ws=FAKE, n=n - 1) == WORKSPACE, name          # one byte short of the twin's size
        seen.add((SC.CASES[name]["C"], SC.CASES[name]["hidden"] > 128))
    assert any(h for _, h in seen) and any(C == 31 for C, _ in seen)


def _roll(lib, d, s, a, dw="zero", x=FAKE, v=FAKE, xf=FAKE + 0x100, vf=FAKE + 0x200, ws=None, n=0):
    dw = L.Weights() if isinstance(dw, str) else dw
    return lib.gnca_rollout_tangent_params(ctypes.byref(d), ctypes.byref(L.Weights()),
                                           None if dw is None else ctypes.byref(dw), ctypes.byref(s), ctypes.byref(a),
                                           x, v, xf, vf, ws, n)


def test_rollout_refusals(lib):
    keep = []
    d = _desc()
    s, a = _sched(6, keep), _args([2, 6], keep)
    size = lib.gnca_rollout_tangent_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(a))
    assert size > 0 and _roll(lib, d, s, a) == WORKSPACE
    assert _roll(lib, d, s, a, ws=FAKE, n=size - 1) == WORKSPACE            # the twin's size is the size
    assert _roll(lib, d, s, a, dw=None) == INVALID
    for kw in (dict(x=None), dict(v=None), dict(xf=None), dict(vf=None), dict(xf=FAKE), dict(vf=FAKE),
               dict(v=FAKE + 8, xf=FAKE + 8), dict(v=FAKE + 8, vf=FAKE + 8), dict(xf=FAKE + 16, vf=FAKE + 16)):
        assert _roll(lib, d, s, a, **kw) == INVALID, kw
    for f in DIR_FIELDS:
        assert _roll(lib, d, s, a, dw=_dw(**{f: FAKE + 0x100})) == INVALID, f
        assert _roll(lib, d, s, a, dw=_dw(**{f: FAKE + 0x200})) == INVALID, f
    for fl in (L.SCHED_RECOMPUTE, L.SCHED_CHECKPOINT, L.SCHED_RECOMPUTE | L.SCHED_CHECKPOINT):   # there is no tape
        assert _roll(lib, d, _sched(6, keep, flags=fl), a) == INVALID, fl
    # renormalising v alone breaks linearity in the pair: refused with a direction, a zero one included,
    # while the twin takes the same arguments; the log norms are still recorded without the flag
    rn = _args([2, 6], keep, flags=L.TANGENT_RENORM)
    assert _roll(lib, d, s, rn) == INVALID
    assert lib.gnca_rollout_tangent(ctypes.byref(d), ctypes.byref(L.Weights()), ctypes.byref(s), ctypes.byref(rn), FAKE,
                                    FAKE, FAKE + 0x100, FAKE + 0x200, None, 0) == WORKSPACE
    for rec in ([0], [7], [2, 2], [3, 2], [-1]):                      # a malformed record list
        assert _roll(lib, d, s, _args(rec, keep)) == INVALID, rec
    assert _roll(lib, d, s, _args([2], keep, log_norm=None)) == INVALID
    assert _roll(lib, d, s, _args([2], keep, flags=2)) == INVALID    # an unknown flag
    zp = _desc(flags=d.flags | L.ZERO_PAD_SHIFT)
    assert _roll(lib, zp, s, a) == UNSUPPORTED


def _block(lib, d, s, a, dw="zero", x=FAKE, v=FAKE, xf=FAKE + 0x100, vf=FAKE + 0x200, ws=None, n=0):
    K = max(1, min(a.num_dirs, L.TANGENT_MAX_DIRS))
    arr = (L.Weights * K)() if isinstance(dw, str) else dw
    return lib.gnca_rollout_tangent_block_params(ctypes.byref(d), ctypes.byref(L.Weights()), arr, ctypes.byref(s),
                                                 ctypes.byref(a), x, v, xf, vf, ws, n)


def test_block_refusals(lib):
    keep = []
    d = _desc()
    s, a = _sched(6, keep), _bargs(3, [2, 6], keep)
    size = lib.gnca_rollout_tangent_block_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(a))
    assert size > 0 and _block(lib, d, s, a) == WORKSPACE
    assert _block(lib, d, s, a, ws=FAKE, n=size - 1) == WORKSPACE
    assert _block(lib, d, s, a, dw=None) == INVALID
    for kw in (dict(x=None), dict(v=None), dict(xf=None), dict(vf=None), dict(xf=FAKE), dict(vf=FAKE),
               dict(xf=FAKE + 16, vf=FAKE + 16)):
        assert _block(lib, d, s, a, **kw) == INVALID, kw
    for j in range(3):                                                # any of the K directions
        for f in DIR_FIELDS:
            arr = (L.Weights * 3)()
            setattr(arr[j], f, FAKE + 0x200)
            assert _block(lib, d, s, a, dw=arr) == INVALID, (j, f)
    for K in (0, 17):
        assert _block(lib, d, s, _bargs(K, [], keep)) == INVALID, K
    ortho = _bargs(3, [2, 6], keep, flags=L.TBLOCK_ORTHO)
    assert _block(lib, d, s, ortho) == INVALID                        # mixing the v_j alone breaks linearity
    assert lib.gnca_rollout_tangent_block(ctypes.byref(d), ctypes.byref(L.Weights()), ctypes.byref(s),
                                          ctypes.byref(ortho), FAKE, FAKE, FAKE + 0x100, FAKE + 0x200, None,
                                          0) == WORKSPACE
    for fl in (L.SCHED_RECOMPUTE, L.SCHED_CHECKPOINT):
        assert _block(lib, d, _sched(6, keep, flags=fl), a) == INVALID, fl
    assert _block(lib, d, s, _bargs(3, [2], keep, log_r=None)) == INVALID
    assert _block(lib, _desc(flags=d.flags | L.ZERO_PAD_SHIFT), s, a) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# The Python layer: every ValueError, before anything is drawn
# ---------------------------------------------------------------------------------------------
def _graph(zp=False, gn=True):
    torch.manual_seed(0)
    return NeuralCAGraph(8, 32, alpha_thr=0.1, graph_attention_radius=2, graph_num_neighbors=4,
                         graph_zero_padded_shift=zp, use_groupnorm=gn)


def _raises_untouched(fn):
    random.seed(5)
    torch.manual_seed(5)
    py, tc = random.getstate(), torch.get_rng_state()
    with pytest.raises(ValueError) as e:
        fn()
    assert random.getstate() == py and torch.equal(torch.get_rng_state(), tc), "a refused call drew something"
    return str(e.value)


def test_signatures_default_to_none():
    for cls in (NeuralCA, NeuralCAGraph):
        for n in ("tangent_step", "rollout_tangent", "rollout_tangent_block"):
            p = inspect.signature(getattr(cls, n)).parameters["dparams"]
            assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, (cls, n)


def test_param_direction():
    for m in (_graph(), NeuralCA(8, 32), _graph(gn=False)):
        names = dict(m.named_parameters())
        d = m.param_direction()
        assert set(d) == set(S.DIRECTION_FIELDS) & set(names)
        for k, t in d.items():
            assert t.shape == names[k].shape and t.dtype == names[k].dtype and not t.any() and not t.requires_grad
        assert all((t == 0.5).all() for t in m.param_direction(fill=0.5).values())
    assert "graph.msg_proj.weight" in _graph().param_direction() and "norm.weight" not in _graph(gn=False).param_direction()
    assert "perception.conv.weight" not in NeuralCA(8, 32).param_direction()


def test_python_refusals():
    m, c, nogn = _graph(), NeuralCA(8, 32), _graph(gn=False)
    x, v = torch.rand(2, 8, 6, 6), torch.rand(2, 8, 6, 6)
    V = torch.rand(3, 2, 8, 6, 6)
    ok = m.param_direction(1.0)
    w1 = ok["update_net.0.weight"]
    meta = torch.empty(w1.shape, device="meta")
    for fn in (
        lambda: m.tangent_step(x, v, dparams={"perception.conv.weight": torch.zeros(24, 1, 3, 3)}),   # frozen
        lambda: m.tangent_step(x, v, dparams={"update_net.1.weight": w1}),                            # unknown
        lambda: m.tangent_step(x, v, dparams={"message_gain": torch.zeros(())}),                      # no parameter
        lambda: c.tangent_step(x, v, dparams={"graph.msg_proj.weight": torch.zeros(8, 8, 1, 1)}),     # classic
        lambda: nogn.tangent_step(x, v, dparams={"norm.weight": torch.zeros(8)}),                     # no GroupNorm
        lambda: nogn.rollout_tangent(x, v, 2, dparams={"norm.bias": torch.zeros(8)}),
        lambda: m.tangent_step(x, v, dparams={"update_net.0.weight": w1[:, :, 0]}),                   # shape
        lambda: m.tangent_step(x, v, dparams={"update_net.0.bias": torch.zeros(33)}),
        lambda: m.tangent_step(x, v, dparams={"update_net.0.weight": w1.double()}),                   # dtype
        lambda: m.tangent_step(x, v, dparams={"update_net.0.weight": meta}),                          # device
        lambda: m.tangent_step(x, v, dparams={"update_net.0.weight": w1.numpy()}),                    # not a tensor
        lambda: m.tangent_step(x, v, dparams=[ok]),                                                   # not a dict
        lambda: m.tangent_step(x, None),                                                              # v=None alone
        lambda: m.rollout_tangent(x, None, 2),
        lambda: m.rollout_tangent_block(x, None, 2),
        lambda: m.tangent_step(x, v[:1], dparams=ok),                                                 # the twin's
        lambda: m.rollout_tangent(x, v, 4, renormalize=True, dparams=ok),
        lambda: m.rollout_tangent(x, v, 4, renormalize=True, dparams={}),                             # a zero one too
        lambda: m.rollout_tangent(x, v, 4, record=[5], dparams=ok),
        lambda: m.rollout_tangent(x, v, -1, dparams=ok),
        lambda: m.rollout_tangent_block(x, V, 4, dparams=[ok] * 3),                                   # ortho default
        lambda: m.rollout_tangent_block(x, V, 4, orthonormalize=True, dparams=[ok] * 3),
        lambda: m.rollout_tangent_block(x, V, 4, orthonormalize=False, dparams=[ok] * 2),             # K differs
        lambda: m.rollout_tangent_block(x, V, 4, orthonormalize=False, dparams=ok),                   # not a list
        lambda: m.rollout_tangent_block(x, V, 4, orthonormalize=False, dparams=[]),
        lambda: m.rollout_tangent_block(x, V, 4, orthonormalize=False, dparams=[ok, ok, {"nope": w1}]),
        lambda: c.rollout_tangent_block(x, V, 4, orthonormalize=False, dparams=[{"norm.weight": torch.zeros(9)}] * 3),
    ):
        _raises_untouched(fn)
    zp = _graph(zp=True)
    for fn in (lambda: zp.tangent_step(x, v, dparams=zp.param_direction()),
               lambda: zp.rollout_tangent(x, None, 3, dparams=zp.param_direction())):
        assert "zero-padded shift" in _raises_untouched(fn)


def test_accepted_directions_reach_the_device_check():
    """A valid call on a CPU state reaches the device check (there is no CPU path): the ignored graph keys, a
    missing key, v=None and a list of K dicts are all accepted."""
    m, c = _graph(), NeuralCA(8, 32)
    x, v = torch.rand(2, 8, 6, 6), torch.rand(2, 8, 6, 6)
    ignored = {n: torch.zeros_like(p) for n, p in m.named_parameters()
               if n.startswith(("graph.query_proj.", "graph.key_proj.", "graph.scaling", "graph.gate_mlp."))}
    assert {"graph.query_proj.weight", "graph.key_proj.bias", "graph.scaling"} <= set(ignored)
    assert any(n.startswith("graph.gate_mlp.") for n in ignored)
    full = dict(m.param_direction(1.0), **ignored)
    for fn in (lambda: m.tangent_step(x, v, dparams=full), lambda: m.tangent_step(x, None, dparams=ignored),
               lambda: m.tangent_step(x, v, dparams={}), lambda: m.rollout_tangent(x, None, 3, dparams=full),
               lambda: m.rollout_tangent(x, v, 3, record=[1, 3], dparams={"norm.bias": torch.ones(8)}),
               lambda: c.rollout_tangent(x, v, 3, dparams=c.param_direction()),
               lambda: m.rollout_tangent_block(x, None, 3, orthonormalize=False, dparams=[full, {}]),
               lambda: m.rollout_tangent_block(x, torch.rand(2, 2, 8, 6, 6), 3, orthonormalize=False, dparams=(full, {}))):
        with pytest.raises(RuntimeError):
            fn()


def test_allocation_sites():
    """step.py's tangent section allocates with torch.empty alone (a zero tangent for v=None is the module
    layer's)."""
    src = open(os.path.join(ROOT, "graph_neural_cellular_automata_amd", "step.py")).read()
    body = src[src.index("def step_tangent"):]
    assert "torch.empty" in body and ".new_empty" not in body and ".new_zeros" not in body and "torch.zeros" not in body
