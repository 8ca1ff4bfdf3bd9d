"""Graph diagnostics on the GPU (gnca_graph_diag / gnca_rollout_trace_diag, GraphAugmentation.diagnostics,
trace(diagnostics=True)): against a float64 oracle built from oracle/nca_oracle.py's blocks, against
the reference's recorded ``debug_graph_from_state`` outputs (tests/golden/diag), against the attention
op, against itself (bitwise run to run, batch independence), inside a trace, and on poisoned buffers.

Tolerance: every float output within ``2e-5 * max|ref|`` of the float64 oracle, the maximum taken per
output and per sample (the attention map's bound of tests/test_gpu_attention_map.py at the plane's
scale).  Every [H,W] oracle plane the bound is applied to has a maximum of at least 1e-2 (asserted on
the oracle; the hidden group of a 4-channel state is empty, its planes are zeros by definition and are
compared exactly).  The masks must match exactly, and no pooled alpha of a test state lies within 1e-6
of the threshold (asserted), so a mask cannot flip on a rounding.

``oracle_diag`` is importable without a GPU: tests/golden/make_golden_diag.py records it beside the
reference's values.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests import liveness_cases as LC
from tests import poison as PZ
from tests.test_gpu_attention_map import SHAPES, _graph_and_state

pytestmark = pytest.mark.gpu

RTOL_PLANE = 2e-5
PLANE_MIN = 1e-2
THR_MARGIN = 1e-6
FLOATS = ("magnitude", "groups", "per_offset", "raw", "attention", "weights")
MASKS = ("sender_union", "receiver")
DIAG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diag")
FIXTURES = ("diag_torus_latest_b1_20x24", "diag_zeropad_ep380_b1_20x24")
# trace: tests/test_gpu_poison.py's TRACE_ROWS shapes (one folds, one does not) and the small batch
TRACE_ROWS = [("graph", 8, 48, 72), ("graph", 8, 40, 40), ("graph", 2, 40, 40)]
TRACE_STEPS = 7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------
# The float64 oracle
# ---------------------------------------------------------------------------------------------
def oracle_diag(x64, p, chosen, *, zp, a2a, thr):
    """The fields of include/gnca.h's gnca_graph_diag_out in float64, from the oracle's blocks.
    ``p``: float64 parameters under their state_dict names ("graph." prefix)."""
    B, C, H, W = x64.shape
    shift = O.shift_pad if zp else O.shift_roll
    absm = np.abs(O.conv1x1(x64, p["graph.msg_proj.weight"], p["graph.msg_proj.bias"]))
    G = np.zeros((B, 3, H, W))
    G[:, 0] = absm[:, 0:3].mean(axis=1)
    G[:, 1] = absm[:, 3]
    if C > 4:
        G[:, 2] = absm[:, 4:].mean(axis=1)
    alive = O.alive_mask(x64, thr)                              # [B,1,H,W]
    src = alive if a2a else np.ones_like(alive)
    S = src * absm.mean(axis=1, keepdims=True)
    k = len(chosen)
    out = dict(magnitude=G, receiver=alive[:, 0], groups=np.zeros((B, 3, H, W)), per_offset=np.zeros((B, k, H, W)),
               raw=np.zeros((B, H, W)), attention=np.zeros((B, H, W)), sender_union=np.zeros((B, H, W)),
               weights=np.zeros((B, k)))
    if k == 0:
        return out
    # the torus roll keeps every pooled key: the softmax is uniform, exactly 1/k
    Wt = O.offset_weights(x64, p, chosen, zero_padded_shift=True).T if zp else np.full((B, k), 1.0 / k)
    out["weights"] = Wt
    for o, (dy, dx) in enumerate(chosen):
        w = Wt[:, o, None, None]
        out["per_offset"][:, o] = w * shift(S, dy, dx)[:, 0]
        out["groups"] += w[:, None] * shift(src * G, dy, dx)
        if a2a:
            out["sender_union"] = np.maximum(out["sender_union"], shift(src, dy, dx)[:, 0])
    raw = out["per_offset"].sum(axis=1)
    out["raw"] = raw
    lo, hi = raw.min(axis=(1, 2), keepdims=True), raw.max(axis=(1, 2), keepdims=True)
    out["attention"] = (raw - lo) / (hi - lo + 1e-8)
    return out


def assert_margin(x, thr):
    """No pooled alpha within THR_MARGIN of the (float32) threshold: the masks cannot flip on a rounding."""
    d = np.abs(LC.pooled(np.asarray(x, np.float64)[:, 3]) - float(np.float32(thr)))
    assert d.min() > THR_MARGIN, f"a pooled alpha lies {d.min():.3e} from the threshold"


def check_fields(got, ref, tag, planes=True, empty_hidden=False):
    """``got`` (GraphDiagnostics or dict of tensors) against ``ref`` (dict of float64 arrays): floats
    within RTOL_PLANE * max|ref| per output and sample, masks exactly.  Returns the measured maxima of
    |got - ref| / max|ref|."""
    rel = {}
    for n in FLOATS + MASKS:
        g = got.get(n) if isinstance(got, dict) else getattr(got, n)
        if g is None:
            continue
        g, r = g.detach().cpu().numpy(), np.asarray(ref[n])
        assert g.shape == r.shape and g.dtype == np.float32, (tag, n, g.shape, r.shape)
        if n in MASKS:
            assert set(np.unique(g)) <= {0.0, 1.0} and np.array_equal(g, r), (tag, n)
            continue
        worst = 0.0
        for b in range(r.shape[0]):
            gb, rb = g[b], r[b]
            if empty_hidden and n in ("magnitude", "groups"):      # C = 4: the hidden group is empty
                assert not gb[2].any() and not rb[2].any(), (tag, n)
                gb, rb = gb[:2], rb[:2]
            if rb.size == 0:
                continue
            if planes and n != "weights":
                pm = np.abs(rb.reshape(-1, rb.shape[-2], rb.shape[-1])).max(axis=(1, 2))
                assert pm.min() >= PLANE_MIN, f"{tag} {n}[{b}]: an oracle plane's maximum is {pm.min():.3e}"
            scale = float(np.abs(rb).max())
            err = float(np.abs(gb - rb).max())
            worst = max(worst, err / scale)
            assert err <= RTOL_PLANE * scale, f"{tag} {n}[{b}]: |got - ref| = {err:.3e} > {RTOL_PLANE} * {scale:.3e}"
        rel[n] = worst
    print(f"[diag] {tag}: max |hip - ref| / max|ref| = " + ", ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    return rel


def _f64_params(g):
    return {"graph." + k: v.detach().cpu().numpy().astype(np.float64) for k, v in g.state_dict().items()}


def same(a, b):
    """Two GraphDiagnostics are bitwise equal (fields that are None in both included)."""
    for n in FLOATS + MASKS:
        u, v = getattr(a, n), getattr(b, n)
        if (u is None) != (v is None) or (u is not None and not PZ.same_bytes(u, v)):
            return False
    return True


# ---------------------------------------------------------------------------------------------
# The standalone op
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a2a", [True, False], ids=["a2a", "all"])
@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_matches_f64_oracle(dev, shape, zp, a2a):
    g, x = _graph_and_state(SHAPES[shape], zp, a2a, dev)
    random.seed(5)
    chosen = g.sample_offsets()
    assert len(chosen) == min(SHAPES[shape][5], len(g.offsets))
    assert_margin(x.numpy(), g.alpha_thr)
    ref = oracle_diag(x.numpy().astype(np.float64), _f64_params(g), chosen, zp=zp, a2a=a2a, thr=g.alpha_thr)
    assert ref["receiver"].min() == 0 and ref["receiver"].max() == 1       # the dead region matters
    xd = x.to(dev)
    got = g.diagnostics(xd, offsets=chosen)
    assert got.offsets == chosen and not got.raw.requires_grad
    check_fields(got, ref, f"{shape} {'zeropad' if zp else 'torus'} a2a={a2a}", empty_hidden=SHAPES[shape][1] == 4)
    # the normalised map is the attention op's, bitwise; the taps add up to the un-normalised map
    assert torch.equal(got.attention, g.attention_map(xd, offsets=chosen))
    tot = got.per_offset.sum(1)
    for b in range(x.shape[0]):
        assert float((tot[b] - got.raw[b]).abs().max()) <= RTOL_PLANE * float(got.raw[b].abs().max())
    if not a2a:
        assert not got.sender_union.any()
    # per_offset=False leaves every other output bitwise unchanged; bitwise run to run
    lean = g.diagnostics(xd, offsets=chosen, per_offset=False)
    assert lean.per_offset is None
    again = g.diagnostics(xd, offsets=chosen)
    assert same(got, again)
    lean.per_offset = got.per_offset
    assert same(got, lean)


@pytest.mark.parametrize("name", FIXTURES)
def test_matches_reference_fixture(dev, name):
    """The reference's own ``debug_graph_from_state`` (fp32) and ``|M|`` group means on a sample of an
    existing fixture's state with a trained checkpoint's weights, recorded by
    tests/golden/make_golden_diag.py (which says why these states)."""
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import desc_for, weights_on
    from tests.golden_io import Case
    z = np.load(os.path.join(DIAG_DIR, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    c = Case(meta["source"])
    x = z["x"]
    assert np.array_equal(x, Case(meta["state"]).x_in[meta["sample"]:meta["sample"] + 1])
    chosen = [tuple(int(v) for v in o) for o in z["offsets"]]
    assert_margin(x, c.meta["alpha_thr"])
    desc = desc_for(c, 1, x.shape[2], x.shape[3], chosen, 0, attention=False)
    w, keep = S.make_weights(weights_on(c, dev))
    got = S.graph_diagnostics(desc, w, torch.from_numpy(x).to(dev))
    ref = {n: z["ref:" + n] for n in FLOATS + MASKS if n not in ("attention", "weights")}
    f64 = {n: z["f64:" + n] for n in FLOATS + MASKS}
    ref["weights"] = f64["weights"]
    tag = f"{name} vs the reference (fp32), weights vs float64"
    check_fields({n: getattr(got, n) for n in ref}, ref, tag, planes=False)
    check_fields(got, f64, f"{name} vs float64", planes=False)
    werr = float(np.abs(got.weights.cpu().numpy() - z["ref:weights"]).max())
    print(f"[diag] {name}: max |weights - the reference's fp32 softmax| = {werr:.3e} "
          f"(the reference's own error against float64: {float(np.abs(z['ref:weights'] - f64['weights']).max()):.3e})")
    del keep


@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
def test_no_offsets(dev, zp):
    """k = 0 (num_neighbors = 0, or an empty offset list): zeros, except magnitude and receiver."""
    g, x = _graph_and_state(SHAPES["ragged_2x16x17x29_r4_k8"], zp, True, dev, K=0)
    assert g.sample_offsets() == []
    ref = oracle_diag(x.numpy().astype(np.float64), _f64_params(g), [], zp=zp, a2a=True, thr=g.alpha_thr)
    for got in (g.diagnostics(x.to(dev)), g.diagnostics(x.to(dev), offsets=[])):
        assert got.per_offset.shape == (2, 0, 17, 29) and got.weights.shape == (2, 0) and got.offsets == []
        for n in ("groups", "raw", "attention", "sender_union"):
            assert getattr(got, n).shape == ref[n].shape and not getattr(got, n).any(), n
        check_fields({n: getattr(got, n) for n in ("magnitude", "receiver")}, ref, f"k = 0 zp={zp}")


@pytest.mark.parametrize("zp", [False, True], ids=["torus", "zeropad"])
def test_sample_is_independent_of_the_batch(dev, zp):
    """Sample b of a B = 3 call equals the B = 1 call on that sample, bitwise."""
    g, x = _graph_and_state(SHAPES["c32_3x32x24x24_r5_k16"], zp, True, dev)
    random.seed(6)
    chosen = g.sample_offsets()
    xd = x.to(dev)
    full = g.diagnostics(xd, offsets=chosen)
    for b in range(3):
        one = g.diagnostics(xd[b:b + 1].contiguous(), offsets=chosen)
        for n in FLOATS + MASKS:
            assert PZ.same_bytes(getattr(full, n)[b:b + 1], getattr(one, n)), (n, b)


def test_offsets_none_draws_one_sample(dev):
    g, x = _graph_and_state(SHAPES["ragged_2x16x17x29_r4_k8"], False, True, dev)
    random.seed(8)
    chosen = random.sample(g.offsets, 8)
    after = random.random()
    random.seed(8)
    got = g.diagnostics(x.to(dev))
    assert random.random() == after and got.offsets == chosen
    assert same(got, g.diagnostics(x.to(dev), offsets=chosen))


# ---------------------------------------------------------------------------------------------
# Inside a trace
# ---------------------------------------------------------------------------------------------
def _trace_model(dev, H, W, B, zp=False):
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    m = LC.MODELS["graph_zp" if zp else "graph"]
    torch.manual_seed(3)
    model = NeuralCAGraph(16, 128, update_gain=m["gain"], alpha_thr=m["thr"], message_gain=m["msg"],
                          graph_zero_padded_shift=zp).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    x = torch.from_numpy(LC.build("sparse", 31, B, 16, H, W, m["thr"], (8, 24)).x).to(dev)
    offs = [LC.offsets(m, t) for t in range(TRACE_STEPS)]
    return model, x, offs


def test_trace_rows_fold_and_do_not():
    """Host-only: of the two TRACE_ROWS shapes of tests/test_gpu_poison.py one folds and one does not."""
    from tests import test_gpu_poison as G
    assert TRACE_ROWS[:2] == G.TRACE_ROWS
    assert sorted(LC.check_plan(*r)["fold"] for r in TRACE_ROWS[:2]) == [False, True]


@pytest.mark.parametrize("row", TRACE_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_trace_records_each_steps_diagnostics(dev, row):
    _, B, H, W = row
    model, x, offs = _trace_model(dev, H, W, B, zp=(B == 2))
    kw = dict(every=1, channels=16, fire_rate=0.5, seed=31, offsets=offs, return_attention=True)
    tgt = torch.rand(4, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    plain = model.trace(x, TRACE_STEPS, target=tgt, **kw)
    res = model.trace(x, TRACE_STEPS, target=tgt, diagnostics=True, per_offset=True, **kw)
    assert plain.diagnostics is None and res.steps == list(range(1, TRACE_STEPS + 1))
    # with diagnostics on, everything else is bitwise what it was
    assert torch.equal(res.frames, plain.frames) and torch.equal(res.x_final, plain.x_final)
    assert PZ.same_bytes(res.attention, plain.attention)
    assert PZ.same_bytes(res.metrics.stacked, plain.metrics.stacked)
    assert not torch.equal(res.x_final, x)
    d = res.diagnostics
    assert d.per_offset.shape == (TRACE_STEPS, B, 8, H, W) and d.offsets == offs
    for r in range(TRACE_STEPS):
        state = x if r == 0 else res.frames[r - 1]
        one = model.graph.diagnostics(state.contiguous(), offsets=offs[r])
        for n in FLOATS + MASKS:
            assert PZ.same_bytes(getattr(d, n)[r], getattr(one, n)), (row, r, n)
        assert PZ.same_bytes(d.attention[r], res.attention[r])
    assert float(d.raw.max()) > 0 and d.receiver.min() == 0 and d.receiver.max() == 1
    # without per_offset the stack is absent and the rest unchanged
    lean = model.trace(x, TRACE_STEPS, diagnostics=True, **kw).diagnostics
    assert lean.per_offset is None and PZ.same_bytes(lean.groups, d.groups) and PZ.same_bytes(lean.raw, d.raw)


@pytest.mark.parametrize("row", TRACE_ROWS[:2], ids=lambda r: "-".join(map(str, r)))
def test_trace_every3_target_no_frames(dev, row):
    _, B, H, W = row
    model, x, offs = _trace_model(dev, H, W, B)
    tgt = torch.rand(4, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    kw = dict(every=3, fire_rate=0.5, seed=31, offsets=offs, target=tgt)
    full = model.trace(x, TRACE_STEPS, channels=16, **kw)
    res = model.trace(x, TRACE_STEPS, frames=False, diagnostics=True, **kw)
    assert res.frames is None and res.attention is None and res.steps == [3, 6, 7]
    assert torch.equal(res.x_final, full.x_final) and PZ.same_bytes(res.metrics.stacked, full.metrics.stacked)
    d = res.diagnostics
    assert d.per_offset is None and d.raw.shape == (3, B, H, W) and d.offsets == [offs[2], offs[5], offs[6]]
    # record r = step record[r]: its input state is the frame of step record[r] - 1
    every1 = model.trace(x, TRACE_STEPS, every=1, channels=16, fire_rate=0.5, seed=31, offsets=offs)
    for r, t in enumerate(res.steps):
        one = model.graph.diagnostics(every1.frames[t - 2].contiguous(), offsets=offs[t - 1], per_offset=False)
        for n in FLOATS + MASKS:
            if n != "per_offset":
                assert PZ.same_bytes(getattr(d, n)[r], getattr(one, n)), (row, t, n)


# ---------------------------------------------------------------------------------------------
# Poisoned, guarded buffers (tests/poison.py): both entry points
# ---------------------------------------------------------------------------------------------
def _t(a, dev, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(dev)


POISON_ROWS = [("graph", 4, 40, 40, "sparse", True), ("graph_zp", 4, 40, 40, "half_dead", True),
               ("graph_zp_open", 3, 17, 29, "sparse", False), ("classic", 4, 40, 40, "sparse", True)]


@pytest.mark.parametrize("row", POISON_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_poison_graph_diag(dev, row):
    from graph_neural_cellular_automata_amd import step as S
    from tests.test_gpu_poison import _dev_params, _side, _weights
    name, B, H, W, pat, per_offset = row
    m, x0, wt = _side(name, B, H, W, pat, dev)
    desc = LC.make_desc(m, B, H, W)

    def call(P):
        w, keep = _weights(P, wt)
        d = S.graph_diagnostics(desc, w, P.guard(x0), per_offset=per_offset)
        return {n: getattr(d, n) for n in FLOATS + MASKS if getattr(d, n) is not None}

    outs = PZ.run_fills(call, f"diag-{row}")
    assert ("per_offset" in outs) == per_offset
    if m["graph"]:
        assert float(outs["attention"].max()) == 1.0 and float(outs["magnitude"].min()) > 0
        w, keep = S.make_weights(wt)
        assert torch.equal(outs["attention"], S.attention_map(desc, w, x0))
    else:          # graph off: zeros, written; the receiver mask is still the state's
        for n in ("magnitude", "groups", "raw", "attention", "sender_union"):
            assert not outs[n].any(), n
        assert outs["weights"].numel() == 0 and outs["per_offset"].numel() == 0
    assert outs["receiver"].min() == 0 and outs["receiver"].max() == 1


@pytest.mark.parametrize("mode", [(1, True, True), (3, True, False), (1, False, False)],
                         ids=lambda v: f"every{v[0]}-{'target' if v[1] else 'plain'}" + "-taps" * v[2])
@pytest.mark.parametrize("row", TRACE_ROWS[:2], ids=lambda r: "-".join(map(str, r)))
def test_poison_trace_diag(dev, row, mode):
    from graph_neural_cellular_automata_amd import step as S
    from tests.test_gpu_poison import _hash_desc, _rollout_setup, _weights
    name, B, H, W = row
    every, with_target, per_offset = mode
    seed, T = 31, 4
    m, plan, x0, wt = _rollout_setup(name, B, H, W, "sparse", dev, seed)
    offs = [LC.offsets(m, t) for t in range(T)]
    desc = _hash_desc(m, B, H, W, seed)
    record = S.expand_record(T, every)
    tgt0 = _t(np.random.default_rng(3).random((4, H, W)), dev, np.float32)

    def call(P):
        w, keep = _weights(P, wt)
        out, frm, attn, met, d = S.trace_diag(desc, w, P.guard(x0), T, offs, record, 4,
                                              P.guard(tgt0) if with_target else None, 0, want_attention=True,
                                              per_offset=per_offset)
        res = {"x_final": out, "frames": frm, "attn": attn}
        if with_target:
            res["metrics"] = met
        res.update({"diag." + n: getattr(d, n) for n in FLOATS + MASKS if getattr(d, n) is not None})
        return res

    outs = PZ.run_fills(call, f"trace-diag-{row}-{mode}")
    w, keep = S.make_weights(wt)
    assert torch.equal(outs["x_final"], S.rollout(desc, w, x0, T, offs)), (row, mode, plan)
    assert torch.equal(outs["frames"][-1], outs["x_final"][:, :4])
    assert PZ.same_bytes(outs["diag.attention"], outs["attn"])
    assert ("diag.per_offset" in outs) == per_offset
