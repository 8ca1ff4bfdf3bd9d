"""The step on padded channel counts and on every row of the two kernel tables (the cases of
tests/shape_class_cases.py, which says what they reach): forward, attention map, diagnostics, backward,
rollout, BPTT rollout, masked step and trace, each against the float64 oracle or bitwise against the
per-step path, and forward and backward again on guarded, poisoned buffers (tests/poison.py), where a
read of channel C..CP-1 or a weight row taken at stride CP meets NaN or a canary and not a plausible
neighbour.

Tolerances are the project's own, none is new:
  forward      |hip - f64| <= 2e-6 + 1e-5 |f64|                      (tests/test_gpu_parity.py)
  attention    |map - f64| <= 2e-5                                   (tests/test_gpu_parity.py)
  diagnostics  tests/test_gpu_diag.py's check_fields (2e-5 * max|ref| per output and sample)
  backward     |g - f64| <= 2e-5 * max|f64| + 1e-6 per tensor        (tests/test_gpu_grad.py)
  BPTT         x_final, gx bitwise; weights RT * max|R| + AT         (tests/test_gpu_rollout_bptt.py)
Every case holds them, the hidden-256 ones included (measured on an MI355X: forward errors 7.7e-8 to
4.1e-7, the largest on q16h200; backward errors at most 0.026 of the bound; the table in DESIGN.md), so
no bound had to be derived from a measurement.
"""
import random

import numpy as np
import pytest
import torch

from tests import poison as PZ
from tests import shape_class_cases as SC

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-6, 1e-5
RT, AT = 2e-5, 1e-6
T = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class _Built:
    pass


_BUILT: dict = {}


def _built(name, dev):
    """The case on the device, once: module, state, cotangent, the offsets ``random.sample`` draws
    and the fire mask ``torch.rand`` draws under the case's seeds, and the float64 reference for them."""
    if name in _BUILT:
        return _BUILT[name]
    c = SC.CASES[name]
    b = _Built()
    b.c, b.m = c, SC.model(name, dev)
    b.x, b.gy = SC.state(name).to(dev), SC.cotangent(name).to(dev)
    b.chosen = SC.offsets(name)[0]
    if c["graph"]:
        random.seed(SC.seed(name))
        assert b.m.graph.sample_offsets() == b.chosen and len(b.chosen) == c["K"]
    b.fire = None
    if c["fire_rate"] < 1.0:
        torch.cuda.manual_seed(SC.seed(name))
        b.fire = (torch.rand(c["B"], 1, c["H"], c["W"], device=dev) <= c["fire_rate"]).to(torch.uint8)
    b.ref = SC.reference(name, fire=None if b.fire is None else b.fire.cpu())
    _BUILT[name] = b
    return b


def _forward(b, name, x=None, **kw):
    """One module step with the reference's draws: ``random.sample`` of the offsets, ``torch.rand``
    of the fire mask."""
    random.seed(SC.seed(name))
    torch.cuda.manual_seed(SC.seed(name))
    return b.m(b.x if x is None else x, fire_rate=b.c["fire_rate"], **kw)


def _plan(name):
    from graph_neural_cellular_automata_amd import step as S
    d = SC.desc(name)
    k1, bb = S.k1_variant(d)[0], S.bb_variant(d)
    assert k1.startswith(SC.k1_name(name)) and bb == SC.bb_name(name), (name, k1, bb)
    return f"{name} {k1} {bb} x{SC.CASES[name]['bb'][2]}"


def _check_grads(tag, got, ref):
    """Per tensor within 2e-5 * max|ref| + 1e-6, the key sets equal, every value finite.  Returns the
    largest err / bound."""
    assert set(got) == set(ref), (tag, sorted(set(got) ^ set(ref)))
    worst = 0.0
    for k, r in ref.items():
        g = got[k].detach().cpu().numpy().reshape(r.shape).astype(np.float64)
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        assert np.isfinite(g).all(), (tag, k)
        assert err <= 2e-5 * scale + 1e-6, (tag, k, f"err={err:.3e} scale={scale:.3e}")
        worst = max(worst, err / (2e-5 * scale + 1e-6))
    return worst


# ---------------------------------------------------------------------------------------------
# Forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.IDS)
def test_forward_matches_oracle(dev, name):
    b = _built(name, dev)
    with torch.no_grad():
        out = _forward(b, name)
    got = out.cpu().numpy()
    print(f"[shape classes] fwd {_plan(name)}: max |hip - f64| = {float(np.abs(got - b.ref['out']).max()):.3e}")
    np.testing.assert_allclose(got, b.ref["out"], rtol=RTOL, atol=ATOL, err_msg=name)


@pytest.mark.parametrize("name", SC.IDS)
def test_forward_on_guarded_buffers(dev, name):
    """The same step through the C ABI with the state, the fire mask and every weight tensor in a
    guarded block of its own: byte-identical under every fill, every canary intact, and the oracle's
    values."""
    from graph_neural_cellular_automata_amd import step as S
    b = _built(name, dev)
    wt = {k: v.detach() for k, v in SC.weight_tensors(b.m).items()}
    desc = SC.desc(name, b.chosen)

    def call(P):
        w, keep = S.make_weights({k: P.guard(v) for k, v in wt.items()})
        out, _ = S.step(desc, w, P.guard(b.x), fire=P.guard(b.fire))
        return {"x_out": out}

    outs = PZ.run_fills(call, "shape-fwd-" + name)
    np.testing.assert_allclose(outs["x_out"].cpu().numpy(), b.ref["out"], rtol=RTOL, atol=ATOL, err_msg=name)


# ---------------------------------------------------------------------------------------------
# Attention map and diagnostics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.GRAPH_IDS)
def test_attention_matches_oracle(dev, name):
    """``return_attention=True`` (K1's attention path) against the oracle, and the standalone op
    against the step's map and the oracle (tests/test_gpu_attention_map.py's bound)."""
    b = _built(name, dev)
    with torch.no_grad():
        out, attn = _forward(b, name, return_attention=True)
    np.testing.assert_allclose(out.cpu().numpy(), b.ref["out"], rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_allclose(attn.cpu().numpy(), b.ref["attn"], rtol=0, atol=2e-5, err_msg=name)
    alone = b.m.graph.attention_map(b.x, offsets=b.chosen)
    assert alone.shape == attn.shape and not alone.requires_grad
    err = float((alone - attn).abs().max())
    print(f"[shape classes] attention {name}: step vs f64 {float(np.abs(attn.cpu().numpy() - b.ref['attn']).max()):.3e}, "
          f"standalone vs step {err:.3e}")
    assert err <= 2e-5, (name, err)
    np.testing.assert_allclose(alone.cpu().numpy(), b.ref["attn"], rtol=0, atol=2e-5, err_msg=name)
    assert torch.equal(alone, b.m.graph.attention_map(b.x, offsets=b.chosen))


@pytest.mark.parametrize("name", SC.GRAPH_IDS)
def test_diagnostics_match_oracle(dev, name):
    """``graph.diagnostics`` against tests/test_gpu_diag.py's float64 ``oracle_diag`` at its bounds: the
    channel-group means divide by the true channel counts (C - 4 hidden channels: 13 for p17, 2 for p6),
    and the hidden group of a 4-channel state (q4) is exactly zero."""
    from tests.test_gpu_diag import assert_margin, check_fields, oracle_diag, same
    b = _built(name, dev)
    c = b.c
    x = SC.state(name).numpy()
    assert_margin(x, c["thr"])
    ref = oracle_diag(x.astype(np.float64), SC.params64(name), b.chosen, zp=c["zp"], a2a=c["a2a"], thr=c["thr"])
    assert ref["receiver"].min() == 0 and ref["receiver"].max() == 1       # the dead band matters
    got = b.m.graph.diagnostics(b.x, offsets=b.chosen)
    assert got.offsets == b.chosen
    check_fields(got, ref, "shape classes " + name, empty_hidden=c["C"] == 4)
    if c["C"] == 4:
        assert not got.magnitude[:, 2].any() and not got.groups[:, 2].any()
    assert torch.equal(got.attention, b.m.graph.attention_map(b.x, offsets=b.chosen))
    assert bool(got.sender_union.any()) == c["a2a"]
    assert same(got, b.m.graph.diagnostics(b.x, offsets=b.chosen))


# ---------------------------------------------------------------------------------------------
# Backward
# ---------------------------------------------------------------------------------------------
def _module_backward(b, name):
    m = SC.model(name, b.x.device).train()
    x = b.x.clone().requires_grad_(True)
    random.seed(SC.seed(name))
    torch.cuda.manual_seed(SC.seed(name))
    out = m(x, fire_rate=b.c["fire_rate"])
    (out * b.gy).sum().backward()
    torch.cuda.synchronize()
    got = {n: q.grad for n, q in m.named_parameters() if q.grad is not None}
    got["gx"] = x.grad
    return out.detach(), got


@pytest.mark.parametrize("name", SC.IDS)
def test_backward_matches_oracle(dev, name):
    b = _built(name, dev)
    out, got = _module_backward(b, name)
    np.testing.assert_allclose(out.cpu().numpy(), b.ref["out"], rtol=RTOL, atol=ATOL, err_msg=name)
    worst = _check_grads(name, got, dict(b.ref["grads"], gx=b.ref["gx"]))
    print(f"[shape classes] bwd {_plan(name)}: max err / bound = {worst:.3f}")
    assert float(got["gx"].abs().max()) > 0 and float(got["update_net.2.weight"].abs().max()) > 0
    _, again = _module_backward(b, name)
    for k in got:
        assert torch.equal(got[k], again[k]), (name, k)


@pytest.mark.parametrize("saved", [False, True], ids=["recompute", "saved"])
@pytest.mark.parametrize("name", SC.IDS)
def test_backward_on_guarded_buffers(dev, name, saved):
    """gnca_step_bwd_f32 with every input in a guarded block: the partial rows (``npart`` columns, no
    multiple of 4 for these C) and the reducer's 128-byte line reads are the unaligned part."""
    from graph_neural_cellular_automata_amd import step as S
    b = _built(name, dev)
    wt = {k: v.detach() for k, v in SC.weight_tensors(b.m).items()}
    want = {n: p for n, p in b.m.named_parameters() if n in S.GRAD_FIELDS}
    desc = SC.desc(name, b.chosen)

    def call(P):
        w, keep = S.make_weights({k: P.guard(v) for k, v in wt.items()})
        x, fire = P.guard(b.x), P.guard(b.fire)
        outs, ws = {}, None
        if saved:
            ws = S.workspace(desc, dev)
            outs["x_out"], _ = S.step(desc, w, x, fire=fire, ws=ws)
        gx, grads = S.step_backward(desc, w, x, P.guard(b.gy), fire=fire, want=want, saved=ws)
        outs["gx"] = gx
        outs.update(grads)
        return outs

    outs = PZ.run_fills(call, f"shape-bwd-{name}-{saved}")
    outs.pop("x_out", None)
    _check_grads(name, outs, dict(b.ref["grads"], gx=b.ref["gx"]))


# ---------------------------------------------------------------------------------------------
# Rollouts
# ---------------------------------------------------------------------------------------------
def _hash_descs(name, offs, gains=None, B=None):
    from graph_neural_cellular_automata_amd import _lib as L
    c = SC.CASES[name]
    mode = L.FIRE_HASH if c["fire_rate"] < 1.0 else L.FIRE_NONE
    return [SC.desc(name, offs[t], B=B, fire_mode=mode, rng_step=t,
                    message_gain=None if gains is None else gains[t]) for t in range(len(offs))]


@pytest.mark.parametrize("name", SC.IDS)
def test_rollout_equals_steps(dev, name):
    """A 3-step gnca_rollout_ex_f32 is bitwise 3 single steps (hash fire masks, fresh offsets per step)."""
    from graph_neural_cellular_automata_amd import step as S
    b = _built(name, dev)
    offs = SC.offsets(name, T)
    w, keep = S.make_weights(SC.weight_tensors(b.m))
    descs = _hash_descs(name, offs)
    r = S.rollout(descs[0], w, b.x, T, offs)
    cur = b.x
    for t in range(T):
        cur, _ = S.step(descs[t], w, cur)
    assert torch.equal(r, cur), name
    assert not torch.equal(r, b.x)


@pytest.mark.parametrize("name", SC.BPTT_IDS)
def test_rollout_bptt_equals_per_step_path(dev, name):
    """``model.rollout`` with grad and per-sample step counts against the per-step path
    (gnca_step_masked_f32 / gnca_step_bwd_f32 once per step), as
    tests/test_gpu_rollout_bptt.py::test_rollout_equals_per_step_path: x_final and gx bitwise, a weight
    gradient within RT * max|R| + AT of R, the float64 sum of the per-step gradients.  The rollout's
    backward runs the accumulating (ACC) twins of the runtime-C kernels."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    b = _built(name, dev)
    c = b.c
    ns = [3, 1, 2][:c["B"]]
    nst = torch.tensor(ns, dtype=torch.int32, device=dev)
    offs = SC.offsets(name, T)
    gains = [c["msg"], 0.0, c["msg"]] if c["graph"] else None
    # the rollout
    m = SC.model(name, dev).train()
    leaf = b.x.clone().requires_grad_(True)
    kw = dict(fire_rate=0.5, seed=SC.FIRE_SEED, nsteps=nst)
    if c["graph"]:
        kw.update(message_gain=gains, offsets=offs)
    out = m.rollout(leaf, T, **kw)
    (out * b.gy).sum().backward()
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    # the per-step path
    w, keep = S.make_weights(SC.weight_tensors(b.m))
    want = {n: p for n, p in b.m.named_parameters() if n in S.GRAD_FIELDS}
    descs = [SC.desc(name, offs[t], fire_mode=L.FIRE_HASH, fire_rate=0.5, rng_step=t,
                     message_gain=gains[t] if gains else 0.0) for t in range(T)]
    states, saves, acts = [b.x], [], []
    for t in range(T):
        act = nst > t
        ws = S.workspace(descs[t], dev)
        nxt, _ = S.step(descs[t], w, states[-1], ws=ws, active=act)
        states.append(nxt); saves.append(ws); acts.append(act)
    R = {k: np.zeros(tuple(p.shape), np.float64) for k, p in want.items()}
    gcur = b.gy
    for t in reversed(range(T)):
        gcur, gr = S.step_backward(descs[t], w, states[t], gcur, want=want, saved=saves[t], active=acts[t])
        for k in want:
            R[k] += gr[k].double().cpu().numpy()
    assert torch.equal(out.detach(), states[-1]), name
    assert torch.equal(leaf.grad, gcur), name
    assert set(got) == set(R), (sorted(got), sorted(R))
    for k, r in R.items():
        g = got[k].double().cpu().numpy().reshape(r.shape)
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        assert np.isfinite(g).all(), (name, k)
        assert err <= RT * scale + AT, (name, k, f"err={err:.3e} scale={scale:.3e}")
    assert float(np.abs(R["update_net.2.weight"]).max()) > 0


@pytest.mark.parametrize("name", SC.IDS)
def test_masked_step_equals_subbatch(dev, name):
    """B = 3 with one inactive sample: the masked step is bitwise the step of the active sub-batch, the
    inactive sample passes through (uniform fire: the draws are made for the whole batch)."""
    b = _built(name, dev)
    x = SC.state(name, B=3).to(dev)
    active = torch.tensor([True, False, True], device=dev)
    with torch.no_grad():
        random.seed(SC.seed(name))
        out = b.m(x, fire_rate=1.0, active=active)
        random.seed(SC.seed(name))
        sub = b.m(x[active].contiguous(), fire_rate=1.0)
    assert torch.equal(out[active], sub), name
    assert torch.equal(out[~active], x[~active]), name
    assert not torch.equal(sub, x[active])


@pytest.mark.parametrize("name", SC.TRACE_IDS)
def test_trace_equals_pieces(dev, name):
    """``trace`` with maps and metrics against its pieces, bitwise as tests/test_gpu_trace.py and
    tests/test_gpu_metrics.py claim: frames = rollout prefixes, maps = ``attention_map`` of the prefix
    states, metrics = ``image_metrics`` of the frames."""
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    b = _built(name, dev)
    c = b.c
    offs = SC.offsets(name, T)
    g = torch.Generator().manual_seed(5 + SC.seed(name))
    tgt = torch.rand(c["B"], 4, c["H"], c["W"], generator=g)
    tgt[:, :3] *= tgt[:, 3:4]
    tgt = tgt.to(dev)
    kw = dict(fire_rate=0.5, seed=SC.FIRE_SEED, offsets=offs)
    tr = b.m.trace(b.x, T, every=1, channels=c["C"], return_attention=True, target=tgt, **kw)
    assert tr.steps == [1, 2, 3] and tr.frames.shape == (T, *b.x.shape)
    with torch.no_grad():
        prev = b.x
        for r, t in enumerate(tr.steps):
            cur = b.m.rollout(b.x, t, fire_rate=0.5, seed=SC.FIRE_SEED, offsets=offs[:t])
            assert torch.equal(tr.frames[r], cur), (name, t)
            assert torch.equal(tr.attention[r], b.m.graph.attention_map(prev, offsets=offs[t - 1])), (name, t)
            prev = cur
        assert torch.equal(tr.x_final, prev)
    assert PZ.same_bytes(tr.metrics.stacked, image_metrics(tr.frames, tgt).stacked)
    assert torch.isfinite(tr.metrics.stacked).all()
    rgba = b.m.trace(b.x, T, every=1, return_attention=True, target=tgt, **kw)
    assert torch.equal(rgba.frames, tr.frames[:, :, :4]) and torch.equal(rgba.attention, tr.attention)
    assert PZ.same_bytes(rgba.metrics.stacked, tr.metrics.stacked)


# ---------------------------------------------------------------------------------------------
# Outside the support set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C,hidden", [("classic", 8, 200), ("graph", 33, 128)])
def test_unsupported_shapes_are_refused(dev, kind, C, hidden):
    """``forward``, ``rollout`` and ``trace`` raise GncaError, with and without grad, and the message
    names the real support set."""
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    from graph_neural_cellular_automata_amd._lib import GncaError
    torch.manual_seed(0)
    m = (NeuralCA(C, hidden) if kind == "classic" else NeuralCAGraph(C, hidden)).to(dev)
    x = torch.rand(2, C, 8, 8, device=dev)
    calls = [lambda: m(x), lambda: m.rollout(x, 2), lambda: m.trace(x, 2)]
    for grad in (False, True):
        for call in calls:
            with torch.set_grad_enabled(grad), pytest.raises(GncaError) as e:
                call()
            msg = str(e.value)
            assert "4 <= C <= 32" in msg and "hidden <= 128" in msg and "13 <= C <= 16" in msg, msg
