"""GPU checks of checkpointed BPTT (``checkpoint_every``, GNCA_SCHED_CHECKPOINT): the tape keeps every
k-th state and the backward re-runs the forward one segment at a time.

The forward is bitwise deterministic (fixed-order fp64 GroupNorm sums, counter RNG or recorded fire
inputs) and the checkpointed backward makes the plain backward's step calls in the plain backward's
order on re-run states, so EVERY comparison here is equality of bytes (``tests/poison.same_bytes``) against
the same call without ``checkpoint_every``: x_final, the losses, x.grad and every parameter gradient.
No tolerance appears in this file.

Shapes: the three bptt_* fixtures (B=3, 16 channels, 32x32, T=6, nsteps 6/4/5, recorded fire masks;
classic, torus, zero-pad), tests/shape_class_cases.py's p5 (classic, C=5, 11x13) and p6 (torus, C=6,
12x16) at T=7 (a prime length: the last segment is ragged), and bptt_long_cases' torus40 at the trainer's
length.  The guarded-buffer test comes first in the file: a mistake in the slot arithmetic lands in a
canary guard.
"""
import pytest
import torch

from tests import poison as PZ
from tests.test_gpu_rollout_objective import (FIXTURES, KINDS, KNOBS, Setup, _cot, _g_losses, _grads, _loss_kwargs,
                                              _segment_kwargs, run_fused, setup_of)

pytestmark = pytest.mark.gpu

CLASSIC, TORUS, ZEROPAD = FIXTURES
SHAPES = {CLASSIC: 6, TORUS: 6, ZEROPAD: 6, "p5": 7, "p6": 7}     # setup -> T


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _setup(name):
    return setup_of(name, SHAPES[name])


def assert_same(tag, got, ref, keys=("x_final", "losses", "gx")):
    for k in keys:
        if k in ref:
            assert PZ.same_bytes(got[k], ref[k]), (tag, k, PZ.diff(got[k], ref[k]))
    assert set(got["grads"]) == set(ref["grads"]), (tag, sorted(got["grads"]), sorted(ref["grads"]))
    for k, r in ref["grads"].items():
        assert PZ.same_bytes(got["grads"][k], r), (tag, k, PZ.diff(got["grads"][k], r))


# ---------------------------------------------------------------------------------------------
# 1. The raw entry points on poisoned, guarded buffers (first: see the module docstring)
# ---------------------------------------------------------------------------------------------
def _bound_call(s, dev, kind, record, every, recompute=False):
    """``test_gpu_rollout_objective._bound_call`` with a checkpointed schedule."""
    from graph_neural_cellular_automata_amd import step as S
    from graph_neural_cellular_automata_amd.modules import _stepper as M
    model = s.make_model(dev)
    x = s.x.to(dev)
    B, C, H, W = x.shape
    graph = getattr(model, "graph", None)
    kw = _segment_kwargs(s, dev, 0, s.T, recompute)
    sched = S.build_schedule(steps=s.T, B=B, H=H, W=W, device=dev, fire_rate=kw["fire_rate"],
                             message_gain=kw.get("message_gain"), nsteps=kw.get("nsteps"), fire=kw.get("fire"),
                             offsets=kw.get("offsets"), recompute=recompute, checkpoint_every=every)
    desc, w, keep, tensors = M._rollout_desc(model, x, s.T, graph, getattr(model, "hidden_only", False), sched)
    target = s.target.to(dev)
    target = (target[None] if target.dim() == 3 else target).contiguous()
    knobs = KNOBS if kind == "masked" else None
    want = {n: p for n, p in model.named_parameters() if n in S.GRAD_FIELDS}
    return model, S.RolloutCall(desc, sched), (lambda tgt: S.RolloutTaps(desc, record, kind, knobs, tgt)), w, \
        keep, want, target


@pytest.mark.parametrize("recompute", [False, True], ids=["tape", "recompute"])
@pytest.mark.parametrize("every", [2, "T"])
@pytest.mark.parametrize("name,record", [(TORUS, [2, 3, 6]), (ZEROPAD, [1, 4]), ("p5", [3, 5, 7])],
                         ids=["torus", "zeropad", "p5"])
def test_entry_points_on_poisoned_guarded_buffers(dev, name, record, every, recompute):
    """gnca_rollout_fwd_f32 / gnca_rollout_bwd_f32 and gnca_rollout_fwd_taps / gnca_rollout_bwd_taps (with
    and without gy) on a tape and workspaces of exactly the queried sizes, between canary guards, under the
    zero, NaN and random fills: no guard is touched, every output is written whole and depends on no
    buffer's prior contents, the tape and x_final are not modified by the backward, and the outputs are
    those of the plain schedule."""
    s = _setup(name)
    k = s.T if every == "T" else every
    kind = "masked" if name == ZEROPAD else "premult"
    model, call, make_taps, w, keep, want, target = _bound_call(s, dev, kind, record, k, recompute)
    x0, gy0, gl0 = s.x.to(dev), _cot(s).to(dev), _g_losses(len(record), s.x.shape[0], dev)
    mem = call.memory()
    state = -(-x0.numel() * 4 // 256) * 256
    assert mem["tape"] == -(-s.T // k) * state

    def run(P):
        x, gl, tgt, gy = P.guard(x0), P.guard(gl0), P.guard(target), P.guard(gy0)
        taps = make_taps(tgt)
        x_final, tape = call.forward(w, x, want_tape=True)
        assert tape.numel() == mem["tape"]
        tape0, xf0 = tape.clone(), x_final.clone()
        gx, grads = call.backward(w, tape, gy, want=want)
        xf_t, tape_t, losses, alive = call.forward_taps(w, taps, x, want_tape=True)
        tape_t0 = tape_t.clone()     # (its own copy: the padding behind each anchor keeps the fill)
        gx_t, grads_t = call.backward_taps(w, taps, tape_t, xf_t, gy, gl, alive, want=want)
        gx_n, grads_n = call.backward_taps(w, taps, tape_t, xf_t, None, gl, alive, want=want)
        xf_nt, none, losses_nt, _ = call.forward_taps(w, taps, x, want_tape=False)
        torch.cuda.synchronize()
        assert none is None
        assert PZ.same_bytes(tape, tape0) and PZ.same_bytes(tape_t, tape_t0), "a backward wrote the tape"
        n = x0.numel() * 4           # the anchors themselves are the same states
        for j in range(mem["tape"] // state):
            assert PZ.same_bytes(tape_t[j * state:j * state + n], tape0[j * state:j * state + n]), f"anchor {j}"
        assert PZ.same_bytes(x_final, xf0) and PZ.same_bytes(xf_t, xf0) and PZ.same_bytes(xf_nt, xf0)
        assert PZ.same_bytes(losses_nt, losses)
        outs = dict(x_final=x_final, gx=gx, losses=losses, gx_taps=gx_t, gx_no_gy=gx_n)
        for tag, g in (("f32", grads), ("taps", grads_t), ("no_gy", grads_n)):
            outs.update({f"grad:{tag}:{n}": v for n, v in g.items()})
        if alive is not None:
            outs["alive_count"] = alive
        return outs

    outs = PZ.run_fills(run, f"checkpoint-{name}-{every}-{recompute}")
    for n, v in outs.items():
        assert torch.isfinite(v.float()).all(), n
    # the plain schedule's outputs (no poison: those entry points have their own guarded tests)
    _, plain, make_taps0, w0, keep0, want0, _ = _bound_call(s, dev, kind, record, None, recompute)
    taps = make_taps0(target)
    xf, tape = plain.forward(w0, x0, want_tape=True)
    losses, alive = plain.tap_losses(taps, tape, xf)
    ref = dict(x_final=xf, losses=losses, gx=plain.backward(w0, tape, gy0, want=want0)[0],
               gx_taps=plain.backward_taps(w0, taps, tape, xf, gy0, gl0, alive)[0],
               gx_no_gy=plain.backward_taps(w0, taps, tape, xf, None, gl0, alive)[0])
    torch.cuda.synchronize()
    for n, v in ref.items():
        assert PZ.same_bytes(outs[n], v), (n, PZ.diff(outs[n], v))


# ---------------------------------------------------------------------------------------------
# 2. rollout() with grad
# ---------------------------------------------------------------------------------------------
_PLAIN = {}


def run_rollout(s, dev, recompute=False, **extra):
    model = s.make_model(dev)
    leaf = s.x.to(dev).requires_grad_(True)
    kw = _segment_kwargs(s, dev, 0, s.T, recompute)
    kw.update(extra)
    out = model.rollout(leaf, s.T, **kw)
    (out * _cot(s).to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(x_final=out.detach(), gx=leaf.grad, grads=_grads(model))


def _plain_rollout(name, recompute, dev):
    key = (name, recompute)
    if key not in _PLAIN:
        _PLAIN[key] = run_rollout(_setup(name), dev, recompute)
    return _PLAIN[key]


@pytest.mark.parametrize("recompute", [False, True], ids=["tape", "recompute"])
@pytest.mark.parametrize("every", [1, 2, 3, 4, "T-1", "T", "T+3"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_rollout_gradients_are_bitwise_the_plain_tapes(dev, name, every, recompute):
    s = _setup(name)
    k = {"T-1": s.T - 1, "T": s.T, "T+3": s.T + 3}.get(every, every)
    got = run_rollout(s, dev, recompute, checkpoint_every=k)
    assert got["grads"], "no parameter gradient came back"
    assert_same(f"{s.name} k={k} recompute={recompute}", got, _plain_rollout(name, recompute, dev))


# ---------------------------------------------------------------------------------------------
# 3. rollout_objective(): where the taps fall, which cotangents arrive
# ---------------------------------------------------------------------------------------------
# k = 3: the anchors are S_0, S_3 (and S_6 of p6's T = 7); segments [0,3), [3,6), [6,7)
RECORDS = {"anchor": [3], "inside": [4], "segment-last": [5], "first": [1], "at-T": None, "mixed": [2, 3, 5],
           "mixed-and-T": None}
_FUSED = {}


def _record(place, T):
    return {"at-T": [T], "mixed-and-T": [1, 3, 4, T]}.get(place) or RECORDS[place]


def _plain_fused(name, kind, record, use, recompute, dev, **extra):
    key = (name, kind, tuple(record) if record else None, use, recompute, tuple(sorted(extra.items())))
    if key not in _FUSED:
        _FUSED[key] = run_fused(_setup(name), dev, kind, record=record, use=use, recompute=recompute, **extra)
    return _FUSED[key]


@pytest.mark.parametrize("use", ["losses", "final", "both"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("place", list(RECORDS))
@pytest.mark.parametrize("name", [TORUS, "p6"])
def test_objective_tap_placements(dev, name, place, kind, use):
    """``use="losses"`` with the last tap before T is the taps-only backward (no gy): the segments after
    the last tap are neither re-run nor walked, and the first injection reads a re-run state."""
    s = _setup(name)
    record = _record(place, s.T)
    got = run_fused(s, dev, kind, record=record, use=use, checkpoint_every=3)
    assert got["steps"] == record
    assert_same(f"{s.name} {place} {kind} {use}", got, _plain_fused(name, kind, record, use, False, dev))


@pytest.mark.parametrize("recompute", [False, True], ids=["tape", "recompute"])
@pytest.mark.parametrize("every", [1, 2, 4, 7, 10])
@pytest.mark.parametrize("kind", KINDS)
def test_objective_every_step_tapped(dev, kind, every, recompute):
    s = _setup("p6")
    got = run_fused(s, dev, kind, every=1, use="both", recompute=recompute, checkpoint_every=every)
    assert got["steps"] == list(range(1, s.T + 1))
    ref = _plain_fused("p6", kind, None, "both", recompute, dev, every=1)
    assert_same(f"{s.name} every=1 k={every} {kind}", got, ref)


@pytest.mark.parametrize("use", ["losses", "both"])
@pytest.mark.parametrize("kind", KINDS)
def test_objective_more_taps_than_one_kernel_argument_chunk(dev, kind, use):
    from graph_neural_cellular_automata_amd import _lib as L
    T = L.TAP_CHUNK + 8
    s = setup_of("p5", T)
    record = list(range(1, T))          # more than one chunk, and the last tap before T
    assert len(record) > L.TAP_CHUNK
    got = run_fused(s, dev, kind, record=record, use=use, checkpoint_every="auto")
    ref = run_fused(s, dev, kind, record=record, use=use)
    assert_same(f"{s.name} {kind} {use}", got, ref)


# ---------------------------------------------------------------------------------------------
# 4. Fire modes: the re-run must regenerate the forward's masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recompute", [False, True], ids=["tape", "recompute"])
@pytest.mark.parametrize("mode", ["hash", "rand_f32"])
def test_fire_modes(dev, mode, recompute):
    s = _setup(TORUS)
    if mode == "hash":      # counter RNG: no recorded masks, rng_step = t
        v = Setup(**dict(s.__dict__, fire=None, rates=[0.5] * s.T))
        extra = dict(seed=1234, sample_base=5)
    else:                   # the uniforms themselves, compared with the rate in the kernel
        g = torch.Generator().manual_seed(77)
        v = Setup(**dict(s.__dict__, fire=torch.rand(s.fire.shape, generator=g), rates=[0.5] * s.T))
        extra = {}
    for k in (2, 4):
        got = run_fused(v, dev, "premult", record=[2, 5], use="both", recompute=recompute, checkpoint_every=k, **extra)
        ref = run_fused(v, dev, "premult", record=[2, 5], use="both", recompute=recompute, **extra)
        assert_same(f"{mode} k={k}", got, ref)
        assert_same(f"{mode} k={k} rollout()", run_rollout(v, dev, recompute, checkpoint_every=k, **extra),
                    run_rollout(v, dev, recompute, **extra))
    # the masks matter: another seed / other uniforms give another state
    if mode == "hash":
        other = run_rollout(v, dev, recompute, checkpoint_every=2, seed=4321, sample_base=5)
        assert not PZ.same_bytes(other["x_final"], ref["x_final"])


# ---------------------------------------------------------------------------------------------
# 5. The trainer's length
# ---------------------------------------------------------------------------------------------
def test_trainer_length_rollout_with_auto(dev):
    """bptt_long_cases' torus40 (B=4, 40x40, T=72, nsteps 72/48/61/55, min_steps=48, hash masks) with
    ``checkpoint_every="auto"`` (k = 9: 8 anchors) against the plain rollout the long-BPTT tests use."""
    from tests import bptt_long_cases as BL
    from tests.test_gpu_bptt_long import _inputs, _module_for, _rollout
    name = "torus40"
    k, c = BL.CASES[name], BL.fixture(name)
    out0, gx0, grads0 = _rollout(name, dev)
    for recompute in (False, True):
        model = _module_for(c, dev)
        x, gy, nst = _inputs(name, dev)
        offs, gains = BL.schedule(name)
        leaf = x.requires_grad_(True)
        kw = dict(fire_rate=BL.FIRE_RATE, seed=BL.FIRE_SEED, nsteps=nst, min_steps=k["min_steps"], recompute=recompute,
                  checkpoint_every="auto")
        if c.meta["graph"]:
            kw.update(message_gain=gains, offsets=offs)
        mem = model.rollout_memory(leaf, k["T"], **kw)
        assert mem["tape"] == 8 * (-(-leaf.numel() * 4 // 256) * 256)
        out = model.rollout(leaf, k["T"], **kw)
        (out * gy).sum().backward()
        torch.cuda.synchronize()
        assert_same(f"{name} auto recompute={recompute}", dict(x_final=out.detach(), gx=leaf.grad, grads=_grads(model)),
                    dict(x_final=out0, gx=gx0, grads=grads0))


# ---------------------------------------------------------------------------------------------
# 6. No grad, repeatability, error paths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_without_grad_records_no_tape(dev, kind, monkeypatch):
    from graph_neural_cellular_automata_amd import step as S
    s = _setup(TORUS)
    ref = _plain_fused(TORUS, kind, [2, 4, 6], "losses", False, dev)
    model = s.make_model(dev)
    seen = []
    real = S.RolloutCall.forward_taps
    monkeypatch.setattr(S.RolloutCall, "forward_taps",
                        lambda self, w, taps, x, want_tape: seen.append(want_tape) or real(self, w, taps, x, want_tape))
    monkeypatch.setattr(S.RolloutCall, "forward", lambda *a, **k: pytest.fail("a tape was recorded"))
    with torch.no_grad():
        res = model.rollout_objective(s.x.to(dev), s.T, s.target.to(dev), record=[2, 4, 6], checkpoint_every=3,
                                      **_loss_kwargs(kind), **_segment_kwargs(s, dev, 0, s.T))
    assert seen == [False]
    assert not res.losses.requires_grad and not res.x_final.requires_grad
    assert PZ.same_bytes(res.x_final, ref["x_final"]) and PZ.same_bytes(res.losses, ref["losses"])


def test_rollout_without_grad_ignores_the_argument(dev):
    s = _setup(ZEROPAD)
    model = s.make_model(dev)
    with torch.no_grad():
        a = model.rollout(s.x.to(dev), s.T, checkpoint_every=2, **_segment_kwargs(s, dev, 0, s.T))
        b = model.rollout(s.x.to(dev), s.T, **_segment_kwargs(s, dev, 0, s.T))
    assert PZ.same_bytes(a, b) and PZ.same_bytes(a, _plain_rollout(ZEROPAD, False, dev)["x_final"])


@pytest.mark.parametrize("name", [ZEROPAD, "p6"])
def test_two_checkpointed_runs_are_bitwise_equal(dev, name):
    s = _setup(name)
    a = run_fused(s, dev, "masked", every=2, use="both", checkpoint_every=2)
    b = run_fused(s, dev, "masked", every=2, use="both", checkpoint_every=2)
    assert_same(name, a, b)
    assert_same(name + " rollout()", run_rollout(s, dev, checkpoint_every=4), run_rollout(s, dev, checkpoint_every=4))


def test_second_backward_and_inplace_update_still_raise(dev):
    s = _setup(TORUS)
    got = run_fused(s, dev, "premult", record=[3], checkpoint_every=2)
    with pytest.raises(RuntimeError, match="second time"):
        got["res"].losses.sum().backward()
    got = run_fused(s, dev, "premult", record=[3], backward=False, checkpoint_every=2)
    with torch.no_grad():
        got["model"].update_net[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        got["res"].losses.sum().backward()
    model = s.make_model(dev)
    leaf = s.x.to(dev).requires_grad_(True)
    out = model.rollout(leaf, s.T, checkpoint_every=2, **_segment_kwargs(s, dev, 0, s.T))
    out.sum().backward()
    with pytest.raises(RuntimeError, match="second time"):
        out.sum().backward()
    out = model.rollout(leaf, s.T, checkpoint_every=2, **_segment_kwargs(s, dev, 0, s.T))
    with torch.no_grad():
        model.update_net[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


def test_bad_checkpoint_every_on_the_device(dev):
    s = _setup(TORUS)
    model, x = s.make_model(dev), s.x.to(dev)
    for bad in (0, -3, 2.5, True, "sqrt"):
        with pytest.raises(ValueError, match="checkpoint_every"):
            model.rollout(x, s.T, checkpoint_every=bad, **_segment_kwargs(s, dev, 0, s.T))
        with pytest.raises(ValueError, match="checkpoint_every"):
            model.rollout_objective(x, s.T, s.target.to(dev), checkpoint_every=bad, **_segment_kwargs(s, dev, 0, s.T))


# ---------------------------------------------------------------------------------------------
# 7. The stream contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,record", [(TORUS, [2, 3, 5]), ("p6", [4, 7])], ids=["torus-2,3,5", "p6-4,7"])
def test_entry_points_on_the_three_stream_legs(dev, name, record, kind):
    """Eager, side stream with delayed inputs, capture and replay twice (tests/streams.py) of
    gnca_rollout_fwd_taps + gnca_rollout_bwd_taps with ``checkpoint_every=2``, with and without gy."""
    from tests import streams as ST
    s = _setup(name)
    model, call, make_taps, w, keep, want, target = _bound_call(s, dev, kind, record, 2)
    R, B = len(record), s.x.shape[0]

    def inputs(seed):
        g = torch.Generator().manual_seed(seed)
        x = s.x.clone()
        x[:, 4:] += 0.1 * torch.randn(x[:, 4:].shape, generator=g)
        return dict(x=x.to(dev), gy=torch.randn(s.x.shape, generator=g).to(dev),
                    g_losses=torch.randn(R, B, generator=g).to(dev),
                    target=(target.cpu() * torch.rand(target.shape, generator=g)).to(dev))

    def run(bufs):
        taps = make_taps(bufs["target"])
        x_final, tape, losses, alive = call.forward_taps(w, taps, bufs["x"], want_tape=True)
        gx, grads = call.backward_taps(w, taps, tape, x_final, bufs["gy"], bufs["g_losses"], alive, want=want)
        gx2, _ = call.backward_taps(w, taps, tape, x_final, None, bufs["g_losses"], alive)
        return dict(x_final=x_final, losses=losses, gx=gx, gx_no_gy=gx2, **{f"grad:{k}": v for k, v in grads.items()})

    ST.run(ST.Case(f"checkpoint-{name}-{kind}", (inputs(1), inputs(2)), run))
