"""GPU checks of model.rollout_objective(): losses at intermediate steps of one rollout, read from its
tape (gnca_rollout_tap_loss), and their gradients added to the running cotangent of one BPTT
(gnca_rollout_bwd_taps).

Shapes: the three bptt_* fixtures (B=3, 16 channels, 32x32, T=6, nsteps 6/4/5, explicit fire masks;
classic, torus, zero-pad) and tests/shape_class_cases.py's p5 (classic, C=5, 11x13: one sample's 143
cells are less than one workgroup) and p6 (torus, C=6, 12x16).

Bounds.
* Float64 reference (a tapped variant of tests/grad_helpers.bptt_oracle, below): loss values 1e-5
  relative (premult, test_gpu_grad.py) and 1e-6 * sum|components| (masked, test_gpu_masked_loss.py); gx
  and every weight gradient 5e-5 * max|ref| + 1e-9 (test_rollout_matches_reference).
* The chain of rollout() segments with a loss on each segment's end: x_final, losses and gx bitwise
  (the same kernels on the same states; the tap's gradient is the loss backward's fp32 value and joins
  the cotangent with the one rounded add autograd's accumulation makes); each weight gradient within
  RT * max|chain| + AT (RT, AT of test_gpu_rollout_bptt.py: the chain reduces once per segment and sums
  the segments in fp32, the fused call reduces once); bitwise too with the single tap record=[T].
* Both outputs used: the backward is linear in its cotangents, so gx(both) and gx(losses) + gx(x_final)
  are the same number in exact arithmetic.  In fp32 they are not within the one rounding of the add that
  forms the sum: the three passes round differently at every one of their steps, and the figure
  measured on the MI355X is 2 to 5 units in the last place of max|sum| (printed before the assertion).
  The bound is a rounding model of the three passes, not the oracle's tolerance.  One element of a
  step's VJP is the cotangent plus D products accumulated in fp32, D = 27 (the three 3x3 perception
  adjoints) + hidden + C (the two layers of the update MLP): D + 1 roundings per element and step,
  3 T (D + 1) for the three passes of T steps, each at most half a unit in the last place of the largest
  cotangent element, ulp = 2^-23 max|gx| (every term is bounded by the cotangent's scale: the update
  branch carries the factor update_gain = 0.05, so this over-counts it).  Independent roundings add in
  quadrature (the probabilistic model of Higham and Mary, 2019, with constant 1), plus the add itself:
  |gx(both) - (gx(losses) + gx(x_final))| <= (sqrt(3 T (D + 1)) / 2 + 1) ulp,
  29 ulp for the fixtures (T = 6, hidden = 128, C = 16; 3.4e-6 max|gx|), some 40 times tighter than
  the gradient bound against the float64 reference.
"""
import numpy as np
import pytest
import torch

from tests import loss_ref as LR
from tests import shape_class_cases as SC
from tests.golden_io import Case, bptt_case_names
from tests.grad_helpers import premult_loss_and_grad

pytestmark = pytest.mark.gpu

RT, AT = 2e-5, 1e-6
KNOBS = (0.2, 5e-5, 1e-3, 2e-4)          # alpha_thr, lam_area, lam_bg_alpha, lam_bg_rgb (the graph trainer's)
KINDS = ("premult", "masked")
TAPS = (2, 4, 6)
FIXTURES = bptt_case_names()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------
# Setups: a model, a state, a target and a per-step schedule with explicit fire masks
# ---------------------------------------------------------------------------------------------
class Setup:
    """name, make_model(dev), x [B,C,H,W], target, T, rates [T], nsteps [B] or None, fire uint8
    [T,B,1,H,W] or None, gains [T] or None, offsets [T][k] or None (CPU tensors / lists)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def sliced(self, B=None, T=None):
        B = self.x.shape[0] if B is None else B
        T = self.T if T is None else T
        return Setup(name=f"{self.name}[B={B},T={T}]", make_model=self.make_model, x=self.x[:B].clone(),
                     target=self.target if self.target.dim() == 3 else self.target[:B].clone(), T=T,
                     rates=self.rates[:T], nsteps=None if self.nsteps is None else self.nsteps[:B].clamp(max=T),
                     fire=None if self.fire is None else self.fire[:T, :B].clone(),
                     gains=None if self.gains is None else self.gains[:T],
                     offsets=None if self.offsets is None else self.offsets[:T])


_SETUPS = {}


def _fixture_setup(name):
    from tests.test_gpu_rollout_bptt import _module_for
    c = Case(name)
    T = int(c.meta["rollout"])
    graph = c.meta["graph"]
    return Setup(name=name, case=c, make_model=lambda dev: _module_for(c, dev), x=torch.from_numpy(c.x_in),
                 target=torch.from_numpy(c.target), T=T, rates=[float(v) for v in c.fire_rates],
                 nsteps=torch.from_numpy(c.steps.astype(np.int32)),
                 fire=torch.from_numpy(np.ascontiguousarray(c.fire_mask)),
                 gains=[c.meta["message_gain"] * float(u) for u in c.use_graph] if graph else None,
                 offsets=[c.chosen(t) for t in range(T)] if graph else None)


def _shape_setup(name, T):
    c = SC.CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    g = torch.Generator().manual_seed(900 + SC.seed(name))
    fire = (torch.rand(T, B, 1, H, W, generator=g) <= 0.5).to(torch.uint8)
    target = torch.rand(B, 4, H, W, generator=g)          # one target per sample: a non-zero target stride
    target[:, 3, :, : W // 2] *= 0.15                     # dead target cells on the left half
    nsteps = torch.tensor([T, max(T - 2, 1), max(T - 1, 1)][:B], dtype=torch.int32)
    graph = c["graph"]
    return Setup(name=f"{name}-T{T}", make_model=lambda dev: SC.model(name, dev), x=SC.state(name), target=target,
                 T=T, rates=[0.5] * T, nsteps=nsteps, fire=fire,
                 gains=[c["msg"] * (t % 3 != 1) for t in range(T)] if graph else None,
                 offsets=SC.offsets(name, T) if graph else None)


def setup_of(name, T=6):
    key = (name, T)
    if key not in _SETUPS:
        _SETUPS[key] = _fixture_setup(name) if name.startswith("bptt_") else _shape_setup(name, T)
    return _SETUPS[key]


def _segment_kwargs(s, dev, lo, hi, recompute=False):
    kw = dict(fire_rate=s.rates[lo:hi], recompute=recompute)
    if s.fire is not None:
        kw["fire"] = s.fire[lo:hi].contiguous().to(dev)
    if s.nsteps is not None:
        kw["nsteps"] = (s.nsteps - lo).clamp(min=0, max=hi - lo).to(dev)
    if s.gains is not None:
        kw.update(message_gain=s.gains[lo:hi], offsets=s.offsets[lo:hi])
    return kw


def _loss_kwargs(kind):
    return dict(loss=kind) if kind == "premult" else dict(
        loss=kind, alpha_thr=KNOBS[0], lam_area=KNOBS[1], lam_bg_alpha=KNOBS[2], lam_bg_rgb=KNOBS[3])


def _cot(s):
    g = torch.Generator().manual_seed(31)
    return torch.randn(s.x.shape, generator=g)


def _scalar(losses, x_final, cot, use):
    """The objective: ``use`` in 'losses', 'both', 'final'."""
    terms = []
    if use in ("losses", "both"):
        terms.append(losses.mean())
    if use in ("both", "final"):
        terms.append((x_final * cot).sum())
    return sum(terms[1:], terms[0])


def _grads(model):
    return {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


def run_fused(s, dev, kind, *, record=None, every=1, recompute=False, use="losses", backward=True, **extra):
    model = s.make_model(dev)
    leaf = s.x.to(dev).requires_grad_(True)
    kw = _segment_kwargs(s, dev, 0, s.T, recompute)
    kw.update(extra)
    res = model.rollout_objective(leaf, s.T, s.target.to(dev), every=every, record=record, **_loss_kwargs(kind), **kw)
    out = dict(res=res, x_final=res.x_final.detach(), losses=res.losses.detach(), steps=res.steps, model=model,
               leaf=leaf)
    if backward:
        _scalar(res.losses, res.x_final, _cot(s).to(dev), use).backward()
        torch.cuda.synchronize()
        out.update(gx=leaf.grad, grads=_grads(model))
    return out


def run_chain(s, dev, kind, taps, *, recompute=False, use="losses"):
    """The same rollout as segments of model.rollout() with a loss node on each segment's end."""
    from graph_neural_cellular_automata_amd.loss import loss_premult_rgba, masked_loss
    model = s.make_model(dev)
    leaf = s.x.to(dev).requires_grad_(True)
    target = s.target.to(dev)
    state, lo, losses = leaf, 0, []
    for t in list(taps) + ([s.T] if taps[-1] < s.T else []):
        state = model.rollout(state, t - lo, **_segment_kwargs(s, dev, lo, t, recompute))
        lo = t
        if t in taps:
            losses.append(loss_premult_rgba(state[:, :4], target) if kind == "premult"
                          else masked_loss(state[:, :4], target, *KNOBS))
    losses = torch.stack(losses)
    _scalar(losses, state, _cot(s).to(dev), use).backward()
    torch.cuda.synchronize()
    return dict(x_final=state.detach(), losses=losses.detach(), gx=leaf.grad, grads=_grads(model))


def check_against_chain(tag, got, ref, weights_bitwise=False):
    assert torch.equal(got["x_final"], ref["x_final"]), tag
    assert torch.equal(got["losses"], ref["losses"]), (tag, got["losses"], ref["losses"])
    assert torch.equal(got["gx"], ref["gx"]), (tag, float((got["gx"] - ref["gx"]).abs().max()))
    assert set(got["grads"]) == set(ref["grads"]), (tag, sorted(got["grads"]), sorted(ref["grads"]))
    for k, r in ref["grads"].items():
        err, scale = float((got["grads"][k] - r).abs().max()), float(r.abs().max())
        print(f"{tag} {k}: |fused - chain| = {err:.3e}, max|chain| = {scale:.3e}")
        assert torch.isfinite(got["grads"][k]).all(), (tag, k)
        if weights_bitwise:
            assert torch.equal(got["grads"][k], r), (tag, k, err)
        else:
            assert err <= RT * scale + AT, (tag, k, f"err={err:.3e} scale={scale:.3e}")


# ---------------------------------------------------------------------------------------------
# 1. The float64 reference: tests/grad_helpers.bptt_oracle with losses at the tapped steps
# ---------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_states(c):
    from oracle import nca_oracle as O
    key = (c.name, "fwd")
    if key not in _ORACLE:
        p = {k: v.astype(np.float64) if v.dtype.kind == "f" else v for k, v in c.weights.items()}
        x = c.x_in.astype(np.float64)
        T = int(c.meta["rollout"])
        base = c.cfg()
        tape, states = [], [x]
        for t in range(T):
            mask = c.active[t].astype(bool)
            cfg = dict(base, message_gain=base["message_gain"] if c.use_graph[t] else 0.0)
            fire = c.fire_mask[t][mask].astype(np.float64) if c.fire_rates[t] < 1.0 else None
            chosen = [tuple(int(v) for v in o) for o in c.offsets[t]]
            sub = x[mask]
            tape.append((sub, mask, cfg, chosen, fire))
            x = x.copy()
            x[mask] = O.nca_step(sub, p, cfg, chosen=chosen, fire_mask=fire)
            states.append(x)
        _ORACLE[key] = (p, tape, states)
    return _ORACLE[key]


def tapped_oracle(c, kind, taps):
    """Per-tap per-sample losses (and the masked kind's component sums) and the gradients of
    ``losses.mean()`` in float64: nca_step forward, nca_step_vjp backward, the loss gradients added at the
    tapped steps.  Computed once per (fixture, kind) and left unchanged."""
    from oracle import nca_oracle_vjp as V
    key = (c.name, kind, tuple(taps))
    if key in _ORACLE:
        return _ORACLE[key]
    p, tape, states = _oracle_states(c)
    T, B, R = len(tape), states[0].shape[0], len(taps)
    target = c.target.astype(np.float64)
    values, scales, tap_grad = {}, {}, {}
    for t in taps:
        st = states[t]
        g = np.zeros_like(st)
        if kind == "premult":
            rgba = np.concatenate([st[:, :3] * st[:, 3:4], st[:, 3:4]], 1)
            values[t] = ((rgba - target[None]) ** 2).mean(axis=(1, 2, 3))
            scales[t] = np.abs(values[t])
            g = premult_loss_and_grad(st, target)[1] / R          # (its gradient is that of the batch mean)
        else:
            m = LR.masked_loss(st[:, :4].astype(np.float32), c.target, *KNOBS, g=np.full(B, 1.0 / (R * B)))
            values[t] = m.value
            scales[t] = np.abs(m.primary) + np.abs(m.bg_alpha) + np.abs(m.bg_rgb) + np.abs(m.area)
            g[:, :4] = m.grad
        tap_grad[t] = g
    g = np.zeros_like(states[0])
    total = {}
    for t in range(T, 0, -1):
        if t in tap_grad:
            g = g + tap_grad[t]
        sub, mask, cfg, chosen, fire = tape[t - 1]
        gx, grads = V.nca_step_vjp(sub, p, cfg, g[mask], chosen=chosen, fire_mask=fire)
        g = g.copy()
        g[mask] = gx
        for k, v in grads.items():
            total[k] = total.get(k, 0) + v
    _ORACLE[key] = (values, scales, g, total)
    return _ORACLE[key]


_FUSED = {}


def _fused_fixture(name, kind, recompute, dev):
    key = (name, kind, recompute)
    if key not in _FUSED:
        _FUSED[key] = run_fused(setup_of(name), dev, kind, record=list(TAPS), recompute=recompute)
    return _FUSED[key]


@pytest.mark.parametrize("recompute", [False, True], ids=["tape", "recompute"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_matches_float64_reference(dev, name, kind, recompute):
    s = setup_of(name)
    values, scales, gx_ref, grads_ref = tapped_oracle(s.case, kind, TAPS)
    got = _fused_fixture(name, kind, recompute, dev)
    assert got["steps"] == list(TAPS) and got["losses"].shape == (len(TAPS), s.x.shape[0])
    assert got["losses"].dtype == torch.float32
    np.testing.assert_allclose(got["x_final"].cpu().numpy(), s.case.x_out_f64, rtol=0, atol=1e-4)
    losses = got["losses"].cpu().numpy().astype(np.float64)
    rel = 1e-5 if kind == "premult" else 1e-6
    for r, t in enumerate(TAPS):
        err = np.abs(losses[r] - values[t])
        print(f"{name} {kind} tap {t}: loss err / scale = {(err / scales[t]).max():.3e} (bound {rel:.0e})")
        assert (err <= rel * scales[t]).all(), (t, losses[r], values[t])
    ref = dict(grads_ref, gx=gx_ref)
    have = dict(got["grads"], gx=got["gx"])
    assert set(have) == set(ref), (sorted(have), sorted(ref))
    for k, r in ref.items():
        g = have[k].detach().cpu().numpy().reshape(r.shape).astype(np.float64)
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        print(f"{name} {kind} {k}: err={err:.3e} scale={scale:.3e} (bound {5e-5 * scale + 1e-9:.3e})")
        assert np.isfinite(g).all(), k
        assert err <= 5e-5 * scale + 1e-9, (k, f"err={err:.3e} scale={scale:.3e}")


# ---------------------------------------------------------------------------------------------
# 2. Against the chain of rollout() + loss nodes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recompute", [False, True], ids=["tape", "recompute"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_equals_the_chain(dev, name, kind, recompute):
    got = _fused_fixture(name, kind, recompute, dev)
    ref = run_chain(setup_of(name), dev, kind, TAPS, recompute=recompute)
    check_against_chain(f"{name} {kind}", got, ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_single_final_tap_is_the_chain_bitwise(dev, name, kind):
    """record=[T]: one rollout node and one loss node, the same launches in the same order."""
    s = setup_of(name)
    got = run_fused(s, dev, kind, record=[s.T])
    check_against_chain(f"{name} {kind} [T]", got, run_chain(s, dev, kind, [s.T]), weights_bitwise=True)


# ---------------------------------------------------------------------------------------------
# 3. Both outputs used
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_both_outputs_used(dev, name, kind):
    s = setup_of(name)
    both = run_fused(s, dev, kind, record=list(TAPS), use="both")
    check_against_chain(f"{name} {kind} both", both, run_chain(s, dev, kind, TAPS, use="both"))
    only_l = _fused_fixture(name, kind, False, dev)
    only_f = run_fused(s, dev, kind, record=list(TAPS), use="final")
    total = only_l["gx"] + only_f["gx"]
    C, hidden = s.x.shape[1], both["model"].update_net[0].weight.shape[0]
    D = 27 + hidden + C
    scale = max(float(g.abs().max()) for g in (both["gx"], only_l["gx"], only_f["gx"], total))
    n_ulp = (3 * s.T * (D + 1)) ** 0.5 / 2 + 1
    bound = n_ulp * 2.0 ** -23 * scale
    err = float((both["gx"] - total).abs().max())
    print(f"{name} {kind}: |gx(both) - (gx(losses) + gx(final))| = {err:.3e} = {err / (2.0 ** -23 * scale):.2f} ulp "
          f"of max|gx| = {scale:.3e} (bound {n_ulp:.1f} ulp = {bound:.3e})")
    assert err <= bound
    # a tap list whose last tap is before T, with both outputs: the steps after it run for g_final alone
    early = run_fused(s, dev, kind, record=[2, 4], use="both")
    check_against_chain(f"{name} {kind} both [2,4]", early, run_chain(s, dev, kind, [2, 4], use="both"))


@pytest.mark.parametrize("name", FIXTURES)
def test_final_cotangent_alone_is_rollouts_backward(dev, name):
    """``losses`` unused: the node gets no cotangent for it and runs gnca_rollout_bwd_f32's launches."""
    s = setup_of(name)
    got = run_fused(s, dev, "masked", record=list(TAPS), use="final")
    model = s.make_model(dev)
    leaf = s.x.to(dev).requires_grad_(True)
    out = model.rollout(leaf, s.T, **_segment_kwargs(s, dev, 0, s.T))
    (out * _cot(s).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(got["x_final"], out.detach()) and torch.equal(got["gx"], leaf.grad)
    ref = _grads(model)
    assert set(got["grads"]) == set(ref)
    for k in ref:
        assert torch.equal(got["grads"][k], ref[k]), k


# ---------------------------------------------------------------------------------------------
# 4. No cotangent for x_final, last tap before T
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_no_final_cotangent_last_tap_before_T(dev, name, kind):
    s = setup_of(name)
    got = run_fused(s, dev, kind, record=[2, 4], backward=False)
    node = got["res"].losses.grad_fn
    assert node is got["res"].x_final.grad_fn and node.tape is not None
    got["res"].losses.mean().backward(retain_graph=True)
    torch.cuda.synchronize()
    assert node.tape is None, "the tape outlives the backward"
    got.update(gx=got["leaf"].grad, grads=_grads(got["model"]))
    check_against_chain(f"{name} {kind} [2,4]", got, run_chain(s, dev, kind, [2, 4]))
    with pytest.raises(RuntimeError, match="second time"):
        got["res"].losses.mean().backward()


def test_inplace_weight_update_before_backward_raises(dev):
    s = setup_of(FIXTURES[0])
    got = run_fused(s, dev, "premult", record=[3], backward=False)
    with torch.no_grad():
        got["model"].update_net[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        got["res"].losses.sum().backward()


def test_schedule_arguments_are_validated_as_rollout_validates_them(dev):
    """The schedule's own checks (step.build_schedule) with the state on the device: ValueError, nothing
    launched."""
    s = setup_of(FIXTURES[1])
    model, x, target = s.make_model(dev), s.x.to(dev), s.target.to(dev)
    B, _, H, W = x.shape
    for bad in (dict(fire_rate=[0.5, 0.5]), dict(nsteps=torch.zeros(B, dtype=torch.int64, device=dev)),
                dict(nsteps=torch.zeros(B, dtype=torch.int32)), dict(fire=torch.zeros(s.T, B, 1, H, W - 1, device=dev)),
                dict(fire_rate=0.5, seed=1.5), dict(min_steps=-1), dict(offsets=[[(2, 0)]] * (s.T - 1)),
                dict(message_gain=[0.25] * (s.T - 1))):
        with pytest.raises(ValueError):
            model.rollout_objective(x, s.T, target, every=2, **bad)


@pytest.mark.parametrize("kind", KINDS)
def test_without_grad_returns_the_same_values(dev, kind):
    s = setup_of(FIXTURES[1])
    ref = _fused_fixture(FIXTURES[1], kind, False, dev)
    model = s.make_model(dev)
    with torch.no_grad():
        res = model.rollout_objective(s.x.to(dev), s.T, s.target.to(dev), record=list(TAPS), **_loss_kwargs(kind),
                                      **_segment_kwargs(s, dev, 0, s.T))
    assert not res.losses.requires_grad and not res.x_final.requires_grad
    assert torch.equal(res.x_final, ref["x_final"]) and torch.equal(res.losses, ref["losses"])
    for p in model.parameters():
        p.requires_grad_(False)
    res = model.rollout_objective(s.x.to(dev), s.T, s.target.to(dev), record=list(TAPS), **_loss_kwargs(kind),
                                  **_segment_kwargs(s, dev, 0, s.T))
    assert res.losses.grad_fn is None and torch.equal(res.losses, ref["losses"])


# ---------------------------------------------------------------------------------------------
# 5. Edge shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_sample_one_step_one_tap(dev, kind):
    s = setup_of(FIXTURES[2]).sliced(B=1, T=1)
    got = run_fused(s, dev, kind)
    assert got["steps"] == [1] and got["losses"].shape == (1, 1)
    check_against_chain(s.name, got, run_chain(s, dev, kind, [1]), weights_bitwise=True)


@pytest.mark.parametrize("kind", KINDS)
def test_every_step_tapped(dev, kind):
    s = setup_of(FIXTURES[1])
    got = run_fused(s, dev, kind, every=1)
    assert got["steps"] == [1, 2, 3, 4, 5, 6]
    check_against_chain(f"{s.name} every=1", got, run_chain(s, dev, kind, got["steps"]))


@pytest.mark.parametrize("kind", KINDS)
def test_more_taps_than_one_kernel_argument_chunk(dev, kind):
    from graph_neural_cellular_automata_amd import _lib as L
    T = L.TAP_CHUNK + 8
    s = setup_of("p5", T)
    got = run_fused(s, dev, kind, every=1)
    assert got["steps"] == list(range(1, T + 1)) and len(got["steps"]) > L.TAP_CHUNK
    check_against_chain(f"{s.name} every=1", got, run_chain(s, dev, kind, got["steps"]))


@pytest.mark.parametrize("use", ["losses", "both"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,taps", [("p5", [2, 4, 6]), ("p6", [1, 4, 6]), ("p6", [3, 5])],
                         ids=["p5-2,4,6", "p6-1,4,6", "p6-3,5"])
def test_padded_channel_shapes(dev, name, taps, kind, use):
    s = setup_of(name)
    got = run_fused(s, dev, kind, record=taps, use=use)
    check_against_chain(f"{s.name} {kind} {taps} {use}", got, run_chain(s, dev, kind, taps, use=use))


# ---------------------------------------------------------------------------------------------
# 6. Determinism and sharding
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [FIXTURES[2], "p6"])
def test_two_runs_are_bitwise_equal(dev, name):
    s = setup_of(name)
    a = run_fused(s, dev, "masked", every=2, use="both")
    b = run_fused(s, dev, "masked", every=2, use="both")
    for k in ("x_final", "losses", "gx"):
        assert torch.equal(a[k], b[k]), k
    assert set(a["grads"]) == set(b["grads"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [FIXTURES[1], "p5"])
def test_halves_with_sample_base_equal_the_whole_batch(dev, name, kind):
    """Hash fire masks (seed, fire_rate 0.5): samples [0,2) and [2,3) run alone with sample_base are the
    matching slices of the whole batch, bitwise, in losses and gx."""
    s = setup_of(name)
    hashed = Setup(**dict(s.__dict__, fire=None, rates=[0.5] * s.T))
    if hashed.target.dim() == 3:
        hashed.target = hashed.target[None].expand(s.x.shape[0], -1, -1, -1).contiguous()
    whole = run_fused(hashed, dev, kind, every=2, seed=77)
    for lo, hi in ((0, 2), (2, 3)):
        part = Setup(**dict(hashed.__dict__, x=hashed.x[lo:hi].clone(), target=hashed.target[lo:hi].clone(),
                            nsteps=hashed.nsteps[lo:hi].clone()))
        model = part.make_model(dev)
        leaf = part.x.to(dev).requires_grad_(True)
        res = model.rollout_objective(leaf, part.T, part.target.to(dev), every=2, seed=77, sample_base=lo,
                                      **_loss_kwargs(kind), **_segment_kwargs(part, dev, 0, part.T))
        # the whole batch's objective is the mean over R x 3 values: the same cotangent for each loss
        (res.losses.sum() / (res.losses.shape[0] * s.x.shape[0])).backward()
        torch.cuda.synchronize()
        assert torch.equal(res.x_final.detach(), whole["x_final"][lo:hi]), (lo, hi)
        assert torch.equal(res.losses.detach(), whole["losses"][:, lo:hi]), (lo, hi)
        assert torch.equal(leaf.grad, whole["gx"][lo:hi]), (lo, hi)


# ---------------------------------------------------------------------------------------------
# 7. Buffers and streams: the two entry points themselves
# ---------------------------------------------------------------------------------------------
def _bound_call(s, dev, kind, record, recompute=False):
    """(model, RolloutCall, target -> RolloutTaps, weights, keep, wanted gradients, target) of the setup, as
    rollout_objective binds them."""
    from graph_neural_cellular_automata_amd import step as S
    from graph_neural_cellular_automata_amd.modules import _stepper as M
    model = s.make_model(dev)
    x = s.x.to(dev)
    B, C, H, W = x.shape
    graph = getattr(model, "graph", None)
    kw = _segment_kwargs(s, dev, 0, s.T, recompute)
    sched = S.build_schedule(steps=s.T, B=B, H=H, W=W, device=dev, fire_rate=kw["fire_rate"],
                             message_gain=kw.get("message_gain"), nsteps=kw.get("nsteps"), fire=kw.get("fire"),
                             offsets=kw.get("offsets"), recompute=recompute)
    desc, w, keep, tensors = M._rollout_desc(model, x, s.T, graph, getattr(model, "hidden_only", False), sched)
    target = s.target.to(dev)
    target = (target[None] if target.dim() == 3 else target).contiguous()
    knobs = KNOBS if kind == "masked" else None
    want = {n: p for n, p in model.named_parameters() if n in S.GRAD_FIELDS}
    return model, S.RolloutCall(desc, sched), (lambda tgt: S.RolloutTaps(desc, record, kind, knobs, tgt)), w, \
        keep, want, target


def _g_losses(R, B, dev):
    g = torch.Generator().manual_seed(5)
    return torch.randn(R, B, generator=g).to(dev)


@pytest.mark.parametrize("gy_given", [True, False], ids=["gy", "no-gy"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,record", [(FIXTURES[2], [2, 4, 6]), (FIXTURES[1], [3, 6]), ("p5", [1, 4])],
                         ids=["zeropad-2,4,6", "torus-3,6", "p5-1,4"])
def test_entry_points_on_poisoned_guarded_buffers(dev, name, record, kind, gy_given):
    """Every element of losses, alive_count and gx is written and nothing outside them; gy, the target,
    the tape and x_final are not modified."""
    from tests import poison as PZ
    s = setup_of(name)
    model, call, make_taps, w, keep, want, target = _bound_call(s, dev, kind, record)
    x0, gy0, gl0 = s.x.to(dev), _cot(s).to(dev), _g_losses(len(record), s.x.shape[0], dev)

    def run(P):
        x, gl, tgt = P.guard(x0), P.guard(gl0), P.guard(target)
        gy = P.guard(gy0) if gy_given else None
        taps = make_taps(tgt)
        x_final, tape = call.forward(w, x, want_tape=True)
        tape0, xf0 = tape.clone(), x_final.clone()
        losses, alive = call.tap_losses(taps, tape, x_final)
        gx, grads = call.backward_taps(w, taps, tape, x_final, gy, gl, alive, want=want)
        torch.cuda.synchronize()
        assert PZ.same_bytes(tape, tape0), "the tape was written"
        assert PZ.same_bytes(x_final, xf0), "x_final was written"
        outs = dict(losses=losses, gx=gx, **{f"grad:{k}": v for k, v in grads.items()})
        if alive is not None:
            outs["alive_count"] = alive
        return outs

    outs = PZ.run_fills(run, f"objective-{name}-{kind}-{record}-{gy_given}")
    assert torch.isfinite(outs["losses"]).all() and torch.isfinite(outs["gx"]).all()
    if kind == "masked":
        tgt = target.expand(s.x.shape[0], -1, -1, -1)
        assert torch.equal(outs["alive_count"].long(), (tgt[:, 3] > KNOBS[0]).sum(dim=(1, 2)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,record", [(FIXTURES[1], [2, 4, 6]), ("p6", [3, 5])], ids=["torus-2,4,6", "p6-3,5"])
def test_entry_points_on_the_three_stream_legs(dev, name, record, kind):
    """Eager, side stream with delayed inputs, capture and replay (tests/streams.py): the tap list reaches
    the device in kernel arguments, so the captured graph holds no host copy.  (These cases are what
    found the accumulating rows dirty on replays while memset nodes zeroed them: DESIGN.md section 19.)"""
    from tests import streams as ST
    s = setup_of(name)
    model, call, make_taps, w, keep, want, target = _bound_call(s, dev, kind, record)
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
        x_final, tape = call.forward(w, bufs["x"], want_tape=True)
        losses, alive = call.tap_losses(taps, tape, x_final)
        gx, grads = call.backward_taps(w, taps, tape, x_final, bufs["gy"], bufs["g_losses"], alive, want=want)
        gx2, _ = call.backward_taps(w, taps, tape, x_final, None, bufs["g_losses"], alive)
        return dict(x_final=x_final, losses=losses, gx=gx, gx_no_gy=gx2, **{f"grad:{k}": v for k, v in grads.items()})

    ST.run(ST.Case(f"objective-{name}-{kind}", (inputs(1), inputs(2)), run))
