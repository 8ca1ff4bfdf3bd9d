"""GPU checks of model.rollout(): the whole-rollout forward (gnca_rollout_fwd_f32) and BPTT
(gnca_rollout_bwd_f32) against the reference's float64 autograd (the bptt_* fixtures) and against
the per-step path (gnca_step_masked_f32 / gnca_step_bwd_f32 once per step), which stays in the tree.

Bounds.  Fixtures: the project's own for this loop (test_gpu_grad.py: loss 1e-5 relative, final
state 1e-4, gradients 5e-5 * max|ref| + 1e-9).  Against the per-step path: x_final and gx do not
depend on the cross-step reduction order, so they are bitwise equal; a weight gradient G is compared
with R, the float64 sum of the per-step path's per-step gradients, within RT * max|R| + AT (RT, AT
of test_gpu_grad.py: one step's bound, applied to the fp32 accumulation over these T <= 4 steps;
each case prints the rollout's and the per-step path's own error against R before asserting).  The
bound at the trainers' lengths (24-72 steps of a state grown from a seed cell) is derived and
checked in tests/test_gpu_bptt_long.py, which also measures this one there: it holds with a factor
of a hundred to spare.
"""
import random

import numpy as np
import pytest
import torch

from tests.golden_io import Case, bptt_case_names

pytestmark = pytest.mark.gpu

RT, AT = 2e-5, 1e-6
SEED = 9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _module_for(case, dev):
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    m = case.meta
    if m["graph"]:
        model = NeuralCAGraph(n_channels=m["C"], update_hidden=m["Hd"], update_gain=m["update_gain"],
                              alpha_thr=m["alpha_thr"], use_groupnorm=m["use_groupnorm"],
                              message_gain=m["message_gain"], hidden_only=m["hidden_only"],
                              graph_d_model=m["d"], graph_attention_radius=m["r"],
                              graph_num_neighbors=m["K"], graph_alive_to_alive=m["alive_to_alive"],
                              graph_zero_padded_shift=m["zero_padded_shift"])
    else:
        model = NeuralCA(n_channels=m["C"], update_hidden=m["Hd"], update_gain=m["update_gain"],
                         alpha_thr=m["alpha_thr"], use_groupnorm=m["use_groupnorm"])
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in case.weights.items()}
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def _grads(model):
    return {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


# ---------------------------------------------------------------------------------------------
# 1 / 2: the reference's float64 autograd (bptt fixtures), saved tape and recompute
# ---------------------------------------------------------------------------------------------
_FIX = {}


def _fixture_run(name, dev, recompute):
    key = (name, recompute)
    if key in _FIX:
        return _FIX[key]
    c = Case(name)
    model = _module_for(c, dev)
    leaf = torch.from_numpy(c.x_in).to(dev).requires_grad_(True)
    T = int(c.meta["rollout"])
    assert np.array_equal(c.active, (c.steps[None, :] > np.arange(T)[:, None]).astype(np.uint8))
    kw = dict(fire_rate=[float(v) for v in c.fire_rates],
              nsteps=torch.from_numpy(c.steps.astype(np.int32)).to(dev),
              fire=torch.from_numpy(np.ascontiguousarray(c.fire_mask)).to(dev), recompute=recompute)
    if c.meta["graph"]:
        kw.update(message_gain=[c.meta["message_gain"] * float(u) for u in c.use_graph],
                  offsets=[c.chosen(t) for t in range(T)])
    state = model.rollout(leaf, T, **kw)
    target = torch.from_numpy(c.target).to(dev)
    rgba = torch.cat([state[:, :3] * state[:, 3:4], state[:, 3:4]], 1)
    loss = ((rgba - target[None]) ** 2).mean(dim=(1, 2, 3)).mean()
    loss.backward()
    torch.cuda.synchronize()
    got = dict(_grads(model), gx=leaf.grad)
    _FIX[key] = (c, float(loss.detach()), state.detach(), got)
    return _FIX[key]


@pytest.mark.parametrize("name", bptt_case_names())
def test_rollout_matches_reference(dev, name):
    """One rollout call and one backward on the recorded offsets, fire masks, rates, gains and
    per-sample step counts, against the reference's float64 autograd; no gradient key left out."""
    c, loss, state, got = _fixture_run(name, dev, False)
    assert abs(loss - float(c.loss_f64)) <= 1e-5 * abs(float(c.loss_f64))
    np.testing.assert_allclose(state.cpu().numpy(), c.x_out_f64, rtol=0, atol=1e-4)
    ref = dict(c.grads(), gx=c.gx_f64)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, r in ref.items():
        g = got[k].detach().cpu().numpy().reshape(r.shape).astype(np.float64)
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        print(f"{name} {k}: err={err:.3e} scale={scale:.3e}")
        assert np.isfinite(g).all(), k
        assert err <= 5e-5 * scale + 1e-9, (k, f"err={err:.3e} scale={scale:.3e}")


@pytest.mark.parametrize("name", bptt_case_names())
def test_rollout_recompute_is_bitwise(dev, name):
    """recompute=True (the tape keeps states only) gives the saved-tape run's bits."""
    _, _, state, got = _fixture_run(name, dev, False)
    _, _, state_r, got_r = _fixture_run(name, dev, True)
    assert torch.equal(state, state_r)
    assert set(got) == set(got_r)
    for k in got:
        assert torch.equal(got[k], got_r[k]), k


# ---------------------------------------------------------------------------------------------
# 3 / 4 / 5: against the per-step path
# ---------------------------------------------------------------------------------------------
def _alt(B):
    return [3 if b % 2 == 0 else 1 for b in range(B)]


# name -> (weights fixture, B, H, W, T, nsteps, gains (x message_gain), min_steps)
SHAPES = {
    "torus_b8_72": ("grad_graph_torus_latest_grown_b2_40", 8, 72, 72, 4, [4, 1, 3, 0, 4, 2, 4, 1], [1, 0, 0, 1], 0),
    "zeropad_b6_40": ("grad_graph_zeropad_latest_grown_b2_40", 6, 40, 40, 4, [4, 2, 0, 3, 4, 1], [1, 1, 1, 1], 0),
    "classic_nogn_20x22": ("grad_classic_c12_hd48_nogn_b2_20", 2, 20, 22, 3, [3, 2], None, 0),
    "c32_r5_k16_32": ("grad_graph_torus_c32_r5_k16_b1_32", 2, 32, 32, 3, [3, 1], [1, 0, 1], 0),
    "torus_b104_72_full1": ("grad_graph_torus_latest_grown_b2_40", 104, 72, 72, 3, _alt(104), [1, 0, 1], 1),
}


def _inputs(case, B, H, W, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    C = case.meta["C"]
    x = torch.rand(B, C, H, W, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, C - 4, H, W, device=dev, generator=g)
    gy = torch.randn(B, C, H, W, device=dev, generator=g)
    return x, gy


def _schedule(case, T, gains):
    random.seed(21)
    m = case.meta
    offs = None
    if m["graph"]:
        all_offs = [(dy, dx) for dy in range(-m["r"], m["r"] + 1) for dx in range(-m["r"], m["r"] + 1)
                    if not (abs(dy) <= 1 and abs(dx) <= 1)]
        offs = [random.sample(all_offs, m["K"]) for _ in range(T)]
    g = None if gains is None else [m["message_gain"] * u for u in gains]
    return offs, g


def _rollout_run(shape, dev, nsteps="shape"):
    fx, B, H, W, T, ns, gains, min_steps = SHAPES[shape]
    c = Case(fx)
    model = _module_for(c, dev)
    x, gy = _inputs(c, B, H, W, dev)
    offs, g = _schedule(c, T, gains)
    leaf = x.clone().requires_grad_(True)
    kw = dict(fire_rate=0.5, seed=SEED, min_steps=min_steps)
    if nsteps == "shape":
        kw["nsteps"] = torch.tensor(ns, dtype=torch.int32, device=dev)
    elif nsteps is not None:
        kw["nsteps"] = nsteps
    if c.meta["graph"]:
        kw.update(message_gain=g, offsets=offs)
    out = model.rollout(leaf, T, **kw)
    (out * gy).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), leaf.grad, _grads(model)


_STEPWISE = {}


def _stepwise_run(shape, dev, all_active=False):
    """The per-step path on the same descriptors: gnca_step_masked_f32 forward keeping each step's
    workspace, gnca_step_bwd_f32 backward with active = nsteps > t.  Returns x_final, gx, R (the
    float64 sum of the per-step gradients) and S32 (their fp32 sum in autograd's order, the
    per-step path's own result)."""
    key = (shape, all_active)
    if key in _STEPWISE:
        return _STEPWISE[key]
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import desc_for, weights_on
    fx, B, H, W, T, ns, gains, _ = SHAPES[shape]
    c = Case(fx)
    x, gy = _inputs(c, B, H, W, dev)
    offs, g = _schedule(c, T, gains)
    if all_active:
        ns = [T] * B
    nst = torch.tensor(ns, dtype=torch.int32, device=dev)
    w, keep = S.make_weights(weights_on(c, dev))
    want = {k: torch.empty(c.weights[k].shape) for k in c.meta["grad_keys"]}
    descs, states, saves, acts = [], [x], [], []
    for t in range(T):
        d = desc_for(c, B, H, W, offs[t] if offs else [], L.FIRE_HASH, fire_rate=0.5, rng_seed=SEED, rng_step=t,
                     message_gain=g[t] if g else 0.0)
        act = nst > t
        ws = S.workspace(d, dev)
        out, _ = S.step(d, w, states[-1], ws=ws, active=act)
        descs.append(d); states.append(out); saves.append(ws); acts.append(act)
    R = {k: np.zeros(c.weights[k].shape, np.float64) for k in want}
    S32 = {k: None for k in want}
    gcur = gy
    for t in reversed(range(T)):
        gcur, gr = S.step_backward(descs[t], w, states[t], gcur, want=want, saved=saves[t], active=acts[t])
        for k in want:
            R[k] += gr[k].double().cpu().numpy()
            S32[k] = gr[k].clone() if S32[k] is None else S32[k] + gr[k]
    torch.cuda.synchronize()
    _STEPWISE[key] = (states[-1], gcur, R, S32)
    return _STEPWISE[key]


def _check_against_R(tag, got, R, S32):
    assert set(got) == set(R), (sorted(got), sorted(R))
    for k, r in R.items():
        gk = got[k].double().cpu().numpy().reshape(r.shape)
        scale = float(np.abs(r).max())
        err = float(np.abs(gk - r).max())
        err_step = float(np.abs(S32[k].double().cpu().numpy().reshape(r.shape) - r).max())
        print(f"{tag} {k}: rollout err={err:.3e} per-step err={err_step:.3e} scale={scale:.3e}")
        assert np.isfinite(gk).all(), k
        assert err <= RT * scale + AT, (tag, k, f"err={err:.3e} per-step err={err_step:.3e} scale={scale:.3e}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rollout_equals_per_step_path(dev, shape):
    out, gx, grads = _rollout_run(shape, dev)
    ref_out, ref_gx, R, S32 = _stepwise_run(shape, dev)
    assert torch.equal(out, ref_out)
    assert torch.equal(gx, ref_gx)
    _check_against_R(shape, grads, R, S32)


def test_rollout_deterministic(dev):
    a = _rollout_run("torus_b8_72", dev)
    b = _rollout_run("torus_b8_72", dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def _identity_case(dev, steps, nsteps):
    c = Case("grad_graph_zeropad_latest_grown_b2_40")
    model = _module_for(c, dev)
    x, gy = _inputs(c, 3, 24, 24, dev)
    leaf = x.clone().requires_grad_(True)
    out = model.rollout(leaf, steps, fire_rate=0.5, seed=SEED, nsteps=nsteps)
    (out * gy).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), x)
    assert torch.equal(leaf.grad, gy)
    grads = _grads(model)
    assert set(grads) == set(c.meta["grad_keys"])
    for k, g in grads.items():
        assert torch.count_nonzero(g) == 0, k


def test_zero_steps_is_identity(dev):
    _identity_case(dev, 0, None)


def test_nsteps_all_zero_is_identity(dev):
    _identity_case(dev, 3, torch.zeros(3, dtype=torch.int32, device=dev))


def test_nsteps_all_T_equals_no_nsteps(dev):
    shape = "torus_b8_72"
    B, T = SHAPES[shape][1], SHAPES[shape][4]
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    out_n, gx_n, gr_n = _rollout_run(shape, dev, nsteps=full)
    out_0, gx_0, gr_0 = _rollout_run(shape, dev, nsteps=None)
    assert torch.equal(out_n, out_0)
    assert torch.equal(gx_n, gx_0)
    _, _, R, S32 = _stepwise_run(shape, dev, all_active=True)
    _check_against_R("nsteps=T", gr_n, R, S32)
    _check_against_R("nsteps=None", gr_0, R, S32)


# ---------------------------------------------------------------------------------------------
# 6: module contract
# ---------------------------------------------------------------------------------------------
def _small_model(dev, zp=False):
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    torch.manual_seed(12)
    model = NeuralCAGraph(16, 64, update_gain=0.05, alpha_thr=0.12, message_gain=0.25,
                          graph_zero_padded_shift=zp).to(dev)
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    return model


@pytest.mark.parametrize("grad", [True, False])
def test_rollout_equals_forward_loop(dev, grad):
    """fire_rate=1.0, offsets=None: the same bits as four forward calls, and Python's ``random`` is
    left where they leave it."""
    model = _small_model(dev)
    x = torch.rand(2, 16, 20, 24, device=dev)
    with torch.set_grad_enabled(grad):
        random.seed(3)
        s = x
        for _ in range(4):
            s = model(s)
        after = random.random()
        random.seed(3)
        out = model.rollout(x, 4)
        assert random.random() == after
    assert out.requires_grad == grad
    assert torch.equal(out.detach(), s.detach())


def test_inplace_weight_update_before_backward_raises(dev):
    model = _small_model(dev)
    x = torch.rand(1, 16, 16, 16, device=dev)
    out = model.rollout(x, 2)
    with torch.no_grad():
        model.update_net[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


def test_rollout_validates_before_launch(dev):
    model = _small_model(dev)
    x = torch.rand(2, 16, 16, 16, device=dev)
    with pytest.raises(ValueError):
        model.rollout(x, 3, fire_rate=[0.5, 0.5])
    with pytest.raises(ValueError):
        model.rollout(x, 3, nsteps=torch.zeros(2, dtype=torch.int32))   # a CPU tensor
    with pytest.raises(TypeError):
        model.rollout(x, 3, return_attention=True)


# ---------------------------------------------------------------------------------------------
# 7: no-grad
# ---------------------------------------------------------------------------------------------
def _nograd_setup(dev, B):
    from graph_neural_cellular_automata_amd import _lib as L
    from tests.fixture_run import desc_for
    c = Case("grad_graph_torus_latest_grown_b2_40")
    model = _module_for(c, dev)
    x, _ = _inputs(c, B, 72, 72, dev)
    offs, _ = _schedule(c, 4, [1, 1, 1, 1])
    mk = lambda t, gain=c.meta["message_gain"]: desc_for(c, B, 72, 72, offs[t], L.FIRE_HASH, fire_rate=0.5,
                                                         rng_seed=SEED, rng_step=t, message_gain=gain)
    return c, model, x, offs, mk


@pytest.mark.parametrize("B", [8, 192])
def test_nograd_uniform_is_the_rollout_pipeline(dev, B):
    """A uniform schedule under no_grad runs gnca_rollout_ex_f32 (B=8: the dense fold; B=192: two
    sub-batch streams on the compact field): the bits of step.rollout on the same descriptor."""
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import weights_on
    c, model, x, offs, mk = _nograd_setup(dev, B)
    assert S.rollout_subs(mk(0)) == (2 if B == 192 else 1)
    with torch.no_grad():
        out = model.rollout(x, 4, fire_rate=0.5, seed=SEED, offsets=offs)
    w, keep = S.make_weights(weights_on(c, dev))
    ref = S.rollout(mk(0), w, x, 4, offs)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_nograd_nsteps_equals_masked_step_loop(dev):
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import weights_on
    B = 8
    c, model, x, offs, mk = _nograd_setup(dev, B)
    ns = torch.tensor([4, 1, 3, 0, 4, 2, 4, 1], dtype=torch.int32, device=dev)
    gains = [0.25, 0.0, 0.0, 0.25]
    with torch.no_grad():
        out = model.rollout(x, 4, fire_rate=0.5, seed=SEED, offsets=offs, nsteps=ns, message_gain=gains)
    w, keep = S.make_weights(weights_on(c, dev))
    s = x
    for t in range(4):
        s, _ = S.step(mk(t, gains[t]), w, s, active=ns > t)
    torch.cuda.synchronize()
    assert torch.equal(out, s)


# ---------------------------------------------------------------------------------------------
# 8: masked single-step backward edges (step_backward(active=...))
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grad_graph_torus_latest_grown_b2_40", "grad_graph_zeropad_latest_grown_b2_40",
                                  "grad_classic_c12_hd48_nogn_b2_20"])
def test_masked_backward_edges(dev, name):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import desc_for, weights_on
    c = Case(name)
    x = torch.from_numpy(c.x_in).to(dev)
    gy = torch.from_numpy(c.cot).to(dev)
    B, _, H, W = x.shape
    d = desc_for(c, B, H, W, c.chosen(0), L.FIRE_HASH, rng_seed=SEED)
    w, keep = S.make_weights(weights_on(c, dev))
    want = {k: torch.empty(c.weights[k].shape) for k in c.grads()}
    none = torch.zeros(B, dtype=torch.bool, device=dev)
    gx, gr = S.step_backward(d, w, x, gy, want=want, active=none)
    torch.cuda.synchronize()
    assert torch.equal(gx, gy)
    for k in want:
        assert torch.count_nonzero(gr[k]) == 0, k
    gx_all, _ = S.step_backward(d, w, x, gy, want=want, active=~none)
    gx_ref, _ = S.step_backward(d, w, x, gy, want=want)
    torch.cuda.synchronize()
    assert torch.equal(gx_all, gx_ref)
