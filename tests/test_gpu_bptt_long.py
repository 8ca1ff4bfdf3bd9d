"""BPTT at the trainers' rollout lengths (tests/bptt_long_cases.py: 24-72 steps of a state grown from
one seed cell) on the GPU: the per-step path (gnca_step_masked_f32 / gnca_step_bwd_f32 once per step)
against the float64 VJP oracle step by step, and model.rollout() (gnca_rollout_fwd_f32 /
gnca_rollout_bwd_f32), its recompute form and the autograd chain of per-step nodes against the
per-step path.

(a) is teacher-forced.  An end-to-end float64 comparison over 72 steps says nothing about the
backward kernels: the forward's rounding (1e-4 after 96 steps, test_gpu_drift.py) moves relu and
alive-mask decisions.  So every step's oracle VJP takes the float64 copy of the GPU's OWN input
state S_t and the GPU's OWN incoming cotangent g_{t+1}, restricted to the samples active at t, and
the step's gx and every weight gradient meet the project's one-step bound (test_gpu_grad.py:
RT * max|ref| + AT), as sharp at step 70 as at step 0.

Masks.  S_t is the same fp32 bits on both sides, so the pre-update alive mask and the sender mask
agree exactly.  The post-update mask thresholds the updated state, which the GPU knows to ~2e-6:
a cell is *doubtful* when the oracle's pooled pre-gate alpha is within MARGIN (2e-5, 10 x the
forward atol) of float32(thr).  The oracle runs with its own post mask, except at doubtful cells,
which take the GPU's: the GPU's mask is read from its S_{t+1} as pooled(alpha of S_{t+1}) > thr.
(That is the GPU's mask exactly: a cell whose window holds an updated alpha above thr is alive, and
so is the cell holding that alpha, whose gated alpha is therefore the updated one; a dead window
holds only gated zeros.)  This is a condition, not a tolerance: the doubtful share is asserted to
stay under 1e-4 of all (active sample, step, cell) triples, and outside the doubtful cells the two
masks must be equal.

(b) x_final and gx of the rollout do not depend on the cross-step reduction order: bitwise equal
to the per-step path's.  A weight gradient G is compared with R, the float64 sum of the per-step
path's per-step gradients gr_t, within sum_t (RT * max|gr_t| + AT): the one-step bound summed by
the triangle inequality, no new number.  The ratio of |G - R| to ONE step's bound on the sum,
RT * max|R| + AT (what test_gpu_rollout_bptt.py asserts for T <= 4), is printed for the rollout and
for the per-step path's own fp32 sum (DESIGN.md section 9 records them).
"""
import numpy as np
import pytest
import torch

from tests import bptt_long_cases as BL
from tests.liveness_cases import pooled
from tests.test_gpu_rollout_bptt import _grads, _module_for

pytestmark = pytest.mark.gpu

RT, AT = 2e-5, 1e-6          # tests/test_gpu_grad.py: one step's bound
DOUBTFUL_SHARE = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(name, dev):
    x = torch.from_numpy(BL.seed_state(name)).to(dev)
    gy = torch.from_numpy(BL.cotangent(name)).to(dev)
    nst = torch.from_numpy(BL.nsteps(name)).to(dev)
    return x, gy, nst


def _f64(t, shape=None):
    a = t.detach().double().cpu().numpy()
    return a if shape is None else a.reshape(shape)


# ---------------------------------------------------------------------------------------------
# the per-step path, with each step's teacher-forced float64 VJP (cached per case)
# ---------------------------------------------------------------------------------------------
_STEPWISE = {}


def _oracle_step(name, t, offs, gains, p64, idx, s_t, s_next, g_in):
    """The float64 VJP of step t on the GPU's own input state and cotangent (active samples
    ``idx``), with the post mask of the module docstring.  Returns (gx, grads, doubtful cells,
    cells outside them where the GPU's post mask differs from the oracle's)."""
    from oracle import nca_oracle_vjp as V
    thr = BL.fixture(name).meta["alpha_thr"]
    c, ch = BL.step_args(name, t, offs, gains)
    kw = dict(chosen=ch, fire_mask=BL.fire(name, t, idx))
    gx, grads, xt, post = V.nca_step_vjp(s_t, p64, c, g_in, return_update=True, **kw)
    doubt = BL.doubtful(xt, thr)
    post_gpu = (pooled(s_next[:, 3]) > np.float32(thr))[:, None]
    differ = post_gpu != (post != 0)
    if (differ & doubt).any():
        # (only then: with the oracle's own mask the result is bit for bit the one above,
        #  tests/test_bptt_long_cases_cpu.py)
        gx, grads = V.nca_step_vjp(s_t, p64, c, g_in, post_alive=np.where(doubt, post_gpu, post != 0), **kw)
    return gx, grads, int(doubt.sum()), int((differ & ~doubt).sum())


def _stepwise(name, dev):
    """Forward with S.step(ws=, active=) keeping states and workspaces, backward with
    S.step_backward(saved=, active=), active = nsteps > t at every step.  Returns a dict: x_final,
    gx, R (float64 sum of the per-step gradients), S32 (their fp32 sum in step order, the per-step
    path's own result), bound (sum_t RT * max|gr_t| + AT per key), and for the oracle cases Rref /
    bound_ref (the same of the teacher-forced float64 gradients) and ``steps``: one record per
    step with the figures test (a) asserts on."""
    if name in _STEPWISE:
        return _STEPWISE[name]
    from graph_neural_cellular_automata_amd import step as S
    from tests.fixture_run import weights_on
    k, c = BL.CASES[name], BL.fixture(name)
    T, oracle = k["T"], k["oracle"]
    x, gy, nst = _inputs(name, dev)
    offs, gains = BL.schedule(name)
    w, keep = S.make_weights(weights_on(c, dev))
    want = {key: torch.empty(c.weights[key].shape) for key in c.meta["grad_keys"]}
    descs, states, saves, acts = [], [x], [], []
    for t in range(T):
        d = BL.desc(name, t, offs, gains)
        act = nst > t
        ws = S.workspace(d, dev)
        out, _ = S.step(d, w, states[-1], ws=ws, active=act)
        descs.append(d); states.append(out); saves.append(ws); acts.append(act)
    p64 = BL.params64(name) if oracle else None
    zeros = lambda: {key: np.zeros(c.weights[key].shape, np.float64) for key in want}  # noqa: E731
    R, Rref = zeros(), zeros()
    bound, bound_ref = {key: 0.0 for key in want}, {key: 0.0 for key in want}
    S32 = {key: None for key in want}
    recs = []
    gcur = gy
    for t in reversed(range(T)):
        g_in = gcur
        gcur, gr = S.step_backward(descs[t], w, states[t], g_in, want=want, saved=saves[t], active=acts[t])
        saves[t] = None
        for key in want:
            g64 = _f64(gr[key])
            R[key] += g64
            bound[key] += RT * float(np.abs(g64).max()) + AT
            S32[key] = gr[key].clone() if S32[key] is None else S32[key] + gr[key]
        act = acts[t]
        rec = dict(t=t, active=int(act.sum()), gmax=float(gcur.abs().max()),
                   inactive_bitwise=bool(torch.equal(gcur[~act], g_in[~act])
                                         and torch.equal(states[t + 1][~act], states[t][~act])))
        if oracle and rec["active"]:
            idx = np.flatnonzero(act.cpu().numpy())
            gx_ref, ref, nd, nbad = _oracle_step(name, t, offs, gains, p64, idx, _f64(states[t][act]),
                                                 states[t + 1][act].cpu().numpy(), _f64(g_in[act]))
            assert set(ref) == set(want), (sorted(ref), sorted(want))
            rec.update(doubtful=nd, mask_differs=nbad, cells=idx.size * k["H"] * k["W"], errs={})
            for key, r in dict(ref, gx=gx_ref).items():
                got = _f64(gcur[act]) if key == "gx" else _f64(gr[key], r.shape)
                scale = float(np.abs(r).max())
                rec["errs"][key] = (float(np.abs(got - r).max()), scale, bool(np.isfinite(got).all()))
                if key != "gx":
                    Rref[key] += r
                    bound_ref[key] += RT * scale + AT
        recs.append(rec)
    torch.cuda.synchronize()
    _STEPWISE[name] = dict(x_final=states[-1], gx=gcur, R=R, S32=S32, bound=bound, Rref=Rref, bound_ref=bound_ref,
                           steps=recs[::-1])
    return _STEPWISE[name]


@pytest.mark.parametrize("name", BL.ORACLE_CASES)
def test_per_step_path_matches_float64_vjp_teacher_forced(dev, name):
    """(a): every step of the per-step path against the float64 VJP of that step on the GPU's own
    state and cotangent; the inactive samples' gradient and state pass through bit for bit."""
    plans = BL.check_plans(name)
    r = _stepwise(name, dev)
    nd = cells = 0
    for s in r["steps"]:
        assert s["inactive_bitwise"], (name, s["t"], plans)
        if not s["active"]:
            continue
        key, (err, scale, _) = max(s["errs"].items(), key=lambda kv: kv[1][0] / (RT * kv[1][1] + AT))
        print(f"{name} t={s['t']:2d} active={s['active']} max|g|={s['gmax']:.3e} doubtful={s['doubtful']} "
              f"worst {key}: err/max|ref|={err / max(scale, 1e-300):.3e} (bound x{err / (RT * scale + AT):.3f})")
        nd += s["doubtful"]
        cells += s["cells"]
    print(f"{name}: {nd} doubtful cells of {cells} (active sample, step, cell) triples")
    assert cells == int(BL.nsteps(name).sum()) * BL.CASES[name]["H"] * BL.CASES[name]["W"]
    assert nd <= DOUBTFUL_SHARE * cells, (name, nd, cells)
    for s in r["steps"]:
        if not s["active"]:
            continue
        assert s["mask_differs"] == 0, (name, s["t"], "post-update mask differs outside the doubtful cells", plans)
        for key, (err, scale, finite) in s["errs"].items():
            assert finite, (name, s["t"], key, plans)
            assert err <= RT * scale + AT, (name, f"t={s['t']}", key, f"err={err:.3e} scale={scale:.3e}", plans)


# ---------------------------------------------------------------------------------------------
# model.rollout() against the per-step path
# ---------------------------------------------------------------------------------------------
_ROLLOUT = {}


def _rollout(name, dev, recompute=False, cached=True):
    key = (name, recompute)
    if cached and key in _ROLLOUT:
        return _ROLLOUT[key]
    k, c = BL.CASES[name], BL.fixture(name)
    model = _module_for(c, dev)
    x, gy, nst = _inputs(name, dev)
    offs, gains = BL.schedule(name)
    leaf = x.requires_grad_(True)
    kw = dict(fire_rate=BL.FIRE_RATE, seed=BL.FIRE_SEED, nsteps=nst, min_steps=k["min_steps"], recompute=recompute)
    if c.meta["graph"]:
        kw.update(message_gain=gains, offsets=offs)
    out = model.rollout(leaf, k["T"], **kw)
    (out * gy).sum().backward()
    torch.cuda.synchronize()
    got = (out.detach(), leaf.grad, _grads(model))
    if cached:
        _ROLLOUT[key] = got
    return got


def _check_sum(tag, grads, r, against_oracle):
    """Every weight gradient within the summed one-step bound of R (and of the teacher-forced
    float64 sum); prints the ratios to one step's bound on the sum."""
    R, S32, bound = r["R"], r["S32"], r["bound"]
    assert set(grads) == set(R), (tag, sorted(grads), sorted(R))
    for key, ref in R.items():
        g = _f64(grads[key], ref.shape)
        one = RT * float(np.abs(ref).max()) + AT
        err = float(np.abs(g - ref).max())
        err32 = float(np.abs(_f64(S32[key], ref.shape) - ref).max())
        print(f"{tag} {key}: |G-R|={err:.3e} bound={bound[key]:.3e} max|R|={np.abs(ref).max():.3e}  "
              f"ratio to one step's bound: {err / one:.3f} (per-step fp32 sum: {err32 / one:.3f})")
        assert np.isfinite(g).all(), (tag, key)
        assert err <= bound[key], (tag, key, f"err={err:.3e} bound={bound[key]:.3e}")
        if against_oracle:
            eo = float(np.abs(g - r["Rref"][key]).max())
            print(f"{tag} {key}: against the teacher-forced float64 sum: err={eo:.3e} bound={r['bound_ref'][key]:.3e}")
            assert eo <= r["bound_ref"][key], (tag, key, f"err={eo:.3e} bound={r['bound_ref'][key]:.3e}")


@pytest.mark.parametrize("name", list(BL.CASES))
def test_rollout_equals_per_step_path(dev, name):
    """(b): one rollout call and one backward against the per-step path on the same schedule."""
    plans = BL.check_plans(name)
    out, gx, grads = _rollout(name, dev)
    r = _stepwise(name, dev)
    assert torch.equal(out, r["x_final"]), (name, plans)
    assert torch.equal(gx, r["gx"]), (name, plans)
    _check_sum(name, grads, r, BL.CASES[name]["oracle"])


@pytest.mark.parametrize("name", ["torus40", "zeropad40"])
def test_rollout_recompute_is_bitwise(dev, name):
    """(c): recompute=True (the tape keeps the states only) gives the saved-tape run's bits."""
    plans = BL.check_plans(name)
    out, gx, grads = _rollout(name, dev)
    out_r, gx_r, grads_r = _rollout(name, dev, recompute=True)
    assert torch.equal(out, out_r) and torch.equal(gx, gx_r), (name, plans)
    assert set(grads) == set(grads_r)
    for key in grads:
        assert torch.equal(grads[key], grads_r[key]), (name, key, plans)


def test_autograd_chain_of_step_nodes(dev):
    """(d): the trainers' default, T per-step autograd nodes (apply_step with the in-kernel active
    mask) and one backward(): the per-step path's bits for the state and the input gradient, its
    sums within the bound of (b) for the parameters."""
    from graph_neural_cellular_automata_amd import step as S
    from graph_neural_cellular_automata_amd.modules._stepper import apply_step
    name = "torus40"
    plans = BL.check_plans(name)
    k, c = BL.CASES[name], BL.fixture(name)
    model = _module_for(c, dev)
    x, gy, nst = _inputs(name, dev)
    offs, gains = BL.schedule(name)
    leaf = x.requires_grad_(True)
    state = leaf * 1.0
    tensors = dict(perception=model.perception.conv.weight, w1=model.update_net[0].weight,
                   b1=model.update_net[0].bias, w2=model.update_net[2].weight,
                   gn_weight=model.norm.weight, gn_bias=model.norm.bias, **model.graph.weight_tensors())
    for t in range(k["T"]):
        w, keep = S.make_weights(tensors)
        state, _ = apply_step(model, state.contiguous(), BL.desc(name, t, offs, gains), w, keep, None, active=nst > t)
    (state * gy).sum().backward()
    torch.cuda.synchronize()
    r = _stepwise(name, dev)
    assert torch.equal(state.detach(), r["x_final"]), plans
    assert torch.equal(leaf.grad, r["gx"]), plans
    _check_sum("autograd chain", _grads(model), r, False)


def test_rollout_backward_deterministic(dev):
    """(e): the same rollout and backward twice, the same bits."""
    plans = BL.check_plans("torus40")
    a = _rollout("torus40", dev)
    b = _rollout("torus40", dev, cached=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), plans
    assert set(a[2]) == set(b[2])
    for key in a[2]:
        assert torch.equal(a[2][key], b[2][key]), key
