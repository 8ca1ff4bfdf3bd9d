"""``optim.FusedAdam`` on the device (``gnca_optim_step``) against torch's Adam in float64.

Reference and tolerance.  Per case the reference is ``torch.optim.Adam`` plus the gradient policy
(``dp.normalize_gradients_`` / ``clip_grad_norm_``) in FLOAT64 on the CPU, started from
fp32-representable parameters and fed fp32-representable gradients (generated in fp32, upcast).  The
same inputs also go through torch's FLOAT32 CPU Adam; ``e_ref`` is the maximum over the case's tensors
of ``|fp32 - f64|``, taken per quantity (``p``, ``exp_avg``, ``exp_avg_sq``: they differ in magnitude by
orders, so one number for all three would leave the moments unchecked), and the fused result must be
within ``4 e_ref`` of the f64 run.  The factor 4 covers a different norm summation order and FMA
contraction.  On the CPU, ``e_ref(p)`` is about 9e-7 after 20 steps of the ``strong`` cases.

Sensitivity.  A tolerance only means something if a wrong formula exceeds it: the CPU-only tests at
the top restate Adam in f64 with knobs that can be dropped one at a time (weight decay, either bias
correction, eps, the policy, the clip clamp), check the restatement against torch, and assert that
each dropped knob moves the f64 result by more than ``100 e_ref(p)`` in every case that lists the
knob in ``sensitive``.  Every knob is listed by at least one case.
"""
import copy
import random

import pytest
import torch

from graph_neural_cellular_automata_amd import dp
from tests import poison as PZ

gpu = pytest.mark.gpu

STEPS = 20
SHAPES = [(1,), (3,), (5, 7), (16,), (128, 48), (16, 128), (4099,)]
KNOBS = ("weight_decay", "bias1", "bias2", "eps", "policy", "clamp")
TRAINER = dict(lr=2e-4, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8)
STRONG = dict(lr=1e-2, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-3)

# name -> shapes, the optimiser's options (groups: per-group overrides, tensors dealt round-robin), the
# policy, the gradients' scale, the variants and the knobs whose loss moves the f64 result > 100 e_ref
CASES = {
    "trainer-normalize": dict(opts=TRAINER, policy="normalize", sensitive=("bias1", "bias2", "policy")),
    "strong-normalize": dict(opts=STRONG, policy="normalize",
                             sensitive=("weight_decay", "bias1", "bias2", "eps", "policy")),
    "strong-none": dict(opts=STRONG, policy=None, gscale=0.01, sensitive=("weight_decay", "bias1", "bias2", "eps")),
    # total norm ~ 115 >> max_norm: coefficient ~ 0.004
    "clip-above": dict(opts=STRONG, policy="clip", sensitive=("weight_decay", "bias1", "bias2", "eps", "policy")),
    # total norm ~ 0.115 < max_norm: the coefficient 0.5 / 0.115 is clamped to 1
    "clip-below": dict(opts=STRONG, policy="clip", gscale=1e-3, sensitive=("weight_decay", "eps", "clamp")),
    "two-groups": dict(opts=STRONG, policy="normalize", groups=[dict(lr=1e-2), dict(lr=1e-3, weight_decay=0.0)],
                       sensitive=("bias1", "bias2", "eps", "policy")),
    "zero-grad": dict(opts=STRONG, policy="normalize", zero=4, sensitive=("bias2", "policy")),
    "none-grad": dict(opts=STRONG, policy="normalize", none=(5, (3, 4, 5)), sensitive=("bias2", "policy")),
    "none-grad-clip": dict(opts=STRONG, policy="clip", none=(4, (3, 4, 5)), sensitive=("policy",)),
    # 27 tensors: more than one table (clip: the total must still cover all of them)
    "many-clip": dict(opts=STRONG, policy="clip", shapes=(SHAPES * 4)[:27], sensitive=("policy", "eps")),
    "many-normalize": dict(opts=STRONG, policy="normalize", shapes=(SHAPES * 4)[:27], sensitive=("policy",)),
    "many-none": dict(opts=STRONG, policy=None, shapes=(SHAPES * 4)[:27], gscale=0.01, sensitive=("eps",)),
    # more than 65536 elements: the sums of squares go through the fp64 workspace (two launches)
    "large-normalize": dict(opts=STRONG, policy="normalize", shapes=SHAPES + [(70001,)], sensitive=("policy",)),
    "large-clip": dict(opts=STRONG, policy="clip", shapes=SHAPES + [(70001,)], sensitive=("policy",)),
}


def _inputs(name):
    """(fp32 parameters, [step][tensor] fp32 gradients or None), seeded by the case's name."""
    case = CASES[name]
    g = torch.Generator().manual_seed(PZ.seed_of(name))
    shapes = case.get("shapes", SHAPES)
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = []
    for step in range(STEPS):
        row = [torch.randn(s, generator=g) * case.get("gscale", 1.0) for s in shapes]
        if "zero" in case:
            row[case["zero"]].zero_()
        if "none" in case and step in case["none"][1]:
            row[case["none"][0]] = None
        grads.append(row)
    return params, grads


def _groups(case, params):
    if "groups" not in case:
        return [dict(params=params)]
    n = len(case["groups"])
    return [dict(params=params[i::n], **g) for i, g in enumerate(case["groups"])]


def _apply_policy(policy, params):
    live = [p for p in params if p.grad is not None]
    if policy == "normalize":
        dp.normalize_gradients_(live)
    elif policy == "clip":
        dp.clip_gradients_(live, 0.5)


def _run_torch(name, dtype):
    """torch.optim.Adam + the policy in ``dtype`` on the CPU: per tensor (p, exp_avg, exp_avg_sq, step)."""
    case = CASES[name]
    p0, grads = _inputs(name)
    params = [torch.nn.Parameter(p.to(dtype)) for p in p0]
    opt = torch.optim.Adam(_groups(case, params), **case["opts"])
    for row in grads:
        for p, g in zip(params, row):
            p.grad = None if g is None else g.to(dtype)
        _apply_policy(case["policy"], params)
        opt.step()
    return _collect(params, opt)


def _collect(params, opt):
    out = []
    for p in params:
        st = opt.state[p]
        out.append((p.detach().double().cpu(), st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu(),
                    float(st["step"])))
    return out


_REF = {}


def _reference(name):
    """(f64 run, e_ref per quantity), computed once per case and shared (never modified)."""
    if name not in _REF:
        f64, f32 = _run_torch(name, torch.float64), _run_torch(name, torch.float32)
        e_ref = [max(float((a[q] - b[q]).abs().max()) for a, b in zip(f64, f32)) for q in range(3)]
        _REF[name] = (f64, e_ref)
    return _REF[name]


def _manual_adam(name, drop=None):
    """Adam restated in f64 (the issue's formulas), with one knob dropped: the final parameters."""
    case = CASES[name]
    p0, grads = _inputs(name)
    params = [p.double() for p in p0]
    opts = []
    for grp in _groups(case, list(range(len(params)))):
        for i in grp["params"]:
            opts.append((i, {**case["opts"], **{k: v for k, v in grp.items() if k != "params"}}))
    opts = dict(opts)
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    t = [0] * len(params)
    policy = None if drop == "policy" else case["policy"]
    for row in grads:
        live = [i for i, g in enumerate(row) if g is not None]
        gs = {i: row[i].double() for i in live}
        if policy == "normalize":
            gs = {i: g / (g.norm() + 1e-8) for i, g in gs.items()}
        elif policy == "clip":
            total = torch.sqrt(sum((g * g).sum() for g in gs.values()))
            coef = 0.5 / (total + 1e-6)
            if drop != "clamp":
                coef = coef.clamp(max=1.0)
            gs = {i: g * coef for i, g in gs.items()}
        for i in live:
            o = opts[i]
            b1, b2 = o["betas"]
            t[i] += 1
            g = gs[i] + (0.0 if drop == "weight_decay" else o["weight_decay"]) * params[i]
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            bias1 = 1.0 if drop == "bias1" else 1 - b1 ** t[i]
            bias2 = 1.0 if drop == "bias2" else 1 - b2 ** t[i]
            eps = 0.0 if drop == "eps" else o["eps"]
            params[i] = params[i] - (o["lr"] / bias1) * m[i] / (v[i].sqrt() / bias2 ** 0.5 + eps)
    return params


# ---------------------------------------------------------------------------------------------
# CPU only: the reference and the tolerance have teeth
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restated_adam_equals_torch_f64(name):
    f64, e_ref = _reference(name)
    mine = _manual_adam(name)
    err = max(float((a - b[0]).abs().max()) for a, b in zip(mine, f64))
    assert err < 1e-3 * e_ref[0], (err, e_ref)      # (two f64 evaluation orders: ~1e-15)


@pytest.mark.parametrize("name", list(CASES))
def test_every_listed_knob_moves_the_reference(name):
    f64, e_ref = _reference(name)
    assert e_ref[0] > 0
    for knob in CASES[name]["sensitive"]:
        moved = max(float((a - b[0]).abs().max()) for a, b in zip(_manual_adam(name, drop=knob), f64))
        print(f"{name}: drop {knob}: moved {moved:.3e}, e_ref {e_ref[0]:.3e}")
        assert moved > 100 * e_ref[0], (name, knob, moved, e_ref[0])


def test_every_knob_is_covered_by_a_case():
    listed = {k for c in CASES.values() for k in c["sensitive"]}
    assert listed == set(KNOBS)
    assert {c["policy"] for c in CASES.values()} == {None, "normalize", "clip"}


def test_clip_cases_sit_on_both_sides_of_the_clamp():
    for name, above in (("clip-above", True), ("clip-below", False)):
        _, grads = _inputs(name)
        for row in grads:
            total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in row)))
            assert (total > 2 * 0.5) if above else (total < 0.5 / 2), (name, total)


def test_none_grad_reference_leaves_the_state_unchanged():
    f64, _ = _reference("none-grad")
    assert [r[3] for r in f64] == [20.0] * 5 + [17.0] + [20.0]


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _run_fused(name, dev, snapshots=None):
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    case = CASES[name]
    p0, grads = _inputs(name)
    params = [torch.nn.Parameter(p.to(dev)) for p in p0]
    opt = FusedAdam(_groups(case, params), grad_policy=case["policy"], max_norm=0.5, **case["opts"])
    for step, row in enumerate(grads):
        for p, g in zip(params, row):
            p.grad = None if g is None else g.to(dev)
        if snapshots is not None:
            snapshots.append([(copy.deepcopy(dict(opt.state[p])) if p in opt.state else None) for p in params])
        opt.step()
    torch.cuda.synchronize()
    return params, opt


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fused_adam_within_4_e_ref_of_f64(dev, name):
    f64, e_ref = _reference(name)
    params, opt = _run_fused(name, dev)
    got = _collect(params, opt)
    err = [max(float((a[q] - b[q]).abs().max()) for a, b in zip(got, f64)) for q in range(3)]
    print(f"{name}: e_ref (p, m, v) = {e_ref[0]:.3e} {e_ref[1]:.3e} {e_ref[2]:.3e}; "
          f"fused error = {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}")
    assert [r[3] for r in got] == [r[3] for r in f64]          # every parameter's own step count
    for a in got:
        assert all(bool(torch.isfinite(x).all()) for x in a[:3])
    for q, what in enumerate(("p", "exp_avg", "exp_avg_sq")):
        assert err[q] <= 4 * e_ref[q], (name, what, err[q], e_ref[q])


@gpu
def test_zero_gradient_normalises_to_zero(dev):
    """``0 / (0 + 1e-8)``: the moments of the all-zero gradient's tensor stay exactly 0 (weight decay off)."""
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.randn(37, device=dev))
    before = p.detach().clone()
    opt = FusedAdam([p], lr=1e-2, grad_policy="normalize")
    p.grad = torch.zeros_like(p)
    opt.step()
    assert torch.equal(opt.state[p]["exp_avg"], torch.zeros_like(p))
    assert torch.equal(opt.state[p]["exp_avg_sq"], torch.zeros_like(p))
    assert torch.equal(p.detach(), before)


@gpu
@pytest.mark.parametrize("name", ["none-grad", "none-grad-clip"])
def test_a_parameter_without_gradient_is_skipped_entirely(dev, name):
    which, steps = CASES[name]["none"]
    snaps = []
    params, opt = _run_fused(name, dev, snaps)
    for step in steps:          # snaps[s]: the state BEFORE step s
        a, b = snaps[step][which], snaps[step + 1][which]
        assert float(a["step"]) == float(b["step"]) == 3.0
        assert PZ.same_bytes(a["exp_avg"], b["exp_avg"]) and PZ.same_bytes(a["exp_avg_sq"], b["exp_avg_sq"])
    assert float(opt.state[params[which]]["step"]) == STEPS - len(steps)
    st = opt.state[params[which]]["step"]
    assert st.dtype == torch.float32 and st.device.type == "cpu" and st.dim() == 0


@gpu
def test_a_parameter_that_never_has_a_gradient_gets_no_state(dev):
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    a, b = (torch.nn.Parameter(torch.randn(5, device=dev)) for _ in range(2))
    opt = FusedAdam([a, b], lr=1e-3, grad_policy="clip")
    a.grad = torch.randn(5, device=dev)
    opt.step()
    assert b not in opt.state or len(opt.state[b]) == 0
    assert sorted(opt.state_dict()["state"]) == [0]


@gpu
@pytest.mark.parametrize("name", ["strong-normalize", "clip-above", "many-clip", "large-clip"])
def test_bitwise_determinism(dev, name):
    runs = [_collect(*_run_fused(name, dev)) for _ in range(2)]
    for a, b in zip(*runs):
        for q in range(3):
            assert PZ.same_bytes(a[q], b[q])


@gpu
@pytest.mark.parametrize("policy", [None, "normalize", "clip"])
def test_gradients_are_read_never_written(dev, policy):
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    p0, grads = _inputs("strong-normalize")
    params = [torch.nn.Parameter(p.to(dev)) for p in p0]
    opt = FusedAdam(params, grad_policy=policy, **STRONG)
    for p, g in zip(params, grads[0]):
        p.grad = g.to(dev)
    before = [p.grad.clone() for p in params]
    opt.step()
    torch.cuda.synchronize()
    for p, g, b in zip(params, grads[0], before):
        assert PZ.same_bytes(p.grad, b) and PZ.same_bytes(p.grad.cpu(), g)


@gpu
def test_state_moves_between_fused_and_torch_adam_on_the_device(dev):
    """FusedAdam -> state_dict -> torch.optim.Adam on the same device parameters, and back."""
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    name = "strong-none"
    p0, grads = _inputs(name)
    params = [torch.nn.Parameter(p.to(dev)) for p in p0]
    fused = FusedAdam(params, **STRONG)
    plain = torch.optim.Adam(params, **STRONG)
    opts = [fused] * 7 + [plain] * 6 + [fused] * 7
    for step, (row, opt) in enumerate(zip(grads, opts)):
        if step in (7, 13):
            opt.load_state_dict(copy.deepcopy(opts[step - 1].state_dict()))
        for p, g in zip(params, row):
            p.grad = g.to(dev)
        opt.step()
    f64, e_ref = _reference(name)
    got = _collect(params, fused)
    for q in range(3):
        err = max(float((a[q] - b[q]).abs().max()) for a, b in zip(got, f64))
        assert err <= 4 * e_ref[q], (q, err, e_ref[q])
    assert [r[3] for r in got] == [20.0] * len(params)


@gpu
def test_poisoned_buffers(dev):
    """Every buffer of one clip step and one large (workspace) normalize step: canaries intact, outputs
    byte-identical across the fills, the gradient read-only."""
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    for name, policy in (("strong-normalize", "normalize"), ("clip-above", "clip"), ("large-clip", "clip"),
                         ("large-normalize", "normalize")):
        p0, grads = _inputs(name)
        m0 = [torch.rand_like(p) * 0.1 for p in p0]
        v0 = [torch.rand_like(p) * 0.01 for p in p0]

        def call(P):
            params = [torch.nn.Parameter(P.guard(p.to(dev), inplace=True)) for p in p0]
            opt = FusedAdam(params, grad_policy=policy, **STRONG)
            for p, g, m, v in zip(params, grads[0], m0, v0):
                p.grad = P.guard(g.to(dev))
                opt.state[p] = dict(step=torch.tensor(4.0), exp_avg=P.guard(m.to(dev), inplace=True),
                                    exp_avg_sq=P.guard(v.to(dev), inplace=True))
            opt.step()
            out = {}
            for i, p in enumerate(params):
                out[f"p{i}"], out[f"m{i}"], out[f"v{i}"] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
            return out

        outs = PZ.run_fills(call, f"optim-{name}")
        assert all(bool(torch.isfinite(t).all()) for t in outs.values())
        assert not PZ.same_bytes(outs["p6"], p0[6].to(dev))


@gpu
def test_step_makes_no_host_wait(dev):
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    p0, grads = _inputs("clip-above")
    params = [torch.nn.Parameter(p.to(dev)) for p in p0]
    opt = FusedAdam(params, grad_policy="clip", **STRONG)
    for p, g in zip(params, grads[0]):
        p.grad = g.to(dev)
    opt.step()                                   # (state creation is outside the checked step)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=dev)
    prev = torch.cuda.get_sync_debug_mode()
    raised = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
        except RuntimeError:
            raised = True
        if raised:
            opt.step()                           # must not raise
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not raised:
        pytest.skip("this torch build does not raise for .item() under set_sync_debug_mode('error') on ROCm")


# ---------------------------------------------------------------------------------------------
# Model level: three training iterations of a small graph model
# ---------------------------------------------------------------------------------------------
@gpu
def test_model_training_iterations_match_torch_adam(dev):
    """rollout -> loss_premult_rgba -> backward -> step, three times: FusedAdam(normalize) on one model,
    normalize_gradients_ + torch.optim.Adam on a deep copy, identical seeds.  Bound: torch's fp32 path
    against an f64 Adam fed the same fp32 gradients gives e_ref per iteration; the fused parameters are
    within 4 e_ref of that f64 run (after step 1 the two trajectories differ by rounding only)."""
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    from graph_neural_cellular_automata_amd.loss import loss_premult_rgba
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    C, HID, H, B, T = 8, 32, 24, 2, 8
    torch.manual_seed(3)
    model_a = NeuralCAGraph(C, HID, update_gain=0.05, alpha_thr=0.1, message_gain=0.25).to(dev)
    with torch.no_grad():
        model_a.update_net[2].weight.normal_(0, 0.05)
    model_b = copy.deepcopy(model_a)
    x0 = torch.zeros(B, C, H, H, device=dev)
    x0[:, 3:, H // 2 - 3:H // 2 + 3, H // 2 - 3:H // 2 + 3] = 1.0
    x0[:, 4:] += 0.1 * torch.randn(B, C - 4, H, H, device=dev)
    x0[:, :3] = torch.rand(B, 3, H, H, device=dev) * x0[:, 3:4]
    target = torch.rand(4, H, H, device=dev)
    target[:3] *= target[3:4]
    kw = dict(lr=2e-3, weight_decay=1e-5)
    opt_a = FusedAdam(model_a.parameters(), grad_policy="normalize", **kw)
    opt_b = torch.optim.Adam(model_b.parameters(), **kw)
    names = [n for n, _ in model_b.named_parameters()]
    p64 = [torch.nn.Parameter(p.detach().double().cpu()) for p in model_b.parameters()]
    opt64 = torch.optim.Adam(p64, **kw)

    def iteration(model, opt, it, normalize):
        random.seed(100 + it)
        opt.zero_grad(set_to_none=True)
        state = model.rollout(x0, T, fire_rate=0.5, seed=7 + it)
        loss = loss_premult_rgba(state[:, :4], target).mean()
        loss.backward()
        params = list(model.parameters())
        raw = [None if p.grad is None else p.grad.detach().clone() for p in params]
        if normalize:
            dp.normalize_gradients_(params)
        opt.step()
        return raw

    for it in range(3):
        iteration(model_a, opt_a, it, False)
        raw = iteration(model_b, opt_b, it, True)
        assert any(g is not None and float(g.abs().max()) > 0 for g in raw)
        for p, g in zip(p64, raw):
            p.grad = None if g is None else g.double().cpu()
        dp.normalize_gradients_(p64)
        opt64.step()
        e_ref = max(float((q.detach().double().cpu() - p.detach()).abs().max())
                    for q, p in zip(model_b.parameters(), p64))
        err = max(float((q.detach().double().cpu() - p.detach()).abs().max())
                  for q, p in zip(model_a.parameters(), p64))
        print(f"model iteration {it + 1}: e_ref = {e_ref:.3e}, fused error = {err:.3e}")
        assert e_ref > 0 and err <= 4 * e_ref, (it, err, e_ref)
    for n, pa, pb in zip(names, model_a.parameters(), model_b.parameters()):
        if "gate_mlp" in n:
            assert pa not in opt_a.state or len(opt_a.state[pa]) == 0, n
            assert pb not in opt_b.state or len(opt_b.state[pb]) == 0, n
    assert any("gate_mlp" in n for n in names)
    assert sorted(opt_a.state_dict()["state"]) == sorted(opt_b.state_dict()["state"])
