"""The weight-direction tangent on the GPU: ``tangent_step`` / ``rollout_tangent`` / ``rollout_tangent_block`` with
``dparams=`` (gnca_step_tangent_params / gnca_rollout_tangent_params / gnca_rollout_tangent_block_params) against
the float64 reference tests/param_tangent_ref.py, against the HIP backward and the shipped BPTT by duality, and
against themselves where the arithmetic is exact (a zero direction, linearity in the pair, the chain of steps,
reproducibility, sample independence), plus the log norms, the guarded and poisoned buffers and the stream legs.
Cases: tests/tangent_cases.py; directions: dense N(0,1) tensors for every parameter the case has.

Parity bound (the backward's): ``2e-5 * max|ref| + 1e-6`` per element.
"""
import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import param_tangent_ref as PR
from tests import poison as PZ
from tests import shape_class_cases as SC
from tests import streams as ST
from tests import tangent_cases as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROLL_IDS = ("p6", "p13", "p5", "neg")
EXACT_IDS = ("p5", "p6", "p13", "p31", "q16h256", "q16h200", "p15")   # every NB, pass-staged, classic, GroupNorm off
T = 4


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import os
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


_MODELS: dict = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = TC.model(name, DEV)
    return _MODELS[name]


def _direction(name, extra=0, dev=None):
    """A dense N(0,1) direction (CPU, or on ``dev``) for every parameter of the case a direction may perturb."""
    g = torch.Generator().manual_seed(909 + TC.seed(name) + 1000 * extra)
    d = {n: torch.randn(tuple(p.shape), generator=g) for n, p in TC.model(name).named_parameters()
         if n in S.DIRECTION_FIELDS}
    return d if dev is None else {k: t.to(dev) for k, t in d.items()}


def _d64(d):
    return {k: t.cpu().numpy().astype(np.float64) for k, t in d.items()}


def _step(name, x, v, dp, *, active=None, fire="case", offs=None):
    """model.tangent_step on the case's first offsets and fire mask."""
    c = TC.case(name)
    m = _model(name)
    kw = {}
    if c["graph"]:
        kw["offsets"] = TC.offsets(name)[0] if offs is None else offs
    f = TC.fire_mask(name) if isinstance(fire, str) else fire
    if f is not None:
        kw["fire"] = f.to(DEV)
    return m.tangent_step(x, v, c["fire_rate"], active=active, dparams=dp, **kw)


def _post_of(xo, thr):
    """The post mask of a GPU state: 3x3 pool of its alpha > float32(thr) (tests/test_gpu_tangent.py)."""
    a = xo[:, 3:4]
    ap = np.full((a.shape[0], 1, a.shape[2] + 2, a.shape[3] + 2), -np.inf, np.float32)
    ap[:, :, 1:-1, 1:-1] = a
    pooled = np.max([ap[:, :, i:i + a.shape[2], j:j + a.shape[3]] for i in range(3) for j in range(3)], axis=0)
    return (pooled > np.float32(thr)).astype(np.float64)


_STEP: dict = {}


def _one_step(name):
    """The case's GPU step (x_out, v_out) and its float64 reference, once per case and left unchanged."""
    if name in _STEP:
        return _STEP[name]
    c = TC.case(name)
    x, v, dp = TC.state(name), TC.tangent(name), _direction(name)
    dpd = {k: t.to(DEV) for k, t in dp.items()}
    x_out, v_out = _step(name, x.to(DEV), v.to(DEV), dpd)
    torch.cuda.synchronize()
    f = TC.fire_mask(name)
    post = _post_of(x_out.cpu().numpy(), c["thr"]) if c["thr"] >= 0 else None   # (a gated +-0 exceeds a negative thr)
    x_ref, v_ref = PR.nca_step_param_jvp(x.numpy().astype(np.float64), TC.params64(name), TC.oracle_cfg(name),
                                         v.numpy().astype(np.float64), _d64(dp),
                                         chosen=TC.offsets(name)[0] if c["graph"] else None,
                                         fire_mask=None if f is None else f.numpy().astype(np.float64), post_alive=post)
    v_ref.setflags(write=False)
    _STEP[name] = dict(x=x, v=v, dp=dp, dpd=dpd, x_out=x_out, v_out=v_out, v_ref=v_ref, x_ref=x_ref)
    return _STEP[name]


def _desc_weights(name):
    c = TC.case(name)
    f = TC.fire_mask(name)
    d = TC.desc(name, TC.offsets(name)[0] if c["graph"] else [], fire_mode=L.FIRE_MASK_U8 if f is not None else L.FIRE_NONE)
    w, keep = S.make_weights(SC.weight_tensors(_model(name)))
    return d, w, keep, None if f is None else f.to(DEV)


def test_cases_reach_every_path():
    cs = {n: TC.case(n) for n in TC.IDS}
    assert len(TC.IDS) == 25 and not any(c["zp"] for c in cs.values())
    assert {1, 2, 4} == {1 if c["hidden"] <= 32 else 2 if c["hidden"] <= 64 else 4 for c in cs.values()}   # all three NB
    assert {"p15", "q16h200", "q16h256", "p31"} <= set(TC.IDS)
    assert all(cs[n]["hidden"] > 128 for n in ("p15", "q16h200", "q16h256"))                 # the pass-staged classes
    assert any(c["C"] % 2 for c in cs.values()) and any(not c["graph"] for c in cs.values())
    assert any(not c["gn"] for c in cs.values()) and any(c["H"] * c["W"] % 32 for c in cs.values())
    assert cs["neg"]["thr"] < 0
    have = set()
    for n in TC.IDS:
        have |= set(_direction(n))
    assert have == set(S.DIRECTION_FIELDS)                                                   # every tensor of a direction


@pytest.mark.parametrize("name", TC.IDS)
def test_step_parity(name):
    r = _one_step(name)
    d, w, keep, f = _desc_weights(name)
    x_plain, _ = S.step(d, w, r["x"].to(DEV), fire=f)
    assert PZ.same_bytes(r["x_out"], x_plain), "x_out is not gnca_step_f32's"
    assert float(np.abs(r["x_out"].cpu().numpy() - r["x_ref"]).max()) <= 2e-5, name
    ref = r["v_ref"]
    bound = 2e-5 * float(np.abs(ref).max()) + 1e-6
    err = float(np.abs(r["v_out"].cpu().numpy() - ref).max())
    print(f"[param tangent parity] {name}: err {err:.3e} bound {bound:.3e} err/bound {err / bound:.3f}")
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("name", TC.IDS)
def test_duality_on_the_device(name):
    """<gy, v'> == <gx, v> + sum_theta <g_theta, dtheta> with (gx, g_theta) from gnca_step_bwd_f32; the dot
    products in float64 on the host."""
    r = _one_step(name)
    d, w, keep, f = _desc_weights(name)
    gy = TC.cotangent(name)
    want = {n: p for n, p in _model(name).named_parameters() if n in S.DIRECTION_FIELDS}
    gx, gw = S.step_backward(d, w, r["x"].to(DEV), gy.to(DEV), fire=f, want=want)
    assert set(gw) >= set(r["dp"])
    gx = gx.cpu().numpy().astype(np.float64)
    gy64, v64 = gy.numpy().astype(np.float64), r["v"].numpy().astype(np.float64)
    lhs = float((gy64 * r["v_out"].cpu().numpy().astype(np.float64)).sum())
    rhs = float((gx * v64).sum())
    tol_v = 2e-5 * float(np.abs(r["v_ref"]).max()) + 1e-6
    tol_gx = 2e-5 * float(np.abs(gx).max()) + 1e-6
    bound = float(np.abs(gy64).sum()) * tol_v + float(np.abs(v64).sum()) * tol_gx
    for k, dt in _d64(r["dp"]).items():
        g = gw[k].cpu().numpy().astype(np.float64).reshape(dt.shape)
        rhs += float((g * dt).sum())
        bound += float(np.abs(dt).sum()) * (2e-5 * float(np.abs(g).max()) + 1e-6)
    print(f"[param tangent duality] {name}: |lhs - rhs| {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound, (name, lhs, rhs, bound)


@pytest.mark.parametrize("name", EXACT_IDS)
def test_exactness(name):
    r = _one_step(name)
    m = _model(name)
    x, v, dp = r["x"].to(DEV), r["v"].to(DEV), r["dpd"]
    zero = {k: torch.zeros_like(t) for k, t in dp.items()}
    c = TC.case(name)
    kw = dict(offsets=TC.offsets(name)[0]) if c["graph"] else {}
    f = TC.fire_mask(name)
    if f is not None:
        kw["fire"] = f.to(DEV)
    x_plain, v_plain = m.tangent_step(x, v, c["fire_rate"], **kw)            # the state tangent, dparams=None
    assert PZ.same_bytes(r["x_out"], x_plain), "x_out moved with a direction"
    for z in (zero, {}):
        xo, vo = _step(name, x, v, z)
        assert torch.equal(vo, v_plain) and PZ.same_bytes(xo, x_plain), "a zero direction is not the state tangent"
    _, z0 = _step(name, x, torch.zeros_like(v), zero)
    assert not z0.any() and torch.equal(z0, torch.zeros_like(z0)), "v = 0, dtheta = 0 does not give zeros"
    _, zn = _step(name, x, None, dp)                                          # v=None: a zero tangent
    _, ze = _step(name, x, torch.zeros_like(v), dp)
    assert PZ.same_bytes(zn, ze) and zn.any()
    _, v2 = _step(name, x, 2 * v, {k: 2 * t for k, t in dp.items()})
    assert PZ.same_bytes(v2, 2 * r["v_out"]), "tangent(x, 2v, 2dtheta) != 2 tangent(x, v, dtheta) bitwise"
    _, again = _step(name, x, v, dp)
    assert PZ.same_bytes(again, r["v_out"]), "not repeatable"
    B = x.shape[0]
    active = torch.ones(B, dtype=torch.bool, device=DEV)
    active[B - 1] = False
    xo, vo = _step(name, x, v, dp, active=active)
    assert PZ.same_bytes(vo[B - 1], v[B - 1]) and PZ.same_bytes(xo[B - 1], x[B - 1]), "an inactive sample changed"
    assert PZ.same_bytes(vo[:B - 1], r["v_out"][:B - 1]) and PZ.same_bytes(xo[:B - 1], r["x_out"][:B - 1])
    # a sample's result does not depend on its batch
    x2, v2 = TC.state(name, extra=1).to(DEV), TC.tangent(name, extra=1).to(DEV)
    x2[0], v2[0] = x[0], v[0]
    fk = dict(fire=f) if f is not None else {}
    if f is not None:
        f2 = TC.fire_mask(name, extra=1).clone()
        f2[0] = f[0]
        fk = dict(fire=f2)
    xo2, vo2 = _step(name, x2, v2, dp, **fk)
    assert PZ.same_bytes(vo2[0], r["v_out"][0]) and PZ.same_bytes(xo2[0], r["x_out"][0])
    if B > 1:
        assert not PZ.same_bytes(vo2[1:], r["v_out"][1:])


# ---------------------------------------------------------------------------------------------
# Rollouts
# ---------------------------------------------------------------------------------------------
def _sched(name, mode):
    """Keyword arguments of a 4-step schedule: nsteps, per-step rates and gains with a message-off step,
    and hash, rand or mask fire (tests/test_gpu_tangent.py's)."""
    c = TC.case(name)
    B = c["B"]
    kw = dict(fire_rate=[0.5, 1.0, 0.7, 0.5], min_steps=1,
              nsteps=torch.tensor([T, 2, 3][:B], dtype=torch.int32, device=DEV))
    if c["graph"]:
        kw.update(message_gain=[c["msg"], 0.0, 0.1, c["msg"]], offsets=TC.offsets(name, T))
    g = torch.Generator().manual_seed(99 + TC.seed(name))
    u = torch.rand(T, B, 1, c["H"], c["W"], generator=g)
    if mode == "hash":
        kw.update(seed=1234, sample_base=5)
    elif mode == "rand":
        kw.update(fire=u.to(DEV))
    else:
        kw.update(fire=(u <= 0.5).to(torch.uint8).to(DEV))
    return kw


def _chain(name, mode, x, v, dp, kw):
    """The same schedule as a chain of tangent_step(..., dparams=) calls: the states and tangents after each step."""
    c = TC.case(name)
    m = _model(name)
    xs, vs = [], []
    for t in range(T):
        active = (t < kw["min_steps"]) | (t < kw["nsteps"])
        rate = kw["fire_rate"][t]
        skw = {}
        if c["graph"]:
            skw["offsets"] = kw["offsets"][t]
        if mode == "hash":
            if rate < 1.0:
                d = TC.desc(name, skw.get("offsets", []), fire_mode=L.FIRE_HASH, fire_rate=rate)
                d.rng_seed, d.rng_step, d.sample_base = 1234, t, 5
                skw["fire"] = S.fire_mask(d, DEV)
        else:
            skw["fire"] = kw["fire"][t]
        old = getattr(m, "message_gain", None)
        if c["graph"]:
            m.message_gain = kw["message_gain"][t]
        try:
            x, v = m.tangent_step(x, v, rate, active=active, dparams=dp, **skw)
        finally:
            if c["graph"]:
                m.message_gain = old
        xs.append(x)
        vs.append(v)
    return xs, vs


@pytest.mark.parametrize("mode", ("hash", "rand", "mask"))
@pytest.mark.parametrize("name", ROLL_IDS)
def test_rollout_is_the_chain_of_steps(name, mode):
    m = _model(name)
    x, v, dp = TC.state(name).to(DEV), TC.tangent(name).to(DEV), _direction(name, dev=DEV)
    kw = _sched(name, mode)
    res = m.rollout_tangent(x, v, T, dparams=dp, **kw)
    xs, vs = _chain(name, mode, x, v, dp, kw)
    assert PZ.same_bytes(res.x_final, xs[-1]) and PZ.same_bytes(res.v_final, vs[-1]), PZ.diff(res.v_final, vs[-1])
    with torch.no_grad():
        plain = m.rollout(x, T, **kw)
    assert PZ.same_bytes(res.x_final, plain), "x_final is not the no-grad rollout()'s"
    assert res.steps == [] and tuple(res.log_norm.shape) == (0, x.shape[0])
    state_only = m.rollout_tangent(x, v, T, **kw)
    assert not PZ.same_bytes(state_only.v_final, res.v_final), "the direction had no effect"
    zero = m.rollout_tangent(x, v, T, dparams={k: torch.zeros_like(t) for k, t in dp.items()}, **kw)
    assert torch.equal(zero.v_final, state_only.v_final)
    again = m.rollout_tangent(x, v, T, dparams=dp, **kw)
    assert PZ.same_bytes(again.v_final, res.v_final) and PZ.same_bytes(again.x_final, res.x_final)
    x2, v2 = TC.state(name, extra=1).to(DEV), TC.tangent(name, extra=1).to(DEV)
    x2[0], v2[0] = x[0], v[0]
    other = m.rollout_tangent(x2, v2, T, dparams=dp, **kw)
    assert PZ.same_bytes(other.v_final[0], res.v_final[0]) and PZ.same_bytes(other.x_final[0], res.x_final[0])


@pytest.mark.parametrize("name", ("p13", "p5"))
def test_log_norms(name):
    m = _model(name)
    c = TC.case(name)
    x, dp = TC.state(name).to(DEV), _direction(name, dev=DEV)
    B = x.shape[0]
    kw = _sched(name, "hash")
    rec = [1, 3, 4]
    res = m.rollout_tangent(x, None, T, record=rec, dparams=dp, **kw)      # v = 0: the weights alone
    _, vs = _chain(name, "hash", x, torch.zeros_like(x), dp, kw)
    assert res.steps == rec and res.log_norm.dtype == torch.float64 and tuple(res.log_norm.shape) == (3, B)
    assert PZ.same_bytes(res.v_final, vs[-1])
    N = c["C"] * c["H"] * c["W"]
    ln = res.log_norm.cpu().numpy()
    for i, r in enumerate(rec):
        v64 = vs[r - 1].cpu().numpy().astype(np.float64).reshape(B, -1)
        ref = 0.5 * np.log((v64 * v64).sum(1))
        assert np.isfinite(ref).all()                   # the norm terms reach every cell: no zero tangent
        err = np.abs(ln[i] - ref)
        assert (err <= N * 2.0 ** -52 * np.maximum(1.0, np.abs(ref))).all(), (name, r, err)   # as test_log_norms
    with pytest.raises(ValueError):
        m.rollout_tangent(x, None, T, record=rec, renormalize=True, dparams=dp, **kw)


def _trainer_case(name):
    """(model, x, schedule keywords, float64 step list) of the rollout duality test: 2 x 24 x 24, T = 24, per-sample
    nsteps, a uint8 fire mask at rate 0.5."""
    c = TC.case(name)
    TT, B, H, W = 24, 2, 24, 24
    g = torch.Generator().manual_seed(4242 + TC.seed(name))
    x = torch.rand(B, c["C"], H, W, generator=g)
    x[:, 4:] = torch.randn(B, c["C"] - 4, H, W, generator=g)
    x[:, 3, :H // 3] = 0.0
    fire = (torch.rand(TT, B, 1, H, W, generator=g) <= 0.5).to(torch.uint8)
    gT = torch.randn(B, c["C"], H, W, generator=g)
    import random
    r, rr = c["radius"], random.Random(TC.seed(name))
    pool = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if not (abs(dy) <= 1 and abs(dx) <= 1)]
    offs = [rr.sample(pool, min(c["K"], len(pool))) for _ in range(TT)]
    nsteps = torch.tensor([TT, 17], dtype=torch.int32)
    return TT, x, fire, gT, offs, nsteps


@pytest.mark.parametrize("name", ("p6", "t72"))
def test_rollout_duality_against_the_shipped_bptt(name):
    """<g, v_T> from rollout_tangent(x, None, dparams=dtheta) against sum_theta <param.grad, dtheta> from
    model.rollout(...) with x_T.backward(g), T = 24 with per-sample nsteps, and both against the float64 reference
    chain.  The reference is teacher-forced as tests/test_gpu_bptt_long.py's: every step takes the float64 copy of
    the GPU's own input state and the GPU's own post mask, and carries the tangent in float64.  Bounds: the
    project's BPTT bound 5e-5 * max|ref| + 1e-6 per element, folded into an inner product as the step duality
    test folds the step bound."""
    c = TC.case(name)
    m = TC.model(name, DEV)
    TT, x, fire, gT, offs, nsteps = _trainer_case(name)
    dp = _direction(name, extra=3)
    dpd = {k: t.to(DEV) for k, t in dp.items()}
    kw = dict(fire_rate=0.5, fire=fire.to(DEV), offsets=offs, nsteps=nsteps.to(DEV))
    xd = x.to(DEV)
    res = m.rollout_tangent(xd, None, TT, dparams=dpd, **kw)
    for p in m.parameters():
        p.grad = None
    x_T = m.rollout(xd.clone().requires_grad_(False), TT, **kw)
    assert PZ.same_bytes(x_T.detach(), res.x_final)
    x_T.backward(gT.to(DEV))
    # the GPU's states, step by step (bitwise the rollout's: test_rollout_is_the_chain_of_steps)
    xs, cur = [xd], xd
    with torch.no_grad():
        for t in range(TT):
            cur = m.tangent_step(cur, torch.zeros_like(cur), 0.5, active=(nsteps > t).to(DEV), offsets=offs[t],
                                 fire=fire[t].to(DEV))[0]
            xs.append(cur)
    assert PZ.same_bytes(xs[-1], res.x_final)
    p64, cfg, d64 = TC.params64(name), TC.oracle_cfg(name), _d64(dp)
    v64 = np.zeros(tuple(x.shape), np.float64)
    for t in range(TT):
        act = (nsteps > t).numpy()
        post = _post_of(xs[t + 1].cpu().numpy(), c["thr"])
        _, v64 = PR.rollout_param_jvp(xs[t].cpu().numpy().astype(np.float64), p64, cfg, v64, d64,
                                      [dict(chosen=offs[t], active=act, fire_mask=fire[t].numpy().astype(np.float64),
                                            post_alive=post)])
    g64 = gT.numpy().astype(np.float64)
    ref = float((g64 * v64).sum())
    lhs = float((g64 * res.v_final.cpu().numpy().astype(np.float64)).sum())
    bound_v = float(np.abs(g64).sum()) * (5e-5 * float(np.abs(v64).max()) + 1e-6)
    rhs, bound_w = 0.0, 0.0
    grads = dict(m.named_parameters())
    for k, dt in d64.items():
        g = grads[k].grad.cpu().numpy().astype(np.float64)
        rhs += float((g * dt).sum())
        bound_w += float(np.abs(dt).sum()) * (5e-5 * float(np.abs(g).max()) + 1e-6)
    print(f"[param tangent rollout duality] {name}: ref {ref:.6e} tangent {lhs:.6e} bptt {rhs:.6e} "
          f"|tangent - ref| {abs(lhs - ref):.3e} / {bound_v:.3e}  |bptt - ref| {abs(rhs - ref):.3e} / {bound_w:.3e}")
    assert abs(lhs - ref) <= bound_v, (name, lhs, ref, bound_v)
    assert abs(rhs - ref) <= bound_w, (name, rhs, ref, bound_w)
    assert abs(lhs - rhs) <= bound_v + bound_w, (name, lhs, rhs)


# ---------------------------------------------------------------------------------------------
# The block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("p13", "q16h200"))
def test_block_is_the_single_direction_call_per_pair(name):
    m = _model(name)
    K = 3
    x = TC.state(name).to(DEV)
    V = torch.stack([TC.tangent(name, extra=j) for j in range(K)]).to(DEV)
    dps = [_direction(name, extra=j, dev=DEV) for j in range(K)]
    dps[1] = {}                                             # a pair with a zero direction
    kw = _sched(name, "hash")
    rec = [2, 4]
    res = m.rollout_tangent_block(x, V, T, record=rec, orthonormalize=False, dparams=dps, **kw)
    for j in range(K):
        one = m.rollout_tangent(x, V[j], T, record=rec, dparams=dps[j], **kw)
        assert PZ.same_bytes(res.v_final[j], one.v_final), j
        assert PZ.same_bytes(res.log_r[:, :, j].contiguous(), one.log_norm), j
        assert PZ.same_bytes(res.x_final, one.x_final)
    zero_v = m.rollout_tangent_block(x, None, T, orthonormalize=False, dparams=dps, **kw)
    assert tuple(zero_v.v_final.shape) == tuple(V.shape) and not zero_v.v_final[1].any() and zero_v.v_final[0].any()
    with pytest.raises(ValueError):
        m.rollout_tangent_block(x, V, T, record=rec, orthonormalize=True, dparams=dps, **kw)
    with pytest.raises(ValueError):
        m.rollout_tangent_block(x, V, T, record=rec, dparams=dps, **kw)


# ---------------------------------------------------------------------------------------------
# Guarded, poisoned buffers and the stream legs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("p13", "p5", "q16h200"))
def test_poisoned_buffers_step(name):
    x, v, dp = TC.state(name).to(DEV), TC.tangent(name).to(DEV), _direction(name, dev=DEV)
    B = x.shape[0]
    active = torch.ones(B, dtype=torch.bool, device=DEV)
    active[0] = False

    def call(P):
        xo, vo = _step(name, P.guard(x), P.guard(v), {k: P.guard(t) for k, t in dp.items()}, active=P.guard(active))
        return {"x_out": xo, "v_out": vo}
    out = PZ.run_fills(call, f"tangent_step_params:{name}")
    assert torch.isfinite(out["v_out"]).all() and torch.isfinite(out["x_out"]).all()   # every byte written


@pytest.mark.parametrize("entry", ("rollout", "block"))
@pytest.mark.parametrize("name", ("p13", "p5"))
def test_poisoned_buffers_rollout(name, entry):
    m = _model(name)
    x, v, dp = TC.state(name).to(DEV), TC.tangent(name).to(DEV), _direction(name, dev=DEV)
    V = torch.stack([TC.tangent(name, extra=j) for j in range(2)]).to(DEV)
    kw = _sched(name, "mask")

    def call(P):
        k = dict(kw, nsteps=P.guard(kw["nsteps"]), fire=P.guard(kw["fire"]))
        d = {n: P.guard(t) for n, t in dp.items()}
        if entry == "rollout":
            r = m.rollout_tangent(P.guard(x), P.guard(v), T, record=[2, 4], dparams=d, **k)
            return {"x_final": r.x_final, "v_final": r.v_final, "log_norm": r.log_norm}
        r = m.rollout_tangent_block(P.guard(x), P.guard(V), T, record=[2, 4], orthonormalize=False, dparams=[d, d], **k)
        return {"x_final": r.x_final, "v_final": r.v_final, "log_r": r.log_r}
    out = PZ.run_fills(call, f"rollout_tangent_params:{entry}:{name}")
    for t in out.values():
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("leg", ("side", "capture"))
@pytest.mark.parametrize("entry", ("step", "rollout", "block"))
def test_stream_legs(entry, leg):
    name = "p13"
    m = _model(name)
    c = TC.case(name)
    B = c["B"]
    sets = []
    for e in (0, 1):
        s = {"x": TC.state(name, extra=e).to(DEV)}
        s.update({"d:" + k: t for k, t in _direction(name, extra=e, dev=DEV).items()})
        if entry == "block":
            s["V"] = torch.stack([TC.tangent(name, extra=e + 2 * j) for j in range(2)]).to(DEV)
        else:
            s["v"] = TC.tangent(name, extra=e).to(DEV)
        if entry == "step":
            s["fire"] = TC.fire_mask(name, extra=e).to(DEV)
            s["active"] = torch.tensor([1, e][:B], dtype=torch.uint8, device=DEV)
        else:
            s["nsteps"] = torch.tensor([T, 2 + e][:B], dtype=torch.int32, device=DEV)
        sets.append(s)
    offs = TC.offsets(name, T)

    def call(b):
        d = {k[2:]: t for k, t in b.items() if k.startswith("d:")}
        if entry == "step":
            xo, vo = m.tangent_step(b["x"], b["v"], c["fire_rate"], active=b["active"], offsets=offs[0], fire=b["fire"],
                                    dparams=d)
            return {"x_out": xo, "v_out": vo}
        if entry == "rollout":
            r = m.rollout_tangent(b["x"], b["v"], T, record=[2, 4], fire_rate=0.5, seed=3, nsteps=b["nsteps"],
                                  offsets=offs, dparams=d)
            return {"x_final": r.x_final, "v_final": r.v_final, "log_norm": r.log_norm}
        r = m.rollout_tangent_block(b["x"], b["V"], T, record=[2, 4], orthonormalize=False, fire_rate=0.5, seed=3,
                                    nsteps=b["nsteps"], offsets=offs, dparams=[d, {}])
        return {"x_final": r.x_final, "v_final": r.v_final, "log_r": r.log_r}
    ST.run(ST.Case(f"param_tangent:{entry}", sets, call), legs=("eager", leg))
