"""The forward-mode tangent on the GPU: ``tangent_step`` / ``rollout_tangent`` (gnca_step_tangent /
gnca_rollout_tangent) against the float64 reference tests/tangent_ref.py, against the HIP backward by
duality, and against themselves where the arithmetic is exact (linearity in v, the chain of steps,
reproducibility, sample independence), plus the log norms, the guarded and poisoned buffers and the
three stream legs.  Cases: tests/tangent_cases.py.

Parity bound (the backward's): ``2e-5 * max|ref| + 1e-6`` per element.
"""
import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import poison as PZ
from tests import shape_class_cases as SC
from tests import streams as ST
from tests import tangent_cases as TC
from tests import tangent_ref as TR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROLL_IDS = ("p6", "p13", "p5", "neg")


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


def _step(name, x, v, *, active=None, fire="case", offs=None):
    """model.tangent_step on the case's first offsets and fire mask."""
    c = TC.case(name)
    m = _model(name)
    kw = {}
    if c["graph"]:
        kw["offsets"] = TC.offsets(name)[0] if offs is None else offs
    f = TC.fire_mask(name) if isinstance(fire, str) else fire
    if f is not None:
        kw["fire"] = f.to(DEV)
    return m.tangent_step(x, v, c["fire_rate"], active=active, **kw)


_STEP: dict = {}


def _one_step(name):
    """The case's GPU step (x_out, v_out) and its float64 reference, once per case and left unchanged."""
    if name in _STEP:
        return _STEP[name]
    c = TC.case(name)
    x, v = TC.state(name), TC.tangent(name)
    x_out, v_out = _step(name, x.to(DEV), v.to(DEV))
    torch.cuda.synchronize()
    xo = x_out.cpu().numpy()
    f = TC.fire_mask(name)
    # the post mask of the GPU's own output (tests/test_gpu_bptt_long.py): 3x3 pool of its alpha > float32(thr)
    a = xo[:, 3:4]
    ap = np.full((a.shape[0], 1, a.shape[2] + 2, a.shape[3] + 2), -np.inf, np.float32)
    ap[:, :, 1:-1, 1:-1] = a
    pooled = np.max([ap[:, :, i:i + a.shape[2], j:j + a.shape[3]] for i in range(3) for j in range(3)], axis=0)
    post = (pooled > np.float32(c["thr"])).astype(np.float64)
    if c["thr"] < 0:
        post = None     # a gated alpha (+-0) exceeds a negative threshold: the oracle's own post mask stands
    x_ref, v_ref = TR.nca_step_jvp(x.numpy().astype(np.float64), TC.params64(name), TC.oracle_cfg(name),
                                   v.numpy().astype(np.float64), chosen=TC.offsets(name)[0] if c["graph"] else None,
                                   fire_mask=None if f is None else f.numpy().astype(np.float64), post_alive=post)
    v_ref.setflags(write=False)
    _STEP[name] = dict(x=x, v=v, x_out=x_out, v_out=v_out, v_ref=v_ref, x_ref=x_ref)
    return _STEP[name]


def _desc_weights(name):
    c = TC.case(name)
    f = TC.fire_mask(name)
    d = TC.desc(name, TC.offsets(name)[0] if c["graph"] else [], fire_mode=L.FIRE_MASK_U8 if f is not None else L.FIRE_NONE)
    w, keep = S.make_weights(SC.weight_tensors(_model(name)))
    return d, w, keep, None if f is None else f.to(DEV)


def test_cases_reach_every_path():
    cs = [TC.case(n) for n in TC.IDS]
    assert not any(c["zp"] for c in cs)
    assert set(TC.SC_IDS) == {n for n in SC.IDS if not SC.CASES[n]["zp"]} and len(TC.SC_IDS) == 23   # all of them
    assert {TC.case(n)["C"] // 2 for n in TC.SC_IDS if TC.case(n)["graph"]} >= {6, 10, 12, 16}   # ragged Wm gather passes
    assert TC.case("neg")["thr"] < 0 and TC.state("neg")[:, 3].min() < TC.case("neg")["thr"] < TC.state("neg")[:, 3].max()
    assert any(c["C"] % 4 for c in cs) and any(not c["graph"] for c in cs) and any(not c["gn"] for c in cs)
    assert "p31" in TC.IDS and any(c["hidden"] > 128 for c in cs)          # hidden slices in TA (two of 128)
    assert {1, 2, 4} == {1 if c["hidden"] <= 32 else 2 if c["hidden"] <= 64 else 4 for c in cs}   # every TA instance
    assert any(c["H"] * c["W"] % 32 for c in cs)                            # a ragged last wave tile
    t = TC.case("t72")
    assert (t["C"], t["hidden"], t["radius"], t["K"], t["B"], t["H"], t["W"]) == (16, 128, 4, 8, 2, 72, 72)


@pytest.mark.parametrize("name", TC.IDS)
def test_step_parity(name):
    r = _one_step(name)
    d, w, keep, f = _desc_weights(name)
    x_plain, _ = S.step(d, w, r["x"].to(DEV), fire=f)
    assert PZ.same_bytes(r["x_out"], x_plain), "x_out is not gnca_step_f32's"
    # (the forward's own bound: the reference ran with the post mask this comparison confirms)
    assert float(np.abs(r["x_out"].cpu().numpy() - r["x_ref"]).max()) <= 2e-5, name
    ref = r["v_ref"]
    bound = 2e-5 * float(np.abs(ref).max()) + 1e-6
    err = float(np.abs(r["v_out"].cpu().numpy() - ref).max())
    print(f"[tangent parity] {name}: err {err:.3e} bound {bound:.3e} err/bound {err / bound:.3f}")
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("name", TC.IDS)
def test_duality_on_the_device(name):
    """<gy, v_out> == <gx, v> with gx from gnca_step_bwd_f32; both dot products in float64 on the host."""
    r = _one_step(name)
    d, w, keep, f = _desc_weights(name)
    gy = TC.cotangent(name)
    gx, _ = S.step_backward(d, w, r["x"].to(DEV), gy.to(DEV), fire=f)
    gx = gx.cpu().numpy().astype(np.float64)
    gy64, v64 = gy.numpy().astype(np.float64), r["v"].numpy().astype(np.float64)
    lhs = float((gy64 * r["v_out"].cpu().numpy().astype(np.float64)).sum())
    rhs = float((gx * v64).sum())
    tol_v = 2e-5 * float(np.abs(r["v_ref"]).max()) + 1e-6
    tol_gx = 2e-5 * float(np.abs(gx).max()) + 1e-6
    bound = float(np.abs(gy64).sum()) * tol_v + float(np.abs(v64).sum()) * tol_gx
    print(f"[tangent duality] {name}: |lhs - rhs| {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound, (name, lhs, rhs, bound)


@pytest.mark.parametrize("name", ("p5", "p13", "p31", "q16h256"))
def test_exact_linearity(name):
    r = _one_step(name)
    x, v = r["x"].to(DEV), r["v"].to(DEV)
    _, z = _step(name, x, torch.zeros_like(v))
    assert not z.any() and PZ.same_bytes(z, torch.zeros_like(z)), "v = 0 does not give bitwise zeros"
    _, v2 = _step(name, x, 2 * v)
    assert PZ.same_bytes(v2, 2 * r["v_out"]), "tangent(x, 2v) != 2 tangent(x, v) bitwise"
    B = x.shape[0]
    active = torch.ones(B, dtype=torch.bool, device=DEV)
    active[B - 1] = False
    xo, vo = _step(name, x, v, active=active)
    assert PZ.same_bytes(vo[B - 1], v[B - 1]) and PZ.same_bytes(xo[B - 1], x[B - 1]), "an inactive sample changed"
    assert PZ.same_bytes(vo[:B - 1], r["v_out"][:B - 1]) and PZ.same_bytes(xo[:B - 1], r["x_out"][:B - 1])
    d, w, keep, f = _desc_weights(name)
    x_masked, _ = S.step(d, w, x, fire=f, active=active)
    assert PZ.same_bytes(xo, x_masked), "x_out is not gnca_step_masked_f32's"


@pytest.mark.parametrize("name", ("p13", "p5"))
def test_draws_are_forward_s(name):
    """With ``offsets`` / ``fire`` omitted, tangent_step consumes Python's random and torch's generator exactly
    as forward does: the same seeds give forward's x_out, and leave both generators where forward leaves them."""
    import random
    m, c = _model(name), TC.case(name)
    x, v = TC.state(name).to(DEV), TC.tangent(name).to(DEV)

    def seeded(fn):
        random.seed(21)
        torch.manual_seed(22)
        out = fn()
        return out, random.getstate(), torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    with torch.no_grad():
        want, py, cu, cpu = seeded(lambda: m(x, c["fire_rate"]))
    (xo, vo), py2, cu2, cpu2 = seeded(lambda: m.tangent_step(x, v, c["fire_rate"]))
    assert PZ.same_bytes(xo, want), "tangent_step drew other offsets or another fire mask than forward"
    assert py2 == py and torch.equal(cu2, cu) and torch.equal(cpu2, cpu)
    assert not vo.requires_grad and not xo.requires_grad


def test_schedule_errors_through_rollout_tangent():
    """build_schedule's ValueErrors reach the caller of rollout_tangent, before anything is drawn."""
    import random
    m = _model("p13")
    x, v = TC.state("p13").to(DEV), TC.tangent("p13").to(DEV)
    offs = TC.offsets("p13", 4)
    bad_fire = torch.rand(3, 2, 1, 24, 24, device=DEV)
    for kw in (dict(fire_rate=[0.5]), dict(message_gain=[0.1] * 3), dict(offsets=offs[:3]), dict(offsets=[o[:2] for o in offs[:1]] + offs[1:]),
               dict(seed="s", fire_rate=0.5), dict(nsteps=torch.zeros(3, dtype=torch.int32, device=DEV)),
               dict(nsteps=torch.zeros(2, dtype=torch.int32)), dict(min_steps=-1), dict(fire=bad_fire),
               dict(offsets=[[(1, 2, 3)]] * 4)):
        random.seed(5)
        torch.manual_seed(5)
        py, cpu, cu = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
        with pytest.raises(ValueError):
            m.rollout_tangent(x, v, 4, **kw)
        assert random.getstate() == py, kw
        assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(DEV), cu), kw


# ---------------------------------------------------------------------------------------------
# Rollouts
# ---------------------------------------------------------------------------------------------
T = 4


def _sched(name, mode):
    """Keyword arguments of a 4-step schedule: nsteps, per-step rates and gains with a message-off step,
    and hash, rand or mask fire."""
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


def _chain(name, mode, x, v, kw):
    """The same schedule as a chain of tangent_step calls; returns the states and tangents after each step."""
    c = TC.case(name)
    m = _model(name)
    B = c["B"]
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
            x, v = m.tangent_step(x, v, rate, active=active, **skw)
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
    x, v = TC.state(name).to(DEV), TC.tangent(name).to(DEV)
    kw = _sched(name, mode)
    res = m.rollout_tangent(x, v, T, **kw)
    xs, vs = _chain(name, mode, x, v, kw)
    assert PZ.same_bytes(res.x_final, xs[-1]) and PZ.same_bytes(res.v_final, vs[-1]), PZ.diff(res.v_final, vs[-1])
    with torch.no_grad():
        plain = m.rollout(x, T, **kw)
    assert PZ.same_bytes(res.x_final, plain), "x_final is not the no-grad rollout()'s"
    assert res.steps == [] and tuple(res.log_norm.shape) == (0, x.shape[0])
    # reproducible, and a sample's outputs do not depend on the other samples
    again = m.rollout_tangent(x, v, T, **kw)
    assert PZ.same_bytes(again.v_final, res.v_final) and PZ.same_bytes(again.x_final, res.x_final)
    x2, v2 = TC.state(name, extra=1).to(DEV), TC.tangent(name, extra=1).to(DEV)
    x2[0], v2[0] = x[0], v[0]
    other = m.rollout_tangent(x2, v2, T, **kw)
    assert PZ.same_bytes(other.v_final[0], res.v_final[0]) and PZ.same_bytes(other.x_final[0], res.x_final[0])
    assert not PZ.same_bytes(other.v_final[1:], res.v_final[1:])


def test_uniform_schedule_matches_the_rollout_pipeline():
    """x_final against the no-grad rollout() of a UNIFORM schedule, which runs the large-batch pipeline."""
    name = "p13"
    m = _model(name)
    x, v = TC.state(name).to(DEV), TC.tangent(name).to(DEV)
    kw = dict(fire_rate=0.5, seed=7, offsets=TC.offsets(name, T))
    res = m.rollout_tangent(x, v, T, **kw)
    with torch.no_grad():
        assert PZ.same_bytes(res.x_final, m.rollout(x, T, **kw))
    zero = m.rollout_tangent(x, v, 0)
    assert PZ.same_bytes(zero.x_final, x) and PZ.same_bytes(zero.v_final, v)


@pytest.mark.parametrize("name", ("p13", "p5"))
def test_log_norms(name):
    m = _model(name)
    c = TC.case(name)
    x, v = TC.state(name).to(DEV), TC.tangent(name).to(DEV)
    B = x.shape[0]
    v[B - 1] = 0.0                                   # a zero tangent: -inf, stays zero
    kw = _sched(name, "hash")
    rec = [1, 3, 4]
    res = m.rollout_tangent(x, v, T, record=rec, **kw)
    _, vs = _chain(name, "hash", x, v, kw)
    assert res.steps == rec and res.log_norm.dtype == torch.float64 and tuple(res.log_norm.shape) == (3, B)
    assert PZ.same_bytes(res.v_final, vs[-1])
    N = c["C"] * c["H"] * c["W"]
    ln = res.log_norm.cpu().numpy()
    for i, r in enumerate(rec):
        v64 = vs[r - 1].cpu().numpy().astype(np.float64).reshape(B, -1)
        with np.errstate(divide="ignore"):
            ref = 0.5 * np.log((v64 * v64).sum(1))
        assert ln[i, B - 1] == -np.inf and ref[B - 1] == -np.inf
        err = np.abs(ln[i, :B - 1] - ref[:B - 1])
        # N * 2^-52 relative; for |log norm| < 1 the bound is taken absolute (N * 2^-52 itself), which is the
        # rounding of the fp64 sum, whose relative error d gives the log the absolute error d / 2
        assert (err <= N * 2.0 ** -52 * np.maximum(1.0, np.abs(ref[:B - 1]))).all(), (name, r, err)
    every = m.rollout_tangent(x, v, T, every=3, **kw)          # trace()'s rule: 3, and 4 as it is no multiple
    assert every.steps == [3, 4] and PZ.same_bytes(every.log_norm, res.log_norm[1:])
    # renormalised: the same curve within the step bound per renormalisation, unit norm, zero stays zero
    rn = m.rollout_tangent(x, v, T, record=rec, renormalize=True, **kw)
    assert PZ.same_bytes(rn.x_final, res.x_final)
    ln2 = rn.log_norm.cpu().numpy()
    for i in range(len(rec)):
        assert ln2[i, B - 1] == -np.inf
        assert (np.abs(ln2[i, :B - 1] - ln[i, :B - 1]) <= (i + 1) * 2e-5).all(), (name, i, ln2[i], ln[i])
    vf = rn.v_final.cpu().numpy().astype(np.float64).reshape(B, -1)
    norms = np.sqrt((vf * vf).sum(1))
    assert (np.abs(norms[:B - 1] - 1.0) <= 2.0 ** -22).all(), norms
    assert not vf[B - 1].any()


# ---------------------------------------------------------------------------------------------
# Guarded, poisoned buffers and the stream legs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("p13", "p5"))
def test_poisoned_buffers_step(name):
    x, v = TC.state(name).to(DEV), TC.tangent(name).to(DEV)
    B = x.shape[0]
    active = torch.ones(B, dtype=torch.bool, device=DEV)
    active[0] = False

    def call(P):
        xo, vo = _step(name, P.guard(x), P.guard(v), active=P.guard(active))
        return {"x_out": xo, "v_out": vo}
    out = PZ.run_fills(call, f"tangent_step:{name}")
    assert torch.isfinite(out["v_out"]).all() and torch.isfinite(out["x_out"]).all()   # every byte written


@pytest.mark.parametrize("name", ("p13", "p5"))
def test_poisoned_buffers_rollout(name):
    m = _model(name)
    x, v = TC.state(name).to(DEV), TC.tangent(name).to(DEV)
    kw = _sched(name, "mask")

    def call(P):
        k = dict(kw, nsteps=P.guard(kw["nsteps"]), fire=P.guard(kw["fire"]))
        r = m.rollout_tangent(P.guard(x), P.guard(v), T, record=[2, 4], renormalize=True, **k)
        return {"x_final": r.x_final, "v_final": r.v_final, "log_norm": r.log_norm}
    out = PZ.run_fills(call, f"rollout_tangent:{name}")
    for t in out.values():
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("leg", ("side", "capture"))
@pytest.mark.parametrize("entry", ("step", "rollout"))
def test_stream_legs(entry, leg):
    name = "p13"
    m = _model(name)
    c = TC.case(name)
    B = c["B"]
    sets = []
    for e in (0, 1):
        s = {"x": TC.state(name, extra=e).to(DEV), "v": TC.tangent(name, extra=e).to(DEV)}
        if entry == "step":
            s["fire"] = TC.fire_mask(name, extra=e).to(DEV)
            s["active"] = torch.tensor([1, e][:B], dtype=torch.uint8, device=DEV)
        else:
            s["nsteps"] = torch.tensor([T, 2 + e][:B], dtype=torch.int32, device=DEV)
        sets.append(s)
    offs = TC.offsets(name, T)

    def call(b):
        if entry == "step":
            xo, vo = m.tangent_step(b["x"], b["v"], c["fire_rate"], active=b["active"], offsets=offs[0], fire=b["fire"])
            return {"x_out": xo, "v_out": vo}
        r = m.rollout_tangent(b["x"], b["v"], T, record=[2, 4], renormalize=True, fire_rate=0.5, seed=3,
                              nsteps=b["nsteps"], offsets=offs)
        return {"x_final": r.x_final, "v_final": r.v_final, "log_norm": r.log_norm}
    ST.run(ST.Case(f"tangent:{entry}", sets, call), legs=("eager", leg))
