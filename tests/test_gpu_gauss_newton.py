"""rollout_gauss_newton(), loss_curvature() and cg_solve() on the GPU.

The curvature kernel alone against the float64 formula (one rounding) and bitwise against the shipped losses and
loss_tangent(); the rollout bitwise against rollout_objective(), rollout_objective_tangent(), rollout_tangent() +
loss_curvature() and rollout(recompute=True) + backward() (the same kernels in the same order), checkpointed against
the plain tape, repeated, and a sample alone against in a batch; the product against tests/gauss_newton_ref.py at the
GPU's own masks, with symmetry and the energy identity; conjugate gradients on the real operator; guarded, poisoned
buffers and the stream legs.  The schedules, states and helpers are tests/test_gpu_objective_tangent.py's.
"""
import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import ParamDirections, cg_solve, loss_curvature, loss_tangent
from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from graph_neural_cellular_automata_amd.loss import loss_premult_rgba, masked_loss
from tests import gauss_newton_ref as GR
from tests import poison as PZ
from tests import streams as ST
from tests import tangent_cases as TC
from tests import test_gpu_objective_tangent as OT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KNOBS = OT.KNOBS
KINDS = ("premult", "masked")
TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import os
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _knob_kw(kind):
    return {} if kind == "premult" else dict(zip(("alpha_thr", "lam_area", "lam_bg_alpha", "lam_bg_rgb"), KNOBS))


# ---------------------------------------------------------------------------------------------
# The kernel alone
# ---------------------------------------------------------------------------------------------
ALONE = ((11, 13, 3, True), (24, 24, 3, True), (24, 24, 3, False), (11, 13, 1, False))   # H, W, B, per-sample target


def _alone_inputs(H, W, B, per_sample):
    """A 5-channel state and tangent whose first four planes are read through their strides (a sample stride that
    is no multiple of 16 bytes); a target whose LAST sample has no alive cell when it is per-sample."""
    g = torch.Generator().manual_seed(8100 + H * W + 10 * B + int(per_sample))
    state = torch.randn(B, 5, H, W, generator=g)
    state[:, 3] = torch.rand(B, H, W, generator=g)
    state[:, :3, : H // 2, : W // 4] = 0.0
    target = OT._target(B, H, W, g, per_sample=per_sample)
    if per_sample and B > 1:
        target[-1, 3] *= 0.15                                  # alpha below the masked kind's threshold everywhere
    v = torch.randn(B, 5, H, W, generator=g)
    return state.to(DEV), target.to(DEV), v.to(DEV)


def _shipped_loss(kind, pred, target):
    with torch.no_grad():
        return loss_premult_rgba(pred, target) if kind == "premult" else masked_loss(pred, target, *KNOBS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,B,per_sample", ALONE)
def test_loss_curvature_alone(H, W, B, per_sample, kind):
    state, target, vt = _alone_inputs(H, W, B, per_sample)
    pred, v = state[:, :4], vt[:, :4]
    assert pred.stride(0) == 5 * H * W and ((H, W) != (11, 13) or (pred.stride(0) * 4) % 16 != 0)
    field, quad, losses, dl = loss_curvature(pred, v, target, kind, **_knob_kw(kind))
    assert field.dtype == torch.float32 and tuple(field.shape) == (B, 4, H, W)
    assert quad.dtype == torch.float64 and dl.dtype == torch.float64 and tuple(quad.shape) == tuple(dl.shape) == (B,)
    # bitwise the shipped loss and the shipped loss tangent with one direction
    assert PZ.same_bytes(losses, _shipped_loss(kind, pred, target))
    l1, d1 = loss_tangent(pred, v.contiguous()[None], target, kind, **_knob_kw(kind))
    assert PZ.same_bytes(l1, losses) and PZ.same_bytes(d1[0], dl)
    # the float64 formula on the float32 inputs: one rounding to float32
    tg = target.cpu().numpy()
    ref_f, ref_q = GR.tap_curvature(kind, pred.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64),
                                    tg if tg.ndim == 4 else tg[None], KNOBS)
    got_f, got_q = field.cpu().numpy().astype(np.float64), quad.cpu().numpy()
    err = np.abs(got_f - ref_f)
    bound = 2.0 ** -24 * np.abs(ref_f) + TINY
    print(f"[curvature] {kind} {H}x{W} B={B}: field max err / bound {float((err / bound).max()):.3e}  "
          f"quad rel err {float((np.abs(got_q - ref_q) / np.maximum(ref_q, TINY)).max()):.3e}")
    assert (err <= bound).all(), float((err / bound).max())
    # quad: 4HW non-negative terms, so sum |terms| is the value itself
    assert (np.abs(got_q - ref_q) <= 4 * H * W * 2.0 ** -52 * ref_q).all(), (got_q, ref_q)
    assert (got_q >= 0).all()
    # sum field * v = quad up to the rounding of the field
    terms = got_f * v.cpu().numpy().astype(np.float64)
    dot, mag = terms.sum(axis=(1, 2, 3)), np.abs(terms).sum(axis=(1, 2, 3))
    assert (np.abs(dot - got_q) <= 2.0 ** -24 * mag).all(), (dot, got_q, mag)
    if kind == "masked":
        alive = (tg.reshape(-1, 4, H, W)[:, 3] > np.float32(KNOBS[0]))
        if per_sample and B > 1:
            assert not alive[-1].any() and not field[-1].any() and float(quad[-1]) == 0.0   # an exactly zero field
        assert alive[0].any() and (~alive[0]).any() and float(quad[0]) > 0.0
    else:
        assert (got_q > 0).all()
    # bitwise repeatable; a sample's numbers do not depend on the batch around it
    f2, q2, l2, d2 = loss_curvature(pred, v, target, kind, **_knob_kw(kind))
    assert PZ.same_bytes(f2, field) and PZ.same_bytes(q2, quad) and PZ.same_bytes(d2, dl) and PZ.same_bytes(l2, losses)
    b = B - 1
    tb = target if target.dim() == 3 else target[b:b + 1]
    f1, q1, lb, db = loss_curvature(state[b:b + 1, :4], vt[b:b + 1, :4], tb, kind, **_knob_kw(kind))
    assert PZ.same_bytes(f1[0], field[b]) and PZ.same_bytes(q1, quad[b:b + 1]) and PZ.same_bytes(db, dl[b:b + 1])
    assert PZ.same_bytes(lb, losses[b:b + 1])


# ---------------------------------------------------------------------------------------------
# The rollout, bitwise
# ---------------------------------------------------------------------------------------------
_MODELS: dict = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = TC.model(name, DEV)
    return _MODELS[name]


def _inputs(name, T, extra=0):
    """(x, v, dparams, target) on the host: p5 takes ONE broadcast target, the others a per-sample one."""
    c = TC.case(name)
    x = TC.state(name)
    v = TC.tangent(name, extra=extra)
    dp = OT._direction(name, extra=extra)
    g = torch.Generator().manual_seed(61 + TC.seed(name))
    target = OT._target(c["B"], c["H"], c["W"], g, per_sample=name != "p5")
    return x, v, dp, target


def _outs(r):
    d = {"x_final": r.x_final, "losses": r.losses, "dlosses": r.dlosses, "quad": r.quad, "gx": r.gx,
         "energy": r.energy.reshape(1)}
    d.update({"p:" + n: t for n, t in r.product.items()})
    if r.fields is not None:
        d["fields"] = r.fields
    return d


def _same(a, b, what):
    a, b = _outs(a), _outs(b)
    assert list(a) == list(b), what
    bad = [k for k in a if not PZ.same_bytes(a[k], b[k])]
    assert not bad, (what, bad)


ROLL = (("p5", 6, dict(every=2), "mask"), ("p13", 6, dict(record=[1, 3, 6]), "hash"), ("p13", 5, dict(record=[2, 4]), "mask"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,T,taps,mode", ROLL, ids=[f"{r[0]}-{r[3]}-T{r[1]}" for r in ROLL])
def test_rollout_bitwise(name, T, taps, mode, kind):
    m = _model(name)
    x, v, dp, target = _inputs(name, T)
    kw, _ = OT._sched(name, T, mode)
    xd, vd, dpd, td = x.to(DEV), v.to(DEV), OT._dev(dp), target.to(DEV)
    B = x.shape[0]
    lk = OT._loss_kw(kind)
    res = m.rollout_gauss_newton(xd, T, td, dparams=dpd, v=vd, return_fields=True, **taps, **lk, **kw)
    R = len(res.steps)
    assert tuple(res.quad.shape) == tuple(res.dlosses.shape) == tuple(res.losses.shape) == (R, B)
    assert res.quad.dtype == torch.float64 and res.dlosses.dtype == torch.float64 and res.energy.dtype == torch.float64
    assert set(res.product) == {n for n, _ in m.named_parameters() if n in S.DIRECTION_FIELDS}
    for n, p in m.named_parameters():
        if n in res.product:
            assert res.product[n].shape == p.shape and torch.isfinite(res.product[n]).all()
    with torch.no_grad():
        obj = m.rollout_objective(xd, T, td, **taps, **lk, **kw)
    assert obj.steps == res.steps and PZ.same_bytes(res.x_final, obj.x_final) and PZ.same_bytes(res.losses, obj.losses)
    ot = m.rollout_objective_tangent(xd, T, td, V=vd[None], dparams=[dpd], **taps, **lk, **kw)
    assert PZ.same_bytes(res.dlosses, ot.dlosses[:, 0].contiguous())
    sc = float(np.float32(1.0 / B))                             # scale_r as the float32 the injection takes
    want = float(sum(sc * float(res.quad[r].sum()) for r in range(R)))
    assert abs(float(res.energy) - want) <= 1e-12 * want and want > 0.0
    # repeatable; the checkpointed tape changes no number, whatever the interval
    run = lambda **e: m.rollout_gauss_newton(xd, T, td, dparams=dpd, v=vd, return_fields=True, **taps, **lk,   # noqa: E731
                                             **kw, **e)
    _same(run(), res, "repeat")
    for k in (1, 2, 4, T, "auto"):
        _same(run(checkpoint_every=k), res, f"checkpoint_every={k}")
    # the parts: v alone and dparams alone run (a zero tangent made on the device, a missing direction)
    only_v = m.rollout_gauss_newton(xd, T, td, v=vd, **taps, **lk, **kw)
    only_d = m.rollout_gauss_newton(xd, T, td, dparams=dpd, **taps, **lk, **kw)
    zero = m.rollout_gauss_newton(xd, T, td, dparams=dpd, v=torch.zeros_like(vd), **taps, **lk, **kw)
    _same(only_d, zero, "v=None is a zero tangent")
    assert PZ.same_bytes(only_v.losses, res.losses) and float(only_v.energy) > 0.0
    # a sample alone against in a batch (mask fire: the masks of a sample do not depend on its index)
    if mode == "mask":
        b = B - 1
        w = [0.5 + 0.25 * r for r in range(R)]
        batch = m.rollout_gauss_newton(xd, T, td, dparams=dpd, v=vd, tap_weights=w, **taps, **lk, **kw)
        kb = dict(kw, nsteps=kw["nsteps"][b:b + 1].contiguous(), fire=kw["fire"][:, b:b + 1].contiguous())
        tb = td if td.dim() == 3 else td[b:b + 1]
        # (scale_r = tap_weights[r] / B: alone, B is 1, so the weights carry the batch's 1 / B)
        one = m.rollout_gauss_newton(xd[b:b + 1], T, tb, dparams=dpd, v=vd[b:b + 1], tap_weights=[t / B for t in w],
                                     **taps, **lk, **kb)
        for key in ("x_final", "gx"):
            assert PZ.same_bytes(getattr(one, key)[0], getattr(batch, key)[b]), key
        for key in ("losses", "dlosses", "quad"):
            assert PZ.same_bytes(getattr(one, key)[:, 0].contiguous(), getattr(batch, key)[:, b].contiguous()), key


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", (("p5", "mask"), ("p13", "hash")))
def test_single_tap_at_T_is_the_shipped_kernels_in_the_same_order(name, mode, kind):
    T = 5
    m = TC.model(name, DEV)
    x, v, dp, target = _inputs(name, T)
    kw, _ = OT._sched(name, T, mode)
    xd, vd, dpd, td = x.to(DEV), v.to(DEV), OT._dev(dp), target.to(DEV)
    B = x.shape[0]
    lk = OT._loss_kw(kind)
    w = 1.75
    res = m.rollout_gauss_newton(xd, T, td, dparams=dpd, v=vd, record=[T], tap_weights=[w], return_fields=True, **lk, **kw)
    tan = m.rollout_tangent(xd, vd, T, dparams=dpd, **kw)
    assert PZ.same_bytes(tan.x_final, res.x_final)
    field, quad, losses, dl = loss_curvature(res.x_final[:, :4], tan.v_final[:, :4], td, kind, **_knob_kw(kind))
    assert PZ.same_bytes(res.fields[0], field) and PZ.same_bytes(res.quad[0], quad)
    assert PZ.same_bytes(res.losses[0], losses) and PZ.same_bytes(res.dlosses[0], dl)
    # rollout(recompute=True) and backward() of the padded, scaled field: the same kernels in the same order
    for p in m.parameters():
        p.grad = None
    leaf = xd.clone().requires_grad_(True)
    out = m.rollout(leaf, T, recompute=True, **kw)
    assert PZ.same_bytes(out.detach(), res.x_final)
    scale = torch.tensor(w / B, dtype=torch.float32, device=DEV)
    gy = torch.zeros_like(out)
    gy[:, :4] = field * scale
    out.backward(gy)
    assert PZ.same_bytes(leaf.grad, res.gx), PZ.diff(leaf.grad, res.gx)
    assert res.gx.abs().max() > 0
    for n, p in m.named_parameters():
        if n in S.DIRECTION_FIELDS:
            assert PZ.same_bytes(p.grad, res.product[n]), (n, PZ.diff(p.grad, res.product[n]))
    assert any(bool(t.abs().max() > 0) for t in res.product.values())
    flat = res.product_flat()
    d = ParamDirections(m, 1)
    assert tuple(flat.shape) == (d.P,)
    for n, p, o in zip(d.names, d.params, d.offsets):
        assert PZ.same_bytes(flat[o:o + p.numel()], res.product[n].reshape(-1)), n


# ---------------------------------------------------------------------------------------------
# The rollout against the float64 reference at the GPU's own masks
# ---------------------------------------------------------------------------------------------
def _reference(name, xs, host, v, dp, taps, kind, target, scale):
    """tests/gauss_newton_ref.py teacher-forced on the GPU's own states and post masks (as
    tests/test_gpu_objective_tangent.py's reference)."""
    c = TC.case(name)
    p64, cfg = TC.params64(name), TC.oracle_cfg(name)
    states = [s.cpu().numpy() for s in xs]
    steps = []
    for t, h in enumerate(host):
        steps.append(dict(chosen=h["offs"] if c["graph"] else None, active=h["active"].numpy(),
                          fire_mask=None if h["fire"] is None else h["fire"].cpu().numpy().astype(np.float64),
                          post_alive=OT._post_of(states[t + 1], c["thr"]) if c["thr"] >= 0 else None,
                          message_gain=h["gain"] if c["graph"] else 0.0))
    tgt = target.numpy()
    tgt = tgt if tgt.ndim == 4 else tgt[None]
    d64 = {k: t.numpy().astype(np.float64) for k, t in dp.items()}
    return GR.gauss_newton(states[0].astype(np.float64), p64, cfg, v.numpy().astype(np.float64), d64, steps, list(taps),
                           kind, tgt, scale, KNOBS, states=states)


def _bounds(ref):
    """The project's BPTT bound (tests/test_gpu_grad.py) per tensor of a reference product."""
    b = {"gx": 5e-5 * float(np.abs(ref["gx"]).max()) + 1e-6}
    b.update({n: 5e-5 * float(np.abs(t).max()) + 1e-6 for n, t in ref["product"].items()})
    return b


def _inner(res, v, dp):
    s = float((res.gx.double().cpu().numpy() * v.numpy().astype(np.float64)).sum())
    for n, t in res.product.items():
        s += float((t.double().cpu().numpy() * dp[n].numpy().astype(np.float64)).sum())
    return s


def _l1(v, dp):
    d = {"gx": float(v.abs().double().sum())}
    d.update({n: float(t.abs().double().sum()) for n, t in dp.items()})
    return d


REF = (("p5", 6, dict(every=2), "mask", "premult"), ("p5", 6, dict(record=[1, 4, 6]), "hash", "masked"),
       ("p13", 6, dict(every=3), "hash", "premult"), ("p13", 6, dict(record=[1, 3, 6]), "mask", "masked"),
       ("t72", 3, dict(record=[1, 3]), "hash", "premult"))


@pytest.mark.parametrize("name,T,taps,mode,kind", REF, ids=[f"{r[0]}-{r[3]}-{r[4]}" for r in REF])
def test_product_against_the_float64_reference(name, T, taps, mode, kind):
    m = _model(name)
    c = TC.case(name)
    kw, host = OT._sched(name, T, mode)
    xa, va, da, target = _inputs(name, T, extra=0)
    _, vb, db, _ = _inputs(name, T, extra=1)
    xd, td = xa.to(DEV), target.to(DEV)
    B = c["B"]
    lk = OT._loss_kw(kind)
    R = len(S.expand_record(T, taps.get("every", 1), taps.get("record")))
    w = [0.5 + 0.5 * r for r in range(R)]
    scale = [float(np.float32(t / B)) for t in w]
    run = lambda v, d: m.rollout_gauss_newton(xd, T, td, dparams=OT._dev(d), v=v.to(DEV), tap_weights=w, **taps,   # noqa: E731
                                              **lk, **kw)
    Ga, Gb = run(va, da), run(vb, db)
    xs = OT._gpu_states(name, xd, host)
    assert PZ.same_bytes(xs[-1], Ga.x_final)
    assert (Ga.steps[-1] == T) and host[1]["gain"] == 0.0 and not bool(host[-1]["active"].all())
    ref_a = _reference(name, xs, host, va, da, Ga.steps, kind, target, scale)
    ref_b = _reference(name, xs, host, vb, db, Ga.steps, kind, target, scale)
    worst = 0.0
    for G, ref in ((Ga, ref_a), (Gb, ref_b)):
        bnd = _bounds(ref)
        got = {"gx": G.gx.cpu().numpy().astype(np.float64)}
        got.update({n: t.cpu().numpy().astype(np.float64) for n, t in G.product.items()})
        want = dict(ref["product"], gx=ref["gx"])
        assert set(want) <= set(got), (sorted(got), sorted(want))
        for n in got:
            want.setdefault(n, np.zeros_like(got[n]))       # (a tensor no step of the reference used)
            err = float(np.abs(got[n] - want[n]).max())
            worst = max(worst, err / bnd[n])
            print(f"[gauss-newton] {name} {mode} {kind} {n}: max|ref| {float(np.abs(want[n]).max()):.3e} "
                  f"err {err:.3e} bound {bnd[n]:.3e}")
            assert np.isfinite(got[n]).all() and err <= bnd[n], (n, err, bnd[n])
            assert float(np.abs(want[n]).max()) > 0 or n.startswith("graph.")
    # symmetry and the energy identity, within the slack the tensor bounds imply
    ba, bb = _bounds(ref_a), _bounds(ref_b)
    la, lb = _l1(va, da), _l1(vb, db)
    a_Gb, b_Ga = _inner(Gb, va, da), _inner(Ga, vb, db)
    slack = sum(bb[n] * la[n] + ba[n] * lb[n] for n in ba)
    print(f"[gauss-newton] {name} {mode} {kind}: <a,Gb> {a_Gb:.6e} <b,Ga> {b_Ga:.6e} slack {slack:.3e}  worst err / bound "
          f"{worst:.3e}")
    assert abs(a_Gb - b_Ga) <= slack, (a_Gb, b_Ga, slack)
    ref_ab = GR.inner(ref_b, va.numpy(), {k: t.numpy() for k, t in da.items()})
    assert abs(a_Gb - ref_ab) <= sum(bb[n] * la[n] for n in bb), (a_Gb, ref_ab)
    for G, ref, bnd, l1, v, d in ((Ga, ref_a, ba, la, va, da), (Gb, ref_b, bb, lb, vb, db)):
        e = float(G.energy)
        assert e >= 0.0 and bool((G.quad >= 0).all())
        own = _inner(G, v, d)
        sl = 2 * sum(bnd[n] * l1[n] for n in bnd)
        print(f"[gauss-newton] {name} {mode} {kind}: energy {e:.6e} <d,Gd> {own:.6e} ref {ref['energy']:.6e} slack {sl:.3e}")
        assert abs(own - e) <= sl, (own, e, sl)
        assert ref["energy"] > 0.0


# ---------------------------------------------------------------------------------------------
# Conjugate gradients on the real operator
# ---------------------------------------------------------------------------------------------
def test_cg_on_the_real_operator():
    name, T = "p5", 4
    m = TC.model(name, DEV)
    x, _, dp, target = _inputs(name, T)
    kw, _ = OT._sched(name, T, "mask")
    xd, td = x.to(DEV), target.to(DEV)
    dirs = ParamDirections(m, 1)
    calls = []

    def matvec(s):
        dirs.flat[0].copy_(s)
        r = m.rollout_gauss_newton(xd, T, td, dparams=dirs.dicts()[0], every=2, **kw)
        calls.append(r.energy)
        return r.product_flat()
    for p in m.parameters():
        p.grad = None
    m.rollout_objective(xd, T, td, every=2, **kw).losses.sum(0).mean().backward()
    params = dict(m.named_parameters())
    b = -torch.cat([params[n].grad.reshape(-1) for n in dirs.names])
    assert float(b.abs().max()) > 0
    s, mk = cg_solve(matvec, b, 4, damping=1e-2)
    assert len(calls) == 4 and mk.dtype == torch.float64 and mk.is_cuda and tuple(mk.shape) == (4,)
    vals = mk.cpu().numpy()
    print(f"[cg] model values {vals}")
    assert np.isfinite(vals).all() and vals[0] < 0.0 and vals[3] <= vals[0]
    assert torch.isfinite(s).all() and float(s.abs().max()) > 0 and all(float(e) >= 0.0 for e in calls)


# ---------------------------------------------------------------------------------------------
# Guarded, poisoned buffers and the stream legs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_poisoned_buffers_loss_curvature(kind):
    state, target, vt = _alone_inputs(11, 13, 3, True)

    def call(P):
        f, q, l, d = loss_curvature(P.guard(state[:, :4].contiguous()), P.guard(vt[:, :4].contiguous()), P.guard(target),
                                    kind, **_knob_kw(kind))
        return {"field": f, "quad": q, "losses": l, "dlosses": d}
    out = PZ.run_fills(call, f"loss_curvature:{kind}")
    for t in out.values():
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,ckpt", (("p13", None), ("p5", None), ("p5", 3)))
def test_poisoned_buffers_rollout(name, ckpt, kind):
    """Both native calls of a product (gnca_rollout_gn_fwd, gnca_rollout_gn_bwd) on guarded, poisoned buffers."""
    m = _model(name)
    T = 4
    x, v, dp, target = _inputs(name, T)
    kw, _ = OT._sched(name, T, "mask")
    xd, vd, dpd, td = x.to(DEV), v.to(DEV), OT._dev(dp), target.to(DEV)

    def call(P):
        k = dict(kw, nsteps=P.guard(kw["nsteps"]), fire=P.guard(kw["fire"]))
        d = {n: P.guard(t) for n, t in dpd.items()}
        r = m.rollout_gauss_newton(P.guard(xd), T, P.guard(td), dparams=d, v=P.guard(vd), record=[2, 4],
                                   checkpoint_every=ckpt, return_fields=True, **OT._loss_kw(kind), **k)
        return _outs(r)
    out = PZ.run_fills(call, f"rollout_gauss_newton:{name}:{ckpt}:{kind}")
    for t in out.values():
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("leg", ("side", "capture"))
@pytest.mark.parametrize("entry", ("loss", "rollout", "rollout-ckpt"))
def test_stream_legs(entry, leg):
    name, T = "p13", 4
    m = _model(name)
    c = TC.case(name)
    B = c["B"]
    offs = TC.offsets(name, T)
    sets = []
    for e in (0, 1):
        g = torch.Generator().manual_seed(29 + e)
        if entry == "loss":
            st, tg, vt = _alone_inputs(24, 24, 3, True)
            s = {"pred": (st[:, :4] + e).contiguous(), "v": (vt[:, :4] + e).contiguous(), "target": tg}
        else:
            s = {"x": TC.state(name, extra=e).to(DEV), "target": OT._target(B, c["H"], c["W"], g).to(DEV),
                 "v": TC.tangent(name, extra=e).to(DEV),
                 "nsteps": torch.tensor([T, 2 + e][:B], dtype=torch.int32, device=DEV)}
            s.update({"d:" + k: t.to(DEV) for k, t in OT._direction(name, extra=e).items()})
        sets.append(s)

    def call(b):
        if entry == "loss":
            f, q, l, d = loss_curvature(b["pred"], b["v"], b["target"], "masked", alpha_thr=KNOBS[0])
            return {"field": f, "quad": q, "losses": l, "dlosses": d}
        d = {k[2:]: t for k, t in b.items() if k.startswith("d:")}
        r = m.rollout_gauss_newton(b["x"], T, b["target"], dparams=d, v=b["v"], record=[2, 4], loss="masked",
                                   tap_weights=[0.5, 2.0], fire_rate=0.5, seed=3, nsteps=b["nsteps"], offsets=offs,
                                   checkpoint_every=3 if entry == "rollout-ckpt" else None)
        return _outs(r)
    ST.run(ST.Case(f"gauss_newton:{entry}", sets, call), legs=("eager", leg))
