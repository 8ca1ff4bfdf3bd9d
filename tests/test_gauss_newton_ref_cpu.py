"""The Gauss-Newton reference (tests/gauss_newton_ref.py) pinned without a GPU: the operator it applies is symmetric
and positive semidefinite, its energy is the quadratic form of its own product, it is linear in the direction, the
premultiplied field is J_p^T H J_p v of an explicit per-pixel Jacobian, and the masked field of an all-dead target
is zero.  Cases p5 and q4h64 (classic) and p13 (graph); both loss kinds; taps at 1, mid and T; a sample that
``nsteps`` finished early; a message-off step.
"""
import numpy as np
import pytest
import torch

from tests import gauss_newton_ref as GR
from tests import shape_class_cases as SC

KNOBS = (0.2, 5e-5, 1e-3, 2e-4)
T, TAPS = 4, [1, 2, 4]
SCALE = [0.5, 0.25, 1.0 / 3.0]
KEYS = ("update_net.0.weight", "update_net.0.bias", "update_net.2.weight", "norm.weight", "norm.bias",
        "graph.msg_proj.weight", "graph.msg_proj.bias")


def _setup(name):
    c = SC.CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    g = torch.Generator().manual_seed(4242 + SC.seed(name))
    x = SC.state(name).numpy().astype(np.float64)
    fire = (torch.rand(T, B, 1, H, W, generator=g) <= 0.5).numpy().astype(np.float64)
    target = torch.rand(B, 4, H, W, generator=g)
    target[:, 3, :, : W // 2] *= 0.15                      # dead target cells on the left half
    target = target.numpy()
    active = np.ones((T, B), bool)
    active[2:, 0] = False                                  # sample 0 finished after two steps: frozen at the tap at T
    offs = SC.offsets(name, T) if c["graph"] else [None] * T
    steps = [dict(chosen=offs[t], fire_mask=fire[t] if t != 1 else None, active=active[t],
                  message_gain=(c["msg"] if c["graph"] and t != 1 else 0.0)) for t in range(T)]   # step 1: message off
    p = SC.params64(name)

    def direction():
        v = torch.randn(*x.shape, generator=g).numpy().astype(np.float64)
        dp = {k: torch.randn(p[k].shape, generator=g).numpy().astype(np.float64) for k in KEYS if k in p}
        return v, dp
    return c, x, p, SC.oracle_cfg(name), steps, target, direction


def _run(name, kind, v, dp, setup=None):
    c, x, p, cfg, steps, target, _ = setup or _setup(name)
    knobs = KNOBS if kind == "masked" else None
    return GR.gauss_newton(x, p, cfg, v, dp, steps, TAPS, kind, target, SCALE, knobs)


@pytest.mark.parametrize("kind", ("premult", "masked"))
@pytest.mark.parametrize("name", ("p5", "p13", "q4h64"))
def test_symmetric_and_energy(name, kind):
    su = _setup(name)
    (va, da), (vb, db) = su[6](), su[6]()
    Ga, Gb = _run(name, kind, va, da, su), _run(name, kind, vb, db, su)
    ab, ba = GR.inner(Gb, va, da), GR.inner(Ga, vb, db)
    assert abs(ab - ba) <= 1e-10 * (abs(ab) + abs(ba)), (ab, ba)
    assert ab != 0.0
    for G, v, d in ((Ga, va, da), (Gb, vb, db)):
        e = GR.inner(G, v, d)
        assert G["energy"] > 0.0 and abs(e - G["energy"]) <= 1e-10 * G["energy"], (e, G["energy"])
        assert (G["quad"] >= 0).all()
        # each tap's quad is the dot of its own field with the tangent it was built from, hence with nothing else
        assert G["losses"].shape == (len(TAPS), su[0]["B"]) and G["dlosses"].shape == (len(TAPS), su[0]["B"])


@pytest.mark.parametrize("kind", ("premult", "masked"))
def test_parts_and_linearity(kind):
    su = _setup("p13")
    v, d = su[6]()
    both = _run("p13", kind, v, d, su)
    v_only, d_only = _run("p13", kind, v, {}, su), _run("p13", kind, None, d, su)
    twice = _run("p13", kind, 2 * v, {k: 2 * t for k, t in d.items()}, su)
    scale = float(np.abs(both["gx"]).max())
    np.testing.assert_allclose(v_only["gx"] + d_only["gx"], both["gx"], rtol=0, atol=1e-12 * scale)
    np.testing.assert_array_equal(twice["gx"], 2 * both["gx"])
    for k in both["product"]:
        s = float(np.abs(both["product"][k]).max())
        np.testing.assert_allclose(v_only["product"][k] + d_only["product"][k], both["product"][k], rtol=0,
                                   atol=1e-12 * s)
        np.testing.assert_array_equal(twice["product"][k], 2 * both["product"][k])
    assert abs(twice["energy"] - 4 * both["energy"]) <= 1e-14 * twice["energy"]
    np.testing.assert_array_equal(twice["losses"], both["losses"])


def test_premult_field_is_jt_h_j_v():
    g = np.random.default_rng(11)
    S, v = g.standard_normal((3, 4, 5, 7)), g.standard_normal((3, 4, 5, 7))
    field, quad = GR.premult_curvature(S, v)
    J = GR.premult_jacobian(S)
    N = 4 * 5 * 7
    vv = np.moveaxis(v, 1, -1)                                  # [B,H,W,4]
    Jv = np.einsum("bhwij,bhwj->bhwi", J, vv)
    want = (2.0 / N) * np.einsum("bhwij,bhwi->bhwj", J, Jv)     # J^T (2/N I) J v
    np.testing.assert_allclose(np.moveaxis(field, 1, -1), want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(quad, (2.0 / N) * (Jv ** 2).sum(axis=(1, 2, 3)), rtol=1e-13)
    np.testing.assert_allclose((field * v).sum(axis=(1, 2, 3)), quad, rtol=1e-12)
    # it is the Hessian of the loss minus the residual term: at a zero residual the two agree
    target = np.concatenate([S[:, :3] * S[:, 3:4], S[:, 3:4]], axis=1)
    eps = 1e-6
    from tests import objective_tangent_ref as OR
    gp, gm = OR.premult_loss(S + eps * v, target)[1], OR.premult_loss(S - eps * v, target)[1]
    np.testing.assert_allclose((gp - gm) / (2 * eps), field, rtol=0, atol=1e-8 * float(np.abs(field).max()))


def test_masked_field_of_an_all_dead_target_is_zero():
    g = np.random.default_rng(12)
    v = g.standard_normal((2, 4, 6, 5))
    target = g.random((2, 4, 6, 5)).astype(np.float32)
    target[1, 3] = 0.1                                          # sample 1: nothing alive at thr 0.2
    field, quad = GR.masked_curvature(target, v, 0.2)
    assert not field[1].any() and quad[1] == 0.0
    assert field[0].any() and quad[0] > 0.0
    alive = target[0, 3] > np.float32(0.2)
    assert not field[0][:, ~alive].any()
    np.testing.assert_allclose((field * v).sum(axis=(1, 2, 3)), quad, rtol=1e-13)
    # and the masked field is the exact Hessian of the masked loss applied to v (its penalties are linear or |.|)
    from tests import loss_ref as LR
    pred = g.random((2, 4, 6, 5)).astype(np.float32) + 0.5      # away from 0: |.| is smooth there
    e = np.float32(2.0 ** -8)
    dv = (v * 0 + 1).astype(np.float32)                         # an exactly representable tangent
    gp = LR.masked_loss(pred + e * dv, target, *KNOBS).grad
    gm = LR.masked_loss(pred - e * dv, target, *KNOBS).grad
    f1, _ = GR.masked_curvature(target, dv, 0.2)
    np.testing.assert_allclose((gp - gm) / (2 * float(e)), f1, rtol=0, atol=1e-9)
