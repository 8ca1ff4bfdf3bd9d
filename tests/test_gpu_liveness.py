"""GPU tests of the alive-mask structure: sparse states, exact thresholds, edge live counts.

The states come from tests/liveness_cases.py (dead background, seeds whose clipped 3x3 dilation
is the alive set; explicit fire masks with per-tile popcounts 0, 1, 31, 32, 33, ...; cells at
exactly float32(thr) and one ulp above), so that the pre-update alive mask, the sender mask and
the keep mask have borders, holes and empty tiles, which the all-alive random states of the
other GPU tests never give them.  References: the float64 oracles (oracle/nca_oracle.py,
oracle/nca_oracle_vjp.py), pinned to the PyTorch-CPU restatement of the reference on the same
patterns by tests/test_liveness_cases_cpu.py, which also asserts that every case compared with
the oracle keeps its pooled post-update alpha >= 2e-5 from the threshold (so a kernel within the
forward tolerance cannot flip a mask), and the per-step path for the rollouts (bitwise).

Tolerances are the project's own: forward atol 2e-6 / rtol 1e-5 with identical alive masks of the
result (tests/test_gpu_parity.py), gradients 2e-5 * max|ref| + 1e-6 per tensor
(tests/test_gpu_grad.py), attention map 2e-5, rollouts against the oracle atol 1e-4 with identical
alive masks (tests/test_gpu_drift.py).  Every case asserts the plan it means to test (K1 variant,
rollout plan, backward MLP kernel) and names it in its assertion messages.
"""
import random

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from oracle import nca_oracle_vjp as V
from tests import liveness_cases as LC

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-6, 1e-5
G_RT, G_AT = 2e-5, 1e-6
DRIFT = 1e-4

_SHORT = {"perception.conv.weight": "perception", "update_net.0.weight": "w1", "update_net.0.bias": "b1",
          "update_net.2.weight": "w2", "norm.weight": "gn_weight", "norm.bias": "gn_bias",
          "graph.query_proj.weight": "wq", "graph.query_proj.bias": "bq", "graph.key_proj.weight": "wk",
          "graph.key_proj.bias": "bk", "graph.msg_proj.weight": "wm", "graph.msg_proj.bias": "bm",
          "graph.scaling": "scaling"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _weights(p, dev):
    from graph_neural_cellular_automata_amd import step as S
    tensors = {_SHORT[k]: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))).to(dev)
               for k, v in p.items()}
    w, keep = S.make_weights(tensors)
    return w, (keep, tensors)


def _fire_args(c, case, dev):
    """(fire tensor or None, fire mode, fire rate) of a one-step case."""
    from graph_neural_cellular_automata_amd import _lib as L
    if c["fire"] == "mask":
        return torch.from_numpy(np.ascontiguousarray(case.fire)).to(dev), L.FIRE_MASK_U8, 0.5
    if c["fire"] == "hash":
        return None, L.FIRE_HASH, 0.5
    return None, L.FIRE_NONE, 1.0


def _build(c, samples=None):
    m = c["m"]
    return LC.build(c["pattern"], c["seed"], c["B"], m["C"], c["H"], c["W"], m["thr"], c["tile"],
                    seed_lo=c.get("seed_lo"), samples=samples)


def _same_masks(got, ref, thr, msg):
    a, b = O.alive_mask(np.asarray(got, np.float64), thr), O.alive_mask(ref, thr)
    assert np.array_equal(a, b), (msg, f"alive-mask flips: {int((a != b).sum())}")


def _check_grads(got, ref, msg):
    worst = 0.0
    assert set(got) == set(ref), (msg, sorted(got), sorted(ref))
    for k, r in ref.items():
        g = got[k].detach().double().cpu().numpy().reshape(np.shape(r))
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        assert np.isfinite(g).all(), (msg, k)
        assert err <= G_RT * scale + G_AT, (msg, k, f"err={err:.3e} scale={scale:.3e}")
        if G_RT * scale > G_AT:      # (a tensor whose bound is its absolute term says nothing relative)
            worst = max(worst, err / scale)
    return worst


# ---------------------------------------------------------------------------------------------
# a, b. One step against the float64 oracle: every pattern x every K1 family; the two thresholds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.step_cases() + LC.thr_step_cases(), ids=lambda c: c["id"])
def test_step_matches_oracle(dev, c):
    from graph_neural_cellular_automata_amd import step as S
    m, B, H, W = c["m"], c["B"], c["H"], c["W"]
    plan = LC.plan_of(m, B, H, W)
    msg = (c["id"], plan["k1"], f"seed={c['seed']}")
    assert plan["k1"].startswith(c.get("k1", "gnca_k1_split<8,24,")), msg
    case = _build(c)
    p = LC.params(m, c["seed"])
    w, keep = _weights(p, dev)
    x = torch.from_numpy(case.x).to(dev)
    fire, mode, rate = _fire_args(c, case, dev)
    out, _ = S.step(LC.make_desc(m, B, H, W, fire_mode=mode, fire_rate=rate, seed=c["seed"]), w, x, fire=fire)
    torch.cuda.synchronize()
    # the oracle, on the compared samples
    sub = _build(c, c["samples"])
    assert np.array_equal(sub.x, case.x[c["samples"]])
    x64, p64, cfg = sub.x.astype(np.float64), LC.f64(p), LC.oracle_cfg(m)
    f64 = LC.step_fire(c, sub)
    ref, ref_attn = O.nca_step(x64, p64, cfg, chosen=LC.offsets(m), fire_mask=f64, return_attention=True)
    got = out[c["samples"]].cpu().numpy()
    err = float(np.abs(got - ref).max())
    keep_m = LC.keep_mask(sub.x, m["thr"], f64)
    print(f"[liveness] step {c['id']} {plan['k1']} live/tile {sorted(set(LC.tile_live_counts(keep_m, c['tile']).reshape(-1).tolist()))[:6]}... "
          f"max|hip - f64| = {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=str(msg))
    _same_masks(got, ref, m["thr"], msg)
    if c["pattern"] == "exact_thr":
        # strict float32 semantics: a cell at exactly the threshold is dead (its alpha zeroed by the
        # post gate), a cell one ulp above is alive (an untouched one keeps its alpha bit for bit)
        eq, quiet = sub.info["eq"], sub.info["quiet"]
        assert (got[:, 3][eq] == 0).all(), msg
        assert (got[:, 3][quiet] == sub.x[:, 3][quiet]).all(), msg
    if m["graph"]:
        # return_attention=True (its own K1 plan): the same state and the normalised map
        da = LC.make_desc(m, B, H, W, fire_mode=mode, fire_rate=rate, seed=c["seed"], attention=True)
        out_a, attn = S.step(da, w, x, fire=fire, want_attention=True)
        got_a = out_a[c["samples"]].cpu().numpy()
        amsg = msg + ("attention", S.k1_variant(da)[0])
        np.testing.assert_allclose(got_a, ref, rtol=RTOL, atol=ATOL, err_msg=str(amsg))
        _same_masks(got_a, ref, m["thr"], amsg)
        np.testing.assert_allclose(attn[c["samples"]].cpu().numpy(), ref_attn, rtol=0, atol=2e-5, err_msg=str(amsg))
    del keep


@pytest.mark.parametrize("mname,lo", LC.THR_ORDERS)
@pytest.mark.parametrize("pattern", ["sparse", "isolated"])
def test_two_threshold_rollout_equals_steps(dev, mname, lo, pattern):
    """graph_alpha_thr above alpha_thr (alive hand-over, fold), below it and a negative alpha_thr
    (the fallback): a 3-step rollout at the compact batch, bitwise against 3 single steps, on states
    whose seeds straddle the larger threshold (so the update's and the senders' masks differ)."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    m, B, H, W, T = LC.MODELS[mname], 128, 48, 72, 3
    plan = LC.check_plan(mname, B, H, W)
    seed = 40 + len(pattern)
    case = LC.build(pattern, seed, B, m["C"], H, W, m["thr"], LC.k1_tile(plan["k1"]), seed_lo=lo)
    pre, snd = O.alive_mask(case.x[:8], m["thr"]), O.alive_mask(case.x[:8], m["gthr"])
    assert (pre != snd).any() and 0 < pre.mean() < 1
    w, keep = _weights(LC.params(m, seed), dev)
    x = torch.from_numpy(case.x).to(dev)
    hashed = pattern == "sparse"

    def desc(t):
        return LC.make_desc(m, B, H, W, step=t, seed=seed, fire_rate=0.5 if hashed else 1.0,
                            fire_mode=L.FIRE_HASH if hashed else L.FIRE_NONE)

    r = S.rollout(desc(0), w, x, T, [LC.offsets(m, t) for t in range(T)])
    cur = x
    for t in range(T):
        cur, _ = S.step(desc(t), w, cur)
    assert torch.equal(r, cur), (mname, pattern, plan)
    assert not torch.equal(r, x)
    del keep


def _module(m, p, dev):
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    if m["graph"]:
        model = NeuralCAGraph(m["C"], m["hidden"], update_gain=m["gain"], alpha_thr=m["thr"],
                              use_groupnorm=m["gn"], message_gain=m["msg"], hidden_only=m["hidden_only"],
                              graph_d_model=m["d_model"], graph_attention_radius=m["radius"],
                              graph_num_neighbors=m["K"], graph_alive_to_alive=m["a2a"],
                              graph_zero_padded_shift=m["zp"])
    else:
        model = NeuralCA(m["C"], m["hidden"], update_gain=m["gain"], alpha_thr=m["thr"], use_groupnorm=m["gn"])
    sd = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))) for k, v in p.items()}
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("graph.gate_mlp") for k in res.missing_keys), res
    return model.to(dev).eval()


def _grads(model):
    return {n: q.grad for n, q in model.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("mname", ["graph_g_gt_a", "graph_g_lt_a"])
def test_module_graph_alpha_thr_forward_and_backward(dev, mname):
    """model.graph.alpha_thr set after construction (the reference's GraphAugmentation.alpha_thr is
    its own attribute): the module's forward and backward against the oracles."""
    m = LC.MODELS[mname]
    B, H, W, seed = 2, 40, 40, 61
    p = LC.params(m, seed)
    model = _module(m, p, dev)
    assert model.graph.alpha_thr == m["thr"]
    model.graph.alpha_thr = m["gthr"]
    case = LC.build("sparse", seed, B, m["C"], H, W, m["thr"], (8, 20), seed_lo=0.12)
    x64 = case.x.astype(np.float64)
    assert (O.alive_mask(x64, m["thr"]) != O.alive_mask(x64, m["gthr"])).any()
    x = torch.from_numpy(case.x).to(dev).requires_grad_(True)
    gy64 = np.random.default_rng(seed).standard_normal(case.x.shape)
    random.seed(seed)
    chosen = model.graph.sample_offsets()
    random.seed(seed)
    out = model(x, fire_rate=1.0)
    (out * torch.from_numpy(gy64.astype(np.float32)).to(dev)).sum().backward()
    torch.cuda.synchronize()
    p64, cfg = LC.f64(p), LC.oracle_cfg(m)
    ref = O.nca_step(x64, p64, cfg, chosen=chosen)
    msg = (mname, LC.plan_of(m, B, H, W))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=RTOL, atol=ATOL, err_msg=str(msg))
    _same_masks(out.detach().cpu().numpy(), ref, m["thr"], msg)
    one = O.nca_step(x64, p64, {k: v for k, v in cfg.items() if k != "graph_alpha_thr"}, chosen=chosen)
    assert np.abs(one - ref).max() > 100 * ATOL            # the second threshold matters on this state
    gx, grads = V.nca_step_vjp(x64, p64, cfg, gy64.astype(np.float32).astype(np.float64), chosen=chosen)
    _check_grads(dict(_grads(model), gx=x.grad), dict(grads, gx=gx), msg)


# ---------------------------------------------------------------------------------------------
# c. Backward against the float64 VJP oracle
# ---------------------------------------------------------------------------------------------
def _backward(c, dev, active=None, samples=None):
    from graph_neural_cellular_automata_amd import step as S
    m, H, W = c["m"], c["H"], c["W"]
    case = _build(c, samples)
    B = case.x.shape[0]
    p = LC.params(m, c["seed"])
    w, keep = _weights(p, dev)
    x = torch.from_numpy(case.x).to(dev)
    gy = np.random.default_rng([9, c["seed"]]).standard_normal((c["B"],) + case.x.shape[1:]).astype(np.float32)
    if samples is not None:
        gy = gy[samples]
    fire, mode, rate = _fire_args(c, case, dev)
    desc = LC.make_desc(m, B, H, W, fire_mode=mode, fire_rate=rate, seed=c["seed"])
    want = {k: torch.empty(np.shape(v)) for k, v in p.items() if k in S.GRAD_FIELDS}
    gx, grads = S.step_backward(desc, w, x, torch.from_numpy(gy).to(dev), fire=fire, want=want, active=active)
    torch.cuda.synchronize()
    del keep
    return case, p, gy, gx, grads, desc


@pytest.mark.parametrize("c", LC.bwd_cases(), ids=lambda c: c["id"])
def test_backward_matches_vjp_oracle(dev, c):
    from graph_neural_cellular_automata_amd import step as S
    m = c["m"]
    case, p, gy, gx, grads, desc = _backward(c, dev)
    bb = S.bb_variant(desc)
    msg = (c["id"], S.k1_variant(desc)[0], bb, f"seed={c['seed']}")
    assert bb.endswith(c["bb"]) if c["bb"] == LC.RUNTIME_BB else bb == c["bb"], msg
    x64, f64 = case.x.astype(np.float64), LC.step_fire(c, case)
    rgx, rgr = V.nca_step_vjp(x64, LC.f64(p), LC.oracle_cfg(m), gy.astype(np.float64), chosen=LC.offsets(m),
                              fire_mask=f64)
    ref = dict(rgr, gx=rgx)
    got = dict({k: v for k, v in grads.items() if k in ref}, gx=gx)
    for k in grads:      # a parameter the reference leaves without a gradient: nothing but zeros
        assert k in ref or float(grads[k].abs().max()) == 0.0, (msg, k)
    worst = _check_grads(got, ref, msg)
    print(f"[liveness] backward {c['id']} {bb}: worst err / max|ref| = {worst:.3e}")
    if not m["gn"] and (not m["graph"] or (m["a2a"] and not m["zp"])):
        # GroupNorm off: a cell with no kept cell in its 3x3 window (and, with the graph, no sender
        # bit) takes part in nothing, so its gx is its gy bit for bit (alpha goes through the gate)
        keep_m = LC.keep_mask(case.x, m["thr"], f64)[:, 0] != 0
        idle = ~LC.dilate(keep_m) & ~(O.alive_mask(x64, m.get("gthr") or m["thr"])[:, 0] != 0)
        assert c["pattern"] == "counts" or 0.1 < idle.mean() < 0.95, (msg, idle.mean())
        ch = [k for k in range(m["C"]) if k != 3]
        sel = torch.from_numpy(idle).to(gx.device)[:, None].expand(-1, len(ch), -1, -1)
        assert torch.equal(gx[:, ch][sel], torch.from_numpy(gy).to(gx.device)[:, ch][sel]), msg


@pytest.mark.parametrize("mname", ["graph", "classic"])
def test_masked_backward_equals_subbatch_on_half_dead(dev, mname):
    """The masked-step backward (active=) on a half-dead batch: gx of the active samples equals the
    sub-batch backward bitwise; the inactive samples pass their gy through."""
    from graph_neural_cellular_automata_amd import step as S
    c = dict(id=f"masked-{mname}", m=dict(LC.MODELS[mname]), B=4, H=48, W=72, tile=(8, 24), pattern="half_dead",
             seed=81, fire=None)
    act = [0, 2, 3]
    active = torch.tensor([True, False, True, True], device=dev)
    case, p, gy, gx, grads, desc = _backward(c, dev, active=active)
    _, _, gy_s, gx_s, _, desc_s = _backward(c, dev, samples=act)
    msg = (c["id"], S.bb_variant(desc), S.bb_variant(desc_s))
    assert S.bb_variant(desc) == S.bb_variant(desc_s), msg
    assert np.array_equal(gy[act], gy_s)
    assert torch.equal(gx[act], gx_s), msg
    assert torch.equal(gx[1].cpu(), torch.from_numpy(gy[1])), msg
    assert not torch.equal(gx[0].cpu(), torch.from_numpy(gy[0]))


# ---------------------------------------------------------------------------------------------
# d. Rollouts: bitwise against single steps over every plan row, two samples against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", LC.rollout_cases(), ids=lambda rc: "-".join(map(str, rc[:6])))
def test_rollout_equals_steps_and_oracle(dev, rc):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W, pat, seed, smp = rc
    m, T = LC.MODELS[name], LC.ROLLOUT_STEPS
    plan = LC.check_plan(name, B, H, W)
    msg = (rc, plan)
    tile = LC.k1_tile(plan["k1"])
    case = LC.build(pat, seed, B, m["C"], H, W, m["thr"], tile)
    p = LC.params(m, seed)
    w, keep = _weights(p, dev)
    x = torch.from_numpy(case.x).to(dev)
    rate, hashed = LC.rollout_fire(pat)
    offs = [LC.offsets(m, t) for t in range(T)]

    def desc(t):
        return LC.make_desc(m, B, H, W, step=t, seed=seed, fire_rate=rate,
                            fire_mode=L.FIRE_HASH if hashed else L.FIRE_NONE)

    r = S.rollout(desc(0), w, x, T, offs)
    cur = x
    for t in range(T):
        cur, _ = S.step(desc(t), w, cur)
    assert torch.equal(r, cur), msg
    if plan["foldable"] and not plan["fold"]:
        assert torch.equal(S.rollout(desc(0), w, x, T, offs, fold=True), cur), ("fold=True", msg)
    # two samples against the float64 oracle rollout (their margins: tests/test_liveness_cases_cpu.py)
    sub = LC.build(pat, seed, B, m["C"], H, W, m["thr"], tile, samples=smp)
    assert np.array_equal(sub.x, case.x[list(smp)])
    frames, _ = LC.oracle_rollout(sub, m, LC.f64(p), seed, T, hashed=hashed, fire_rate=rate)
    got = r[list(smp)].cpu().numpy()
    err = float(np.abs(got - frames[-1]).max())
    print(f"[liveness] rollout {rc[:6]} {plan['k1']} compact={plan['compact']} subs={plan['subs']} "
          f"fold={plan['fold']}: max|hip - f64| after {T} steps = {err:.3e}")
    assert err <= DRIFT, (msg, err)
    _same_masks(got, frames[-1], m["thr"], msg)
    del keep


# ---------------------------------------------------------------------------------------------
# e. trace() and the grad rollout, once each on a sparse state
# ---------------------------------------------------------------------------------------------
def _e_case(name):
    c = LC.E_CASES[name]
    m = LC.MODELS[c["mname"]]
    case = LC.build("sparse", c["seed"], c["B"], m["C"], c["H"], c["W"], m["thr"], c["tile"])
    return c, m, case, LC.params(m, c["seed"])


def test_trace_on_sparse_state_matches_oracle(dev):
    c, m, case, p = _e_case("trace")
    T = c["steps"]
    model = _module(m, p, dev)
    offs = [LC.offsets(m, t) for t in range(T)]
    res = model.trace(torch.from_numpy(case.x).to(dev), T, every=1, channels=4, return_attention=True,
                      fire_rate=c["fire_rate"], seed=c["seed"], offsets=offs)
    torch.cuda.synchronize()
    cfg, p64 = LC.oracle_cfg(m), LC.f64(p)
    x = case.x.astype(np.float64)
    msg = ("trace", LC.plan_of(m, c["B"], c["H"], c["W"]))
    assert res.steps == list(range(1, T + 1))
    for t in range(T):
        fire = O.hash_fire_mask(c["seed"], t, 0, c["B"], c["H"], c["W"], c["fire_rate"])
        x, attn = O.nca_step(x, p64, cfg, chosen=offs[t], fire_mask=fire, return_attention=True)
        got = res.frames[t].cpu().numpy()
        np.testing.assert_allclose(got, x[:, :4], rtol=0, atol=DRIFT, err_msg=str((msg, t)))
        assert np.array_equal(O.alive_mask(got.astype(np.float64), m["thr"]), O.alive_mask(x, m["thr"])), (msg, t)
        np.testing.assert_allclose(res.attention[t].cpu().numpy(), attn, rtol=0, atol=DRIFT, err_msg=str((msg, t)))
    np.testing.assert_allclose(res.x_final.cpu().numpy(), x, rtol=0, atol=DRIFT, err_msg=str(msg))


def test_grad_rollout_on_sparse_state_matches_chained_vjp(dev):
    c, m, case, p = _e_case("bptt")
    T = c["steps"]
    model = _module(m, p, dev)
    offs = [LC.offsets(m, t) for t in range(T)]
    leaf = torch.from_numpy(case.x).to(dev).requires_grad_(True)
    gy = np.random.default_rng(c["seed"]).standard_normal(case.x.shape).astype(np.float32)
    out = model.rollout(leaf, T, fire_rate=c["fire_rate"], seed=c["seed"], offsets=offs)
    (out * torch.from_numpy(gy).to(dev)).sum().backward()
    torch.cuda.synchronize()
    cfg, p64 = LC.oracle_cfg(m), LC.f64(p)
    fires = [O.hash_fire_mask(c["seed"], t, 0, c["B"], c["H"], c["W"], c["fire_rate"]) for t in range(T)]
    states = [case.x.astype(np.float64)]
    for t in range(T):
        states.append(O.nca_step(states[-1], p64, cfg, chosen=offs[t], fire_mask=fires[t]))
    msg = ("bptt", LC.plan_of(m, c["B"], c["H"], c["W"]))
    np.testing.assert_allclose(out.detach().cpu().numpy(), states[-1], rtol=0, atol=DRIFT, err_msg=str(msg))
    _same_masks(out.detach().cpu().numpy(), states[-1], m["thr"], msg)
    g, total = gy.astype(np.float64), {}
    for t in reversed(range(T)):
        g, gr = V.nca_step_vjp(states[t], p64, cfg, g, chosen=offs[t], fire_mask=fires[t])
        for k, v in gr.items():
            total[k] = total.get(k, 0) + v
    worst = _check_grads(dict(_grads(model), gx=leaf.grad), dict(total, gx=g), msg)
    print(f"[liveness] bptt {T} steps: worst err / max|ref| = {worst:.3e}")
