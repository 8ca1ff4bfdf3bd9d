"""The device damage policy (gnca_damage_policy, damage.DamagePolicy, damage.regrow_trace) on the GPU.

Shapes: B=5, C=6 at 11x13 (4-byte accesses) and 12x12 (16-byte accesses), one row band per sample, and
for the draws, the effects and the shards also 37x23 (4 bands of 12 rows, the last one short) and 40x36
(2 bands of 29 rows); C=4 for the hidden-noise no-op.  States hold negative values, +0 and -0.  Equality
is on int32 bit patterns.

1. draws_out and the uniform planes of noise_out equal tests/damage_policy_ref.py exactly: both scopes,
   every kind, several events, size_max > H.
2. Every normal of noise_out is within 16 * 2^-24 * max(1, sqrt(-2 ln u1)) of the float64 value.  The
   bound is derived, not measured: the argument 2 pi u2 rounded to fp32 carries <= 2 pi 2^-24 into cosf,
   scaled by the radius <= 5.8, plus a few ulp of logf, sqrtf, cosf and two products.
3. For every primitive kind the state after the policy launch is bitwise what gnca_damage_f32 makes of
   the dumped draws and noise sample by sample, and equals the numpy oracle to atol 1e-6.
4. A mixed batch (a kind per sample, one sample untouched) matches each kind's own batch row by row.
5. The batch of 5 in one call equals rows [0:2] and [2:5] in two calls with sample_base 0 and 2.
6. Determinism; a different event draws differently; torch's and Python's RNG states are untouched.
7. No host wait (torch.cuda.set_sync_debug_mode("error")); apply_damage_policy_ raises there.
8. Side stream and graph capture (tests/streams.py); a captured loop with a device event counter.
9. Guarded, poisoned buffers (tests/poison.py): guards intact, unwritten noise rows keep their poison.
10. regrow_trace is bitwise the two manual trace calls with apply_ in between."""
import random

import numpy as np
import pytest
import torch

from tests import damage_policy_ref as PR
from tests import poison as PZ
from tests import streams as ST

pytestmark = pytest.mark.gpu

B, C = 5, 6
FIELDS = {"scalar": (11, 13), "vector": (12, 12)}
BANDED = {"scalar-bands": (37, 23), "vector-bands": (40, 36)}       # more than one row band per sample
SCOPES = ("batch", "sample")
EVENTS = (0, 1, 7, 1 << 40)
CFG = {"start_epoch": 0, "prob": 1.0, "per_sample_prob": 1.0, "size_min": 2, "size_max": 7,
       "kinds": {"square": 1.0, "circle": 1.0, "stripes": 1.0, "alpha_drop": 1.0, "saltpepper": 1.0, "gaussian": 1.0,
                 "hidden_noise": 1.0},
       "alpha_thr": 0.1, "alpha_dropout_p": 0.4, "salt_pepper_p": 0.3, "hidden_noise_sigma": 0.25,
       "gaussian_softness": 0.5}
SEED = 20240611
NORMAL_BOUND = 16.0 * 2.0 ** -24
ALL_KINDS = tuple(range(10))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    from graph_neural_cellular_automata_amd import damage
    return damage


def make_state(field, dev, channels=C, batch=B, seed=3):
    """Values on both sides of 0 and of the alive threshold, about one in eight +0 and one in eight -0."""
    H, W = {**FIELDS, **BANDED}[field]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, channels, H, W, generator=g) * 0.6
    x[:, 3] = torch.rand(batch, H, W, generator=g) * 0.4 - 0.05
    r = torch.rand(x.shape, generator=g)
    x[r < 0.125] = 0.0
    x[r > 0.875] = -0.0
    return x.to(dev)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def run(policy, x, event, **kw):
    """(state after, draws [B,8] numpy, noise [B,NP,H,W] device) of one policy call on a copy of ``x``."""
    st = x.clone()
    draws, noise = policy.apply_(st, 0, event, return_draws=True, return_noise=True, **kw)
    return st, draws.cpu().numpy(), noise


def check_against_reference(policy, x, event, got, forced=None, sample_base=0):
    """Checks 1 and 2 on one call's outputs; returns the largest normal error over its bound."""
    _, draws, noise = got
    fields = PR.policy_fields(policy)
    want, planes = PR.reference(fields, tuple(x.shape), event, sample_base, forced)
    assert np.array_equal(draws, want), (event, forced, draws.tolist(), want.tolist())
    worst = 0.0
    noise = noise.cpu().numpy()
    for b, ref in planes.items():
        if isinstance(ref, tuple):
            n64, radius = ref
            err = np.abs(noise[b].astype(np.float64) - n64) / (NORMAL_BOUND * np.maximum(1.0, radius))
            worst = max(worst, float(err.max()))
        else:
            assert np.array_equal(noise[b, 0].view(np.int32), ref.view(np.int32)), (event, b)
    return worst


# ---------------------------------------------------------------------------------------------
# 1, 2. draws and noise against the numpy restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", sorted(FIELDS) + sorted(BANDED))
@pytest.mark.parametrize("scope", SCOPES)
def test_draws_and_noise_equal_the_reference(dev, D, scope, field):
    x = make_state(field, dev)
    worst, kinds_seen = 0.0, set()
    for cfg in (CFG, dict(CFG, size_min=1, size_max=20, stripe_width=3)):       # size_max > H
        policy = D.DamagePolicy(cfg, SEED, scope)
        for event in EVENTS + tuple(range(20, 32)):
            got = run(policy, x, event, sample_base=3)
            worst = max(worst, check_against_reference(policy, x, event, got, sample_base=3))
            kinds_seen |= set(got[1][:, 1].tolist())
        for kind in ALL_KINDS:                                                   # every kind, whatever was drawn
            forced = [kind, -1, kind, kind, kind]
            got = run(policy, x, 5, kinds=torch.tensor(forced, dtype=torch.int32, device=dev))
            worst = max(worst, check_against_reference(policy, x, 5, got, forced=forced))
            assert got[1][1].tolist() == list(PR.NOT_APPLIED) and got[1][0, 0] == 1
    print(f"{scope} {field}: max normal error / bound = {worst:.3f}; kinds drawn {sorted(kinds_seen)}")
    assert len(kinds_seen - {-1}) >= (7 if scope == "sample" else 5)
    assert worst <= 1.0, worst


def test_gates_and_noops(dev, D):
    x = make_state("vector", dev)
    closed = D.DamagePolicy(dict(CFG, prob=0.5, per_sample_prob=0.5), SEED, "sample")
    applied = []
    for event in range(24):
        got = run(closed, x, event)
        check_against_reference(closed, x, event, got)
        applied.append(got[1][:, 0])
        for b in range(B):
            if not got[1][b, 0]:
                assert same(got[0][b], x[b])
    applied = np.array(applied)
    assert 0 < applied.sum() < applied.size and (applied.sum(1) == 0).any()     # some events gated whole
    batch = D.DamagePolicy(dict(CFG, prob=0.5), SEED, "batch")
    rows = np.array([run(batch, x, e)[1][:, 0] for e in range(16)])
    assert set(rows.sum(1)) == {0, B}                                            # the batch gate: all or none
    # the reference's early returns: nothing is applied and the state keeps its bits
    off = D.DamagePolicy(dict(CFG, alpha_dropout_p=0.0, salt_pepper_p=0.0, hidden_noise_sigma=0.0), SEED, "sample")
    for kind in (PR.ALPHA_DROP, PR.ALPHA_DROP_SOFT, PR.SALT_PEPPER, PR.HIDDEN_NOISE):
        st, draws, _ = run(off, x, 1, kinds=torch.full((B,), kind, dtype=torch.int32, device=dev))
        assert not draws[:, 0].any() and same(st, x)
    x4 = make_state("scalar", dev, channels=4)
    policy = D.DamagePolicy(CFG, SEED, "sample")
    st, draws, _ = run(policy, x4, 1, kinds=torch.full((B,), PR.HIDDEN_NOISE, dtype=torch.int32, device=dev))
    assert not draws[:, 0].any() and same(st, x4)                                # hidden noise at C = 4
    assert policy.apply_(x4, -1, 0) is None                                      # before start_epoch: no launch
    assert D.DamagePolicy(dict(CFG, prob=0.0), SEED).apply_(x4, 0, 0) is None


# ---------------------------------------------------------------------------------------------
# 3. effects: bitwise gnca_damage_f32 from the dumped draws, and the numpy oracle
# ---------------------------------------------------------------------------------------------
def _old_kernel(D, policy, x, draws, noise):
    """gnca_damage_f32 sample by sample from the policy launch's dumped draws and noise."""
    from graph_neural_cellular_automata_amd import _lib as L
    out = x.clone()
    for b in range(x.shape[0]):
        applied, prim, arg, y, x0 = (int(v) for v in draws[b, :5])
        if not applied:
            continue
        sb = out[b:b + 1]
        pos = torch.tensor([[y, x0]], dtype=torch.int32, device=x.device)
        if prim in (L.DMG_SQUARE, L.DMG_CIRCLE, L.DMG_STRIPE_H, L.DMG_STRIPE_V):
            D._launch(sb, prim, arg, pos=pos)
        elif prim == L.DMG_GAUSSIAN:
            D._launch(sb, prim, arg, pos=pos, softness=policy.gaussian_softness)
        elif prim in (L.DMG_ALPHA_DROP, L.DMG_ALPHA_DROP_SOFT):
            D._launch(sb, prim, noise=noise[b:b + 1, :1], p=policy.alpha_dropout_p, alpha_thr=policy.alpha_thr)
        elif prim == L.DMG_SALT_PEPPER:
            D._launch(sb, prim, noise=noise[b:b + 1, :1], p=policy.salt_pepper_p)
        else:
            assert prim == L.DMG_HIDDEN_NOISE
            D._launch(sb, prim, noise=noise[b:b + 1], sigma=policy.hidden_sigma)
    return out


@pytest.mark.parametrize("field", sorted(FIELDS) + sorted(BANDED))
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_effects_are_gnca_damage_f32s(dev, D, kind, field):
    x = make_state(field, dev)
    for cfg, event in ((CFG, 2), (dict(CFG, size_min=9, size_max=20, gaussian_softness=0.2), 3)):
        policy = D.DamagePolicy(cfg, SEED, "sample")
        st, draws, noise = run(policy, x, event, kinds=torch.full((B,), kind, dtype=torch.int32, device=dev))
        assert draws[:, 0].all() and not same(st, x)
        want = _old_kernel(D, policy, x, draws, noise)
        assert same(st, want), PZ.diff(want, st)
        ref = PR.apply_effects(x.cpu().numpy(), PR.policy_fields(policy), draws, noise.cpu().numpy())
        np.testing.assert_allclose(st.cpu().numpy(), ref, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# 4, 5, 6. mixed batches, shards, determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", SCOPES)
def test_mixed_batch_matches_each_kinds_own_batch(dev, D, scope):
    x = make_state("vector", dev)
    policy = D.DamagePolicy(CFG, SEED, scope)
    names = ["gaussian", "alpha_drop", None, "hidden_noise", "stripes"]
    st, draws, _ = run(policy, x, 4, kinds=names)
    assert same(st[2], x[2]) and draws[2].tolist() == list(PR.NOT_APPLIED)
    for b, name in enumerate(names):
        if name is None:
            continue
        alone, d1, _ = run(policy, x, 4, kinds=D.DamagePolicy.codes([name] * B, dev))
        assert same(st[b], alone[b]) and not same(st[b], x[b]), name
        assert draws[b].tolist() == d1[b].tolist()


@pytest.mark.parametrize("field", sorted(FIELDS) + sorted(BANDED))
@pytest.mark.parametrize("scope", SCOPES)
def test_shards_draw_what_the_whole_batch_draws(dev, D, scope, field):
    x = make_state(field, dev)
    policy = D.DamagePolicy(CFG, SEED, scope)
    mixed = D.DamagePolicy.codes(["hidden_noise", "saltpepper", "circle", "stripes", "alpha_drop_soft"], dev)
    for event, kinds in [(e, None) for e in range(8)] + [(3, mixed)]:
        whole, dw, nw = run(policy, x, event, kinds=kinds, sample_base=10)
        lo, dl, _ = run(policy, x[0:2], event, kinds=None if kinds is None else kinds[0:2].clone(), sample_base=10)
        hi, dh, _ = run(policy, x[2:5], event, kinds=None if kinds is None else kinds[2:5].clone(), sample_base=12)
        assert same(whole[0:2], lo) and same(whole[2:5], hi), (event, scope)
        assert np.array_equal(dw, np.concatenate([dl, dh]))


def test_deterministic_and_independent_of_the_other_generators(dev, D):
    x = make_state("scalar", dev)
    policy = D.DamagePolicy(CFG, SEED, "sample")
    torch.manual_seed(12)
    random.seed(12)
    cpu_state, gpu_state, py_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev), random.getstate()
    a = run(policy, x, 6)
    torch.manual_seed(99)
    random.seed(99)
    torch.rand(7, device=dev)
    b = run(policy, x, 6)
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1])
    hidden = [i for i in range(B) if a[1][i, 1] == PR.HIDDEN_NOISE]         # (the other rows of noise are not written)
    assert hidden and same(a[2][hidden], b[2][hidden])
    torch.manual_seed(12)
    random.seed(12)
    run(policy, x, 6)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
    assert random.getstate() == py_state
    c = run(policy, x, 7)
    assert not np.array_equal(a[1], c[1]) and not same(a[0], c[0])
    other = run(D.DamagePolicy(CFG, SEED + 1, "sample"), x, 6)
    assert not np.array_equal(a[1], other[1])
    # a device event counter draws what the same int draws
    ev = torch.tensor([6], dtype=torch.int64, device=dev)
    d = run(policy, x, ev)
    assert same(a[0], d[0]) and np.array_equal(a[1], d[1])


# ---------------------------------------------------------------------------------------------
# 7. no host wait
# ---------------------------------------------------------------------------------------------
def test_apply_makes_no_host_wait_and_the_host_policy_does(dev, D):
    x = make_state("vector", dev)
    policy = D.DamagePolicy(CFG, SEED, "sample")
    kinds = D.DamagePolicy.codes(["square"] * B, dev)
    ev = torch.tensor([3], dtype=torch.int64, device=dev)
    run(policy, x, 0)                                    # (warm: the library and the kernel are loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    raised = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            D.apply_damage_policy_(x.clone(), CFG, 0)
        except RuntimeError:
            raised = True                                # its .item(): the check has teeth
        if raised:                                       # none of these may raise
            st = x.clone()
            policy.apply_(st, 0, 1)
            policy.apply_(st, 0, ev, kinds=kinds)
            draws, noise = policy.apply_(st, 0, 2, return_draws=True, return_noise=True)
            assert draws.is_cuda and noise.is_cuda
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not raised:
        pytest.skip("this torch build does not raise for .item() under set_sync_debug_mode('error') on ROCm")


# ---------------------------------------------------------------------------------------------
# 8. streams and capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_side_stream_and_capture(dev, D, field):
    policy = D.DamagePolicy(CFG, SEED, "sample")
    sets = tuple({"state": make_state(field, dev, seed=s), "event": torch.tensor([e], dtype=torch.int64, device=dev),
                  "kinds": D.DamagePolicy.codes(k, dev)}
                 for s, e, k in ((3, 5, ["square", "hidden_noise", None, "alpha_drop", "gaussian"]),
                                 (4, 9, ["saltpepper", "stripes", "circle", None, "hidden_noise"])))

    def call(bufs):
        draws, noise = policy.apply_(bufs["state"], 0, bufs["event"], kinds=bufs["kinds"], return_draws=True)
        return {"state": bufs["state"], "draws": draws}

    case = ST.Case(f"damage-policy-{field}", sets, call)
    ST.run(case)
    want, _ = case.eager
    assert not same(want[0]["draws"], want[1]["draws"])


def test_a_captured_loop_draws_afresh_on_every_replay(dev, D):
    """One chain on one stream: increment the device event counter, then apply the policy."""
    policy = D.DamagePolicy(dict(CFG, kinds={"square": 1.0, "saltpepper": 1.0, "circle": 1.0}), SEED, "sample")
    x = make_state("vector", dev)
    e0 = 40
    eager = x.clone()
    policy.apply_(eager, 0, e0 + 1)
    first = eager.clone()
    policy.apply_(eager, 0, e0 + 2)
    torch.cuda.synchronize()
    state = torch.empty_like(x)
    event = torch.zeros(1, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    state.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        event.add_(1)
        policy.apply_(state, 0, event)
    state.copy_(x)
    event.fill_(e0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert same(state, first) and int(event.item()) == e0 + 1
    g.replay()
    torch.cuda.synchronize()
    assert same(state, eager) and int(event.item()) == e0 + 2
    assert not same(first, eager) and not same(first, x)


# ---------------------------------------------------------------------------------------------
# 9. guards and poison
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_guards_and_unwritten_noise_rows(dev, D, kind, field):
    x = make_state(field, dev)
    policy = D.DamagePolicy(dict(CFG, size_min=1, size_max=20), SEED, "sample")
    forced = [kind, kind, -1, kind, kind]
    HW = x.shape[2] * x.shape[3]

    def call(P):
        st = P.guard(x, inplace=True)
        kinds = P.guard(torch.tensor(forced, dtype=torch.int32, device=dev))
        draws, noise = policy.apply_(st, 0, 8, kinds=kinds, return_draws=True, return_noise=True)
        if P.fill == "ones":                             # every byte 0xFF: what is not written reads -1
            torch.cuda.synchronize()
            nb, dr = bits(noise).reshape(B, C - 4, HW), draws.cpu().numpy()
            for b in range(B):
                prim = int(dr[b, 1])
                written = 0 if not dr[b, 0] else {PR.ALPHA_DROP: 1, PR.ALPHA_DROP_SOFT: 1, PR.SALT_PEPPER: 1,
                                                  PR.HIDDEN_NOISE: C - 4}.get(prim, 0)
                assert bool((nb[b, written:] == -1).all()), (b, prim, "a row the contract leaves alone was written")
                if written:
                    assert torch.isfinite(noise[b, :written]).all(), (b, prim)
        return {"state": st, "draws": draws}

    outs = PZ.run_fills(call, f"damage-policy-{kind}-{field}")
    assert same(outs["state"][2], x[2]) and not same(outs["state"], x)
    plain = run(policy, x, 8, kinds=torch.tensor(forced, dtype=torch.int32, device=dev))
    assert same(outs["state"], plain[0]) and np.array_equal(outs["draws"].cpu().numpy(), plain[1])


# ---------------------------------------------------------------------------------------------
# 10. regrow_trace
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage_step", [2, 0])
def test_regrow_trace_is_two_traces_with_the_policy_in_between(dev, D, damage_step):
    from graph_neural_cellular_automata_amd import NeuralCAGraph
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=0.25).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    g = torch.Generator().manual_seed(31)
    x = torch.rand(3, 16, 20, 24, generator=g)
    x[:, 4:] = torch.randn(3, 12, 20, 24, generator=g)
    x = x.to(dev)
    target = torch.rand(4, 20, 24, generator=g).to(dev)
    policy = D.DamagePolicy(dict(CFG, size_min=6, size_max=10), SEED, "sample")
    names = ["circle", "hidden_noise", "alpha_drop"]
    steps = 6
    kw = dict(return_attention=True, fire_rate=0.5, seed=5, target=target, render=True, sample_base=4)
    random.seed(17)
    res = D.regrow_trace(model, x, steps, policy, damage_step, event=3, kinds=names, every=2, **kw)
    random.seed(17)
    parts = []
    mid = x.clone()
    if damage_step:
        parts.append(model.trace(x, damage_step, record=[2], **kw))
        mid = parts[0].x_final.clone()
    policy.apply_(mid, 0, 3, kinds=names, sample_base=4)
    rec2 = [r - damage_step for r in (2, 4, 6) if r > damage_step]
    parts.append(model.trace(mid, steps - damage_step, record=rec2, first_step=damage_step, **kw))
    assert res.steps == [2, 4, 6]
    assert same(res.x_final, parts[-1].x_final)
    for name in ("frames", "attention", "rgb_u8", "attention_u8"):
        want = torch.cat([getattr(p, name) for p in parts], 0)
        assert PZ.same_bytes(getattr(res, name), want), name
        assert want.shape[0] == 3
    assert PZ.same_bytes(res.metrics.stacked, torch.cat([p.metrics.stacked for p in parts], 0))
    assert tuple(res.metrics.mse.shape) == (3, 3)
    # the damage is in the curve: the damaged run differs from the undamaged one after the damage only
    random.seed(17)
    plain = model.trace(x, steps, every=2, **kw)
    first_damaged = 0 if damage_step == 0 else 1
    assert PZ.same_bytes(res.frames[:first_damaged], plain.frames[:first_damaged])
    assert not PZ.same_bytes(res.frames[first_damaged], plain.frames[first_damaged])
    with pytest.raises(ValueError):
        D.regrow_trace(model, x, steps, policy, steps, **kw)
