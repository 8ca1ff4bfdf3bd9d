"""The split K1's fp32-class claim at the GEMM (gnca_k1_split.h, gnca_k1_split32.h): every fp32 product
is six bf16 part products, a0b0 a0b1 a1b0 a0b2 a2b0 a1b1.  A dropped third-order product moves the
step's OUTPUT by ~1e-6, below the 2e-6 the parity and fuzz tests allow, so these tests read K1's
update field itself, before GroupNorm and tanh (tests/k1_probe.py), on every split instantiation of
``kVariants`` (the plan asserted by name) and one generic fp32-MFMA shape as the control:

* term selectors: integer operands whose exact result every correct fp32-class GEMM returns in any
  summation order, the low bits carried by one group of part products at a time; bitwise against the
  float64 oracle, over weight patterns that make every slot of the targeted matrix nonzero once;
* the error budget: realistic operands, |dx - dl64| in units of u |W2| (|W1| yhat + |b1|) within 4x the
  torch-CPU fp32 reference's on the same inputs (rms and max), logged per variant;
* the exponent range: W1, b1 scaled by 2^s and W2 by 2^-s leave every bit unchanged; a NaN in W2;
* the message GEMM through K1's tanh: third-order products of one sign summing to > 1e-4.

tests/test_split_emul_cpu.py proves on the CPU that these inputs tell the six-term scheme from every
five-term one.  Reference path: ncagraph.py:128-150 (update_net on the perception, the message policy,
the pre-update alive mask)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests import split_emul as E
from tests.k1_probe import Probe, torch_ref_dl32
from tests.test_gpu_drift import DRIFT_LOG

pytestmark = pytest.mark.gpu

# every variant's figures are appended here (JSON lines), beside the drift log
LOG = os.environ.get("GNCA_K1_PRECISION_LOG", os.path.join(os.path.dirname(DRIFT_LOG), "k1_precision.jsonl"))
SCALES = (-64, -20, 20, 64)
MESSAGE_VARIANTS = ("g8x24", "g8x24zp", "g32")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _log(rec):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps(dict(rec, time=time.time())) + "\n")


def _masked(d64, live):
    """The expected field: the oracle's dl at live cells, exact zeros at dead ones."""
    return np.where(np.broadcast_to(live, d64.shape), d64, 0.0)


@pytest.mark.parametrize("kind", sorted(E.SELECTORS))
@pytest.mark.parametrize("vid", sorted(E.VARIANTS))
def test_term_selectors_bitwise(dev, vid, kind):
    """Integer operands (every kept product and partial sum an integer below 2^23, split_emul.LIMIT, no
    dropped product nonzero): the update field equals the float64 oracle's dl bit for bit at live cells
    and is an exact zero at dead ones, for every weight pattern of the case.  Graph variants run with wm = bm = 0: the
    message term is tanh(0) * gain = 0."""
    p = Probe(vid, dev)
    xb = E.selector_state(kind, p.C, p.H, p.W, p.nb)
    live = E.live_mask(xb)
    assert live.any() and not live.all()
    y64 = O.perceive(xb.astype(np.float64), O.sobel_weights(p.C, np.float64))
    x = p.state(xb)
    bad, worst = [], 0.0
    for rnd in range(E.selector_rounds(kind, p.C, p.HD)):
        W1, b1, W2 = E.selector_weights(kind, p.C, p.HD, rnd)
        worst = max(worst, E.selector_check(xb, W1, b1, W2, y64))
        p.set(w1=W1, b1=b1, w2=W2)
        bad.append(p.mismatches(p.dx(x), _masked(E.dl64(xb, W1, b1, W2, y64), live)))
    assert worst < E.LIMIT
    bad = torch.stack(bad).cpu().numpy()
    print(f"[k1-selector] {vid} {p.name} {kind}: {len(bad)} weight patterns, largest sum of |products| "
          f"2^{np.log2(worst):.2f}, mismatching values {int(bad.sum())}")
    assert bad.sum() == 0, f"{vid} {kind}: rounds with wrong values {np.nonzero(bad)[0].tolist()}, counts {bad[bad != 0].tolist()}"


@pytest.fixture(scope="module")
def budget_refs():
    """Per input shape: the inputs, the float64 oracle, the bound and the fp32 reference's error,
    computed once."""
    cache = {}

    def get(C, HD, H, W, nb):
        key = (C, HD, H, W, nb)
        if key not in cache:
            x, W1, b1, W2 = E.budget_inputs(C, HD, H, W, nb)
            d64, bnd, live = E.dl64(x, W1, b1, W2), E.bound(x, W1, b1, W2), E.live_mask(x)
            ref = E.norm_err(torch_ref_dl32(x, W1, b1, W2), d64, bnd, live)
            cache[key] = (x, W1, b1, W2, d64, bnd, live, ref)
        return cache[key]
    return get


def _budget_run(p, budget_refs):
    x, W1, b1, W2, d64, bnd, live, ref = budget_refs(p.C, p.HD, p.H, p.W, p.nb)
    p.set(w1=W1, b1=b1, w2=W2)
    xd = p.state(x)
    dx = p.dx(xd)
    return xd, dx, (x, W1, b1, W2, d64, bnd, live, ref)


@pytest.mark.parametrize("vid", sorted(E.VARIANTS))
def test_error_budget(dev, vid, budget_refs):
    """Realistic operands (alpha ~ U(0,1), hidden ~ N(0,1) 2^e per channel, W ~ N(0, 0.3), full mantissas,
    GroupNorm off, message zeroed): e = |dx - dl64| / (u |W2| (|W1| yhat + |b1|)) at live cells, against
    the same measure of oracle/torch_cpu_ref.py's fp32 update on the same inputs:
    rms(e) <= 4 rms(e_ref32) and max(e) <= 4 max(e_ref32).  The factor 4 is the margin for summation
    order and the MFMA's internal accumulation; the weakest five-term mutant of the emulator sits at
    12x (tests/test_split_emul_cpu.py).  Measured values: DESIGN.md, "K1 precision at the GEMM"."""
    p = Probe(vid, dev)
    _, dx, (x, W1, b1, W2, d64, bnd, live, (ref_rms, ref_max)) = _budget_run(p, budget_refs)
    got = dx.cpu().numpy().reshape(p.B // p.nb, *x.shape)
    assert (got == got[0]).all(), "repeated samples differ"
    got = got[0]
    m = np.broadcast_to(live, got.shape)
    assert np.isfinite(got).all() and (got[~m] == 0).all(), "dead cells hold exact zeros"
    rms, mx = E.norm_err(got, d64, bnd, live)
    print(f"[k1-budget] {vid} {p.name}: rms {rms:.4f} max {mx:.3f} (fp32 reference: rms {ref_rms:.4f} max {ref_max:.3f}; "
          f"{int(m.sum())} values)")
    _log({"test": "budget", "variant": vid, "k1": p.name, "arith": p.arith, "zero_pad": p.zp, "batch": p.B,
          "canvas": [p.H, p.W], "values": int(m.sum()), "rms": rms, "max": mx, "ref32_rms": ref_rms,
          "ref32_max": ref_max, "factor": 4})
    assert rms <= 4 * ref_rms, (rms, ref_rms)
    assert mx <= 4 * ref_max, (mx, ref_max)


@pytest.mark.parametrize("vid", ["g8x24", "g24x36zp", "c8x20", "g32", "f32_16x64"])
def test_probe_is_zero_at_dead_and_unfired_cells(dev, vid, budget_refs):
    """The probe's own check: with a uint8 fire mask the field is an exact zero wherever the cell is dead
    or did not fire, and bit for bit the unmasked run's value wherever it is live and fired."""
    p = Probe(vid, dev)
    x, W1, b1, W2, *_rest = budget_refs(p.C, p.HD, p.H, p.W, p.nb)
    x = x.copy()
    x[:, 3, 1:7, 2:9] = 0          # a block without alpha: its interior is dead
    live = E.live_mask(x)
    p.set(w1=W1, b1=b1, w2=W2)
    xd = p.state(x)
    dx_all = p.dx(xd)
    q = Probe(vid, dev, fire_mask=True)
    q.set(w1=W1, b1=b1, w2=W2)
    fire = torch.from_numpy((np.random.default_rng(9).random((p.B, 1, p.H, p.W)) < 0.5).astype(np.uint8)).to(dev)
    dx = q.dx(xd, fire)
    alive = torch.from_numpy(np.ascontiguousarray(live)).to(dev).repeat(p.B // p.nb, 1, 1, 1)
    keep = fire.bool() & alive
    assert keep.any() and (fire.bool() & ~alive).any() and (~fire.bool() & alive).any()
    zero = torch.zeros_like(dx_all)
    assert torch.equal(dx_all, torch.where(alive, dx_all, zero)), "FIRE_NONE: dead cells hold exact zeros"
    assert torch.equal(dx, torch.where(keep, dx_all, zero))
    assert (dx_all[alive.expand_as(dx_all)] != 0).all()


@pytest.mark.parametrize("vid", sorted(E.VARIANTS))
def test_exponent_range_is_bitwise_neutral(dev, vid, budget_refs):
    """W1 and b1 scaled by 2^s, W2 by 2^-s, s in {-64, -20, 20, 64}: within the header's documented range
    nothing is subnormal and the halved third W2 image stays exact, so h scales by 2^s exactly and the
    update field keeps every bit of the s = 0 run."""
    p = Probe(vid, dev)
    xd, dx0, (x, W1, b1, W2, *_rest) = _budget_run(p, budget_refs)
    assert torch.isfinite(dx0).all() and (dx0 != 0).any()
    bad = []
    for s in SCALES:
        up, down = np.float32(2.0 ** s), np.float32(2.0 ** -s)
        p.set(w1=W1 * up, b1=b1 * up, w2=W2 * down)
        bad.append((p.dx(xd) != dx0).sum())
    bad = torch.stack(bad).cpu().numpy()
    print(f"[k1-range] {vid} {p.name}: values differing from s = 0 at s = {list(SCALES)}: {bad.tolist()}")
    assert bad.sum() == 0, dict(zip(SCALES, bad.tolist()))


@pytest.mark.parametrize("vid", sorted(E.VARIANTS))
def test_w2_nan_pattern_like_oracle(dev, vid, budget_refs):
    """A NaN in W2 (test_relu_keeps_nan_like_torch's counterpart for the second GEMM): NaN times
    anything, a relu zero included, is NaN, so the NaN's output channel is NaN at every live cell and no
    other value is, as in the oracle."""
    p = Probe(vid, dev)
    x, W1, b1, W2, _, _, live, _ = budget_refs(p.C, p.HD, p.H, p.W, p.nb)
    W2 = W2.copy()
    W2[5, p.HD // 2 + 3] = np.nan
    p.set(w1=W1, b1=b1, w2=W2)
    got = p.dx(p.state(x)).cpu().numpy()[:p.nb]
    with np.errstate(invalid="ignore"):
        ref = E.dl64(x, W1, b1, W2)
    m = np.broadcast_to(live, ref.shape)
    assert np.isnan(ref[:, 5][live[:, 0]]).all() and np.isnan(ref).sum() == live.size
    np.testing.assert_array_equal(np.isnan(got)[m], np.isnan(ref)[m])


@pytest.mark.parametrize("role", sorted(E.MESSAGE_ROLES))
@pytest.mark.parametrize("vid", MESSAGE_VARIANTS)
def test_message_gemm_third_order(dev, vid, role):
    """The message GEMM inside K1's tanh.  wm rows and states built from parts (split_emul.message_inputs):
    m near 0.4 - 0.5 from sign-alternating first- and second-order products, the role's third-order
    products (wm2 g0, wm0 g2 or wm1 g1) all positive and summing to > 1e-4, which moves tanh(m) by
    > 1e-4 (each mutant misses by > 1e-5: tests/test_split_emul_cpu.py).  W2 = 0, one offset (k copies,
    so that the plan keeps the split K1: the gather's sum and 1/k weight are exact), alive_to_alive off,
    message_gain 1, hidden_only off: dx = tanh(m).  Bound: 1e-6, five times fast_tanh's stated error
    (gnca_device.h)."""
    k = E.VARIANTS[vid][8]
    p = Probe(vid, dev, message_gain=1.0, offsets=[E.MESSAGE_OFFSET] * k, a2a=False, hidden_only=False)
    x, wm = E.message_inputs(role, p.C, p.H, p.W, p.nb)
    assert E.live_mask(x).all()
    rng = np.random.default_rng(5)
    p.set(w1=rng.standard_normal((p.HD, 3 * p.C)) * 0.3, b1=rng.standard_normal(p.HD) * 0.2,
          w2=np.zeros((p.C, p.HD)), wm=wm, bm=np.zeros(p.C))
    got = p.dx(p.state(x)).cpu().numpy()[:p.nb].astype(np.float64)
    prm = {"graph.query_proj.weight": p.t["wq"], "graph.query_proj.bias": p.t["bq"],
           "graph.key_proj.weight": p.t["wk"], "graph.key_proj.bias": p.t["bk"], "graph.scaling": p.t["scaling"]}
    prm = {n: t.cpu().numpy().astype(np.float64) for n, t in prm.items()}
    prm.update({"graph.msg_proj.weight": wm.astype(np.float64), "graph.msg_proj.bias": np.zeros(p.C)})
    m64 = O.graph_message(x.astype(np.float64), prm, p.offsets, zero_padded_shift=p.zp, alive_to_alive=False,
                          alpha_thr=E.ALPHA_THR)
    # (equal logits for the k copies: softmax weights of exactly 1/k, so m64 is wm times the shifted state)
    np.testing.assert_allclose(m64, np.einsum("ck,bkhw->bchw", wm.astype(np.float64),
                                              E.message_shift(x, p.zp).astype(np.float64)), rtol=0, atol=1e-14)
    err = np.abs(got - np.tanh(m64))
    print(f"[k1-message] {vid} {p.name} {role}: max |dx - tanh(m64)| = {err.max():.3e}, mean {err.mean():.3e}")
    _log({"test": "message", "variant": vid, "k1": p.name, "zero_pad": p.zp, "role": role,
          "max_abs_err": float(err.max()), "mean_abs_err": float(err.mean()), "bound": 1e-6})
    assert err.max() <= 1e-6, err.max()
