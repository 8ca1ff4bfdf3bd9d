"""The state vitals on the GPU (gnca_state_vitals / gnca_rollout_trace_vitals, ``state_vitals``,
``trace(vitals=...)``) against the float64 oracle of tests/vitals_ref.py.

Exact cases use dyadic data: every value is k/1024 with |k| <= 2048 and alpha_thr = 0.125 = 128/1024, so
every term of every sum (values, squares k^2/2^20, clip * index) and every partial sum is an integer
multiple of 2^-20 far below 2^53 of them: the sums are exact in fp64 in any order.  Counts, the bounding
box, ``max_abs`` and the sums must then equal the oracle exactly, and ``cy``, ``cx`` and ``hidden_rms``
(one correctly rounded division, or a division and a square root, of exact sums) within 1 ulp.

General fp32 data: each sum is within n * 2^-52 * sum|term| of the oracle's (n terms; either side's
error is at most (n-1) * 2^-53 * sum|term| in any order).  For the derived fields that bound is carried
through the definition: with E_s and E_m the bounds of the numerator and of the mass,
|d cy| <= (E_s + |cy| E_m) / mass + 2 ulp(cy), and with E_q the bound of the hidden sum of squares over
N values, |d rms| <= E_q / (2 N rms) + 4 ulp(rms) (d sqrt(q) = dq / (2 sqrt(q)); the ulps are the
final roundings of both sides)."""
import random

import numpy as np
import pytest
import torch

from tests import poison as P
from tests import vitals_ref as VR

pytestmark = pytest.mark.gpu

THR = 0.125
EXACT = [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]
F = {n: i for i, n in enumerate(VR.FIELDS)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _vitals(x, thr=THR):
    from graph_neural_cellular_automata_amd import state_vitals
    return state_vitals(x, thr)


def _dyadic(N, C, H, W, seed):
    """N samples of k/1024 values, |k| <= 2048; sample n is of kind n % 3: 0 has no mature cell (and cells
    with a == alpha_thr exactly), 1 is fully mature, 2 is mixed with a == alpha_thr cells planted."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-2048, 2049, size=(N, C, H, W)) / 1024.0).astype(np.float32)
    a = (rng.integers(-512, 1537, size=(N, H, W)) / 1024.0).astype(np.float32)
    at_thr = rng.random((N, H, W)) < 0.2
    for n in range(N):
        if n % 3 == 0:
            a[n] = np.minimum(a[n], np.float32(THR))
        elif n % 3 == 1:
            a[n] = np.maximum(a[n], np.float32(THR + 1 / 1024.0))
        else:
            a[n][at_thr[n]] = THR
            a[n, H // 2, W // 2] = THR          # (at least one, whatever the draw)
    x[:, 3] = a
    assert (x[0::3, 3] <= THR).all() and (x[0::3, 3] == THR).any()
    assert N < 2 or (x[1::3, 3] > THR).all()
    return x


def _assert_exact(got, ref, what):
    for f in EXACT:
        assert np.array_equal(got[:, f], ref[:, f]), (what, VR.FIELDS[f], got[:, f], ref[:, f])
    for f in (F["cy"], F["cx"], F["hidden_rms"]):
        g, r = got[:, f], ref[:, f]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, VR.FIELDS[f], g, r)
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        print(f"{what} {VR.FIELDS[f]}: max |got - ref| = {err.max() if err.size else 0.0:.3e}")
        assert (err <= np.spacing(np.abs(r[ok]))).all(), (what, VR.FIELDS[f], g, r)


# the issue's four shapes, then two that cross a column-tile boundary (W > 256; the second with four
# channels only and W % 4 != 0) and one row
SHAPES = [(3, 4, 9, 13), (2, 6, 40, 40), (5, 16, 72, 72), (1, 32, 16, 200), (1, 5, 11, 300), (2, 4, 3, 259),
          (3, 7, 1, 5)]


def test_the_cases_cross_a_band_boundary():
    from graph_neural_cellular_automata_amd import _lib as L
    band, cols = L.VITALS_BAND_ROWS, L.VITALS_TILE_COLS
    print(f"band height {band} rows, tile width {cols} columns")
    assert any(H > band for _, _, H, _ in SHAPES[:4])
    assert any(H > band and H % band for _, _, H, _ in SHAPES) and any(H > 2 * band for _, _, H, _ in SHAPES)
    assert any(W > cols for _, _, _, W in SHAPES)
    assert any(W % 4 == 0 for _, _, _, W in SHAPES) and any(W % 4 for _, _, _, W in SHAPES)


@pytest.mark.parametrize("B,C,H,W", SHAPES, ids=[f"{b}x{c}x{h}x{w}" for b, c, h, w in SHAPES])
def test_dyadic_states_equal_the_oracle(dev, B, C, H, W):
    N = -(-max(B, 3) // B) * B          # every kind of sample appears, B at a time
    x = _dyadic(N, C, H, W, seed=1000 * H + W)
    ref = VR.state_vitals(x, THR)
    assert (ref[0::3, F["mature"]] == 0).all() and (ref[0::3, F["y0"]] == -1).all()
    assert (ref[1::3, F["mature"]] == H * W).all() and (ref[1::3, F["alive"]] == H * W).all()
    for n0 in range(0, N, B):
        v = _vitals(torch.from_numpy(x[n0:n0 + B]).to(dev))
        assert v.stacked.shape == (B, 13) and v.stacked.dtype == torch.float64 and not v.stacked.requires_grad
        assert v.alive.shape == (B,)
        _assert_exact(v.stacked.cpu().numpy(), ref[n0:n0 + B], f"{B}x{C}x{H}x{W}@{n0}")


def _general(B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32) * np.float32(1.7)
    a = (rng.random((B, H, W), dtype=np.float32) * np.float32(1.6) - np.float32(0.3))
    near = np.abs(a - np.float32(THR)) < 1e-6
    a[near] = np.float32(THR + 2e-6)        # moved away from the threshold here, not skipped later
    x[:, 3] = a
    assert (np.abs(x[:, 3].astype(np.float64) - THR) >= 1e-6).all()
    return x


@pytest.mark.parametrize("B,C,H,W", SHAPES[:4], ids=[f"{b}x{c}x{h}x{w}" for b, c, h, w in SHAPES[:4]])
def test_general_states_within_the_summation_bound(dev, B, C, H, W):
    x = _general(B, C, H, W, seed=7 * H + W)
    ref = VR.state_vitals(x, THR)
    got = _vitals(torch.from_numpy(x).to(dev)).stacked.cpu().numpy()
    for f in (0, 1, 6, 7, 8, 9, 10, 11):          # counts, the box and max_abs: still exact
        assert np.array_equal(got[:, f], ref[:, f]), (VR.FIELDS[f], got[:, f], ref[:, f])
    t = VR.sum_terms(x)
    u = 2.0 ** -52
    E = {k: n * u * mag for k, (n, mag) in t.items()}
    for name, key in (("alpha_sum", "alpha_sum"), ("mass", "mass")):
        err = np.abs(got[:, F[name]] - ref[:, F[name]])
        print(f"{name}: max err {err.max():.3e}, bound {E[key].min():.3e}")
        assert (err <= E[key]).all(), (name, err, E[key])
    mass = np.minimum(got[:, F["mass"]], ref[:, F["mass"]])
    assert (mass > 0).all()
    for name, key in (("cy", "sy"), ("cx", "sx")):
        r = ref[:, F[name]]
        bound = (E[key] + np.abs(r) * E["mass"]) / mass + 2 * np.spacing(np.abs(r))
        err = np.abs(got[:, F[name]] - r)
        print(f"{name}: max err {err.max():.3e}, bound {bound.min():.3e}")
        assert (err <= bound).all(), (name, err, bound)
    r = ref[:, F["hidden_rms"]]
    if C > 4:
        n = (C - 4) * H * W
        bound = E["hidden_sq"] / (2.0 * n * np.minimum(r, got[:, F["hidden_rms"]])) + 4 * np.spacing(r)
        err = np.abs(got[:, F["hidden_rms"]] - r)
        print(f"hidden_rms: max err {err.max():.3e}, bound {bound.min():.3e}")
        assert (err <= bound).all(), (err, bound)
    else:
        assert (got[:, F["hidden_rms"]] == 0).all() and (r == 0).all()


@pytest.mark.parametrize("C,H,W", [(16, 72, 72), (6, 9, 13)], ids=["16x72x72", "6x9x13"])
def test_a_sample_does_not_depend_on_its_batch(dev, C, H, W):
    x = torch.from_numpy(_general(5, C, H, W, seed=11)).to(dev)
    full = _vitals(x).stacked
    assert P.same_bytes(full, _vitals(x).stacked)                     # two runs of the same call
    alone = _vitals(x[2:3].clone()).stacked
    assert P.same_bytes(alone[0], full[2]), P.diff(alone[0], full[2])
    for n in range(5):
        assert P.same_bytes(_vitals(x[n:n + 1]).stacked[0], full[n]), n
    perm = [3, 0, 4, 2, 1]
    assert P.same_bytes(_vitals(x[perm]).stacked, full[perm])


def test_nonfinite_hidden_values(dev):
    B, C, H, W = 3, 16, 40, 40
    clean = _dyadic(B, C, H, W, seed=5)
    dirty = clean.copy()
    rng = np.random.default_rng(6)
    for b, count in ((0, 1), (1, 37), (2, 400)):
        idx = rng.choice((C - 4) * H * W, size=count, replace=False)
        vals = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=count)
        dirty[b, 4:].reshape(-1)[idx] = vals
    assert np.isfinite(dirty[:, :4]).all()
    ref = VR.state_vitals(dirty, THR)
    assert np.array_equal(ref[:, F["nonfinite"]], [1, 37, 400])
    got = _vitals(torch.from_numpy(dirty).to(dev)).stacked.cpu().numpy()
    base = _vitals(torch.from_numpy(clean).to(dev)).stacked.cpu().numpy()
    _assert_exact(got, ref, "nonfinite")
    assert np.array_equal(got[:, F["nonfinite"]], [1, 37, 400])
    assert np.isfinite(got[:, F["max_abs"]]).all() and np.isfinite(got[:, F["hidden_rms"]]).all()
    assert np.array_equal(got[:, :10].view(np.int64), base[:, :10].view(np.int64))     # fields 0..9: the clean bits
    # every value non-finite, alpha too: fields 10 and 11 are still defined
    allnan = torch.full((1, 5, 9, 13), float("nan"), device=dev)
    v = _vitals(allnan)
    assert v.nonfinite.item() == 5 * 9 * 13 and v.max_abs.item() == 0.0 and v.hidden_rms.item() == 0.0


def test_strided_inputs_give_the_bits_of_their_copies(dev):
    B, C, H, W = 3, 16, 24, 24
    gen = torch.Generator(device=dev).manual_seed(3)
    wide = torch.randn(5, 20, H, W, device=dev, generator=gen)
    wide[:, 4] = torch.rand(5, H, W, device=dev, generator=gen)
    for view in (wide[:, 1:17], wide[1:4, :16], wide[::2, 1:5], wide[:, 1:17].transpose(2, 3),
                 wide.flatten()[1:1 + 2 * 8 * H * W].view(2, 8, H, W)):       # the last: a 4-byte-aligned base
        a, b = _vitals(view).stacked, _vitals(view.contiguous().clone()).stacked
        assert P.same_bytes(a, b), P.diff(a, b)
    # an [R,B,...] input: each record is the [B,...] call
    rb = wide[:4].reshape(2, 2, 20, H, W)[:, :, 1:17]
    v = _vitals(rb)
    assert v.stacked.shape == (2, 2, 13) and v.cx.shape == (2, 2)
    for r in range(2):
        assert P.same_bytes(v.stacked[r], _vitals(rb[r].contiguous()).stacked)
    ref = VR.state_vitals(rb.reshape(4, 16, H, W).cpu().numpy(), THR)
    assert np.array_equal(v.stacked.reshape(4, 13).cpu().numpy()[:, [0, 1, 6, 7, 8, 9, 10, 11]],
                          ref[:, [0, 1, 6, 7, 8, 9, 10, 11]])


@pytest.mark.parametrize("B,C,H,W", [(3, 4, 9, 13), (2, 16, 40, 40), (1, 6, 11, 300)],
                         ids=["3x4x9x13", "2x16x40x40", "1x6x11x300"])
def test_poisoned_buffers(dev, B, C, H, W):
    """``out`` and ``ws`` come from the poisoned allocator: the guards stay intact, and every one of the
    B x 13 outputs is written (the same bytes from a 0x00, a 0xFF and a random prefill)."""
    x = torch.from_numpy(_dyadic(B, C, H, W, seed=9)).to(dev)

    def call(Pz):
        v = _vitals(Pz.guard(x))
        assert len(Pz.blocks) == 3, [b.name() for b in Pz.blocks]      # the input, out and ws
        return {"vitals": v.stacked}

    got = P.run_fills(call, f"vitals-{B}x{C}x{H}x{W}")["vitals"]
    _assert_exact(got.cpu().numpy(), VR.state_vitals(x.cpu().numpy(), THR), "poison")


def test_side_stream_gives_the_default_streams_bits(dev):
    x = torch.from_numpy(_general(4, 16, 40, 40, seed=21)).to(dev)
    base = _vitals(x).stacked
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        y = x * 1.0                      # produced on the side stream: the call must be ordered after it
        got = _vitals(y).stacked
    side.synchronize()
    assert P.same_bytes(got, base), P.diff(got, base)


def test_stream_contract_state_vitals(dev):
    """The three legs of tests/streams.py (eager, side stream with delayed inputs, capture and replay):
    the two launches are ordered on the caller's stream, nothing synchronises, the call can be captured."""
    from tests import streams as ST
    sets = tuple({"x": torch.from_numpy(_general(3, 16, 40, 40, seed=s)).to(dev)} for s in (41, 42))
    case = ST.Case("gnca_state_vitals", sets, lambda b: {"vitals": _vitals(b["x"]).stacked})
    ST.run(case, ST.LEGS)
    want, _ = case.eager
    assert not P.same_bytes(want[0]["vitals"], want[1]["vitals"])          # the two sets differ


def test_stream_contract_trace_vitals(dev):
    """gnca_rollout_trace_vitals on the same three legs, on the dense row of tests/test_gpu_streams.py
    (its trace cases' setup): the vitals launches follow the pieces in stream order."""
    from graph_neural_cellular_automata_amd import step as S
    from tests import streams as ST
    from tests import test_gpu_streams as G
    name, B, H, W = G.DENSE_ROW
    seed, T = 31, G.ROLLOUT_STEPS
    m, _, sets, offs = G._rollout_setup(name, B, H, W, "sparse", dev, seed)
    desc = G._hash_desc(m, B, H, W, seed)
    record = S.expand_record(T, G.TRACE_EVERY)

    def call(b):
        out, frm, attn, _, _, vit = S.trace_vitals(desc, G._W(b), b["x"], T, offs, record, 4, 0.1,
                                                   want_attention=True)
        return {"x_final": out, "frames": frm, "attn": attn, "vitals": vit}

    case = ST.Case("trace-vitals", sets, call)
    ST.run(case, ST.LEGS)
    base = S.trace(desc, G._W(sets[0]), sets[0]["x"], T, offs, record, 4, want_attention=True)
    want = case.eager[0][0]
    assert torch.equal(want["x_final"], base[0]) and torch.equal(want["frames"], base[1])
    assert torch.equal(want["attn"], base[2])


# ---- trace(vitals=...) ----
GAIN, MSG, FIRE, SEED = 0.05, 0.25, 0.5, 5
TB, TH, TT, RECORD = 2, 24, 6, [2, 5, 6]


def _models(dev):
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    torch.manual_seed(0)
    g = NeuralCAGraph(16, 128, update_gain=GAIN, alpha_thr=0.12, message_gain=MSG,
                      graph_zero_padded_shift=False).to(dev).eval()
    c = NeuralCA(16, 128, update_gain=GAIN, alpha_thr=0.12).to(dev).eval()
    with torch.no_grad():
        g.update_net[2].weight.normal_(0, 0.05)
        c.update_net[2].weight.normal_(0, 0.05)
    return g, c


def _state(dev):
    gen = torch.Generator(device=dev).manual_seed(31)
    x = torch.rand(TB, 16, TH, TH, device=dev, generator=gen)
    x[:, 4:] = torch.randn(TB, 12, TH, TH, device=dev, generator=gen)
    return x


def _same_trace(a, b):
    assert torch.equal(a.x_final, b.x_final) and a.steps == b.steps
    for n in ("frames", "attention"):
        ta, tb = getattr(a, n), getattr(b, n)
        assert (ta is None) == (tb is None) and (ta is None or torch.equal(ta, tb)), n
    assert (a.metrics is None) == (b.metrics is None)
    if a.metrics is not None:
        assert P.same_bytes(a.metrics.stacked, b.metrics.stacked)


@pytest.mark.parametrize("kind", ["graph", "classic"])
def test_trace_vitals(dev, kind):
    g, c = _models(dev)
    model = g if kind == "graph" else c
    x = _state(dev)
    kw = dict(record=RECORD, fire_rate=FIRE, seed=SEED)
    if kind == "graph":
        rr = random.Random(17)
        assert max(max(abs(dy), abs(dx)) for dy, dx in model.graph.offsets) == 4          # torus, r = 4
        kw["offsets"] = [rr.sample(model.graph.offsets, 8) for _ in range(TT)]            # K = 8
    t = torch.rand(4, TH, TH, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    base = model.trace(x, TT, channels=16, **kw)
    assert base.vitals is None
    tr = model.trace(x, TT, channels=16, vitals=True, **kw)
    assert tr.steps == RECORD and tr.vitals.stacked.shape == (3, TB, 13) and tr.vitals.alive.shape == (3, TB)
    assert tr.vitals.stacked.dtype == torch.float64 and not tr.vitals.stacked.requires_grad
    _same_trace(tr, base)
    want = _vitals(tr.frames, model.alpha_thr).stacked
    assert P.same_bytes(tr.vitals.stacked, want), P.diff(tr.vitals.stacked, want)
    ref = VR.state_vitals(tr.frames.reshape(-1, 16, TH, TH).cpu().numpy(), np.float32(model.alpha_thr))
    got = tr.vitals.stacked.reshape(-1, 13).cpu().numpy()
    for f in (0, 1, 6, 7, 8, 9, 10, 11):
        assert np.array_equal(got[:, f], ref[:, f]), VR.FIELDS[f]
    # without frames: the same numbers, and nothing else moves
    nf = model.trace(x, TT, frames=False, vitals=True, **kw)
    assert nf.frames is None and P.same_bytes(nf.vitals.stacked, tr.vitals.stacked)
    assert torch.equal(nf.x_final, base.x_final)
    # a number overrides the model's threshold
    ov = model.trace(x, TT, frames=False, vitals=0.3, **kw)
    assert P.same_bytes(ov.vitals.stacked, _vitals(tr.frames, 0.3).stacked)
    assert not torch.equal(ov.vitals.mature, tr.vitals.mature)
    # beside the metrics (and, on the graph model, the maps and the diagnostics): all bitwise unchanged
    extra = dict(return_attention=True, diagnostics=True) if kind == "graph" else {}
    full0 = model.trace(x, TT, channels=16, target=t, **extra, **kw)
    full1 = model.trace(x, TT, channels=16, target=t, vitals=True, **extra, **kw)
    _same_trace(full1, full0)
    assert P.same_bytes(full1.vitals.stacked, tr.vitals.stacked)
    if kind == "graph":
        from graph_neural_cellular_automata_amd import _lib as L
        for n in L.DIAG_FIELDS:
            a, b = getattr(full1.diagnostics, n), getattr(full0.diagnostics, n)
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), n
        mt = model.trace(x, TT, frames=False, target=t, vitals=True, **kw)
        assert P.same_bytes(mt.metrics.stacked, full0.metrics.stacked)
        assert P.same_bytes(mt.vitals.stacked, tr.vitals.stacked) and mt.diagnostics is None


def test_regrow_trace_passes_vitals_through(dev):
    from graph_neural_cellular_automata_amd import DamagePolicy, regrow_trace
    g, _ = _models(dev)
    x = _state(dev)
    pol = DamagePolicy(dict(prob=1.0, start_epoch=0, kinds={"square": 1.0}, size_min=6, size_max=6), 3)
    rr = random.Random(17)
    offs = [rr.sample(g.graph.offsets, 8) for _ in range(TT)]
    tr = regrow_trace(g, x, TT, pol, 3, every=1, channels=16, vitals=True, fire_rate=FIRE, seed=SEED, offsets=offs)
    assert tr.vitals.stacked.shape == (TT, TB, 13)
    assert P.same_bytes(tr.vitals.stacked, _vitals(tr.frames, g.alpha_thr).stacked)


@pytest.mark.parametrize("kind", ["graph", "classic"])
def test_a_fresh_model_keeps_its_seed(dev, kind):
    """A freshly constructed model has W2 = 0: the state does not move (on the graph model with the
    message switched off: its projection's bias alone would move every cell), and the vitals say so."""
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    model = (NeuralCAGraph(16) if kind == "graph" else NeuralCA(16)).to(dev).eval()
    assert float(model.update_net[2].weight.detach().abs().max()) == 0.0
    kw = dict(message_gain=0.0) if kind == "graph" else {}
    H, W = 24, 20
    x = torch.zeros(2, 16, H, W, device=dev)
    x[:, 3:, H // 2, W // 2] = 1.0
    tr = model.trace(x, 4, every=1, frames=False, vitals=True, seed=1, **kw)
    assert torch.equal(tr.x_final, x)
    v = tr.vitals
    assert v.stacked.shape == (4, 2, 13)
    one = torch.ones(4, 2, dtype=torch.float64, device=dev)
    assert torch.equal(v.alive, 9 * one) and torch.equal(v.mature, one) and torch.equal(v.alpha_sum, one)
    assert torch.equal(v.mass, one)
    assert torch.equal(v.cy, (H // 2) * one) and torch.equal(v.cx, (W // 2) * one)
    assert torch.equal(v.y0, v.y1) and torch.equal(v.x0, v.x1)
    assert torch.equal(v.y0, (H // 2) * one) and torch.equal(v.x0, (W // 2) * one)
    assert torch.equal(v.max_abs, one) and torch.equal(v.nonfinite, 0 * one)
    rms = (1.0 / (H * W)) ** 0.5          # 12 hidden ones over 12 H W values
    assert float((v.hidden_rms - rms).abs().max()) <= float(np.spacing(rms))
