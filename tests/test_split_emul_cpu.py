"""CPU test of the K1 precision tests (tests/test_gpu_k1_precision.py): on the inputs the GPU tests use,
the emulated six-term scheme (tests/split_emul.py) passes what they assert and every five-term mutant
fails it.  The mutants are term lists of the emulator; no mutated kernel exists."""
import numpy as np
import pytest

from oracle import nca_oracle as O
from tests import split_emul as E
from tests.k1_probe import torch_ref_dl32

BOTH = [(g, t) for g in (1, 2) for t in E.TERMS[1:]]


def _terms(gemm, g, terms):
    return terms if gemm == g else E.TERMS


# ---------------------------------------------------------------------------------------------
# The split is exact
# ---------------------------------------------------------------------------------------------
def _split_inputs():
    rng = np.random.default_rng(7)
    n = 1 << 16
    mant = rng.integers(0, 1 << 23, n).astype(np.uint32)
    expo = rng.integers(127 - 90, 127 + 91, n).astype(np.uint32)
    sign = rng.integers(0, 2, n).astype(np.uint32)
    rand = ((sign << 31) | (expo << 23) | mant).view(np.float32)
    # residuals of either sign at every level: v0 rounds up / down, v1 rounds up / down
    m = np.array([0x7F8001, 0x007FFF, 0x008001, 0x7F7FFF, 0x00807F, 0x008081, 0x7FFFFF, 0x000001, 0x008000,
                  0x018000, 0x000080, 0x000180], np.uint32)
    e = np.arange(127 - 90, 127 + 91, dtype=np.uint32)
    edge = ((e[:, None] << 23) | m[None, :]).reshape(-1).view(np.float32)
    exact = E.bf16_rne(rand[:4096])
    special = np.array([1 + 2.0 ** -23, -(1 + 2.0 ** -23), 1.0, 0.0, 2.0 ** -90, 2.0 ** 90, -(2.0 ** 90) * (2 - 2.0 ** -23)],
                       np.float32)
    return np.concatenate([rand, edge, -edge, exact, special])


def test_split3_is_exact():
    v = _split_inputs()
    assert (np.abs(v[v != 0]) >= 2.0 ** -90).all() and (np.abs(v) < 2.0 ** 91).all()
    v0, v1, v2 = E.split3(v)
    for p in (v0, v1, v2):   # each part is a bf16 value
        assert (p.view(np.uint32) & np.uint32(0xFFFF) == 0).all()
    s = (v0.astype(np.float32) + v1) + v2     # fp32: every partial sum is exact
    np.testing.assert_array_equal(s.view(np.uint32), v.view(np.uint32))
    s64 = v0.astype(np.float64) + v1.astype(np.float64) + v2.astype(np.float64)
    assert (s64 == v.astype(np.float64)).all()
    # residuals of both signs at both levels, bf16-exact values and 1 + 2^-23 are all in there
    assert (v1 > 0).any() and (v1 < 0).any() and (v2 > 0).any() and (v2 < 0).any()
    assert ((v1 == 0) & (v2 == 0) & (v != 0)).sum() >= 4000
    one = E.split3(np.float32(1 + 2.0 ** -23))
    assert [float(p) for p in one] == [1.0, 2.0 ** -23, 0.0]   # the residual is a bf16 value: the second part


def test_bf16_rne_ties_to_even_and_keeps_nan():
    v = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, np.inf, -np.inf], np.float32)
    np.testing.assert_array_equal(E.bf16_rne(v), np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, np.inf, -np.inf], np.float32))
    assert np.isnan(E.bf16_rne(np.float32(np.nan)))


def test_from_parts_round_trips_and_rejects_overlapping_parts():
    v = E.from_parts(np.float32(3.5), np.float32(2.0 ** -8 * 1.5), np.float32(2.0 ** -17))
    assert float(v) == 3.5 + 1.5 * 2.0 ** -8 + 2.0 ** -17
    with pytest.raises(AssertionError):
        E.from_parts(np.float32(1.0), np.float32(2.0 ** -7), np.float32(0))    # v1 above half an ulp of v0
    with pytest.raises(AssertionError):
        E.from_parts(np.float32(1.0), np.float32(2.0 ** -10), np.float32(2.0 ** -30))   # not an fp32 value


def test_gemm_split_all_nine_terms_is_the_fp32_product():
    """With all nine part products the scheme is an exactly-multiplied GEMM: the test of the
    emulator's own bookkeeping."""
    rng = np.random.default_rng(1)
    A, B = rng.standard_normal((8, 16)).astype(np.float32), rng.standard_normal((16, 5)).astype(np.float32)
    got = E.gemm_split(A, B, E.TERMS + E.DROPPED)
    # nine accumulator roundings, each at most u times the running sum's bound
    tol = 9 * E.U * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64))
    assert (np.abs(got - A.astype(np.float64) @ B.astype(np.float64)) <= tol).all()


# ---------------------------------------------------------------------------------------------
# Term selectors: exact under six terms, wrong under the mutant that drops a targeted term
# ---------------------------------------------------------------------------------------------
SHAPES = sorted({(v[2], v[3]) for v in E.VARIANTS.values()})   # (C, hidden)


@pytest.mark.parametrize("C,HD", SHAPES)
@pytest.mark.parametrize("kind", sorted(E.SELECTORS))
def test_selectors_discriminate(kind, C, HD):
    g, targeted = E.SELECTORS[kind]
    x = E.selector_state(kind, C, 10, 12, 1)
    y64 = O.perceive(x.astype(np.float64), O.sobel_weights(C, np.float64))
    live = E.live_mask(x)
    assert live.any() and not live.all()
    m = np.broadcast_to(live, x.shape)
    seen1, seen2 = np.zeros((HD, 3 * C), bool), np.zeros((C, HD), bool)
    R = E.selector_rounds(kind, C, HD)
    for rnd in range(R):
        W1, b1, W2 = E.selector_weights(kind, C, HD, rnd)
        assert E.selector_check(x, W1, b1, W2, y64) < E.LIMIT
        exact = E.dl64(x, W1, b1, W2, y64)
        assert (exact % 1 == 0).all() and np.abs(exact).max() < E.LIMIT
        # no kept or dropped product is lost: six terms and nine terms give the exact integer
        assert (E.emul_dl(x, W1, b1, W2) == exact).all(), (kind, rnd)
        for t in targeted:
            mut = E.emul_dl(x, W1, b1, W2, _terms(g, 1, E.without(t)), _terms(g, 2, E.without(t)))
            frac = float((mut != exact)[m].mean())
            assert frac > 0.02, (kind, rnd, t, frac)
        # the third W2 image stored halved without its compensation (gnca_k1_split.h: [P2/2; P2/2])
        if kind == "g2_w":
            half = tuple((i, j, 0.5) if (i, j) == (2, 0) else (i, j) for i, j in E.TERMS)
            assert ((E.emul_dl(x, W1, b1, W2, E.TERMS, half) != exact)[m]).mean() > 0.02
        # the hidden rows the output observes this round, and the weight slots that are live in them
        obs = (W2 != 0).any(axis=0)
        seen1 |= (W1 != 0) & obs[:, None]
        seen2 |= W2 != 0
    if g == 1:
        assert seen1.all(), "every (row, k) slot of W1 is nonzero and observed in some round"
    else:
        assert seen2.all(), "every (row, k) slot of W2 is nonzero in some round"


def test_selector_operands_have_the_parts_they_claim():
    C, HD = 16, 128
    for kind in sorted(E.SELECTORS):
        x = E.selector_state(kind, C, 10, 12, 1)
        W1, b1, W2 = E.selector_weights(kind, C, HD, 0)
        y = O.perceive(x, O.sobel_weights(C, np.float32))
        h = np.maximum(O.conv1x1(y.astype(np.float64), W1.astype(np.float64), b1.astype(np.float64)), 0).astype(np.float32)
        parts = {n: E.n_parts(a[a != 0]) for n, a in dict(W1=W1, y=y, h=h, W2=W2).items()}
        want = {"g1_w": dict(W1=3, y=1), "g1_y": dict(W1=1, y=3), "g1_11": dict(W1=2, y=2),
                "g2_h": dict(W2=1, h=3), "g2_w": dict(W2=3, h=1), "g2_11": dict(W2=2, h=2)}[kind]
        for n, k in want.items():
            assert parts[n].max() == k, (kind, n)
            assert (parts[n] == k).mean() > 0.5, (kind, n, float((parts[n] == k).mean()))


# ---------------------------------------------------------------------------------------------
# Error budget: six terms within 2x the fp32 reference, every five-term mutant at least 8x
# ---------------------------------------------------------------------------------------------
BUDGET_SHAPES = sorted({v[2:6] + (v[7],) for v in E.VARIANTS.values() if v[1] == "bf16x6"})


@pytest.mark.parametrize("C,HD,H,W,nb", BUDGET_SHAPES)
def test_budget_separates_six_terms_from_five(C, HD, H, W, nb):
    x, W1, b1, W2 = E.budget_inputs(C, HD, H, W, nb)
    d64, bnd, live = E.dl64(x, W1, b1, W2), E.bound(x, W1, b1, W2), E.live_mask(x)
    ref_rms, ref_max = E.norm_err(torch_ref_dl32(x, W1, b1, W2), d64, bnd, live)
    six_rms, six_max = E.norm_err(E.emul_dl(x, W1, b1, W2), d64, bnd, live)
    print(f"[budget] {C}ch {H}x{W} x{nb}: fp32 ref rms {ref_rms:.4f} max {ref_max:.3f}; six terms rms {six_rms:.4f} "
          f"max {six_max:.3f}")
    assert six_rms <= 2 * ref_rms, (six_rms, ref_rms)
    weakest = np.inf
    for g, t in BOTH:
        rms, mx = E.norm_err(E.emul_dl(x, W1, b1, W2, _terms(g, 1, E.without(t)), _terms(g, 2, E.without(t))),
                             d64, bnd, live)
        print(f"[budget]   GEMM{g} without a{t[0]}b{t[1]}: rms {rms:.3f} ({rms / ref_rms:.1f}x ref) max {mx:.2f}")
        assert rms >= 8 * ref_rms, (g, t, rms, ref_rms)
        weakest = min(weakest, rms / ref_rms)
    # the GPU test's factor 4 stays under half the weakest mutant
    assert 4 <= weakest / 2, weakest


# ---------------------------------------------------------------------------------------------
# Message GEMM: third-order mutants miss tanh(m) by more than 1e-5
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zp", [False, True])
@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("role", sorted(E.MESSAGE_ROLES))
def test_message_inputs_discriminate(role, C, zp):
    x, wm = E.message_inputs(role, C, 12, 14, 1)
    assert E.live_mask(x).all()
    g = E.message_shift(x, zp)
    rows = (np.abs(g).sum(axis=(1, 3)) != 0)[0]          # zero-padded shift: the rows shifted in from outside are 0
    assert rows.sum() >= 10
    g = g[:, :, rows]
    # the gather is exact: k copies of the one offset summed in fp32, then the 1/k weight
    for k in (8, 16):
        acc = np.zeros_like(g)
        for _ in range(k):
            acc = acc + g
        assert ((acc * np.float32(1.0 / k)) == g).all()
    m64 = np.einsum("ck,bkhw->bchw", wm.astype(np.float64), g.astype(np.float64))
    assert 0.2 < m64.min() and m64.max() < 0.9, (m64.min(), m64.max())
    i, j = E.MESSAGE_ROLES[role]
    parts_w = [p.astype(np.float64) for p in E.split3(wm)]
    parts_g = [p.astype(np.float64) for p in E.split3(g)]
    third = parts_w[i][None, :, :, None, None] * parts_g[j][:, None]           # [b,c,k,h,w]
    assert (third >= 0).all() and third.sum(axis=2).min() >= 1e-4
    six = np.abs(np.tanh(E.emul_message(g, wm).astype(np.float64)) - np.tanh(m64)).max()
    assert six <= 1.5e-7, six
    mut = np.abs(np.tanh(E.emul_message(g, wm, E.without((i, j))).astype(np.float64)) - np.tanh(m64))
    print(f"[message] {role} C={C} zp={zp}: six terms {six:.2e}, without a{i}b{j}: min {mut.min():.2e}")
    assert mut.min() > 1e-5, mut.min()
    # the other third-order products carry nothing here: each role pins its own
    for t in E.THIRD:
        if t != (i, j):
            assert np.abs(parts_w[t[0]][None, :, :, None, None] * parts_g[t[1]][:, None]).sum(axis=2).max() < 1e-6
