"""CPU emulation of the bf16-split K1's arithmetic (gnca_k1_split.h, gnca_k1_split32.h) and the
inputs of the K1 precision tests — TEST INFRASTRUCTURE ONLY, numpy only.

The split K1s write every fp32 operand as three bf16 parts, v = v0 + v1 + v2 exactly, and keep six of
the nine part products of each fp32 product: a0b0, a0b1, a1b0, a0b2, a2b0, a1b1 (a = the weight, b =
the activation, in both GEMMs).  This module restates that scheme with exact products and fp32
accumulation, with the list of kept terms as an argument, so that a CPU test can show that the GPU
tests' inputs tell the six-term scheme from every five-term one (tests/test_split_emul_cpu.py).  No
mutated kernel exists anywhere: the mutants are term lists of this emulator.

It also builds the inputs shared by the CPU and the GPU tests (tests/test_gpu_k1_precision.py):

* the term selectors: integer-valued operands for which every kept product and every partial sum is
  an integer below 2^23 (``LIMIT``), so that any correct fp32-class GEMM returns the exact integer in
  any summation order, and exactly one group of part products carries the low bits;
* the error-budget inputs: realistic full-mantissa operands;
* the message-GEMM inputs: rows built from chosen parts.
"""
from __future__ import annotations

import numpy as np

from oracle import nca_oracle as O

U = 2.0 ** -24                      # the unit roundoff of fp32
ALPHA_THR = 0.1
# (i, j): part i of the weight times part j of the activation
TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))      # what the kernels keep
DROPPED = ((1, 2), (2, 1), (2, 2))                            # each <= 2^-24 |a||b|
SECOND, THIRD = ((0, 1), (1, 0)), ((0, 2), (2, 0), (1, 1))


def without(term, terms=TERMS):
    """The term list of the mutant that drops ``term``."""
    assert term in terms
    return tuple(t for t in terms if t != term)


# ---------------------------------------------------------------------------------------------
# The split
# ---------------------------------------------------------------------------------------------
def bf16_rne(v) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even) as an fp32 array; NaN stays NaN (v_cvt_pk_bf16_f32)."""
    v = np.asarray(v, np.float32)
    u = np.ascontiguousarray(v).reshape(-1).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    out = r.view(np.float32).reshape(v.shape)
    return np.where(np.isnan(v), v, out)


def split3(v):
    """split3_pair of gnca_k1_split.h: v0 = rne(v), v1 = rne(v - v0), v2 = rne(v - v0 - v1), all
    differences in fp32."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v0 = bf16_rne(v)
        r1 = v - v0
        v1 = bf16_rne(r1)
        v2 = bf16_rne(r1 - v1)
    return v0, v1, v2


def from_parts(v0, v1, v2) -> np.ndarray:
    """The fp32 values v0 + v1 + v2 of chosen bf16 parts; asserts that the sum is an fp32 value and
    that ``split3`` gives exactly these parts back."""
    parts = [np.asarray(p, np.float32) for p in np.broadcast_arrays(v0, v1, v2)]
    s = parts[0].astype(np.float64) + parts[1].astype(np.float64) + parts[2].astype(np.float64)
    v = s.astype(np.float32)
    assert (v.astype(np.float64) == s).all(), "the parts' sum is not an fp32 value"
    for got, want, name in zip(split3(v), parts, ("v0", "v1", "v2")):
        assert (got == want).all(), f"split3 does not give the chosen {name} back"
    return v


def n_parts(v) -> np.ndarray:
    """How many of the three parts are nonzero (1: bf16-exact)."""
    return sum((p != 0).astype(np.int32) for p in split3(v))


# ---------------------------------------------------------------------------------------------
# The GEMM
# ---------------------------------------------------------------------------------------------
def gemm_split(A, B, terms=TERMS, bias=None, chunk: int = 16) -> np.ndarray:
    """A[M,K] . B[K,N] (+ bias[M]) as the split kernels compute it: both operands split in three,
    for every ``chunk``-wide k slice (one MFMA) and every term (i, j) — or (i, j, scale) — of
    ``terms`` the exact sum of the slice's A_i B_j products (bf16 x bf16 is exact; summed in f64),
    added to an fp32 accumulator that starts at the fp32 bias."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    (M, K), N = A.shape, B.shape[1]
    Ap = [p.astype(np.float64) for p in split3(A)]
    Bp = [p.astype(np.float64) for p in split3(B)]
    acc = np.zeros((M, N), np.float32)
    if bias is not None:
        acc += np.asarray(bias, np.float32)[:, None]
    for k0 in range(0, K, chunk):
        for t in terms:
            i, j, scale = (*t, 1.0)[:3]
            prod = (Ap[i][:, k0:k0 + chunk] * scale) @ Bp[j][k0:k0 + chunk]
            acc = (acc.astype(np.float64) + prod).astype(np.float32)
    return acc


def _rows(z):     # [B,Cin,H,W] -> [Cin, B*H*W]
    return z.transpose(1, 0, 2, 3).reshape(z.shape[1], -1)


def _unrows(m, B, H, W):
    return m.reshape(m.shape[0], B, H, W).transpose(1, 0, 2, 3)


def emul_dl(x, W1, b1, W2, terms1=TERMS, terms2=TERMS) -> np.ndarray:
    """K1's update field before the message and the masks, D = W2 relu(W1 Y + b1), on the emulated
    scheme; the perception Y in fp32."""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    y = O.perceive(x, O.sobel_weights(C, np.float32))
    h = np.maximum(gemm_split(W1, _rows(y), terms1, b1), 0)
    return _unrows(gemm_split(W2, h, terms2), B, H, W)


def emul_message(x_shifted, WM, terms=TERMS) -> np.ndarray:
    """The message GEMM M = WM G of gathered states G (= ``x_shifted``, [B,C,H,W])."""
    B, C, H, W = x_shifted.shape
    return _unrows(gemm_split(WM, _rows(np.asarray(x_shifted, np.float32)), terms), B, H, W)


# ---------------------------------------------------------------------------------------------
# The float64 oracle's pieces (oracle/nca_oracle.py's _update, before tanh)
# ---------------------------------------------------------------------------------------------
def dl64(x, W1, b1, W2, y64=None) -> np.ndarray:
    """W2 relu(W1 perceive(x) + b1) in float64 (nca_oracle._update's first three lines)."""
    x = np.asarray(x, np.float64)
    if y64 is None:
        y64 = O.perceive(x, O.sobel_weights(x.shape[1], np.float64))
    h = np.maximum(O.conv1x1(y64, np.asarray(W1, np.float64), np.asarray(b1, np.float64)), 0)
    return O.conv1x1(h, np.asarray(W2, np.float64), None)


def live_mask(x, thr: float = ALPHA_THR) -> np.ndarray:
    """[B,1,H,W] bool: the pre-update alive mask."""
    return O.alive_mask(np.asarray(x, np.float64), thr) != 0


def bound(x, W1, b1, W2) -> np.ndarray:
    """|W2| (|W1| yhat + |b1|) with yhat = |K_sobel| (*) |x|: the magnitude every rounding of the
    perception, of GEMM1 and of GEMM2 is relative to."""
    x = np.abs(np.asarray(x, np.float64))
    yh = O.perceive(x, np.abs(O.sobel_weights(x.shape[1], np.float64)))
    hb = O.conv1x1(yh, np.abs(np.asarray(W1, np.float64)), np.abs(np.asarray(b1, np.float64)))
    return O.conv1x1(hb, np.abs(np.asarray(W2, np.float64)), None)


def norm_err(d, d64, bnd, live):
    """(rms, max) over the live cells of e = |d - d64| / (u bound)."""
    m = np.broadcast_to(live, d64.shape)
    e = np.abs(np.asarray(d, np.float64) - d64)[m] / (U * bnd[m])
    return float(np.sqrt(np.mean(e * e))), float(e.max())


# ---------------------------------------------------------------------------------------------
# The K1 instantiations under test (kVariants of gnca_step.hip) and the smallest shapes that plan them
# ---------------------------------------------------------------------------------------------
# id -> (expected kernel, arithmetic, C, hidden, H, W, B, distinct samples nb, offsets k, zero-padded shift).
# B > nb: the batch repeats nb distinct samples (samples are independent); the large batch is what makes
# the planner take the 24x24 tile (at least two tiles per CU before it prefers a variant with more tiles).
VARIANTS = {
    "g24x36": ("gnca_k1_split<24,36,4,4,8>", "bf16x6", 16, 128, 48, 36, 2, 2, 8, False),
    "g36x24": ("gnca_k1_split<36,24,4,4,8>", "bf16x6", 16, 128, 36, 48, 2, 2, 8, False),
    "g24x24": ("gnca_k1_split<24,24,4,4,8>", "bf16x6", 16, 128, 24, 24, 640, 4, 8, False),
    "g8x24": ("gnca_k1_split<8,24,4,4,8>", "bf16x6", 16, 128, 16, 48, 4, 4, 8, False),
    "c24x36": ("gnca_k1_split<24,36,1,4,0>", "bf16x6", 16, 128, 48, 36, 2, 2, 0, False),
    "c8x24": ("gnca_k1_split<8,24,1,4,0>", "bf16x6", 16, 128, 16, 48, 4, 4, 0, False),
    "g8x20": ("gnca_k1_split<8,20,4,4,8>", "bf16x6", 16, 128, 16, 40, 5, 5, 8, False),
    "c8x20": ("gnca_k1_split<8,20,1,4,0>", "bf16x6", 16, 128, 16, 40, 5, 5, 0, False),
    "g24x36zp": ("gnca_k1_split<24,36,4,4,8>", "bf16x6", 16, 128, 48, 36, 2, 2, 8, True),
    "g36x24zp": ("gnca_k1_split<36,24,4,4,8>", "bf16x6", 16, 128, 36, 48, 2, 2, 8, True),
    "g24x24zp": ("gnca_k1_split<24,24,4,4,8>", "bf16x6", 16, 128, 24, 24, 640, 4, 8, True),
    "g8x24zp": ("gnca_k1_split<8,24,4,4,8>", "bf16x6", 16, 128, 16, 48, 4, 4, 8, True),
    "g8x20zp": ("gnca_k1_split<8,20,4,4,8>", "bf16x6", 16, 128, 16, 40, 5, 5, 8, True),
    "g32": ("gnca_k1_split32<16,16,5,8,16>", "bf16x6", 32, 128, 32, 32, 3, 3, 16, False),
    "c32": ("gnca_k1_split32<16,16,1,4,0>", "bf16x6", 32, 128, 32, 32, 3, 3, 0, False),
    # the control: a generic fp32-MFMA shape (odd canvas, more than one tile)
    "f32_16x64": ("gnca_k1_update<16,64,0,0,0,0,0,256>", "f32", 16, 64, 13, 38, 6, 6, 0, False),
}


def variant_offsets(vid: str):
    """The step's offsets: k distinct ones within the variant's radius (seeded)."""
    _, _, C, _, _, _, _, _, k, _ = VARIANTS[vid]
    if k == 0:
        return []
    table = O.build_offsets(4 if C == 16 else 5)
    idx = np.random.default_rng(41).permutation(len(table))[:k]
    return [table[i] for i in sorted(idx)]


# ---------------------------------------------------------------------------------------------
# Term selectors
# ---------------------------------------------------------------------------------------------
# kind -> (which GEMM carries the low bits, the part products that carry them)
SELECTORS = {
    "g1_w": (1, ((1, 0), (2, 0))),    # W1 3-part, y bf16-exact
    "g1_y": (1, ((0, 1), (0, 2))),    # y 3-part, W1 bf16-exact
    "g1_11": (1, ((1, 1),)),          # W1 and y 2-part
    "g2_h": (2, ((0, 1), (0, 2))),    # h 3-part (~2^21), W2 +-1
    "g2_w": (2, ((1, 0), (2, 0))),    # W2 3-part (the halved third image), h <= 14
    "g2_11": (2, ((1, 1),)),          # W2 and h 2-part
}
_NZ2 = {"g2_h": 3, "g2_w": 2, "g2_11": 4}    # nonzeros per W2 row of the GEMM2 kinds
# Sums of |part products| stay below 2^23, one bit under fp32's 2^24 integers: the lean group body stores
# the third W2 image halved ([P2/2; P2/2] in both accumulator halves, gnca_k1_split.h), so its products
# are multiples of 1/2, and a partial sum of such values is exact only below 2^23.  (At 2^23 <= |dl| an
# odd P2.H0 rounds once in a half: measured, one value of the first version of these inputs; an error
# of u |dl|, inside the fp32 class, but not bitwise.)
LIMIT = 2.0 ** 23


def _int3(rng, shape):
    """3-part integers below 2^18: a 2^10 +- r with an 8-bit a and an odd 9-bit r (v0 = a 2^10, v1 =
    the even neighbour of r, v2 = +-1)."""
    a = rng.integers(128, 256, shape)
    r = 2 * rng.integers(128, 256, shape) + 1
    return (a * 1024 + np.where(rng.integers(0, 2, shape) == 1, r, -r)).astype(np.float64)


def _int2(rng, shape):
    """2-part integers: odd, 9 bits (257..511)."""
    return (2 * rng.integers(128, 256, shape) + 1).astype(np.float64)


def _sign(rng, shape):
    return np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0)


def selector_state(kind: str, C: int, H: int, W: int, B: int, seed: int = 0) -> np.ndarray:
    """Integer states: every hidden / RGB value is s m with s in {-1, 0, 1} and m = 1 (bf16-exact
    perception), a 3-part integer (g1_y) or a 2-part one (g1_11), so that the Sobel sums (at most 8
    times the largest value) are exact integers; alpha is one positive m above the threshold, zero in
    a block that leaves dead cells."""
    rng = np.random.default_rng([seed, 1])
    shape = (B, C, H, W)
    mag = _int3(rng, shape) if kind == "g1_y" else _int2(rng, shape) if kind == "g1_11" else np.ones(shape)
    x = rng.integers(-1, 2, shape) * mag
    x[:, 3] = mag[:, 3]
    x[:, 3, 1:min(7, H - 1), 2:min(9, W - 1)] = 0
    return x.astype(np.float32)


def selector_rounds(kind: str, C: int, HD: int) -> int:
    """Weight patterns per case: over the rounds every slot (row, k) of the targeted weight matrix is
    nonzero at least once while its row is observed, so no single misplaced slot of an A image
    escapes (all k-chunks, both lane halves and every row block included)."""
    if SELECTORS[kind][0] == 1:
        return C * (HD // (2 * C))
    return -(-HD // _NZ2[kind])


def selector_weights(kind: str, C: int, HD: int, rnd: int, seed: int = 0):
    """(W1 [HD,3C], b1 [HD], W2 [C,HD]) of round ``rnd``: sparse integer rows.

    GEMM1 kinds: W1 has 3 nonzeros per row (one per feature block, the channel rotating with the
    round); W2 is a +-1 carrier with 2 nonzeros per row that observes 2C hidden rows per round.
    GEMM2 kinds: W1 is a +-1 carrier and the integer b1 sets the size of h; W2 has 2-4 nonzeros per
    row, rotating with the round.  Sums of |products| stay below ``LIMIT`` (``selector_check``)."""
    rng = np.random.default_rng([seed, 2, rnd, sorted(SELECTORS).index(kind)])
    g, _ = SELECTORS[kind]
    K1 = 3 * C
    W1 = np.zeros((HD, K1))
    W2 = np.zeros((C, HD))
    rows = np.arange(HD)
    nz1 = 1 if kind == "g2_w" else 3
    v1 = {"g1_w": _int3(rng, (HD, 3)) * _sign(rng, (HD, 3)), "g1_11": _int2(rng, (HD, 3)) * _sign(rng, (HD, 3))
          }.get(kind, _sign(rng, (HD, 3)))
    for f in range(nz1):
        W1[rows, ((f + rnd) % 3 if nz1 == 1 else f) * C + (rows * 5 + rnd) % C] = v1[:, f]
    if g == 1:
        b1 = rng.integers(-4, 5, HD).astype(np.float64)
        phase = rnd // C
        for c in range(C):
            for t in range(2):
                W2[c, c + C * (2 * phase + t)] = _sign(rng, ())
    else:
        if kind == "g2_h":
            b1 = 2.0 * rng.integers(2 ** 19, 2 ** 20 - 64, HD) + 1
        elif kind == "g2_w":
            b1 = rng.integers(0, 7, HD).astype(np.float64)
        else:
            b1 = 2.0 * rng.integers(129, 1010, HD) + 1
        nz2 = _NZ2[kind]
        R = selector_rounds(kind, C, HD)
        v2 = {"g2_w": _int3(rng, (C, nz2)) * _sign(rng, (C, nz2)), "g2_11": _int2(rng, (C, nz2)) * _sign(rng, (C, nz2))
              }.get(kind, _sign(rng, (C, nz2)))
        for c in range(C):
            for t in range(nz2):
                W2[c, (3 * c + rnd + t * R) % HD] = v2[c, t]
    return W1.astype(np.float32), b1.astype(np.float32), W2.astype(np.float32)


def _abs_parts(v):
    return sum(np.abs(p.astype(np.float64)) for p in split3(v))


def selector_check(x, W1, b1, W2, y64=None) -> float:
    """The largest sum of |part products| (+ |b1|) any accumulator of either GEMM can see, which must
    stay below ``LIMIT`` for the result to be exact in every summation order; also asserts that all
    operands are integers."""
    x = np.asarray(x, np.float64)
    for a in (x, W1, b1, W2):
        assert (np.asarray(a, np.float64) % 1 == 0).all()
    if y64 is None:
        y64 = O.perceive(x, O.sobel_weights(x.shape[1], np.float64))
    y32 = y64.astype(np.float32)
    assert (y32 == y64).all()
    h_abs = O.conv1x1(_abs_parts(y32), _abs_parts(W1), np.abs(np.asarray(b1, np.float64)))
    h = np.maximum(O.conv1x1(y64, np.asarray(W1, np.float64), np.asarray(b1, np.float64)), 0).astype(np.float32)
    d_abs = O.conv1x1(_abs_parts(h), _abs_parts(W2), None)
    return float(max(h_abs.max(), d_abs.max()))


# ---------------------------------------------------------------------------------------------
# Error budget
# ---------------------------------------------------------------------------------------------
def budget_inputs(C: int, HD: int, H: int, W: int, B: int, seed: int = 0):
    """(x, W1, b1, W2), fp32 with full mantissas: RGB and alpha ~ U(0,1), hidden ~ N(0,1) 2^e per channel
    with e in [-3, 3]; W1, W2 ~ N(0, 0.3), b1 ~ N(0, 0.2)."""
    rng = np.random.default_rng([seed, 3, C, HD, H, W])
    x = rng.random((B, C, H, W))
    e = rng.integers(-3, 4, C - 4)
    x[:, 4:] = rng.standard_normal((B, C - 4, H, W)) * (2.0 ** e)[None, :, None, None]
    W1 = rng.standard_normal((HD, 3 * C)) * 0.3
    b1 = rng.standard_normal(HD) * 0.2
    W2 = rng.standard_normal((C, HD)) * 0.3
    return tuple(a.astype(np.float32) for a in (x, W1, b1, W2))


# ---------------------------------------------------------------------------------------------
# Message GEMM
# ---------------------------------------------------------------------------------------------
MESSAGE_OFFSET = (-2, 3)
# role -> the third-order part product the inputs load with >= 1e-4 of one sign
MESSAGE_ROLES = {"wm": (2, 0), "g": (0, 2), "a1b1": (1, 1)}


def message_inputs(role: str, C: int, H: int, W: int, B: int, seed: int = 0):
    """(x [B,C,H,W], wm [C,C]) built from parts (``from_parts``).

    Channels come in pairs (2i, 2i+1) whose states share the leading parts and whose weights have
    opposite signs with leading parts 2^-6 (64 / C) apart: the first- and second-order products
    alternate in sign and leave m = sum_k wm[c][k] g[k] near 0.4 - 0.5 for every row and cell, while
    the targeted third-order products (wm2 g0, wm0 g2 or wm1 g1) are positive for every k and sum to
    more than 1e-4.  |wm| in [3, 4), g in [0.625, 1).  States have at most 20 significant bits, so the
    gather's sum over the k <= 16 copies of the one offset and its 1/k weight are exact."""
    rng = np.random.default_rng([seed, 4, C, sorted(MESSAGE_ROLES).index(role)])
    P = C // 2
    two = lambda a: np.repeat(a, 2, axis=-1)
    # weights: rows c, pairs i
    a0 = rng.integers(192 + 8, 256, (C, P)) * 2.0 ** -6                      # [3.125, 4)
    d0 = (64 // C) * 2.0 ** -6
    w0 = np.stack([a0, -(a0 - d0)], -1).reshape(C, C)
    sgn_w = np.sign(w0)
    # states: cells, pairs i (channel-last here)
    g0 = two(rng.integers(160, 256, (B, H, W, P)) * 2.0 ** -8)               # [0.625, 1)
    zero_w, zero_g = np.zeros((C, C)), np.zeros((B, H, W, C))
    if role == "wm":      # wm = (w0, +-w1 cancelling in pairs, +w2); g bf16-exact
        w1 = two(_sign(rng, (C, P)) * rng.integers(129, 256, (C, P)) * 2.0 ** -15) * sgn_w
        w2 = rng.integers(48, 64, (C, C)) * 2.0 ** -22
        wm, g = from_parts(w0, w1, w2), from_parts(g0, zero_g, zero_g)
    elif role == "g":     # wm bf16-exact; g = (g0, g1 shared by the pair, g2 with the weight's sign)
        g1 = two(_sign(rng, (B, H, W, P)) * rng.integers(129, 256, (B, H, W, P)) * 2.0 ** -17)
        g2 = np.full((B, H, W, C), 3 * 2.0 ** -20) * np.tile([1.0, -1.0], P)
        wm, g = from_parts(w0, zero_w, zero_w), from_parts(g0, g1, g2)
    else:                 # both 2-part, wm1 g1 > 0 for every k
        w1 = rng.integers(192, 256, (C, C)) * 2.0 ** -15 * sgn_w
        g1 = rng.integers(192, 256, (B, H, W, C)) * 2.0 ** -17 * np.tile([1.0, -1.0], P)
        wm, g = from_parts(w0, w1, zero_w), from_parts(g0, g1, zero_g)
    return np.ascontiguousarray(g.transpose(0, 3, 1, 2)), wm


def message_shift(x, zero_pad: bool, offset=MESSAGE_OFFSET):
    """The gathered state of the one offset (the oracle's shift)."""
    return (O.shift_pad if zero_pad else O.shift_roll)(x, *offset)
