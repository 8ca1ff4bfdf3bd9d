"""Deterministic states and fire masks that give the alive masks STRUCTURE, and the case tables
of tests/test_liveness_cases_cpu.py and tests/test_gpu_liveness.py (test infrastructure only).

Every seeded random state of the other tests has alpha ~ U(0,1): after the 3x3 max-pool a cell is
dead with probability ~0.12^9, so the pre-update alive mask, the sender mask and the keep mask
(alive AND fire) are all ones up to the fire draw.  The patterns here write the alpha plane on
purpose: a dead background with alpha in [0, thr/2] and *seeds*, single cells with alpha in
[2 thr, 1], whose clipped 3x3 dilation is the alive set.

``build(pattern, seed, B, C, H, W, thr, tile, band)`` returns a ``Case``:

* ``x``      float32 [n,C,H,W]: RGB ~ U(0,1), hidden channels ~ N(0,1), alpha from the pattern;
* ``fire``   uint8 [n,1,H,W] (an explicit GNCA_FIRE_MASK_U8 mask) or None;
* ``seeds``  bool [n,H,W], the seed cells;
* ``exact``  bool [n,H,W], the cells of ``exact_thr`` placed at float32(thr) or one ulp above
  that the step leaves untouched (dead, or not firing): the cells ``min_margin`` leaves out.

Every sample is generated from its own stream keyed by (seed, pattern, sample index, shape), so
``samples=[...]`` builds a few samples of a large batch (n = len(samples)) exactly as the whole
batch (n = B) holds them.  The masks the tests assert on come from the oracle
(``oracle.nca_oracle.alive_mask``) alone.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import nca_oracle as O

PATTERNS = ("isolated", "border_ring", "half_dead", "stripes", "sparse", "counts", "counts_rollout",
            "exact_thr")
COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, -1, -2)   # -1: TH*TW - 1, -2: TH*TW
BANDS = (4, 6)                                     # K2 band heights (make_plan: dense ~4, compact 6)


@dataclass
class Case:
    pattern: str
    x: np.ndarray
    fire: np.ndarray | None
    seeds: np.ndarray
    exact: np.ndarray
    thr: float
    tile: tuple
    info: dict = field(default_factory=dict)


def dilate(m: np.ndarray) -> np.ndarray:
    """Clipped 3x3 dilation of a bool [...,H,W] mask: shifted ORs, nothing wraps."""
    H, W = m.shape[-2:]
    p = np.zeros(m.shape[:-2] + (H + 2, W + 2), bool)
    p[..., 1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for di in range(3):
        for dj in range(3):
            out |= p[..., di:di + H, dj:dj + W]
    return out


def pooled(a: np.ndarray) -> np.ndarray:
    """3x3 max-pool of alpha [...,H,W] with -inf padding (the quantity both masks threshold)."""
    H, W = a.shape[-2:]
    p = np.full(a.shape[:-2] + (H + 2, W + 2), -np.inf, a.dtype)
    p[..., 1:-1, 1:-1] = a
    out = np.full_like(a, -np.inf)
    for di in range(3):
        for dj in range(3):
            out = np.maximum(out, p[..., di:di + H, dj:dj + W])
    return out


def _isolated_candidates(H, W, tile, bands):
    """Corners, edge mid-points, both sides of every K1 tile boundary and tile corner, the first and
    last row of every K2 band, the interior."""
    TH, TW = tile
    c = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
         (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    rows = list(range(TH, H, TH))
    cols = list(range(TW, W, TW))
    for r in rows:                                  # tile corners: the four cells around each
        for q in cols:
            c += [(r - 1, q - 1), (r, q), (r - 1, q), (r, q - 1)]
    for r in rows:                                  # tile boundary rows, away from the corners
        for q in range(TW // 2, W, TW):
            c += [(r - 1, q), (r, q)]
    for q in cols:
        for r in range(TH // 2, H, TH):
            c += [(r, q - 1), (r, q)]
    for b in bands:                                 # K2 band edges
        for r in range(b, H, b):
            c += [(r - 1, (r * 7) % W), (r, (r * 11 + 3) % W)]
    c += [(H // 2, W // 2), (H // 3, W // 3), (2 * H // 3, W // 4)]
    return [(r, q) for r, q in c if 0 <= r < H and 0 <= q < W]


def _place_apart(cands, start, dist, limit=None):
    """Greedy subset of ``cands`` (rotated by ``start``) with Chebyshev distance >= ``dist``."""
    n = len(cands)
    got = []
    for i in range(n):
        r, q = cands[(start + i) % n]
        if all(max(abs(r - a), abs(q - b)) >= dist for a, b in got):
            got.append((int(r), int(q)))
            if limit and len(got) >= limit:
                break
    return got


ISOLATED_SLOTS = 8
_SLOTS: dict = {}


def isolated_slots(H, W, tile, bands):
    """The candidates of ``isolated`` dealt into ISOLATED_SLOTS seed sets, each with Chebyshev
    distance >= 4 between its seeds (a dead cell between any two blocks); sample b takes set
    (seed + b) mod ISOLATED_SLOTS, so eight consecutive samples hold every candidate."""
    key = (H, W, tuple(tile), tuple(bands))
    if key not in _SLOTS:
        slots = [[] for _ in range(ISOLATED_SLOTS)]
        for i, (r, q) in enumerate(dict.fromkeys(_isolated_candidates(H, W, tile, bands))):
            for k in range(ISOLATED_SLOTS):
                s = slots[(i + k) % ISOLATED_SLOTS]
                if all(max(abs(r - a), abs(q - b)) >= 4 for a, b in s):
                    s.append((r, q))
                    break
        _SLOTS[key] = slots
    return _SLOTS[key]


def border_sides(b: int) -> list:
    """The seeded sides of sample ``b`` of ``border_ring`` (0 top, 1 right, 2 bottom, 3 left): one
    side for the first four samples, two adjacent ones after."""
    return [b % 4] + ([(b + 1) % 4] if b % 8 >= 4 else [])


def _tiles(H, W, TH, TW):
    for ty in range(-(-H // TH)):
        for tx in range(-(-W // TW)):
            yield ty, tx, ty * TH, min(H, ty * TH + TH), tx * TW, min(W, tx * TW + TW)


def _sample(pattern, seed, b, C, H, W, thr, tile, band, seed_lo):
    g = np.random.default_rng([seed, PATTERNS.index(pattern), b, C, H, W])
    TH, TW = tile
    x = g.random((C, H, W), dtype=np.float32)
    if C > 4:
        x[4:] = g.standard_normal((C - 4, H, W), dtype=np.float32)
    athr = abs(thr)
    bg = g.random((H, W), dtype=np.float32) * np.float32(athr / 2)
    if thr < 0:                                      # negative threshold: a dead cell sits below it
        bg = np.float32(thr) - np.float32(3 * athr) - bg   # (well below: GroupNorm drifts dead cells)
    lo = 2 * athr if seed_lo is None else seed_lo
    sval = np.float32(lo) + g.random((H, W), dtype=np.float32) * np.float32(1 - lo)
    seeds = np.zeros((H, W), bool)
    exact = np.zeros((H, W), bool)
    fire = None
    info = {}
    tps = -(-H // TH) * -(-W // TW)

    if pattern == "isolated":
        for r, q in isolated_slots(H, W, tile, tuple(band))[(seed + b) % ISOLATED_SLOTS]:
            seeds[r, q] = True
    elif pattern == "border_ring":
        ph = (seed + b) % 3                          # every third border cell, phase-shifted
        for s in border_sides(b):
            if s == 0:
                seeds[0, ph::3] = True
            elif s == 1:
                seeds[ph::3, W - 1] = True
            elif s == 2:
                seeds[H - 1, ph::3] = True
            else:
                seeds[ph::3, 0] = True
    elif pattern == "half_dead":
        # alternate whole tiles alive / empty: by tile row (even b + seed) or tile column (odd), the
        # phase moving with the sample.  Seeds fill the tile but for its rim towards the neighbours,
        # which the dilation covers, so an empty tile stays exactly empty.
        by_col = (b + seed) % 2 == 1
        ph = ((b + seed) // 2) % 2
        for ty, tx, r0, r1, q0, q1 in _tiles(H, W, TH, TW):
            if ((tx if by_col else ty) + ph) % 2:
                continue
            if by_col:
                seeds[r0:r1, q0 + 1:q1 - 1] = True
            else:
                seeds[r0 + 1:r1 - 1, q0:q1] = True
        info["by_col"] = by_col
    elif pattern == "stripes":
        # seeds on every 4th row (even b + seed) or column (odd): alive 3, dead 1, phase-shifted
        ph = ((b + seed) // 2) % 4
        if (b + seed) % 2:
            seeds[:, ph::4] = True
        else:
            seeds[ph::4, :] = True
    elif pattern == "sparse":
        seeds = g.random((H, W)) < 0.03
    elif pattern == "counts":
        # alive everywhere; an explicit fire mask with the listed popcount per tile, in tile order
        # over the batch (reversed for odd seeds), the fired cells drawn at random inside the tile
        seeds[:] = True
        fire = np.zeros((1, H, W), np.uint8)
        order = COUNTS[::-1] if seed % 2 else COUNTS
        want = []
        for i, (ty, tx, r0, r1, q0, q1) in enumerate(_tiles(H, W, TH, TW)):
            n = (r1 - r0) * (q1 - q0)
            k = order[(b * tps + i + seed // 2) % len(order)]
            k = {-1: n - 1, -2: n}[k] if k < 0 else min(k, n)
            blk = np.zeros(n, np.uint8)
            blk[g.choice(n, size=k, replace=False)] = 1
            fire[0, r0:r1, q0:q1] = blk.reshape(r1 - r0, q1 - q0)
            want.append(k)
        info["want"] = want
    elif pattern == "counts_rollout":
        # FIRE_NONE rollouts: per tile nothing / one seed (9 cells) / a 2x6 block (4x8 = 32 cells) /
        # the whole tile, in tile order over the batch (reversed for odd seeds)
        assert H % TH == 0 and W % TW == 0 and TH >= 6 and TW >= 10
        kinds = (3, 2, 1, 0) if seed % 2 else (0, 1, 2, 3)
        want = []
        for i, (ty, tx, r0, r1, q0, q1) in enumerate(_tiles(H, W, TH, TW)):
            k = kinds[(b * (tps + 1) + i + seed // 2) % 4]
            if k == 1:
                seeds[r0 + 2, q0 + 2 + (i % 3)] = True
            elif k == 2:
                seeds[r0 + 2:r0 + 4, q0 + 2:q0 + 8] = True
            elif k == 3:
                seeds[r0 + 1:r1 - 1, q0 + 1:q1 - 1] = True
            want.append((0, 9, 32, TH * TW)[k])
        info["want"] = want
    elif pattern == "exact_thr":
        # a sparse state whose dead background also holds cells at float32(thr) ("eq": dead, and
        # zeroed by the post gate) and one ulp above ("ulp": alive), >= 4 dead cells away from any
        # seed and 6 from each other.  Half of the ulp cells sit in a 5x5 window where nothing
        # fires, so that the step (GroupNorm off) leaves their alpha alone and the POST gate sees
        # the ulp too ("quiet"); the others are updated like any alive cell (the PRE mask sees it).
        t32 = np.float32(thr)
        seeds = g.random((H, W)) < 0.02
        fire = (g.random((1, H, W)) <= 0.5).astype(np.uint8)
        eq, ulp, quiet = (np.zeros((H, W), bool) for _ in range(3))
        near = seeds
        for _ in range(4):
            near = dilate(near)
        free = np.argwhere(~near)
        placed = _place_apart(free[g.permutation(len(free))], 0, 6, limit=9)
        for j, (r, q) in enumerate(placed):
            if (j + b) % 3 == 0:
                eq[r, q] = True
            else:
                ulp[r, q] = True
                if (j + b) % 3 == 1:
                    quiet[r, q] = True
                    fire[0, max(0, r - 2):r + 3, max(0, q - 2):q + 3] = 0
                else:
                    fire[0, r, q] = 1                # updated for certain: its alpha moves away
        info.update(eq=eq, ulp=ulp, quiet=quiet)
        exact = eq | quiet

    a = np.where(seeds, sval, bg).astype(np.float32)
    if pattern == "exact_thr":
        a[info["eq"]] = np.float32(thr)
        a[info["ulp"]] = np.nextafter(np.float32(thr), np.float32(1))
    x[3] = a
    return x, fire, seeds, exact, info


def build(pattern: str, seed: int, B: int, C: int, H: int, W: int, thr: float, tile=(8, 24),
          band=BANDS, seed_lo: float | None = None, samples=None) -> Case:
    """``tile`` = (TH, TW) of the K1 the case is meant for, ``band`` the K2 band heights.
    ``seed_lo``: lower end of the seeds' alpha (default 2 |thr|); the two-threshold cases spread the
    seeds over [seed_lo, 1] so that the update's and the senders' masks differ.  ``samples``: build
    only these sample indices of the batch."""
    assert pattern in PATTERNS, pattern
    idx = list(range(B)) if samples is None else list(samples)
    parts = [_sample(pattern, seed, b, C, H, W, thr, tuple(tile), band, seed_lo) for b in idx]
    x = np.stack([p[0] for p in parts])
    fire = None if parts[0][1] is None else np.stack([p[1] for p in parts])
    info = {k: (np.stack([p[4][k] for p in parts]) if isinstance(parts[0][4][k], np.ndarray)
                else [p[4][k] for p in parts]) for k in parts[0][4]}
    info["samples"] = idx
    return Case(pattern, x, fire, np.stack([p[2] for p in parts]), np.stack([p[3] for p in parts]),
                float(thr), tuple(tile), info)


def expected_alive(case: Case) -> np.ndarray:
    """The alive set the pattern is built to give: the clipped 3x3 dilation of the seeds (and of
    the one-ulp cells of ``exact_thr``), written without a max-pool."""
    s = case.seeds | case.info["ulp"] if case.pattern == "exact_thr" else case.seeds
    return dilate(s)


def tile_live_counts(keep: np.ndarray, tile) -> np.ndarray:
    """Per-tile popcounts [n, tiles_y, tiles_x] of a keep mask [n,1,H,W] or [n,H,W] (ragged edge
    tiles count their cells inside the image)."""
    k = np.asarray(keep).reshape(keep.shape[0], keep.shape[-2], keep.shape[-1]) != 0
    B, H, W = k.shape
    TH, TW = tile
    ty, tx = -(-H // TH), -(-W // TW)
    p = np.zeros((B, ty * TH, tx * TW), np.int64)
    p[:, :H, :W] = k
    return p.reshape(B, ty, TH, tx, TW).sum(axis=(2, 4))


def keep_mask(x: np.ndarray, thr: float, fire: np.ndarray | None = None) -> np.ndarray:
    """[n,1,H,W] {0,1}: the oracle's pre-update alive mask AND the fire mask."""
    m = O.alive_mask(np.asarray(x, np.float64), thr)
    return m if fire is None else m * (np.asarray(fire) != 0)


def min_margin(xt: np.ndarray, thr: float, exact: np.ndarray | None = None) -> float:
    """min over cells of |3x3-pooled alpha of ``xt`` - float32(thr)|, where ``xt`` is the state the
    mask is taken of: a step's input, or ``oracle.nca_update``'s result (the updated state BEFORE
    the post gate, which is what the post-update mask thresholds).  Cells within the 3x3 window of
    a deliberately placed exact cell (``exact`` [n,H,W]) are left out: their pooled value IS the
    threshold or its successor, bit for bit, and no arithmetic touches it."""
    a = np.asarray(xt)[:, 3].astype(np.float64)
    d = np.abs(pooled(a) - np.float64(np.float32(thr)))
    if exact is not None and exact.any():
        d = np.where(dilate(exact), np.inf, d)
    return float(d.min())


# ---------------------------------------------------------------------------------------------
# Models: configuration dicts, numpy parameters (state_dict names), oracle configurations
# ---------------------------------------------------------------------------------------------
MARGIN = 2e-5      # 10 x the forward parity atol (tests/test_gpu_parity.py): a kernel within parity
#                    cannot flip a mask of a case whose oracle margin is at least this

_BASE = dict(graph=True, C=16, hidden=128, d_model=16, K=8, radius=4, zp=False, gn=True, hidden_only=True,
             a2a=True, msg=0.25, gain=0.05, thr=0.12, gthr=None)
MODELS = {
    "graph": dict(_BASE),
    "classic": dict(_BASE, graph=False, K=0, msg=0.0),
    "graph_zp": dict(_BASE, zp=True),
    "graph_zp_open": dict(_BASE, zp=True, a2a=False, hidden_only=False),
    "graph_open": dict(_BASE, a2a=False, hidden_only=False, thr=0.1),
    "graph_nogn": dict(_BASE, gn=False, thr=0.1),
    "classic_nogn": dict(_BASE, graph=False, K=0, msg=0.0, gn=False, thr=0.2),
    "g32": dict(_BASE, C=32, K=16, radius=5),
    "g32_nogn": dict(_BASE, C=32, K=16, radius=5, gn=False),
    "graph_g_gt_a": dict(_BASE, thr=0.1, gthr=0.3),
    "graph_g_lt_a": dict(_BASE, thr=0.3, gthr=0.1),
    "graph_neg_a": dict(_BASE, thr=-0.05, gthr=0.1),
}


def small_model(name: str, C: int, hidden: int) -> dict:
    """The runtime-geometry shapes' models: ``name`` at C channels, ``hidden`` units, radius 2,
    4 offsets."""
    m = dict(MODELS[name], C=C, hidden=hidden, d_model=8, radius=2)
    m["K"] = 4 if m["graph"] else 0
    return m


def oracle_cfg(m: dict) -> dict:
    cfg = dict(update_gain=m["gain"], alpha_thr=m["thr"], use_groupnorm=m["gn"], graph=m["graph"],
               message_gain=m["msg"], hidden_only=m["hidden_only"], zero_padded_shift=m["zp"],
               alive_to_alive=m["a2a"])
    if m.get("gthr") is not None:
        cfg["graph_alpha_thr"] = m["gthr"]
    return cfg


def params(m: dict, seed: int) -> dict:
    """float32 parameters under the modules' state_dict names (reference layouts)."""
    g = np.random.default_rng([77, seed, m["C"], m["hidden"]])
    C, Hd, d = m["C"], m["hidden"], m["d_model"]
    n = lambda *s, sd=1.0: (g.standard_normal(s) * sd).astype(np.float32)  # noqa: E731
    p = {"perception.conv.weight": O.sobel_weights(C),
         "update_net.0.weight": n(Hd, 3 * C, 1, 1, sd=(3 * C) ** -0.5),
         "update_net.0.bias": n(Hd, sd=0.1),
         "update_net.2.weight": n(C, Hd, 1, 1, sd=0.05)}
    if m["gn"]:
        p["norm.weight"] = g.uniform(0.5, 1.5, C).astype(np.float32)
        p["norm.bias"] = g.uniform(-0.2, 0.2, C).astype(np.float32)
    if m["graph"]:
        p.update({"graph.query_proj.weight": n(d, C, 1, 1, sd=0.3), "graph.query_proj.bias": n(d, sd=0.1),
                  "graph.key_proj.weight": n(d, C, 1, 1, sd=0.3), "graph.key_proj.bias": n(d, sd=0.1),
                  "graph.msg_proj.weight": n(C, C, 1, 1, sd=C ** -0.5), "graph.msg_proj.bias": n(C, sd=0.1),
                  "graph.scaling": np.float32(np.sqrt(d))})
    return p


def offsets(m: dict, step: int = 0) -> list:
    """``K`` offsets of radius ``r`` for step ``step``: the four diagonal corners (+-r, +-r) and the
    axis ends first, so that a torus gather crosses every image border by the full radius."""
    if not m["graph"] or m["K"] == 0:
        return []
    r = m["radius"]
    ring = [(-r, -r), (r, r), (-r, r), (r, -r), (0, r), (r, 0), (0, -r), (-r, 0),
            (2, r), (-r, 2), (-2, -r), (r, -2), (2, 0), (0, -2), (-2, 2), (2, 2)]
    ring = [o for i, o in enumerate(ring) if o not in ring[:i]]
    k = m["K"]
    s = (3 * step) % len(ring)
    return (ring[s:] + ring[:s])[:k]


# ---------------------------------------------------------------------------------------------
# Plans (host-only introspection) and the case tables
# ---------------------------------------------------------------------------------------------
def make_desc(m: dict, B: int, H: int, W: int, *, offs=None, fire_mode=None, fire_rate=1.0, seed=0,
              step=0, attention=False):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    flags = L.USE_GROUPNORM if m["gn"] else 0
    if m["graph"]:
        flags |= L.GRAPH | (L.ALIVE_TO_ALIVE if m["a2a"] else 0) | (L.ZERO_PAD_SHIFT if m["zp"] else 0) | \
            (L.HIDDEN_ONLY if m["hidden_only"] else 0) | (L.ATTENTION if attention else 0)
    return S.make_desc(B=B, C=m["C"], H=H, W=W, hidden=m["hidden"], d_model=m["d_model"],
                       offsets=offsets(m, step) if offs is None else offs, flags=flags,
                       update_gain=m["gain"], alpha_thr=m["thr"], graph_alpha_thr=m.get("gthr"),
                       message_gain=m["msg"], fire_rate=fire_rate,
                       fire_mode=L.FIRE_NONE if fire_mode is None else fire_mode, rng_seed=seed, rng_step=step)


def plan_of(m: dict, B: int, H: int, W: int) -> dict:
    """What the library plans for this model and shape (gnca_k1_variant / gnca_bb_variant)."""
    from graph_neural_cellular_automata_amd import step as S
    d = make_desc(m, B, H, W)
    return dict(k1=S.k1_variant(d)[0], compact=S.rollout_compact(d), subs=S.rollout_subs(d),
                fold=S.rollout_fold(d), foldable=S.rollout_fold(d, possible=True), bb=S.bb_variant(d))


def k1_tile(k1: str):
    """(TH, TW) of a split K1's name, None for the runtime-geometry kernel."""
    if not k1.startswith("gnca_k1_split"):
        return None
    th, tw = k1[k1.index("<") + 1:].split(",")[:2]
    return int(th), int(tw)


RUNTIME_BB = ",0,0,0,0,-1,0>"
# (model, B, H, W) -> the plan the case means to test; a key that is absent is not asserted
PLAN_ROWS = [
    ("graph", 2, 48, 72, dict(k1="gnca_k1_split<8,24,4,4,8>", bb="gnca_b_mlp<16,128,1,0,0,0,0,-1,0>")),
    ("graph", 8, 48, 72, dict(k1="gnca_k1_split<8,24,4,4,8>", compact=False, subs=1, fold=True,
                              bb="gnca_b_mlp<16,128,1,8,16,4,4,8,0>")),
    ("graph", 32, 48, 72, dict(k1="gnca_k1_split<8,24,4,4,8>", compact=True, subs=1, fold=True)),
    ("graph", 64, 48, 72, dict(k1="gnca_k1_split<8,24,4,4,8>", compact=True, subs=2, fold=False, foldable=True)),
    ("graph", 128, 48, 72, dict(k1="gnca_k1_split<24,36,4,4,8>", compact=True, subs=1, fold=True,
                                bb="gnca_b_mlp<16,128,1,24,24,4,4,8,1>")),
    ("graph", 256, 48, 72, dict(k1="gnca_k1_split<24,36,4,4,8>", compact=True, subs=2, fold=False, foldable=True)),
    ("graph", 8, 40, 40, dict(k1="gnca_k1_split<8,20,4,4,8>", compact=False, subs=1, fold=False, foldable=False)),
    ("graph", 64, 40, 40, dict(k1="gnca_k1_split<8,20,4,4,8>", compact=True, subs=1,
                               bb="gnca_b_mlp<16,128,1,24,24,4,4,8,1>")),
    ("graph", 128, 40, 40, dict(k1="gnca_k1_split<8,20,4,4,8>", compact=True, subs=2,
                                bb="gnca_b_mlp<16,128,1,8,24,4,4,8,0>")),
    ("g32", 128, 32, 32, dict(k1="gnca_k1_split32<16,16,5,8,16>", compact=True)),
    ("g32", 8, 32, 32, dict(k1="gnca_k1_split32<16,16,5,8,16>", compact=False)),
    ("graph_zp", 128, 48, 72, dict(k1="gnca_k1_split<24,36,4,4,8>", compact=True, fold=False, foldable=False)),
    ("graph_g_lt_a", 128, 48, 72, dict(k1="gnca_k1_split<24,36,4,4,8>", compact=True, fold=False, foldable=False)),
    ("graph_neg_a", 128, 48, 72, dict(k1="gnca_k1_split<24,36,4,4,8>", compact=True, fold=False, foldable=False)),
    ("graph_g_gt_a", 128, 48, 72, dict(k1="gnca_k1_split<24,36,4,4,8>", compact=True, fold=True)),
    # the classic model (K = 0): the same tiles and plans
    ("classic", 8, 48, 72, dict(k1="gnca_k1_split<8,24,1,4,0>", compact=False, subs=1, fold=True,
                                bb="gnca_b_mlp<16,128,1,8,16,1,4,0,0>")),
    ("classic", 64, 48, 72, dict(k1="gnca_k1_split<8,24,1,4,0>", compact=True, subs=2, fold=False, foldable=True)),
    ("classic", 128, 48, 72, dict(k1="gnca_k1_split<24,36,1,4,0>", compact=True, subs=1, fold=True)),
    ("classic", 64, 40, 40, dict(k1="gnca_k1_split<8,20,1,4,0>", compact=True, subs=1,
                                 bb="gnca_b_mlp<16,128,1,24,24,1,4,0,1>")),
    ("classic", 128, 40, 40, dict(k1="gnca_k1_split<8,20,1,4,0>", compact=True, subs=2,
                                  bb="gnca_b_mlp<16,128,1,8,24,1,4,0,0>")),
    ("classic", 2, 48, 72, dict(k1="gnca_k1_split<8,24,1,4,0>", bb="gnca_b_mlp<16,128,1,0,0,0,0,-1,0>")),
]


def check_plan(m_name: str, B: int, H: int, W: int, want: dict | None = None) -> dict:
    """Assert the planned kernels of a case against its PLAN_ROWS entry (or ``want``) and return the
    plan, for the assertion messages."""
    if want is None:
        want = next((w for n, b, h, w_, w in PLAN_ROWS if (n, b, h, w_) == (m_name, B, H, W)), {})
    got = plan_of(MODELS[m_name], B, H, W)
    for k, v in want.items():
        assert got[k] == v, (m_name, B, H, W, k, got)
    return got


ROLLOUT_PATTERNS = ("half_dead", "stripes", "isolated", "border_ring", "counts_rollout", "sparse")
ROLLOUT_STEPS = 4
# (model, B, H, W, pattern, seed, the two samples compared with the float64 oracle): every plan row
# with a rollout plan x every rollout pattern.  The seeds and samples are chosen so that every step
# of the two samples keeps the threshold margin (tests/test_liveness_cases_cpu.py asserts it).
_ROLLOUT_SEEDS: dict = {
    # default seeds whose two samples came within MARGIN of the threshold at some step: replaced
    ("graph", 8, 48, 72, "counts_rollout"): 1044, ("graph", 32, 48, 72, "stripes"): 1112,
    ("graph", 32, 48, 72, "isolated"): 1121, ("graph", 32, 48, 72, "sparse"): 1151,
    ("graph", 64, 48, 72, "stripes"): 1213, ("graph", 128, 48, 72, "stripes"): 1311,
    ("graph", 128, 48, 72, "counts_rollout"): 1341, ("graph", 128, 48, 72, "sparse"): 1351,
    ("graph", 256, 48, 72, "stripes"): 1411, ("graph", 8, 40, 40, "stripes"): 1511,
    ("g32", 8, 32, 32, "isolated"): 1921, ("graph_zp", 128, 48, 72, "stripes"): 2011,
    ("graph_zp", 128, 48, 72, "sparse"): 2051, ("graph_g_gt_a", 128, 48, 72, "stripes"): 2313,
    ("classic", 64, 48, 72, "stripes"): 2511, ("classic", 128, 48, 72, "counts_rollout"): 2641,
}


def rollout_cases():
    out = []
    rows = [r for r in PLAN_ROWS if "compact" in r[4]]
    for i, (name, B, H, W, _) in enumerate(rows):
        for j, pat in enumerate(ROLLOUT_PATTERNS):
            if name == "classic" and (i + j) % 2:    # the classic rows: every other pattern
                continue
            seed = _ROLLOUT_SEEDS.get((name, B, H, W, pat), 10 * i + j)
            out.append((name, B, H, W, pat, seed, (j % B, B - 1 - (i % 2))))
    return out


def rollout_fire(pattern: str):
    """(fire_rate, hashed?) of a rollout pattern: ``sparse`` runs under GNCA_FIRE_HASH, the others
    under GNCA_FIRE_NONE."""
    return (0.5, True) if pattern == "sparse" else (1.0, False)


def oracle_rollout(case: Case, m: dict, p64: dict, seed: int, steps: int, *, hashed: bool, fire_rate: float):
    """The float64 oracle rollout of the built samples: (states after each step, min margin over
    the steps' post-update masks and, for two-threshold models, nothing else: the sender mask of a
    later step thresholds a state the bitwise comparison with single steps already pins)."""
    cfg = oracle_cfg(m)
    x = case.x.astype(np.float64)
    H, W = x.shape[-2:]
    frames, margin = [], np.inf
    for t in range(steps):
        fire = None
        if hashed:
            fire = np.concatenate([O.hash_fire_mask(seed, t, b, 1, H, W, fire_rate) for b in case.info["samples"]])
        xt, _ = O.nca_update(x, p64, cfg, chosen=offsets(m, t), fire_mask=fire)
        margin = min(margin, min_margin(xt, m["thr"]))
        x = O.nca_step(x, p64, cfg, chosen=offsets(m, t), fire_mask=fire)
        frames.append(x)
    return frames, margin


def f64(p: dict) -> dict:
    return {k: np.asarray(v, np.float64) for k, v in p.items()}


# ---------------------------------------------------------------------------------------------
# One-step cases (against the float64 oracle): every pattern x every K1 family
# ---------------------------------------------------------------------------------------------
STEP_PATTERNS = ("isolated", "border_ring", "half_dead", "stripes", "sparse", "counts", "exact_thr")
# name, B, H, W, the K1 tile the patterns are laid out for, the K1 the plan must name (prefix),
# the samples compared with the oracle (None: all)
STEP_SHAPES = [
    ("s8x24", 4, 48, 72, (8, 24), "gnca_k1_split<8,24,", None),
    ("s24x36", 128, 48, 72, (24, 36), "gnca_k1_split<24,36,", (0, 1, 127)),
    ("s8x20", 4, 40, 40, (8, 20), "gnca_k1_split<8,20,", None),
    ("ragged", 3, 17, 29, (4, 8), "gnca_k1_update<", None),
    ("tiny", 4, 5, 7, (4, 8), "gnca_k1_update<", None),
    ("c32", 4, 32, 32, (16, 16), "gnca_k1_split32<16,16,", None),
]
_V16 = ("graph", "graph_zp_open", "graph_nogn", "classic", "graph_open", "graph_zp", "classic_nogn")
_SMALL = ((4, 32), (12, 64), (20, 32), (4, 64), (12, 32), (20, 64))
_STEP_SEEDS: dict = {}


def step_cases():
    """dicts: id, model (dict), shape fields, pattern, seed, fire ('mask' | 'hash' | None)."""
    out = []
    for si, (sname, B, H, W, tile, k1, cmp_) in enumerate(STEP_SHAPES):
        for pi, pat in enumerate(STEP_PATTERNS):
            thrs = (0.1, 0.12, 0.2) if pat == "exact_thr" else (None,)
            for ti, thr in enumerate(thrs):
                v = (pi + 2 * si + ti) % len(_V16)
                if sname == "c32":
                    mname = "g32_nogn" if pat == "exact_thr" else "g32"
                    m = dict(MODELS[mname])
                else:
                    mname = _V16[v]
                    if pat == "exact_thr":      # GroupNorm shifts dead cells too: only without it
                        mname = ("graph_nogn", "classic_nogn", "graph_nogn")[(si + ti) % 3]
                    if sname in ("ragged", "tiny"):
                        C, hid = _SMALL[(pi + si + ti) % len(_SMALL)]
                        m = small_model(mname, C, hid)
                        mname = f"{mname}/C{C}h{hid}"
                    else:
                        m = dict(MODELS[mname])
                if thr is not None:
                    m["thr"] = thr
                fire = "mask" if pat in ("counts", "exact_thr") else ("hash", None)[(pi + si) % 2]
                cid = f"{sname}-{pat}-{mname}" + (f"-thr{thr}" if thr is not None else "")
                out.append(dict(id=cid, m=m, mname=mname, B=B, H=H, W=W, tile=tile, k1=k1, pattern=pat,
                                seed=_STEP_SEEDS.get(cid, 100 + 7 * si + pi), fire=fire,
                                samples=list(range(B)) if cmp_ is None else list(cmp_)))
    return out


def step_fire(c: dict, case: Case):
    """The {0,1} fire mask [n,1,H,W] of the built samples of a step case, or None."""
    if c["fire"] == "mask":
        return case.fire
    if c["fire"] == "hash":
        return np.concatenate([O.hash_fire_mask(c["seed"], 0, b, 1, c["H"], c["W"], 0.5)
                               for b in case.info["samples"]])
    return None


# ---------------------------------------------------------------------------------------------
# Two-threshold one-step cases (C ABI, graph_alpha_thr != alpha_thr), 48x72, B = 4
# ---------------------------------------------------------------------------------------------
# model, lower end of the seeds' alpha: the seeds spread over [seed_lo, 1] fall on both sides of
# the larger threshold, so the update's mask and the senders' mask differ
THR_ORDERS = (("graph_g_gt_a", 0.12), ("graph_g_lt_a", 0.12), ("graph_neg_a", 0.0))
_THR_SEEDS: dict = {}


def thr_step_cases():
    out = []
    for i, (mname, lo) in enumerate(THR_ORDERS):
        for j, pat in enumerate(("sparse", "isolated")):
            cid = f"{mname}-{pat}"
            out.append(dict(id=cid, mname=mname, m=dict(MODELS[mname]), B=4, H=48, W=72, tile=(8, 24),
                            pattern=pat, seed=_THR_SEEDS.get(cid, 300 + 2 * i + j), seed_lo=lo,
                            fire=("hash", None)[j], samples=[0, 1, 2, 3]))
    return out


# ---------------------------------------------------------------------------------------------
# Backward cases (against the float64 VJP oracle; the weight gradients need the whole batch)
# ---------------------------------------------------------------------------------------------
BWD_PATTERNS = ("sparse", "half_dead", "border_ring", "counts")
# family, B, H, W, K1 tile, backward MLP kernel of the graph (K = 8) and the classic (K = 0) model
BWD_FAMILIES = [
    ("runtime", 2, 48, 72, (8, 24), "gnca_b_mlp<16,128,1,0,0,0,0,-1,0>", "gnca_b_mlp<16,128,1,0,0,0,0,-1,0>"),
    ("8x16", 8, 48, 72, (8, 24), "gnca_b_mlp<16,128,1,8,16,4,4,8,0>", "gnca_b_mlp<16,128,1,8,16,1,4,0,0>"),
    ("8x24", 128, 40, 40, (8, 20), "gnca_b_mlp<16,128,1,8,24,4,4,8,0>", "gnca_b_mlp<16,128,1,8,24,1,4,0,0>"),
    ("lean", 64, 40, 40, (8, 20), "gnca_b_mlp<16,128,1,24,24,4,4,8,1>", "gnca_b_mlp<16,128,1,24,24,1,4,0,1>"),
]
_BWD_SEEDS: dict = {}


def bwd_cases():
    out = []

    def add(fam, mname, m, B, H, W, tile, pat, bb, k):
        cid = f"{fam}-{pat}-{mname}"
        out.append(dict(id=cid, mname=mname, m=m, B=B, H=H, W=W, tile=tile, pattern=pat, bb=bb,
                        seed=_BWD_SEEDS.get(cid, 500 + k), samples=list(range(B)),
                        fire={"counts": "mask", "sparse": "hash"}.get(pat)))

    k = 0
    for fi, (fam, B, H, W, tile, bb_g, bb_c) in enumerate(BWD_FAMILIES):
        for pi, pat in enumerate(BWD_PATTERNS):
            g = (fi + pi) % 2 == 0
            mname = "graph" if g else "classic"
            add(fam, mname, dict(MODELS[mname]), B, H, W, tile, pat, bb_g if g else bb_c, k)
            k += 1
    # GroupNorm off (the dead cells' gx = gy property), on the two small families
    add("runtime", "graph_nogn", dict(MODELS["graph_nogn"]), 2, 48, 72, (8, 24), "sparse", BWD_FAMILIES[0][5], k)
    add("8x16", "classic_nogn", dict(MODELS["classic_nogn"]), 8, 48, 72, (8, 24), "half_dead", BWD_FAMILIES[1][6], k + 1)
    k += 2
    # the ragged and the tiny runtime-geometry shapes
    names = ("graph", "classic_nogn", "graph_zp_open", "graph_nogn")
    for si, (fam, B, H, W) in enumerate((("ragged", 3, 17, 29), ("tiny", 4, 5, 7))):
        for pi, pat in enumerate(BWD_PATTERNS):
            C, hid = _SMALL[(pi + 3 * si) % len(_SMALL)]
            base = names[(pi + si) % 4]
            add(fam, f"{base}/C{C}h{hid}", small_model(base, C, hid), B, H, W, (4, 8), pat, RUNTIME_BB, k)
            k += 1
    return out


# trace() and the grad rollout, once each on a sparse state (40x40, B = 4, hash fire masks)
E_CASES = {
    "trace": dict(mname="graph", B=4, H=40, W=40, tile=(8, 20), seed=702, steps=4, fire_rate=0.5),
    "bptt": dict(mname="graph", B=4, H=40, W=40, tile=(8, 20), seed=701, steps=3, fire_rate=0.5),
}
