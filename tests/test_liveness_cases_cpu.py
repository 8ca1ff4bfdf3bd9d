"""CPU checks of the alive-mask patterns (tests/liveness_cases.py) and of the oracle they are
compared with in tests/test_gpu_liveness.py:

* the patterns have the structure they claim (from the oracle's masks alone);
* every case the GPU tests compare with the float64 oracle keeps every cell's pooled post-update
  alpha at least ``MARGIN`` = 2e-5 away from the threshold (10 x the forward parity atol: a kernel
  within parity cannot flip a mask there).  This is a condition on the INPUTS: a seed that fails
  it is replaced in the case table, cells are never excluded (but for the cells ``exact_thr``
  places at the threshold on purpose, which no arithmetic touches);
* the float32 oracle equals the PyTorch-CPU restatement of the reference on every pattern, masks
  included, and the float64 oracle draws the same masks at an exact float32 threshold;
* the case tables reach every plan of the rollout / backward table (host-only introspection).
"""
import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from oracle import nca_oracle as O
from oracle.torch_cpu_ref import TorchCpuStep
from tests import liveness_cases as LC

TILES = [(24, 36), (8, 24), (8, 20), (16, 16)]
CANVAS = {(24, 36): (48, 72), (8, 24): (48, 72), (8, 20): (40, 40), (16, 16): (32, 32)}


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _alive(x, thr):
    return O.alive_mask(np.asarray(x, np.float64), thr)[:, 0] != 0


def _blocks(seeds):
    """Union of the clipped 3x3 blocks of the seed cells, one seed at a time."""
    out = np.zeros_like(seeds)
    B, H, W = seeds.shape
    for b, r, q in np.argwhere(seeds):
        out[b, max(0, r - 1):min(H, r + 2), max(0, q - 1):min(W, q + 2)] = True
    return out


# ---------------------------------------------------------------------------------------------
# Pattern properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,hw", [(t, CANVAS[t]) for t in TILES] + [((4, 8), (17, 29)), ((4, 8), (5, 7))])
@pytest.mark.parametrize("thr", [0.1, 0.12])
def test_isolated_gives_exactly_the_clipped_blocks(tile, hw, thr):
    H, W = hw
    c = LC.build("isolated", 3, 12, 16, H, W, thr, tile)
    alive = _alive(c.x, thr)
    assert (alive == _blocks(c.seeds)).all()
    assert (alive == LC.expected_alive(c)).all()
    # the seeds are single cells, apart: each block is its own
    for b, r, q in np.argwhere(c.seeds):
        assert c.seeds[b, max(0, r - 3):r + 4, max(0, q - 3):q + 4].sum() == 1
    # over the batch they sit at every corner, on every edge, on both sides of every tile boundary
    # row and column, on the first and last row of the 4- and 6-row bands, and in the interior
    any_ = c.seeds.any(axis=0)
    for r, q in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        assert any_[r, q], (r, q)
        b = int(np.argmax(c.seeds[:, r, q]))
        # ... and light nothing on the opposite border (a pool that wrapped would)
        assert not alive[b, H - 1 - r, :].any() or c.seeds[b, max(0, H - 3 - r):H - r + 2].any() or H < 8
        assert not alive[b, :, W - 1 - q].any() or c.seeds[b, :, max(0, W - 3 - q):W - q + 2].any() or W < 8
    assert any_[0, 1:-1].any() and any_[-1, 1:-1].any() and any_[1:-1, 0].any() and any_[1:-1, -1].any()
    TH, TW = tile
    for r in range(TH, H, TH):
        assert any_[r - 1].any() and any_[r].any(), r
    for q in range(TW, W, TW):
        assert any_[:, q - 1].any() and any_[:, q].any(), q
    if H >= 32:   # (the small runtime-geometry canvases cannot hold every band edge apart)
        for band in LC.BANDS:
            for r in range(band, H, band):
                assert any_[r - 1].any() and any_[r].any(), (band, r)
        assert any_[2:-2, 2:-2].any()


@pytest.mark.parametrize("hw", [(48, 72), (40, 40), (32, 32), (17, 29), (5, 7)])
def test_border_ring_leaves_the_opposite_border_dead(hw):
    H, W = hw
    c = LC.build("border_ring", 1, 8, 16, H, W, 0.12, (8, 24))
    alive = _alive(c.x, 0.12)
    assert (alive == _blocks(c.seeds)).all()
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    assert not (c.seeds & inner).any()                      # seeds on the border lines only
    assert not alive[:, 2:-2, 2:-2].any()
    seen = set()
    for b in range(8):
        sides = LC.border_sides(b)
        seen.update(sides)
        for s in range(4):
            if s in sides or (s + 2) % 4 not in sides:
                continue
            # side s is opposite a seeded side and not seeded itself: its line and the line inside
            # it are dead, but for the corners' blocks of an adjacent seeded side
            adj = [(s + 1) % 4 in sides, (s + 3) % 4 in sides]
            line = {0: alive[b, :2, :], 1: alive[b, :, -2:].T, 2: alive[b, -2:, :], 3: alive[b, :, :2].T}[s]
            lo, hi = (2 if any(adj) else 0), (line.shape[1] - 2 if any(adj) else line.shape[1])
            assert not line[:, lo:hi].any(), (b, s)
    assert seen == {0, 1, 2, 3}
    assert alive.any(axis=(1, 2)).all()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("seed", [0, 1])
def test_counts_holds_every_listed_live_count(tile, seed):
    H, W = CANVAS[tile]
    TH, TW = tile
    tps = (H // TH) * (W // TW)
    B = -(-len(LC.COUNTS) // tps) + 1
    c = LC.build("counts", seed, B, 16, H, W, 0.12, tile)
    assert _alive(c.x, 0.12).all()                          # alive everywhere
    got = LC.tile_live_counts(LC.keep_mask(c.x, 0.12, c.fire), tile).reshape(-1)
    want = [0, 1, 31, 32, 33, 63, 64, 65, TH * TW - 1, TH * TW]
    assert set(want) <= set(got.tolist()), sorted(set(got.tolist()))
    assert got.tolist() == [k for s in c.info["want"] for k in s]
    # in tile order the listed counts follow one another: ascending for even seeds, descending for odd
    seq = got.tolist()
    run = want[::-1] if seed % 2 else want
    i = seq.index(run[0])
    assert any(seq[j:j + len(run)] == run for j in range(len(seq))), (seq, run, i)
    # an empty tile next to a full one, in both orders over the two seeds
    full, pairs = TH * TW, list(zip(seq, seq[1:]))
    assert ((full, 0) in pairs) or ((0, full) in pairs)


@pytest.mark.parametrize("tile", TILES)
def test_counts_rollout_holds_empty_small_32_and_full(tile):
    H, W = CANVAS[tile]
    TH, TW = tile
    for seed in (0, 1):
        c = LC.build("counts_rollout", seed, 4, 16, H, W, 0.12, tile)
        got = LC.tile_live_counts(LC.keep_mask(c.x, 0.12), tile).reshape(-1).tolist()
        assert got == [k for s in c.info["want"] for k in s]
        assert {0, 9, 32, TH * TW} <= set(got)


@pytest.mark.parametrize("tile", TILES)
def test_half_dead_has_both_transitions(tile):
    H, W = CANVAS[tile]
    TH, TW = tile
    c = LC.build("half_dead", 0, 4, 16, H, W, 0.12, tile)
    cnt = LC.tile_live_counts(LC.keep_mask(c.x, 0.12), tile)
    assert set(np.unique(cnt).tolist()) == {0, TH * TW}     # whole tiles: empty or alive everywhere
    by_col = c.info["by_col"]
    assert True in by_col and False in by_col
    for b in range(4):
        a = cnt[b] > 0
        if by_col[b]:
            assert (a == a[:1]).all() and (a[0, 1:] != a[0, :-1]).all()
        else:
            assert (a.T == a.T[:1]).all() and (a[1:, 0] != a[:-1, 0]).all()
    seq = (cnt.reshape(-1) > 0).tolist()                    # the order a persistent workgroup walks
    pairs = set(zip(seq, seq[1:]))
    assert (False, True) in pairs and (True, False) in pairs
    # both phases: a sample that starts empty and one that starts full
    assert {bool(cnt[b, 0, 0]) for b in range(4)} == {True, False}


@pytest.mark.parametrize("tile", [(24, 36), (8, 24), (8, 20)])
def test_stripes_leave_one_cell_gaps_at_every_phase(tile):
    H, W = CANVAS[tile]
    TW = tile[1]
    c = LC.build("stripes", 0, 8, 16, H, W, 0.12, tile)
    alive = _alive(c.x, 0.12)
    row_ph, col_ph, masks = set(), set(), set()
    for b in range(8):
        a = alive[b]
        if (a == a[:, :1]).all():                            # row stripes
            dead = np.flatnonzero(~a[:, 0])
            assert len(dead) > 4 and (np.diff(dead)[1:-1] == 4).all()   # (two dead lines at a border)
            row_ph.add(int(dead[0]) % 4)
        else:
            assert (a == a[:1]).all()
            dead = np.flatnonzero(~a[0])
            assert len(dead) > 4 and (np.diff(dead)[1:-1] == 4).all()   # one-cell gaps, three alive between
            col_ph.add(int(dead[0]) % 4)
            for tx in range(W // TW):                        # the tile rows' live masks
                masks.add(tuple(a[0, tx * TW:(tx + 1) * TW].tolist()))
    assert len(row_ph) >= 2 and len(col_ph) >= 2
    # tile-row masks of differing phase, none full, none empty: 36 and 20 are no multiples of 64 / 4
    # bits, so the packed rows of a tile straddle the 64-bit ballot words at shifting positions
    assert len(masks) >= 2 and all(0 < sum(m) < TW for m in masks)


def test_sparse_is_about_a_fifth_alive():
    c = LC.build("sparse", 0, 4, 16, 48, 72, 0.12, (8, 24))
    f = _alive(c.x, 0.12).mean()
    assert 0.15 < f < 0.3, f
    s = LC.build("sparse", 0, 128, 16, 48, 72, 0.12, (8, 24), samples=[5, 77])
    full = LC.build("sparse", 0, 8, 16, 48, 72, 0.12, (8, 24))
    assert np.array_equal(s.x[0], full.x[5])                # a sample does not depend on the batch


@pytest.mark.parametrize("thr", [0.1, 0.12, 0.2])
def test_exact_thr_places_cells_at_the_threshold_and_one_ulp_above(thr):
    c = LC.build("exact_thr", 2, 4, 16, 40, 40, thr, (8, 20))
    eq, ulp, quiet = c.info["eq"], c.info["ulp"], c.info["quiet"]
    assert eq.sum() >= 4 and quiet.sum() >= 4 and (ulp & ~quiet).sum() >= 4
    a = c.x[:, 3]
    assert (a[eq] == np.float32(thr)).all() and (a[ulp] == np.nextafter(np.float32(thr), np.float32(1))).all()
    placed = eq | ulp
    for b, r, q in np.argwhere(placed):                      # isolated by two or more cells
        win = (placed | c.seeds)[b, max(0, r - 2):r + 3, max(0, q - 2):q + 3]
        assert win.sum() == 1
    # strict float32 semantics: equal is dead, one ulp above is alive
    alive = _alive(c.x, thr)
    assert not alive[eq].any() and alive[ulp].all()
    assert (alive == LC.dilate(c.seeds | ulp)).all()
    for b, r, q in np.argwhere(quiet):
        assert not c.fire[b, 0, max(0, r - 2):r + 3, max(0, q - 2):q + 3].any()


# ---------------------------------------------------------------------------------------------
# Threshold margin of every case compared with the oracle
# ---------------------------------------------------------------------------------------------
def _one_step_margin(c):
    m = c["m"]
    case = LC.build(c["pattern"], c["seed"], c["B"], m["C"], c["H"], c["W"], m["thr"], c["tile"],
                    seed_lo=c.get("seed_lo"), samples=c["samples"])
    xt, _ = O.nca_update(case.x.astype(np.float64), LC.f64(LC.params(m, c["seed"])), LC.oracle_cfg(m),
                         chosen=LC.offsets(m), fire_mask=LC.step_fire(c, case))
    return LC.min_margin(xt, m["thr"], case.exact)


@pytest.mark.parametrize("c", LC.step_cases() + LC.thr_step_cases() + LC.bwd_cases(), ids=lambda c: c["id"])
def test_one_step_cases_keep_the_threshold_margin(c):
    mg = _one_step_margin(c)
    assert mg >= LC.MARGIN, f"{c['id']}: margin {mg:.3e}: choose another seed in the case table"


@pytest.mark.parametrize("rc", LC.rollout_cases(), ids=lambda rc: "-".join(map(str, rc[:6])))
def test_rollout_cases_keep_the_threshold_margin_at_every_step(lib, rc):
    name, B, H, W, pat, seed, smp = rc
    m = LC.MODELS[name]
    tile = LC.k1_tile(LC.plan_of(m, B, H, W)["k1"])
    case = LC.build(pat, seed, B, m["C"], H, W, m["thr"], tile, samples=smp)
    fr, hashed = LC.rollout_fire(pat)
    _, mg = LC.oracle_rollout(case, m, LC.f64(LC.params(m, seed)), seed, LC.ROLLOUT_STEPS, hashed=hashed,
                              fire_rate=fr)
    assert mg >= LC.MARGIN, f"{rc}: margin {mg:.3e}: choose another seed or samples in the case table"


@pytest.mark.parametrize("name,c", list(LC.E_CASES.items()))
def test_trace_and_bptt_cases_keep_the_threshold_margin(name, c):
    m = LC.MODELS[c["mname"]]
    case = LC.build("sparse", c["seed"], c["B"], m["C"], c["H"], c["W"], m["thr"], c["tile"])
    _, mg = LC.oracle_rollout(case, m, LC.f64(LC.params(m, c["seed"])), c["seed"], c["steps"],
                              hashed=c["fire_rate"] < 1, fire_rate=c["fire_rate"])
    assert mg >= LC.MARGIN, (name, mg)


# ---------------------------------------------------------------------------------------------
# Oracle against the PyTorch-CPU restatement of the reference
# ---------------------------------------------------------------------------------------------
def _torch_step(m, p):
    return TorchCpuStep(p, graph=m["graph"], update_gain=m["gain"], alpha_thr=m["thr"], message_gain=m["msg"],
                        hidden_only=m["hidden_only"], alive_to_alive=m["a2a"], zero_padded_shift=m["zp"],
                        use_groupnorm=m["gn"])


_REF_CASES = [c for c in LC.step_cases() if c["id"].startswith(("s8x20-", "ragged-", "c32-exact", "s8x24-exact"))]


@pytest.mark.parametrize("c", _REF_CASES, ids=lambda c: c["id"])
def test_oracle_f32_equals_torch_cpu_reference(c):
    """oracle.nca_step in float32 against the reference's op sequence on CPU ATen kernels, at
    tests/test_torch_cpu_ref.py's tolerance, with identical alive masks of the result; on
    ``exact_thr`` the float64 oracle's masks equal them too (it compared with the double 0.1 > float32(0.1)
    before, so a cell at exactly float32(0.1) or float32(0.2) was alive for it alone)."""
    m = c["m"]
    case = LC.build(c["pattern"], c["seed"], c["B"], m["C"], c["H"], c["W"], m["thr"], c["tile"], samples=c["samples"])
    p = LC.params(m, c["seed"])
    fire = LC.step_fire(c, case)
    fire32 = None if fire is None else np.asarray(fire, np.float32)
    ref = _torch_step(m, p)(torch.from_numpy(case.x), chosen=LC.offsets(m),
                            fire_mask=None if fire32 is None else torch.from_numpy(fire32)).numpy()
    out32 = O.nca_step(case.x, p, LC.oracle_cfg(m), chosen=LC.offsets(m), fire_mask=fire32)
    np.testing.assert_allclose(out32, ref, rtol=1e-5, atol=2e-6)
    thr = m["thr"]
    ref_pre = torch.nn.functional.max_pool2d(torch.from_numpy(case.x[:, 3:4]), 3, 1, 1) > thr
    ref_post = torch.nn.functional.max_pool2d(torch.from_numpy(ref[:, 3:4]), 3, 1, 1) > thr
    assert np.array_equal(O.alive_mask(case.x, thr) != 0, ref_pre.numpy())
    assert np.array_equal(O.alive_mask(out32, thr) != 0, ref_post.numpy())
    assert np.array_equal(out32[:, 3] == 0, ref[:, 3] == 0)          # the gate zeroed the same cells
    if c["pattern"] == "exact_thr":
        out64 = O.nca_step(case.x.astype(np.float64), LC.f64(p), LC.oracle_cfg(m), chosen=LC.offsets(m),
                           fire_mask=fire)
        assert np.array_equal(O.alive_mask(case.x.astype(np.float64), thr) != 0, ref_pre.numpy())
        assert np.array_equal(O.alive_mask(out64, thr) != 0, ref_post.numpy())
        eq, quiet = case.info["eq"], case.info["quiet"]
        # equal is dead: the post gate zeroes the cell; one ulp above is alive: it keeps its alpha
        for out in (ref, out32, out64):
            assert (out[:, 3][eq] == 0).all()
            assert (out[:, 3][quiet] == case.x[:, 3][quiet]).all()


def test_graph_alpha_thr_gates_the_senders_only():
    """cfg['graph_alpha_thr'] changes the sender mask and nothing else: with alive_to_alive off it
    is inert, and with equal thresholds it is the default."""
    m = dict(LC.MODELS["graph_g_gt_a"])
    case = LC.build("sparse", 1, 2, 16, 40, 40, m["thr"], (8, 20), seed_lo=0.12)
    p = LC.f64(LC.params(m, 1))
    x = case.x.astype(np.float64)
    cfg = LC.oracle_cfg(m)
    base = O.nca_step(x, p, dict(cfg, graph_alpha_thr=m["thr"]), chosen=LC.offsets(m))
    assert np.array_equal(base, O.nca_step(x, p, {k: v for k, v in cfg.items() if k != "graph_alpha_thr"},
                                           chosen=LC.offsets(m)))
    two = O.nca_step(x, p, cfg, chosen=LC.offsets(m))
    assert not np.array_equal(two, base)
    off = dict(cfg, alive_to_alive=False)
    assert np.array_equal(O.nca_step(x, p, off, chosen=LC.offsets(m)),
                          O.nca_step(x, p, dict(off, graph_alpha_thr=0.9), chosen=LC.offsets(m)))
    # the message with the sender mask at graph_alpha_thr = the message of a state whose sub-threshold
    # senders' messages are masked by hand
    msg = O.graph_message(x, p, LC.offsets(m), zero_padded_shift=False, alive_to_alive=True,
                          alpha_thr=m["thr"], graph_alpha_thr=m["gthr"])
    msg_same = O.graph_message(x, p, LC.offsets(m), zero_padded_shift=False, alive_to_alive=True, alpha_thr=m["gthr"])
    assert np.array_equal(msg, msg_same)


# ---------------------------------------------------------------------------------------------
# Plan table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", LC.PLAN_ROWS, ids=lambda r: f"{r[0]}-{r[1]}-{r[2]}x{r[3]}")
def test_plan_rows(lib, row):
    name, B, H, W, want = row
    got = LC.check_plan(name, B, H, W, want)
    if "compact" in want:
        assert LC.k1_tile(got["k1"]) is not None


def test_case_tables_reach_every_plan(lib):
    rows = {(n, b, h, w) for n, b, h, w, want in LC.PLAN_ROWS if "compact" in want}
    assert rows == {rc[:4] for rc in LC.rollout_cases()}
    for pat in LC.ROLLOUT_PATTERNS:
        assert {rc[:4] for rc in LC.rollout_cases() if rc[4] == pat} >= {r for r in rows if r[0] != "classic"}
    # rollout plans: dense / compact, one / two streams, default fold / fold on request / no fold
    plans = {(p["compact"], p["subs"], p["fold"], p["foldable"])
             for p in (LC.plan_of(LC.MODELS[n], b, h, w) for n, b, h, w in rows)}
    assert {(False, 1, True, True), (True, 1, True, True), (True, 2, False, True), (False, 1, False, False),
            (True, 1, False, False), (True, 2, False, False)} <= plans
    # one-step cases: every K1 family the shapes name
    k1s = set()
    for c in LC.step_cases():
        got = LC.plan_of(c["m"], c["B"], c["H"], c["W"])
        assert got["k1"].startswith(c["k1"]), (c["id"], got)
        k1s.add(c["k1"])
    assert k1s == {s[5] for s in LC.STEP_SHAPES}
    # backward cases: every backward MLP kernel family, graph (K = 8) and classic (K = 0)
    bbs = set()
    for c in LC.bwd_cases():
        got = LC.plan_of(c["m"], c["B"], c["H"], c["W"])
        assert got["bb"].endswith(c["bb"]) if c["bb"] == LC.RUNTIME_BB else got["bb"] == c["bb"], (c["id"], got)
        bbs.add(got["bb"])
    for fam in LC.BWD_FAMILIES:
        assert fam[5] in bbs and fam[6] in bbs, fam
