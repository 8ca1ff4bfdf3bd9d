"""GPU tests of the flat finalize kernel (``gnca_k2_finalize_flat``): one thread per 4-cell vector on the
compact update field, no LDS, planned for the K2 of the rollout's sub-batch pipeline.

Every case asserts through ``S.k2_variant`` that a sub-batch step of its rollout launches the flat
kernel and that a single step launches the band kernel on the dense field, then compares a 5-step
rollout bitwise with 5 single steps (the band kernel, ``gnca_k2_finalize<4,false,..>``): 5 steps, so that
the alive bytes the flat kernel writes are what the next step's K1 reads.  The two kernels evaluate the
same functions (``fin_alpha``, ``k2_update``, ``wave_sum2``'s fixed-order sums) on the same inputs, so
the comparison is exact and has no tolerance.

The flat kernel is planned beside a K1 only (alone on the chip the band kernel is kept),
and the 32-channel K1 runs no sub-batch pipeline, so there is no one-stream case and no 32-channel case
here; tests/test_k2_variant_cpu.py asserts that those plans name the band kernel.  One case runs a model
without GroupNorm.
"""
import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests import liveness_cases as LC
from tests.golden_io import Case

pytestmark = pytest.mark.gpu

T = 5
FLAT = "gnca_k2_finalize_flat<4,"
DENSE = "gnca_k2_finalize<4,false,"
B72 = 192          # two sub-batch streams of 96 samples: 576 tiles of 24x36 each
SEAMS = [(0, 0), (0, 71), (71, 0), (71, 71),                    # image corners
         (0, 35), (35, 0), (71, 36), (36, 71),                  # image edges
         (23, 35), (23, 36), (24, 35), (24, 36),                # the four cells round a tile corner
         (23, 0), (24, 71), (0, 36), (71, 35), (23, 50), (24, 10), (50, 35), (10, 36)]   # seams at the edges / inside


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _fixture_weights(fx, graph, dev):
    from graph_neural_cellular_automata_amd import step as S
    c = Case(fx)
    wt = {k: torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))).to(dev) for k, v in c.weights.items()}
    tensors = dict(perception=wt["perception.conv.weight"], w1=wt["update_net.0.weight"], b1=wt["update_net.0.bias"],
                   w2=wt["update_net.2.weight"], gn_weight=wt["norm.weight"], gn_bias=wt["norm.bias"])
    if graph:
        tensors.update(wq=wt["graph.query_proj.weight"], bq=wt["graph.query_proj.bias"],
                       wk=wt["graph.key_proj.weight"], bk=wt["graph.key_proj.bias"],
                       wm=wt["graph.msg_proj.weight"], bm=wt["graph.msg_proj.bias"], scaling=wt["graph.scaling"])
    w, keep = S.make_weights(tensors)
    return w, (keep, tensors)


def _lc_weights(m, seed, dev):
    from graph_neural_cellular_automata_amd import step as S
    from tests.test_gpu_liveness import _SHORT
    tensors = {_SHORT[k]: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))).to(dev)
               for k, v in LC.params(m, seed).items()}
    w, keep = S.make_weights(tensors)
    return w, (keep, tensors)


def _state(B, C, H, W, dev, seed, alpha=None):
    """The bench's synthetic state (RGB, alpha ~ U(0,1), hidden ~ N(0,1)), or a given alpha plane."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(B, C, H, W, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, C - 4, H, W, device=dev, generator=g)
    if alpha is not None:
        x[:, 3] = alpha
    return x.contiguous()


def _check(model, B, H, W, w, x, *, fire=0.5, seed=5):
    """The rollout's plan names the flat kernel; 5 rollout steps == 5 single (band, dense) steps, bitwise."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    m = LC.MODELS[model]

    def desc(t):
        return LC.make_desc(m, B, H, W, step=t, seed=seed, fire_rate=fire,
                            fire_mode=L.FIRE_HASH if fire < 1.0 else L.FIRE_NONE)

    d0 = desc(0)
    plan = (S.k1_variant(d0)[0], S.rollout_compact(d0), S.rollout_subs(d0), S.k2_variant(d0, 1), S.k2_variant(d0, -1))
    assert plan[1] and plan[2] == 2 and plan[3].startswith(FLAT) and plan[4].startswith(DENSE), plan
    offs = [LC.offsets(m, t) for t in range(T)]
    r = S.rollout(d0, w, x, T, offs)
    cur = x
    for t in range(T):
        cur, _ = S.step(desc(t), w, cur)
    assert torch.isfinite(cur).all(), plan
    same = torch.equal(r, cur)
    if not same:
        bad = (r != cur).nonzero()
        print(f"[k2_flat] {model} B={B} {H}x{W} {plan}: {bad.shape[0]} values differ, first (b, c, i, j) = "
              f"{bad[0].tolist()}, channels {sorted(set(bad[:, 1].tolist()))}, max |diff| = "
              f"{float((r - cur).abs().max()):.3e}")
    assert same, plan
    return r


@pytest.fixture(scope="module")
def graph72(dev):
    return _fixture_weights("graph_torus_latest_grown_b1_72", True, dev)


def test_headline_shape_trained_weights(dev, graph72):
    """Headline flags and the trained fixture weights at B=192 x 72^2: two sub-batch streams, K2 every
    step; 1,296 vectors per sample, so a sample's last workgroup has 16 active threads."""
    assert (72 * 72 // 4) % 256 == 16
    r = _check("graph", B72, 72, 72, graph72[0], _state(B72, 16, 72, 72, dev, 31))
    alive = O.alive_mask(r[:4].cpu().numpy(), 0.12)
    assert 0 < alive.mean() < 1 or alive.all()      # a live state came out (not all gated to zero)


def test_classic_plan(dev):
    """The classic large-batch plan (KU = 0: gnca_k1_split<24,36,1,4,0>) at B=192 x 72^2."""
    from graph_neural_cellular_automata_amd import step as S
    w, keep = _fixture_weights("classic_ep980_b2_32", False, dev)
    assert S.k1_variant(LC.make_desc(LC.MODELS["classic"], B72, 72, 72))[0] == "gnca_k1_split<24,36,1,4,0>"
    _check("classic", B72, 72, 72, w, _state(B72, 16, 72, 72, dev, 32))
    del keep


def test_without_groupnorm(dev):
    """use_groupnorm off (graph_nogn, threshold 0.1): the flat kernel reads neither the partials nor the
    affine parameters, as the band kernel."""
    m = LC.MODELS["graph_nogn"]
    w, keep = _lc_weights(m, 4, dev)
    _check("graph_nogn", B72, 72, 72, w, _state(B72, 16, 72, 72, dev, 34))
    del keep


# (B, H, W, vectors per sample, tile columns): 768 vectors = 3 full workgroups; one tile column and a single
# partial workgroup; 20-cell tile columns (5 vectors per tile row)
CANVASES = [(128, 64, 48, 768, 2), (256, 32, 24, 192, 1), (128, 40, 40, 400, 2)]


@pytest.mark.parametrize("B,H,W,nv,txn", CANVASES, ids=lambda v: str(v))
def test_other_canvases(dev, B, H, W, nv, txn):
    from graph_neural_cellular_automata_amd import step as S
    m = LC.MODELS["graph"]
    d = LC.make_desc(m, B, H, W)
    # all three are in the support set and plan the sub-batch pipeline (tests/test_k2_variant_cpu.py)
    k1 = S.k1_variant(d)[0]
    tile = LC.k1_tile(k1)
    assert tile is not None and S.rollout_compact(d) and S.rollout_subs(d) == 2, (B, H, W, k1)
    assert H * W // 4 == nv and -(-W // tile[1]) == txn, (k1, tile)
    w, keep = _lc_weights(m, 3, dev)
    _check("graph", B, H, W, w, _state(B, 16, H, W, dev, 33 + H))
    del keep


def _alpha(kind, dev):
    """Alpha planes [B72, 72, 72] whose values are 0 or in [0.5, 1]: at least 0.38 from the threshold
    0.12 (the graph threshold is the same), so the structure is in the masks, not in ties."""
    a = torch.zeros(B72, 72, 72, device=dev)
    if kind == "dead":
        return a
    if kind == "alive":
        g = torch.Generator(device=dev).manual_seed(7)
        return 0.5 + 0.5 * torch.rand(B72, 72, 72, device=dev, generator=g)
    if kind == "singles":            # one live cell per sample, on corners, edges and tile seams
        for b in range(B72):
            i, j = SEAMS[b % len(SEAMS)]
            a[b, i, j] = 1.0
        return a
    assert kind == "blocks"          # a live block per sample whose edges cut vectors and tiles unevenly
    for b in range(B72):
        i0, j0 = 3 + b % 17, 1 + b % 13
        a[b, i0:i0 + 30 + b % 9, j0:j0 + 33 + b % 7] = 0.9
    return a


@pytest.mark.parametrize("kind", ["dead", "alive", "singles", "blocks"])
def test_edge_states(dev, graph72, kind):
    """B=192 x 72^2: every sample dead; every cell alive; single live cells on image corners, edges and
    the tile seams at rows 23/24 and columns 35/36; live blocks under the hashed fire mask (rate 0.5),
    whose live rows hold vectors with 0, 1 and 4 live cells."""
    alpha = _alpha(kind, dev)
    assert float((alpha - 0.12).abs().min()) >= 1e-3
    if kind == "blocks":     # sample 0, step 0: the vectors' live-cell counts (live = fired and pre-alive)
        pre = LC.pooled(alpha[0].cpu().numpy()[None, None])[0, 0] > 0.12
        live = pre & (O.hash_fire_mask(5, 0, 0, 1, 72, 72, 0.5)[0, 0] > 0)
        counts = live.reshape(72, 18, 4).sum(-1)[live.any(1)]
        assert {0, 1, 4} <= set(counts.ravel().tolist())
    r = _check("graph", B72, 72, 72, graph72[0], _state(B72, 16, 72, 72, dev, 41, alpha=alpha),
               fire=1.0 if kind in ("alive", "singles") else 0.5)
    if kind == "dead":       # nothing is alive: the gate zeroes alpha, nothing else moves
        assert float(r[:, 3].abs().max()) == 0.0
