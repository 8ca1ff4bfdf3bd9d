"""Every entry point of libgnca.so on poisoned, guarded buffers (tests/poison.py).

Each case runs one call four times: with every workspace, output, tape and gradient buffer the
wrapper allocates filled with 0x00, 0x00 again, 0xFF and a seeded random byte stream, its inputs
copied into blocks whose slack holds the same fill, and 4096 canary bytes around every buffer.
It asserts that the two 0x00 runs are byte-identical (determinism), that every DEFINED output is
byte-identical across the fills (nothing is read before this call wrote it, every output is
completely written) and that no canary was touched (nothing is written out of bounds).  All
reductions are fixed-order, so bit for bit is the bound.  What gnca.h leaves undefined is not
compared: a rollout's scratch, the workspace after a call, the tape's bytes (only the backward
that reads them is) and gradients whose pointer is NULL.

The states are the sparse ones of tests/liveness_cases.py (``half_dead``, ``sparse``): on an
alive-everywhere state the compact update field is fully written and proves nothing.  The step
cases are rows of ``LC.step_cases()`` (whose threshold margins tests/test_liveness_cases_cpu.py
asserts) and also compare the 0xFF run with the float64 oracle at the parity tolerance of
tests/test_gpu_parity.py, so the poisoned path is anchored to the reference, not only to itself.

The tables below are importable without a GPU: tests/test_poison_cpu.py checks that COVERED
(with its exclusions) names every entry point of include/gnca.h and that the tables reach every
rollout plan row, K1 family and backward family of tests/liveness_cases.py.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests import liveness_cases as LC
from tests import poison as PZ

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-6, 1e-5      # tests/test_gpu_parity.py

# entry point -> the tests here that run it on poisoned buffers
COVERED = {
    "gnca_step_f32": "test_step, test_step_backward (saved=ws), test_module_api",
    "gnca_step_masked_f32": "test_step (masked rows), test_step_backward_masked",
    "gnca_message_f32": "test_message",
    "gnca_perceive_f32": "test_perceive",
    "gnca_attention_f32": "test_attention_map",
    "gnca_fire_mask_u8": "test_fire_mask",
    "gnca_rollout_f32": "test_rollout_plain_entry",
    "gnca_rollout_ex_f32": "test_rollout, test_piece_chain",
    "gnca_rollout_trace_f32": "test_trace (no target), test_module_api",
    "gnca_rollout_trace_metrics_f32": "test_trace (target)",
    "gnca_step_bwd_f32": "test_step_backward, test_step_backward_masked, test_module_api",
    "gnca_rollout_fwd_f32": "test_rollout_fwd_bwd, test_module_api",
    "gnca_rollout_bwd_f32": "test_rollout_fwd_bwd, test_module_api",
    "gnca_image_metrics_f32": "test_image_metrics",
    "gnca_loss_premult_f32": "test_loss_premult",
    "gnca_loss_premult_bwd_f32": "test_loss_premult",
    "gnca_loss_masked_f32": "test_masked_loss",
    "gnca_loss_masked_bwd_f32": "test_masked_loss",
    "gnca_loss_stability_f32": "test_stability_loss",
    "gnca_loss_stability_bwd_f32": "test_stability_loss",
    "gnca_damage_f32": "test_damage",
}

# (STEP_SHAPES family, pattern, how the case's fire mask is presented, GNCA_ATTENTION, masked step)
# the row of LC.step_cases() with that family and pattern gives the model, the seed and the mask:
# s8x24 graph_nogn / graph_open, s24x36 graph_open / classic_nogn, s8x20 classic_nogn /
# graph_zp_open, ragged graph_zp_open / classic, tiny classic / graph_zp, c32 g32 (torus, zero-pad
# and classic; every fire mode; attention; the masked step with active = [1,0,1,1])
STEP_CASES = [
    ("s8x24", "half_dead", "hash", True, False),
    ("s8x24", "sparse", "rand", False, True),
    ("s24x36", "half_dead", "none", False, False),
    ("s24x36", "sparse", "mask", False, False),
    ("s8x20", "half_dead", "mask", False, True),
    ("s8x20", "sparse", "hash", True, False),
    ("ragged", "half_dead", "rand", True, False),
    ("ragged", "sparse", "none", False, False),
    ("tiny", "half_dead", "hash", False, True),
    ("tiny", "sparse", "mask", True, False),
    ("c32", "half_dead", "none", True, False),
    ("c32", "sparse", "rand", False, True),
]
ACTIVE = [1, 0, 1, 1]

# every PLAN_ROWS row with a rollout plan, the state pattern alternating
ROLLOUT_ROWS = [(n, B, H, W, ("half_dead", "sparse")[i % 2])
                for i, (n, B, H, W, plan) in enumerate(r for r in LC.PLAN_ROWS if "compact" in r[4])]
ROLLOUT_STEPS = 4

# trace: one row that folds, one that does not; (every, with target)
TRACE_ROWS = [("graph", 8, 48, 72), ("graph", 8, 40, 40)]
TRACE_MODES = [(1, True), (3, True), (1, False)]
# two-piece chains through one poisoned workspace: hand-over kind, PLAN_ROWS row
CHAIN_CASES = [("alive", "graph", 64, 40, 40), ("alive", "graph_zp", 128, 48, 72),
               ("pending", "graph", 8, 48, 72), ("pending", "graph", 32, 48, 72)]

# step backward: per BWD_FAMILIES row its graph and its classic case, and the runtime shapes
BWD_PATTERNS = ("sparse", "half_dead")
BWD_CASES = [c for c in LC.bwd_cases() if c["pattern"] in BWD_PATTERNS
             and (c["mname"] in ("graph", "classic") or c["id"].split("-")[0] in ("ragged", "tiny"))]
# whole-rollout forward and BPTT: (BWD_FAMILIES row, model, fire)
BPTT_ROWS = [("runtime", "graph", "hash"), ("8x16", "classic", "mask"), ("8x24", "graph", "mask"),
             ("lean", "classic", "hash")]
BPTT_MODES = ("tape", "recompute", "notape")
BPTT_STEPS = 3
NSTEPS = [3, 1, 0, 2]

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


def _t(a, dev, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(dev)


def _dev_params(p, dev):
    return {_SHORT[k]: _t(v, dev, np.float32) for k, v in p.items()}


def _weights(P, wt):
    """The weight struct over guarded copies of the device tensors ``wt`` (and what keeps them alive)."""
    from graph_neural_cellular_automata_amd import step as S
    return S.make_weights({k: P.guard(v) for k, v in wt.items()})


def _want(p):
    from graph_neural_cellular_automata_amd import step as S
    return {k: torch.zeros(np.shape(v)) for k, v in p.items() if k in S.GRAD_FIELDS}


def _present(mode, f64, shape, dev):
    """(fire tensor, fire mode, fire rate): the {0,1} mask ``f64`` [B,1,H,W] (None: every cell fires)
    as GNCA_FIRE_NONE / HASH (the case's own hash draw) / MASK_U8 / RAND_F32 (uniforms on the right
    side of the rate)."""
    from graph_neural_cellular_automata_amd import _lib as L
    if mode == "none":
        assert f64 is None
        return None, L.FIRE_NONE, 1.0
    if mode == "hash":
        assert f64 is not None
        return None, L.FIRE_HASH, 0.5
    mask = np.ones(shape, bool) if f64 is None else np.asarray(f64) != 0
    if mode == "mask":
        return _t(mask.astype(np.uint8), dev), L.FIRE_MASK_U8, 0.5
    return _t(np.where(mask, 0.25, 0.75).astype(np.float32), dev), L.FIRE_RAND_F32, 0.5


def _lc_step_case(fam, pat):
    return next(c for c in LC.step_cases() if c["id"].startswith(f"{fam}-{pat}-"))


def _build(c, samples=None):
    m = c["m"]
    return LC.build(c["pattern"], c["seed"], c["B"], m["C"], c["H"], c["W"], m["thr"], c["tile"], samples=samples)


# ---------------------------------------------------------------------------------------------
# One step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", STEP_CASES, ids=lambda sc: f"{sc[0]}-{sc[1]}-{sc[2]}" + "-attn" * sc[3] + "-masked" * sc[4])
def test_step(dev, sc):
    from graph_neural_cellular_automata_amd import step as S
    fam, pat, mode, attention, masked = sc
    c = _lc_step_case(fam, pat)
    m, B, H, W = c["m"], c["B"], c["H"], c["W"]
    attention = attention and m["graph"]
    plan = LC.plan_of(m, B, H, W)
    msg = (c["id"], sc, plan["k1"])
    assert plan["k1"].startswith(c["k1"]), msg
    assert mode != "hash" or c["fire"] == "hash", msg
    case = _build(c)
    p = LC.params(m, c["seed"])
    wt = _dev_params(p, dev)
    x0 = _t(case.x, dev)
    fire0, fmode, rate = _present(mode, LC.step_fire(c, case), (B, 1, H, W), dev)
    active0 = torch.tensor(ACTIVE, dtype=torch.uint8, device=dev) if masked else None
    assert not masked or B == len(ACTIVE)
    desc = LC.make_desc(m, B, H, W, fire_mode=fmode, fire_rate=rate, seed=c["seed"], attention=attention)

    def call(P):
        w, keep = _weights(P, wt)
        out, attn = S.step(desc, w, P.guard(x0), fire=P.guard(fire0), want_attention=attention,
                           active=P.guard(active0))
        return {"x_out": out} if attn is None else {"x_out": out, "attn": attn}

    outs = PZ.run_fills(call, "step-" + c["id"])
    # the 0xFF run against the float64 oracle, on the compared samples
    smp = c["samples"]
    sub = _build(c, smp)
    x64 = sub.x.astype(np.float64)
    ref, ref_attn = O.nca_step(x64, LC.f64(p), LC.oracle_cfg(m), chosen=LC.offsets(m), fire_mask=LC.step_fire(c, sub),
                               return_attention=True)
    if masked:
        for i, b in enumerate(smp):
            if not ACTIVE[b]:
                ref[i] = x64[i]
    got = outs["x_out"][smp].cpu().numpy()
    print(f"[poison] step {msg}: max|hip(0xFF fill) - f64| = {float(np.abs(got - ref).max()):.3e}")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=str(msg))
    if attention:
        np.testing.assert_allclose(outs["attn"][smp].cpu().numpy(), ref_attn, rtol=0, atol=2e-5, err_msg=str(msg))


# ---------------------------------------------------------------------------------------------
# Side computations
# ---------------------------------------------------------------------------------------------
SIDE_ROWS = [("graph", 4, 40, 40, "sparse"), ("graph_zp", 4, 40, 40, "half_dead"), ("graph_zp_open", 3, 17, 29, "sparse")]


def _side(name, B, H, W, pat, dev, seed=41):
    m = LC.MODELS[name] if H >= 32 else LC.small_model(name, 12, 32)
    tile = (8, 20) if H >= 32 else (4, 8)
    case = LC.build(pat, seed, B, m["C"], H, W, m["thr"], tile)
    return m, _t(case.x, dev), _dev_params(LC.params(m, seed), dev)


@pytest.mark.parametrize("row", SIDE_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_message(dev, row):
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W, pat = row
    m, x0, wt = _side(name, B, H, W, pat, dev)
    desc = LC.make_desc(m, B, H, W, attention=True)

    def call(P):
        w, keep = _weights(P, wt)
        msg, attn = S.message(desc, w, P.guard(x0), want_attention=True)
        return {"message": msg, "attn": attn}

    outs = PZ.run_fills(call, f"message-{row}")
    assert float(outs["message"].abs().max()) > 0


@pytest.mark.parametrize("row", SIDE_ROWS + [("classic", 4, 40, 40, "sparse")], ids=lambda r: "-".join(map(str, r)))
def test_attention_map(dev, row):
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W, pat = row
    m, x0, wt = _side(name, B, H, W, pat, dev)
    desc = LC.make_desc(m, B, H, W)

    def call(P):
        w, keep = _weights(P, wt)
        return {"attn": S.attention_map(desc, w, P.guard(x0))}

    outs = PZ.run_fills(call, f"attention-{row}")
    if m["graph"]:
        assert float(outs["attn"].max()) == 1.0
    else:          # graph off: zeros, written
        assert float(outs["attn"].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(3, 12, 17, 29), (4, 16, 5, 7), (2, 32, 32, 32)], ids=str)
def test_perceive(dev, shape):
    from graph_neural_cellular_automata_amd import step as S
    B, C, H, W = shape
    x0 = _t(np.random.default_rng(5).standard_normal(shape), dev, np.float32)
    w0 = _t(O.sobel_weights(C), dev, np.float32)
    outs = PZ.run_fills(lambda P: {"y": S.perceive(P.guard(w0), P.guard(x0))}, f"perceive-{shape}")
    assert outs["y"].shape == (B, 3 * C, H, W) and torch.equal(outs["y"][:, :C], x0)


@pytest.mark.parametrize("shape", [(3, 17, 29), (4, 5, 7), (2, 48, 72)], ids=str)
def test_fire_mask(dev, shape):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    B, H, W = shape
    desc = LC.make_desc(LC.MODELS["graph"], B, H, W, fire_mode=L.FIRE_HASH, fire_rate=0.5, seed=7, step=2)
    outs = PZ.run_fills(lambda P: {"mask": S.fire_mask(desc, dev)}, f"fire-{shape}")
    ref = np.concatenate([O.hash_fire_mask(7, 2, b, 1, H, W, 0.5) for b in range(B)])
    assert np.array_equal(outs["mask"].cpu().numpy(), ref.astype(np.uint8))


# ---------------------------------------------------------------------------------------------
# Rollouts (gnca_rollout_ex_f32): every plan row
# ---------------------------------------------------------------------------------------------
def _rollout_setup(name, B, H, W, pat, dev, seed):
    m = LC.MODELS[name]
    plan = LC.check_plan(name, B, H, W)          # fails loudly if the planner moves
    case = LC.build(pat, seed, B, m["C"], H, W, m["thr"], LC.k1_tile(plan["k1"]))
    return m, plan, _t(case.x, dev), _dev_params(LC.params(m, seed), dev)


def _hash_desc(m, B, H, W, seed, t=0):
    from graph_neural_cellular_automata_amd import _lib as L
    return LC.make_desc(m, B, H, W, step=t, seed=seed, fire_rate=0.5, fire_mode=L.FIRE_HASH)


@pytest.mark.parametrize("row", ROLLOUT_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_rollout(dev, row):
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W, pat = row
    seed, T = 900 + B, ROLLOUT_STEPS
    m, plan, x0, wt = _rollout_setup(name, B, H, W, pat, dev, seed)
    offs = [LC.offsets(m, t) for t in range(T)]
    desc = _hash_desc(m, B, H, W, seed)
    folds = [False] + ([True] if plan["foldable"] and not plan["fold"] else [])

    def call(P):
        w, keep = _weights(P, wt)
        x = P.guard(x0)
        return {f"x_final(fold={f})": S.rollout(desc, w, x, T, offs, fold=f) for f in folds}

    outs = PZ.run_fills(call, f"rollout-{row}")
    first = outs["x_final(fold=False)"]
    assert not torch.equal(first, x0), (row, plan)
    for k, v in outs.items():        # the fold computes the unfused rollout, bitwise
        assert PZ.same_bytes(v, first), (row, plan, k)


def test_rollout_plain_entry(dev):
    """gnca_rollout_f32 (= gnca_rollout_ex_f32 with flags 0) through ctypes."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W, T, seed = "graph", 8, 48, 72, ROLLOUT_STEPS, 77
    m, plan, x0, wt = _rollout_setup(name, B, H, W, "sparse", dev, seed)
    offs = [LC.offsets(m, t) for t in range(T)]
    desc = _hash_desc(m, B, H, W, seed)
    flat = [v for o in offs for pr in o for v in pr]
    arr = (ctypes.c_int8 * len(flat))(*flat)
    lib = L.load()

    def call(P):
        w, keep = _weights(P, wt)
        x, out, scratch, ws = P.guard(x0), torch.empty_like(x0), torch.empty_like(x0), S.workspace(desc, dev)
        L.check(lib.gnca_rollout_f32(ctypes.byref(desc), ctypes.byref(w), T, arr, x.data_ptr(), out.data_ptr(),
                                     scratch.data_ptr(), ws.data_ptr(), ws.numel(), S.stream_ptr(dev)),
                "gnca_rollout_f32")
        return {"x_final": out}

    outs = PZ.run_fills(call, "rollout_f32")
    w, keep = S.make_weights(wt)
    assert torch.equal(outs["x_final"], S.rollout(desc, w, x0, T, offs))


# ---------------------------------------------------------------------------------------------
# Piece chains: trace (pieces inside one workspace) and explicit two-piece chains
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TRACE_MODES, ids=lambda v: f"every{v[0]}-{'target' if v[1] else 'plain'}")
@pytest.mark.parametrize("row", TRACE_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_trace(dev, row, mode):
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W = row
    every, with_target = mode
    seed, T = 31, ROLLOUT_STEPS
    m, plan, x0, wt = _rollout_setup(name, B, H, W, "sparse", dev, seed)
    offs = [LC.offsets(m, t) for t in range(T)]
    desc = _hash_desc(m, B, H, W, seed)
    record = S.expand_record(T, every)
    tgt0 = _t(np.random.default_rng(3).random((4, H, W)), dev, np.float32)

    def call(P):
        w, keep = _weights(P, wt)
        if with_target:
            out, frm, attn, met = S.trace_metrics(desc, w, P.guard(x0), T, offs, record, 4, P.guard(tgt0), 0,
                                                  want_attention=True)
            return {"x_final": out, "frames": frm, "attn": attn, "metrics": met}
        out, frm, attn = S.trace(desc, w, P.guard(x0), T, offs, record, 4, want_attention=True)
        return {"x_final": out, "frames": frm, "attn": attn}

    outs = PZ.run_fills(call, f"trace-{row}-{mode}")
    w, keep = S.make_weights(wt)
    assert torch.equal(outs["x_final"], S.rollout(desc, w, x0, T, offs)), (row, mode, plan)
    assert torch.equal(outs["frames"][-1], outs["x_final"][:, :4])


@pytest.mark.parametrize("cc", CHAIN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_piece_chain(dev, cc):
    """Two pieces of gnca_rollout_ex_f32 (2 + 2 steps) that hand over through ONE poisoned workspace:
    what the second piece reads of it is what the first wrote, never the fill."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    kind, name, B, H, W = cc
    seed, T = 53, ROLLOUT_STEPS
    m, plan, x0, wt = _rollout_setup(name, B, H, W, "half_dead", dev, seed)
    assert plan["subs"] == 1 and (kind == "alive" or plan["fold"]), plan
    offs = [LC.offsets(m, t) for t in range(T)]
    fl_out, fl_in = (L.ROLLOUT_ALIVE_OUT, L.ROLLOUT_ALIVE_IN) if kind == "alive" else \
        (L.ROLLOUT_PENDING_OUT, L.ROLLOUT_PENDING_IN)
    lib = L.load()

    def call(P):
        w, keep = _weights(P, wt)
        x = P.guard(x0)
        mid, out, scratch = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        ws = S.workspace(_hash_desc(m, B, H, W, seed), dev)
        for s0, n, src, dst, fl in ((0, 2, x, mid, fl_out), (2, 2, mid, out, fl_in)):
            flat = [v for o in offs[s0:s0 + n] for pr in o for v in pr]
            arr = (ctypes.c_int8 * len(flat))(*flat) if flat else None
            L.check(lib.gnca_rollout_ex_f32(ctypes.byref(_hash_desc(m, B, H, W, seed, s0)), ctypes.byref(w), n, arr,
                                            src.data_ptr(), dst.data_ptr(), scratch.data_ptr(), ws.data_ptr(),
                                            ws.numel(), fl, S.stream_ptr(dev)), "gnca_rollout_ex_f32")
        return {"x_final": out}

    outs = PZ.run_fills(call, f"chain-{cc}")
    w, keep = S.make_weights(wt)
    assert torch.equal(outs["x_final"], S.rollout(_hash_desc(m, B, H, W, seed), w, x0, T, offs)), (cc, plan)


# ---------------------------------------------------------------------------------------------
# Step backward
# ---------------------------------------------------------------------------------------------
def _bwd_setup(c, dev):
    m, B, H, W = c["m"], c["B"], c["H"], c["W"]
    case = _build(c)
    p = LC.params(m, c["seed"])
    f64 = LC.step_fire(c, case)
    mode = {"hash": "hash", "mask": "mask", None: "none"}[c["fire"]]
    fire0, fmode, rate = _present(mode, f64, (B, 1, H, W), dev)
    gy0 = _t(np.random.default_rng([9, c["seed"]]).standard_normal(case.x.shape), dev, np.float32)
    desc = LC.make_desc(m, B, H, W, fire_mode=fmode, fire_rate=rate, seed=c["seed"])
    return m, p, _t(case.x, dev), gy0, fire0, desc


def _run_bwd(dev, c, saved, active=None):
    from graph_neural_cellular_automata_amd import step as S
    m, p, x0, gy0, fire0, desc = _bwd_setup(c, dev)
    wt, want = _dev_params(p, dev), _want(p)
    act0 = None if active is None else torch.tensor(active, dtype=torch.uint8, device=dev)

    def call(P):
        w, keep = _weights(P, wt)
        x, fire, act = P.guard(x0), P.guard(fire0), P.guard(act0)
        outs, ws = {}, None
        if saved:
            ws = S.workspace(desc, dev)
            outs["x_out"], _ = S.step(desc, w, x, fire=fire, ws=ws, active=act)
        gx, grads = S.step_backward(desc, w, x, P.guard(gy0), fire=fire, want=want, saved=ws, active=act)
        outs["gx"] = gx
        outs.update({"d " + k: v for k, v in grads.items()})
        return outs

    outs = PZ.run_fills(call, f"bwd-{c['id']}-saved{saved}-{active}")
    assert float(outs["gx"].abs().max()) > 0 and float(outs["d update_net.2.weight"].abs().max()) > 0
    if m["graph"] and not m["zp"]:     # torus: exactly zero, and written as zeros
        for k in ("graph.query_proj.weight", "graph.key_proj.weight", "graph.scaling"):
            assert float(outs["d " + k].abs().max()) == 0.0, (c["id"], k)
    return outs, gy0


@pytest.mark.parametrize("saved", [False, True], ids=["recompute", "saved"])
@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c["id"])
def test_step_backward(dev, c, saved):
    from graph_neural_cellular_automata_amd import step as S
    m, B, H, W = c["m"], c["B"], c["H"], c["W"]
    bb = S.bb_variant(LC.make_desc(m, B, H, W))
    assert bb.endswith(c["bb"]) if c["bb"] == LC.RUNTIME_BB else bb == c["bb"], (c["id"], bb)
    _run_bwd(dev, c, saved)


@pytest.mark.parametrize("saved", [False, True], ids=["recompute", "saved"])
def test_step_backward_masked(dev, saved):
    c = next(c for c in BWD_CASES if c["id"].startswith("8x16-") and c["m"]["graph"])
    active = [1, 0, 1, 1, 0, 1, 1, 1]
    outs, gy0 = _run_bwd(dev, c, saved, active=active)
    for b, a in enumerate(active):      # inactive samples: gx = gy, written
        assert a or torch.equal(outs["gx"][b], gy0[b])


# ---------------------------------------------------------------------------------------------
# Whole-rollout forward and BPTT
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BPTT_MODES)
@pytest.mark.parametrize("row", BPTT_ROWS, ids=lambda r: "-".join(r))
def test_rollout_fwd_bwd(dev, row, mode):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    fam, name, fire = row
    _, B, H, W, tile = next(f for f in LC.BWD_FAMILIES if f[0] == fam)[:5]
    m, T, seed = LC.MODELS[name], BPTT_STEPS, 600 + B
    case = LC.build("sparse", seed, B, m["C"], H, W, m["thr"], tile)
    p = LC.params(m, seed)
    wt, want = _dev_params(p, dev), _want(p)
    x0 = _t(case.x, dev)
    gy0 = _t(np.random.default_rng(seed).standard_normal(case.x.shape), dev, np.float32)
    ns0 = torch.tensor((NSTEPS * B)[:B], dtype=torch.int32, device=dev)
    fire0 = None
    if fire == "mask":
        fire0 = _t(np.stack([np.concatenate([O.hash_fire_mask(seed, t, b, 1, H, W, 0.5) for b in range(B)])
                             for t in range(T)]).astype(np.uint8), dev)
    offs = [LC.offsets(m, t) for t in range(T)] if m["graph"] else None

    def call(P):
        w, keep = _weights(P, wt)
        sched = S.build_schedule(steps=T, B=B, H=H, W=W, device=dev, fire_rate=0.5,
                                 message_gain=m["msg"] if m["graph"] else None, nsteps=P.guard(ns0), min_steps=1,
                                 fire=P.guard(fire0), seed=seed, offsets=offs, recompute=mode == "recompute")
        desc = LC.make_desc(m, B, H, W, fire_mode=sched.fire_mode, fire_rate=0.5, seed=sched.seed)
        rc = S.RolloutCall(desc, sched)
        out, tape = rc.forward(w, P.guard(x0), want_tape=mode != "notape")
        outs = {"x_final": out}
        if tape is not None:
            gx, grads = rc.backward(w, tape, P.guard(gy0), want=want)
            outs["gx"] = gx
            outs.update({"d " + k: v for k, v in grads.items()})
        return outs

    outs = PZ.run_fills(call, f"bptt-{row}-{mode}")
    ns = (NSTEPS * B)[:B]
    for b in range(min(B, 4)):       # full_steps = 1: every sample takes step 0
        assert not torch.equal(outs["x_final"][b], x0[b]), (row, mode, b, ns[b])
    if mode != "notape":
        assert float(outs["d update_net.2.weight"].abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# Losses and metrics (B = 3, 9 x 13, as the loss fixtures)
# ---------------------------------------------------------------------------------------------
def _loss_inputs(dev, B=3, H=9, W=13, seed=11):
    g = np.random.default_rng(seed)
    state = g.random((B, 16, H, W)).astype(np.float32)
    target = g.random((B, 4, H, W)).astype(np.float32)
    target[:, 3] = (g.random((B, H, W)) < 0.4) * target[:, 3]        # a target with dead cells
    return _t(state, dev), _t(target, dev), _t(g.standard_normal(B), dev, np.float32)


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "state-slice"])
def test_loss_premult(dev, strided):
    from graph_neural_cellular_automata_amd.loss import loss_premult_rgba
    state0, tgt0, g0 = _loss_inputs(dev)

    def call(P):
        leaf = P.guard(state0 if strided else state0[:, :4].contiguous()).requires_grad_(True)
        per = loss_premult_rgba(leaf[:, :4] if strided else leaf, P.guard(tgt0))
        per.backward(P.guard(g0))
        return {"per_sample": per, "grad": leaf.grad}

    outs = PZ.run_fills(call, f"premult-{strided}")
    assert float(outs["grad"][:, :4].abs().max()) > 0


@pytest.mark.parametrize("broadcast", [False, True], ids=["per-sample-target", "broadcast-target"])
def test_masked_loss(dev, broadcast):
    from graph_neural_cellular_automata_amd.loss import masked_loss
    state0, tgt0, g0 = _loss_inputs(dev)
    tgt0 = tgt0[0] if broadcast else tgt0

    def call(P):
        leaf = P.guard(state0).requires_grad_(True)
        per, k = masked_loss(leaf[:, :4], P.guard(tgt0), 0.2, 5e-5, 1e-3, 2e-4, stability=(0.12, 24))
        alive = per.grad_fn.saved_tensors[2]
        per.backward(P.guard(g0))
        return {"per_sample": per, "nsteps": k, "alive_count": alive, "grad": leaf.grad}

    outs = PZ.run_fills(call, f"masked-{broadcast}")
    ref = (tgt0.reshape(-1, 4, 9, 13)[:, 3] > 0.2).flatten(1).sum(1).to(torch.int32).expand(3)
    assert torch.equal(outs["alive_count"], ref)
    assert set(outs["nsteps"].tolist()) <= {0, 24}


@pytest.mark.parametrize("close", [[1, 0, 1], [0, 0, 0]], ids=["some-close", "none-close"])
def test_stability_loss(dev, close):
    from graph_neural_cellular_automata_amd.loss import stability_loss
    state0, tgt0, _ = _loss_inputs(dev)
    close0 = torch.tensor(close, dtype=torch.uint8, device=dev)

    def call(P):
        leaf = P.guard(state0[:, :4].contiguous()).requires_grad_(True)
        loss = stability_loss(leaf, P.guard(tgt0), P.guard(close0))
        loss.backward()
        return {"loss": loss, "grad": leaf.grad}

    outs = PZ.run_fills(call, f"stability-{close}")
    for b, c in enumerate(close):        # samples that are not close: zeros, written
        assert (float(outs["grad"][b].abs().max()) > 0) == bool(c), (close, b)
    assert (float(outs["loss"]) > 0) == any(close)


@pytest.mark.parametrize("case", [(9, 13, False), (6, 20, False), (9, 13, True)],
                         ids=["9x13", "6x20-nan-ssim", "9x13-broadcast"])
def test_image_metrics(dev, case):
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    H, W, broadcast = case
    state0, tgt0, _ = _loss_inputs(dev, H=H, W=W)
    tgt0 = tgt0[0] if broadcast else tgt0
    outs = PZ.run_fills(lambda P: {"metrics": image_metrics(P.guard(state0), P.guard(tgt0)).stacked}, f"metrics-{case}")
    assert bool(torch.isnan(outs["metrics"][:, 3]).all()) == (H < 7)
    assert bool(torch.isfinite(outs["metrics"][:, :2]).all())


# ---------------------------------------------------------------------------------------------
# Damage: in place on a guarded state
# ---------------------------------------------------------------------------------------------
def _damage_names():
    from tests.test_damage import NAMES
    return NAMES


@pytest.mark.parametrize("name", _damage_names())
def test_damage(dev, name):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd.damage import _launch
    from tests.test_damage import _load, _oracle
    a, m = _load(name)
    kind = {"square": L.DMG_SQUARE, "circle": L.DMG_CIRCLE, "saltpepper": L.DMG_SALT_PEPPER,
            "hidden_noise": L.DMG_HIDDEN_NOISE, "gaussian": L.DMG_GAUSSIAN}.get(m["kind"])
    if m["kind"] == "stripe":
        kind = L.DMG_STRIPE_H if m["orientation"] == "h" else L.DMG_STRIPE_V
    if m["kind"] == "alpha_drop":
        kind = L.DMG_ALPHA_DROP if m["hard"] else L.DMG_ALPHA_DROP_SOFT
    x0 = _t(a["x_in"], dev, np.float32)
    pos0 = _t(a["pos"], dev, np.int32) if "pos" in a else None
    noise0 = _t(a["noise"], dev, np.float32) if "noise" in a else None

    def call(P):
        x = P.guard(x0, inplace=True)
        _launch(x, kind, m.get("size", 0), pos=P.guard(pos0), noise=P.guard(noise0), p=m.get("p", 0.0),
                alpha_thr=m.get("alpha_thr", 0.1), softness=m.get("softness", 0.35), sigma=m.get("sigma", 0.0))
        return {"state": x}

    outs = PZ.run_fills(call, f"damage-{name}")
    np.testing.assert_allclose(outs["state"].cpu().numpy(), _oracle(a, m), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# Module API through autograd (the flat gradient buffers of modules/_stepper.py)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("api", ["forward", "rollout", "trace"])
def test_module_api(dev, api):
    from tests.test_gpu_liveness import _module
    c = LC.E_CASES["bptt"]
    m = LC.MODELS[c["mname"]]
    B, H, W, seed, T = c["B"], c["H"], c["W"], c["seed"], c["steps"]
    case = LC.build("sparse", seed, B, m["C"], H, W, m["thr"], c["tile"])
    model = _module(m, LC.params(m, seed), dev)
    x0 = _t(case.x, dev)
    gy0 = _t(np.random.default_rng(seed).standard_normal(case.x.shape), dev, np.float32)
    offs = [LC.offsets(m, t) for t in range(T)]

    def call(P):
        model.zero_grad(set_to_none=True)
        if api == "trace":
            r = model.trace(P.guard(x0), T, every=1, channels=4, return_attention=True, fire_rate=0.5, seed=seed,
                            offsets=offs)
            return {"x_final": r.x_final, "frames": r.frames, "attn": r.attention}
        leaf = P.guard(x0).requires_grad_(True)
        if api == "forward":
            random.seed(seed)
            torch.manual_seed(seed)
            out = model(leaf, fire_rate=0.5)
        else:
            out = model.rollout(leaf, T, fire_rate=0.5, seed=seed, offsets=offs)
        out.backward(P.guard(gy0))
        outs = {"out": out, "gx": leaf.grad}
        outs.update({"d " + n: q.grad for n, q in model.named_parameters() if q.grad is not None})
        return outs

    outs = PZ.run_fills(call, f"module-{api}")
    assert api == "trace" or float(outs["d update_net.2.weight"].abs().max()) > 0
