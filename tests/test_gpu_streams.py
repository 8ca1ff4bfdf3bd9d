"""The stream contract of libgnca.so (tests/streams.py): every stream-taking entry point on a side
stream with delayed inputs and through capture and replay, bitwise against its own default-stream
call; two host threads on the shared helper streams; a device that is not current.

Every GPU test before this file passes the null stream, where a launch that forgot its stream
argument, a helper stream forked from the wrong place, a host-side synchronisation or work that runs
eagerly instead of on the caller's stream are all invisible.  The cases here are the smallest shapes
that reach each stream-relevant path: the one-stream rollouts (dense and compact fold, zero-pad), the
two-sub-batch rollout whose second sub-batch runs on a per-device helper stream (``subs == 2``), the
piece chain whose helper stream stays forked between two calls, and the step backward at
``B*H*W >= kSideMinCells`` (gnca_bwd.hip), whose weight-gradient reductions run on a side stream.  No
other test runs that last path, so its default-stream result is also held to the float64 VJP oracle
at the bounds of tests/test_gpu_grad.py.

The tables are importable without a GPU: tests/test_streams_cpu.py checks that they name every
stream-taking entry point of include/gnca.h and reach the plans they are chosen for.  The module API
(``model.rollout``, ``trace``, ``FusedAdam.step``, ``SamplePool.commit``) uploads host values inside the
call: it is outside the capture claim and gets the side-stream leg only.
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from tests import liveness_cases as LC
from tests import streams as ST
from tests.poison import diff, same_bytes

pytestmark = pytest.mark.gpu

G_RT, G_AT = 2e-5, 1e-6      # tests/test_gpu_grad.py: RT, AT of _check

# (STEP_SHAPES family, pattern, how the fire mask is presented, GNCA_ATTENTION, masked step): the row of
# LC.step_cases() with that family and pattern gives the model: s8x24 graph_nogn (torus) / graph_open,
# tiny classic / graph_zp (the runtime-geometry f32 K1; K0 for the zero-padded shift), c32 g32
STEP_CASES = [
    ("s8x24", "half_dead", "hash", True, False),
    ("s8x24", "sparse", "rand", False, True),
    ("tiny", "half_dead", "mask", False, False),
    ("tiny", "sparse", "hash", False, False),
    ("c32", "half_dead", "none", False, False),
]
ACTIVE = ([1, 0, 1, 1], [1, 1, 0, 1])
SIDE_ROW = ("graph_zp", 4, 40, 40, "half_dead")
PERCEIVE_SHAPE = (3, 12, 17, 29)
FIRE_SHAPE = (3, 17, 29)

# PLAN_ROWS rows: dense fold, compact fold, subs = 2 (the fork / join), zero-pad
ROLLOUT_ROWS = [("graph", 8, 48, 72, "sparse"), ("graph", 32, 48, 72, "half_dead"),
                ("graph", 64, 48, 72, "sparse"), ("graph_zp", 128, 48, 72, "half_dead")]
ROLLOUT_STEPS = 4
SUBS2_ROW = ("graph", 64, 48, 72)
DENSE_ROW = ("graph", 8, 48, 72)
# two pieces of gnca_rollout_ex_f32 (2 + 2 steps); the ALIVE chain's helper stream stays forked between them
CHAIN_CASES = [("pending",) + DENSE_ROW, ("alive",) + SUBS2_ROW]
TRACE_EVERY = 3

# the forked step backward: B*H*W >= kSideMinCells = 1 << 19 (101 samples would be 523,584 cells)
FORK_B, FORK_H, FORK_W = 102, 72, 72
FORK_MODELS = {"torus": "graph", "zp": "graph_zp"}
BPTT_MODES = ("tape", "recompute", "notape")
BPTT_STEPS = 3
NSTEPS = ([3, 1], [2, 3])

_SHORT = {"perception.conv.weight": "perception", "update_net.0.weight": "w1", "update_net.0.bias": "b1",
          "update_net.2.weight": "w2", "norm.weight": "gn_weight", "norm.bias": "gn_bias",
          "graph.query_proj.weight": "wq", "graph.query_proj.bias": "bq", "graph.key_proj.weight": "wk",
          "graph.key_proj.bias": "bk", "graph.msg_proj.weight": "wm", "graph.msg_proj.bias": "bm",
          "graph.scaling": "scaling"}

# case id -> dict(build=callable(dev) -> streams.Case, eps=entry points the call runs, forked=None or the
# forked plan it belongs to ("rollout", "chain-trace", "backward"), legs)
CASES: dict = {}


def _register(cid, eps, build, forked=None, legs=ST.LEGS):
    assert cid not in CASES, cid
    CASES[cid] = dict(build=build, eps=tuple(eps), forked=forked, legs=tuple(legs))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------
# Input sets
# ---------------------------------------------------------------------------------------------
def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(dev)


def _wset(m, seed, dev):
    """The model's float32 parameters as inputs ``w.<gnca_weights field>``."""
    return {"w." + _SHORT[k]: _t(v, dev, np.float32) for k, v in LC.params(m, seed).items()}


def _W(b):
    """The weight struct over the buffers' ``w.*`` entries (cached by address: nothing is uploaded)."""
    from graph_neural_cellular_automata_amd import step as S
    return S.make_weights({k[2:]: v for k, v in b.items() if k.startswith("w.")})[0]


def _want(m):
    from graph_neural_cellular_automata_amd import step as S
    return {k: torch.zeros(np.shape(v)) for k, v in LC.params(m, 0).items() if k in S.GRAD_FIELDS}


def _state_sets(m, pat, seeds, B, H, W, tile, dev):
    return [dict({"x": _t(LC.build(pat, s, B, m["C"], H, W, m["thr"], tile).x, dev)}, **_wset(m, s, dev))
            for s in seeds]


def _fire(mode, shape, seed, dev):
    """(fire tensor or None, fire mode, fire rate) of one input set."""
    from graph_neural_cellular_automata_amd import _lib as L
    if mode == "none":
        return None, L.FIRE_NONE, 1.0
    if mode == "hash":
        return None, L.FIRE_HASH, 0.5
    g = np.random.default_rng([17, seed])
    if mode == "mask":
        return _t((g.random(shape) < 0.5).astype(np.uint8), dev), L.FIRE_MASK_U8, 0.5
    return _t(g.random(shape).astype(np.float32), dev), L.FIRE_RAND_F32, 0.5


def _lc_step_case(fam, pat):
    return next(c for c in LC.step_cases() if c["id"].startswith(f"{fam}-{pat}-"))


def _hash_desc(m, B, H, W, seed, t=0, attention=False):
    from graph_neural_cellular_automata_amd import _lib as L
    return LC.make_desc(m, B, H, W, step=t, seed=seed, fire_rate=0.5, fire_mode=L.FIRE_HASH, attention=attention)


def _flat(offs):
    flat = [v for o in offs for pr in o for v in pr]
    return (ctypes.c_int8 * len(flat))(*flat) if flat else None


# ---------------------------------------------------------------------------------------------
# Steps and side computations
# ---------------------------------------------------------------------------------------------
def _step_builder(sc):
    fam, pat, mode, attention, masked = sc

    def build(dev):
        from graph_neural_cellular_automata_amd import step as S
        c = _lc_step_case(fam, pat)
        m, B, H, W = c["m"], c["B"], c["H"], c["W"]
        assert LC.plan_of(m, B, H, W)["k1"].startswith(c["k1"]), c["id"]
        sets = _state_sets(m, pat, (c["seed"], c["seed"] + 1000), B, H, W, c["tile"], dev)
        for i, s in enumerate(sets):
            f, fmode, rate = _fire(mode, (B, 1, H, W), c["seed"] + i, dev)
            if f is not None:
                s["fire"] = f
            if masked:
                s["active"] = torch.tensor(ACTIVE[i], dtype=torch.uint8, device=dev)
        desc = LC.make_desc(m, B, H, W, fire_mode=fmode, fire_rate=rate, seed=c["seed"], attention=attention)

        def call(b):
            out, attn = S.step(desc, _W(b), b["x"], fire=b.get("fire"), want_attention=attention,
                               active=b.get("active"))
            return {"x_out": out} if attn is None else {"x_out": out, "attn": attn}

        return ST.Case(_step_id(sc), sets, call)
    return build


def _step_id(sc):
    return f"step-{sc[0]}-{sc[1]}-{sc[2]}" + "-attn" * sc[3] + "-masked" * sc[4]


for _sc in STEP_CASES:
    _register(_step_id(_sc), ["gnca_step_masked_f32" if _sc[4] else "gnca_step_f32"], _step_builder(_sc))


def _side_sets(dev):
    name, B, H, W, pat = SIDE_ROW
    m = LC.MODELS[name]
    return m, B, H, W, _state_sets(m, pat, (41, 1041), B, H, W, (8, 20), dev)


def _build_message(dev):
    from graph_neural_cellular_automata_amd import step as S
    m, B, H, W, sets = _side_sets(dev)
    desc = LC.make_desc(m, B, H, W, attention=True)

    def call(b):
        msg, attn = S.message(desc, _W(b), b["x"], want_attention=True)
        return {"message": msg, "attn": attn}

    return ST.Case("message", sets, call)


def _build_attention(dev):
    from graph_neural_cellular_automata_amd import step as S
    m, B, H, W, sets = _side_sets(dev)
    desc = LC.make_desc(m, B, H, W)
    return ST.Case("attention", sets, lambda b: {"attn": S.attention_map(desc, _W(b), b["x"])})


def _diag_outs(d, prefix=""):
    from graph_neural_cellular_automata_amd import _lib as L
    return {prefix + n: getattr(d, n) for n in L.DIAG_FIELDS if getattr(d, n) is not None}


def _build_graph_diag(dev):
    from graph_neural_cellular_automata_amd import step as S
    m, B, H, W, sets = _side_sets(dev)
    desc = LC.make_desc(m, B, H, W)
    return ST.Case("graph-diag", sets, lambda b: _diag_outs(S.graph_diagnostics(desc, _W(b), b["x"], per_offset=True)))


def _build_perceive(dev):
    from graph_neural_cellular_automata_amd import step as S
    B, C, H, W = PERCEIVE_SHAPE
    sets = [{"x": _t(np.random.default_rng(5 + i).standard_normal(PERCEIVE_SHAPE), dev, np.float32),
             "weight": _t(O.sobel_weights(C) * (1 + i), dev, np.float32)} for i in (0, 1)]
    return ST.Case("perceive", sets, lambda b: {"y": S.perceive(b["weight"], b["x"])})


def _build_fire_mask(dev):
    """No device input: the two sets are empty, and the legs compare the mask with itself."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    B, H, W = FIRE_SHAPE
    desc = LC.make_desc(LC.MODELS["graph"], B, H, W, fire_mode=L.FIRE_HASH, fire_rate=0.5, seed=7, step=2)
    return ST.Case("fire-mask", ({}, {}), lambda b: {"mask": S.fire_mask(desc, dev)})


_register("message", ["gnca_message_f32"], _build_message)
_register("attention", ["gnca_attention_f32"], _build_attention)
_register("graph-diag", ["gnca_graph_diag"], _build_graph_diag)
_register("perceive", ["gnca_perceive_f32"], _build_perceive)
_register("fire-mask", ["gnca_fire_mask_u8"], _build_fire_mask)


# ---------------------------------------------------------------------------------------------
# Rollouts, piece chains, traces
# ---------------------------------------------------------------------------------------------
def _rollout_setup(name, B, H, W, pat, dev, seed):
    m = LC.MODELS[name]
    plan = LC.check_plan(name, B, H, W)          # fails loudly if the planner moves
    sets = _state_sets(m, pat, (seed, seed + 1000), B, H, W, LC.k1_tile(plan["k1"]), dev)
    offs = [LC.offsets(m, t) for t in range(ROLLOUT_STEPS)]
    return m, plan, sets, offs


def _rollout_id(row):
    return "rollout-" + "-".join(map(str, row[:4]))


def _rollout_builder(row):
    name, B, H, W, pat = row

    def build(dev):
        from graph_neural_cellular_automata_amd import step as S
        m, plan, sets, offs = _rollout_setup(name, B, H, W, pat, dev, 900 + B)
        assert plan["subs"] == (2 if row[:4] == SUBS2_ROW else 1), plan
        desc = _hash_desc(m, B, H, W, 900 + B)
        return ST.Case(_rollout_id(row), sets,
                       lambda b: {"x_final": S.rollout(desc, _W(b), b["x"], ROLLOUT_STEPS, offs)})
    return build


for _row in ROLLOUT_ROWS:
    _register(_rollout_id(_row), ["gnca_rollout_ex_f32"], _rollout_builder(_row),
              forked="rollout" if _row[:4] == SUBS2_ROW else None)


def _build_rollout_plain(dev):
    """gnca_rollout_f32 (= gnca_rollout_ex_f32 with flags 0) through ctypes."""
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd import step as S
    name, B, H, W = DENSE_ROW
    m, plan, sets, offs = _rollout_setup(name, B, H, W, "sparse", dev, 77)
    desc, arr, lib = _hash_desc(m, B, H, W, 77), _flat(offs), L.load()

    def call(b):
        x = b["x"]
        out, scratch, ws = torch.empty_like(x), torch.empty_like(x), S.workspace(desc, x.device)
        L.check(lib.gnca_rollout_f32(ctypes.byref(desc), ctypes.byref(_W(b)), ROLLOUT_STEPS, arr, x.data_ptr(),
                                     out.data_ptr(), scratch.data_ptr(), ws.data_ptr(), ws.numel(),
                                     S.stream_ptr(x.device)), "gnca_rollout_f32")
        return {"x_final": out}

    return ST.Case("rollout-plain-entry", sets, call)


_register("rollout-plain-entry", ["gnca_rollout_f32"], _build_rollout_plain)


def _chain_id(cc):
    return "chain-" + "-".join(map(str, cc))


def _chain_builder(cc):
    kind, name, B, H, W = cc

    def build(dev):
        from graph_neural_cellular_automata_amd import _lib as L
        from graph_neural_cellular_automata_amd import step as S
        seed = 53
        m, plan, sets, offs = _rollout_setup(name, B, H, W, "half_dead", dev, seed)
        assert plan["subs"] == 2 if kind == "alive" else plan["fold"], plan
        fl_out, fl_in = (L.ROLLOUT_ALIVE_OUT, L.ROLLOUT_ALIVE_IN) if kind == "alive" else \
            (L.ROLLOUT_PENDING_OUT, L.ROLLOUT_PENDING_IN)
        lib = L.load()
        pieces = [(_hash_desc(m, B, H, W, seed, s0), n, _flat(offs[s0:s0 + n]), fl)
                  for s0, n, fl in ((0, 2, fl_out), (2, 2, fl_in))]

        def call(b):
            x, w = b["x"], _W(b)
            mid, out, scratch = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            ws = S.workspace(pieces[0][0], x.device)
            for (desc, n, arr, fl), src, dst in zip(pieces, (x, mid), (mid, out)):
                L.check(lib.gnca_rollout_ex_f32(ctypes.byref(desc), ctypes.byref(w), n, arr, src.data_ptr(),
                                                dst.data_ptr(), scratch.data_ptr(), ws.data_ptr(), ws.numel(), fl,
                                                S.stream_ptr(x.device)), "gnca_rollout_ex_f32")
            return {"x_final": out}

        return ST.Case(_chain_id(cc), sets, call)
    return build


for _cc in CHAIN_CASES:
    _register(_chain_id(_cc), ["gnca_rollout_ex_f32"], _chain_builder(_cc),
              forked="chain-trace" if _cc[1:] == SUBS2_ROW else None)


def _trace_builder(cid, row, kind):
    name, B, H, W = row

    def build(dev):
        from graph_neural_cellular_automata_amd import step as S
        seed, T = 31, ROLLOUT_STEPS
        m, plan, sets, offs = _rollout_setup(name, B, H, W, "sparse", dev, seed)
        for i, s in enumerate(sets):
            s["target"] = _t(np.random.default_rng(3 + i).random((4, H, W)), dev, np.float32)
        desc = _hash_desc(m, B, H, W, seed)
        record = S.expand_record(T, TRACE_EVERY)
        assert record == [3, 4]

        def call(b):
            w, x = _W(b), b["x"]
            if kind == "plain":
                out, frm, attn = S.trace(desc, w, x, T, offs, record, 4, want_attention=True)
                return {"x_final": out, "frames": frm, "attn": attn}
            if kind == "metrics":
                out, frm, attn, met = S.trace_metrics(desc, w, x, T, offs, record, 4, b["target"], 0,
                                                      want_attention=True)
                return {"x_final": out, "frames": frm, "attn": attn, "metrics": met}
            out, frm, attn, met, dg = S.trace_diag(desc, w, x, T, offs, record, 4, b["target"], 0,
                                                   want_attention=True, per_offset=True)
            return dict({"x_final": out, "frames": frm, "attn": attn, "metrics": met}, **_diag_outs(dg, "diag."))

        return ST.Case(cid, sets, call)
    return build


_register("trace", ["gnca_rollout_trace_f32"], _trace_builder("trace", DENSE_ROW, "plain"))
_register("trace-metrics", ["gnca_rollout_trace_metrics_f32"], _trace_builder("trace-metrics", DENSE_ROW, "metrics"))
_register("trace-diag", ["gnca_rollout_trace_diag"], _trace_builder("trace-diag", DENSE_ROW, "diag"))
_register("trace-subs2", ["gnca_rollout_trace_f32"], _trace_builder("trace-subs2", SUBS2_ROW, "plain"),
          forked="chain-trace")


# ---------------------------------------------------------------------------------------------
# Step backward; whole-rollout forward and BPTT
# ---------------------------------------------------------------------------------------------
def _bwd_builder(cid, mname, B, H, W, tile, pat, seed, saved=False, active=None):
    def build(dev):
        from graph_neural_cellular_automata_amd import step as S
        m = LC.MODELS[mname]
        sets = _state_sets(m, pat, (seed, seed + 1000), B, H, W, tile, dev)
        host = []
        for i, s in enumerate(sets):
            gy = np.random.default_rng([9, seed + i]).standard_normal((B, m["C"], H, W)).astype(np.float32)
            s["gy"] = _t(gy, dev)
            if active is not None:
                s["active"] = torch.tensor(active[i], dtype=torch.uint8, device=dev)
            host.append(gy)
        desc = _hash_desc(m, B, H, W, seed)
        want = _want(m)

        def call(b):
            w, x, act = _W(b), b["x"], b.get("active")
            outs, ws = {}, None
            if saved:
                ws = S.workspace(desc, x.device)
                outs["x_out"], _ = S.step(desc, w, x, ws=ws, active=act)
            gx, grads = S.step_backward(desc, w, x, b["gy"], want=want, saved=ws, active=act)
            outs["gx"] = gx
            outs.update({"d " + k: v for k, v in grads.items()})
            return outs

        case = ST.Case(cid, sets, call)
        case.desc, case.model, case.seed, case.gy0 = desc, m, seed, host[0]
        return case
    return build


_RUNTIME = next(f for f in LC.BWD_FAMILIES if f[0] == "runtime")
_F8X16 = next(f for f in LC.BWD_FAMILIES if f[0] == "8x16")
_register("bwd-runtime-recompute", ["gnca_step_bwd_f32"],
          _bwd_builder("bwd-runtime-recompute", "graph", *_RUNTIME[1:5], "sparse", 500))
_register("bwd-runtime-saved", ["gnca_step_bwd_f32", "gnca_step_f32"],
          _bwd_builder("bwd-runtime-saved", "graph", *_RUNTIME[1:5], "sparse", 500, saved=True))
_register("bwd-masked", ["gnca_step_bwd_f32", "gnca_step_masked_f32"],
          _bwd_builder("bwd-masked", "graph", *_F8X16[1:5], "half_dead", 505, saved=True,
                       active=([1, 0, 1, 1, 0, 1, 1, 1], [0, 1, 1, 0, 1, 1, 1, 1])))
for _k, _mname in FORK_MODELS.items():
    _register(f"bwd-forked-{_k}", ["gnca_step_bwd_f32"],
              _bwd_builder(f"bwd-forked-{_k}", _mname, FORK_B, FORK_H, FORK_W, (24, 24), "sparse", 540),
              forked="backward")


def _bptt_builder(mode):
    def build(dev):
        from graph_neural_cellular_automata_amd import step as S
        _, B, H, W, tile = _RUNTIME[:5]
        m, T, seed = LC.MODELS["graph"], BPTT_STEPS, 600 + B
        sets = _state_sets(m, "sparse", (seed, seed + 1000), B, H, W, tile, dev)
        for i, s in enumerate(sets):
            s["gy"] = _t(np.random.default_rng(seed + i).standard_normal((B, m["C"], H, W)), dev, np.float32)
            s["nsteps"] = torch.tensor(NSTEPS[i], dtype=torch.int32, device=dev)
        offs = [LC.offsets(m, t) for t in range(T)]
        want = _want(m)

        def call(b):
            w = _W(b)
            sched = S.build_schedule(steps=T, B=B, H=H, W=W, device=b["x"].device, fire_rate=0.5,
                                     message_gain=m["msg"], nsteps=b["nsteps"], min_steps=1, seed=seed,
                                     offsets=offs, recompute=mode == "recompute")
            desc = LC.make_desc(m, B, H, W, fire_mode=sched.fire_mode, fire_rate=0.5, seed=sched.seed)
            rc = S.RolloutCall(desc, sched)
            out, tape = rc.forward(w, b["x"], want_tape=mode != "notape")
            outs = {"x_final": out}
            if tape is not None:       # forward and backward in one call, so in one captured graph
                gx, grads = rc.backward(w, tape, b["gy"], want=want)
                outs["gx"] = gx
                outs.update({"d " + k: v for k, v in grads.items()})
            return outs

        return ST.Case(f"bptt-{mode}", sets, call)
    return build


for _mode in BPTT_MODES:
    _register(f"bptt-{_mode}", ["gnca_rollout_fwd_f32"] + ["gnca_rollout_bwd_f32"] * (_mode != "notape"),
              _bptt_builder(_mode))


# ---------------------------------------------------------------------------------------------
# Losses, metrics, damage, the optimiser step, the pool write-back
# ---------------------------------------------------------------------------------------------
def _loss_sets(dev, B=3, H=9, W=13):
    sets = []
    for i in (0, 1):
        g = np.random.default_rng(11 + i)
        state = g.random((B, 4, H, W)).astype(np.float32)
        target = g.random((B, 4, H, W)).astype(np.float32)
        target[:, 3] = (g.random((B, H, W)) < 0.4) * target[:, 3]        # a target with dead cells
        sets.append({"state": _t(state, dev), "target": _t(target, dev),
                     "g": _t(g.standard_normal(B), dev, np.float32),
                     "close": torch.tensor(([1, 0, 1], [0, 1, 1])[i], dtype=torch.uint8, device=dev)})
    return sets


def _build_loss_premult(dev):
    from graph_neural_cellular_automata_amd.loss import loss_premult_rgba

    def call(b):
        leaf = b["state"].detach().requires_grad_(True)
        per = loss_premult_rgba(leaf, b["target"])
        (grad,) = torch.autograd.grad(per, leaf, b["g"])
        return {"per_sample": per.detach(), "grad": grad}

    return ST.Case("loss-premult", _loss_sets(dev), call)


def _build_loss_masked(dev):
    from graph_neural_cellular_automata_amd.loss import masked_loss

    def call(b):
        leaf = b["state"].detach().requires_grad_(True)
        per, k = masked_loss(leaf, b["target"], 0.2, 5e-5, 1e-3, 2e-4, stability=(0.12, 24))
        (grad,) = torch.autograd.grad(per, leaf, b["g"])
        return {"per_sample": per.detach(), "nsteps": k, "grad": grad}

    return ST.Case("loss-masked", _loss_sets(dev), call)


def _build_loss_stability(dev):
    from graph_neural_cellular_automata_amd.loss import stability_loss

    def call(b):
        leaf = b["state"].detach().requires_grad_(True)
        loss = stability_loss(leaf, b["target"], b["close"])
        (grad,) = torch.autograd.grad(loss, leaf)
        return {"loss": loss.detach(), "grad": grad}

    return ST.Case("loss-stability", _loss_sets(dev), call)


def _build_image_metrics(dev):
    from graph_neural_cellular_automata_amd.metrics import image_metrics
    return ST.Case("image-metrics", _loss_sets(dev),
                   lambda b: {"metrics": image_metrics(b["state"], b["target"]).stacked})


def _damage_builder(kind):
    def build(dev):
        from graph_neural_cellular_automata_amd import _lib as L
        from graph_neural_cellular_automata_amd.damage import _launch
        B, C, H, W = 3, 8, 9, 13
        sets = []
        for i in (0, 1):
            g = np.random.default_rng(21 + i)
            s = {"state": _t(g.random((B, C, H, W)), dev, np.float32)}
            if kind == "square":
                s["pos"] = _t(np.stack([g.integers(0, H - 3, B), g.integers(0, W - 3, B)], 1), dev, np.int32)
            else:
                s["noise"] = _t(g.standard_normal((B, C - 4, H, W)), dev, np.float32)
            sets.append(s)

        def call(b):       # in place: loading a set restores the state
            if kind == "square":
                _launch(b["state"], L.DMG_SQUARE, 4, pos=b["pos"])
            else:
                _launch(b["state"], L.DMG_HIDDEN_NOISE, noise=b["noise"], sigma=0.2)
            return {"state": b["state"]}

        return ST.Case(f"damage-{kind}", sets, call)
    return build


OPTIM_SHAPES = [(5, 7), (16,), (4099,)]


def _optim_sets(dev):
    sets = []
    for i in (0, 1):
        g = torch.Generator().manual_seed(31 + i)
        s = {}
        for j, shp in enumerate(OPTIM_SHAPES):
            s[f"p{j}"] = torch.randn(shp, generator=g).to(dev)
            s[f"g{j}"] = torch.randn(shp, generator=g).to(dev)
            s[f"m{j}"] = (0.1 * torch.randn(shp, generator=g)).to(dev)
            s[f"v{j}"] = (torch.randn(shp, generator=g) ** 2).to(dev)
        sets.append(s)
    return sets


def _optim_builder(form):
    def build(dev):
        from graph_neural_cellular_automata_amd import _lib as L
        lib, n = L.load(), len(OPTIM_SHAPES)

        def call(b):       # in place on p / m / v: loading a set restores them
            d = L.OptimDesc()
            d.policy = L.OPTIM_POLICY_NORMALIZE if form == "one-launch" else L.OPTIM_POLICY_CLIP
            d.num_tensors, d.flags, d.sumsq_base = n, 0, 0
            d.beta1, d.beta2, d.eps, d.max_norm, d.norm_eps = 0.9, 0.999, 1e-3, 0.5, 1e-8
            ws = None
            if form == "sumsq":      # flags 0 with a sumsq workspace: both launches
                ws = torch.empty(n, dtype=torch.float64, device=b["p0"].device)
                d.sumsq, d.sumsq_count = ws.data_ptr(), n
            for j in range(n):
                e = d.t[j]
                e.p, e.g, e.m, e.v = (b[f"{q}{j}"].data_ptr() for q in "pgmv")
                e.numel, e.lr, e.weight_decay = b[f"p{j}"].numel(), 1e-2, 0.1
                e.bias1, e.bias2 = 1.0 - 0.9 ** 3, 1.0 - 0.999 ** 3
            from graph_neural_cellular_automata_amd.step import stream_ptr
            L.check(lib.gnca_optim_step(ctypes.byref(d), stream_ptr(b["p0"].device)), "gnca_optim_step")
            return {f"{q}{j}": b[f"{q}{j}"] for j in range(n) for q in "pmv"}

        return ST.Case(f"optim-{form}", _optim_sets(dev), call)
    return build


POOL_SHAPE = (7, 5, 5, 3, 7)       # P, B, C, H, W (tests/test_gpu_pool_commit.py: tiny)


def _pool_sets(dev):
    P, B, C, H, W = POOL_SHAPE
    sets = []
    for i in (0, 1):
        g = torch.Generator().manual_seed(41 + i)
        sets.append({"pool": torch.randn(P, C, H, W, generator=g).to(dev),
                     "slots": torch.tensor(([0, 2, 3, 5, 6], [6, 1, 4, 0, 2])[i], dtype=torch.int64, device=dev),
                     "state": torch.randn(B, C, H, W, generator=g).to(dev),
                     "per": ((torch.randperm(B, generator=g).float() + 1.0) * 0.037).to(dev),
                     "seeds": torch.randn(2, C, H, W, generator=g).to(dev),
                     "seed1": torch.randn(1, C, H, W, generator=g).to(dev),
                     "rand_idx": torch.tensor([(3, 0)[i]], dtype=torch.int64, device=dev)})
    return sets


def _build_pool_commit(dev):
    from graph_neural_cellular_automata_amd import _lib as L
    from graph_neural_cellular_automata_amd.step import stream_ptr
    P, B, C, H, W = POOL_SHAPE
    lib = L.load()
    d = L.PoolCommitDesc()
    d.pool_slots, d.sample_elems, d.B, d.n_reset = P, C * H * W, B, 2       # worst-2 reset and a reseed

    def call(b):       # in place on the pool: loading a set restores it
        L.check(lib.gnca_pool_commit(ctypes.byref(d), b["pool"].data_ptr(), b["slots"].data_ptr(),
                                     b["state"].data_ptr(), b["per"].data_ptr(), b["seeds"].data_ptr(),
                                     b["seed1"].data_ptr(), b["rand_idx"].data_ptr(),
                                     stream_ptr(b["pool"].device)), "gnca_pool_commit")
        return {"pool": b["pool"]}

    return ST.Case("pool-commit", _pool_sets(dev), call)


_register("loss-premult", ["gnca_loss_premult_f32", "gnca_loss_premult_bwd_f32"], _build_loss_premult)
_register("loss-masked", ["gnca_loss_masked_f32", "gnca_loss_masked_bwd_f32"], _build_loss_masked)
_register("loss-stability", ["gnca_loss_stability_f32", "gnca_loss_stability_bwd_f32"], _build_loss_stability)
_register("image-metrics", ["gnca_image_metrics_f32"], _build_image_metrics)
_register("damage-square", ["gnca_damage_f32"], _damage_builder("square"))
_register("damage-hidden-noise", ["gnca_damage_f32"], _damage_builder("hidden-noise"))
_register("optim-one-launch", ["gnca_optim_step"], _optim_builder("one-launch"))
_register("optim-sumsq", ["gnca_optim_step"], _optim_builder("sumsq"))
_register("pool-commit", ["gnca_pool_commit"], _build_pool_commit)


# ---------------------------------------------------------------------------------------------
# The module API: host values are uploaded inside the call, so the side-stream leg only
# ---------------------------------------------------------------------------------------------
SIDE_ONLY = ("eager", "side")


def _module_builder(api):
    def build(dev):
        from tests.test_gpu_liveness import _module
        c = LC.E_CASES["bptt"]
        m = LC.MODELS[c["mname"]]
        B, H, W, seed, T = c["B"], c["H"], c["W"], c["seed"], c["steps"]
        model = _module(m, LC.params(m, seed), dev)
        sets = [{"x": _t(LC.build("sparse", s, B, m["C"], H, W, m["thr"], c["tile"]).x, dev),
                 "gy": _t(np.random.default_rng(s).standard_normal((B, m["C"], H, W)), dev, np.float32)}
                for s in (seed, seed + 1000)]
        offs = [LC.offsets(m, t) for t in range(T)]

        def call(b):
            if api == "trace":
                r = model.trace(b["x"], T, every=1, channels=4, return_attention=True, fire_rate=0.5, seed=seed,
                                offsets=offs)
                return {"x_final": r.x_final, "frames": r.frames, "attn": r.attention}
            model.zero_grad(set_to_none=True)
            leaf = b["x"].detach().requires_grad_(True)
            out = model.rollout(leaf, T, fire_rate=0.5, seed=seed, offsets=offs)
            out.backward(b["gy"])
            outs = {"out": out.detach(), "gx": leaf.grad}
            outs.update({"d " + n: q.grad for n, q in model.named_parameters() if q.grad is not None})
            return outs

        return ST.Case(f"module-{api}", sets, call)
    return build


def _build_module_adam(dev):
    from graph_neural_cellular_automata_amd.optim import FusedAdam
    n = len(OPTIM_SHAPES)
    box = {}

    def call(b):       # (the parameters ARE the buffers; the state is reset to step 2 with the buffers' moments)
        if "opt" not in box:
            box["params"] = [torch.nn.Parameter(b[f"p{j}"]) for j in range(n)]
            box["opt"] = FusedAdam(box["params"], lr=1e-2, weight_decay=0.1, eps=1e-3, grad_policy="normalize")
        opt = box["opt"]
        for j, p in enumerate(box["params"]):
            assert p.data_ptr() == b[f"p{j}"].data_ptr()
            p.grad = b[f"g{j}"]
            opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": b[f"m{j}"], "exp_avg_sq": b[f"v{j}"]}
        opt.step()
        return {f"{q}{j}": b[f"{q}{j}"] for j in range(n) for q in "pmv"}

    return ST.Case("module-adam", _optim_sets(dev), call)


def _build_module_pool(dev):
    from graph_neural_cellular_automata_amd.pool import SamplePool
    P, B, C, H, W = POOL_SHAPE
    pool = SamplePool(P, lambda batch_size=1: torch.zeros(batch_size, C, H, W), device=dev)
    idx = [0, 2, 3, 5, 6]
    sets = [{k: v for k, v in s.items() if k in ("pool", "state", "per", "seeds")} for s in _pool_sets(dev)]

    def call(b):
        pool.states = b["pool"]
        pool.commit(idx, b["state"], b["per"], n_reset=2, seed_fn=lambda n: b["seeds"][:n])
        return {"pool": b["pool"]}

    return ST.Case("module-pool-commit", sets, call)


_register("module-rollout", [], _module_builder("rollout"), legs=SIDE_ONLY)
_register("module-trace", [], _module_builder("trace"), legs=SIDE_ONLY)
_register("module-adam", [], _build_module_adam, legs=SIDE_ONLY)
_register("module-pool-commit", [], _build_module_pool, legs=SIDE_ONLY)


# ---------------------------------------------------------------------------------------------
# What the gate reads (tests/test_streams_cpu.py)
# ---------------------------------------------------------------------------------------------
PLAIN_IDS = [k for k, v in CASES.items() if v["forked"] is None and v["legs"] == ST.LEGS]
FORKED_IDS = [k for k, v in CASES.items() if v["forked"] is not None]
MODULE_IDS = [k for k, v in CASES.items() if v["legs"] == SIDE_ONLY]
_FORKED_CAPTURE = {"rollout": "test_forked_rollout_capture", "chain-trace": "test_forked_chain_and_trace_capture",
                   "backward": "test_forked_backward_capture"}


def _covered():
    cov = {}
    for cid, v in CASES.items():
        tests = ["test_streams"] if v["forked"] is None else ["test_forked_side_stream", _FORKED_CAPTURE[v["forked"]]]
        for ep in v["eps"]:
            cov.setdefault(ep, set()).update(tests)
    return {ep: ", ".join(sorted(t)) for ep, t in cov.items()}


# entry point -> the tests here that run it on all three legs
COVERED = _covered()

_BUILT: dict = {}


def _get(cid, dev):
    """The built case; the forked ones are kept (their eager results serve several tests)."""
    if cid in _BUILT:
        return _BUILT[cid]
    case = CASES[cid]["build"](dev)
    assert case.id == cid, (case.id, cid)
    if CASES[cid]["forked"] is not None:
        _BUILT[cid] = case
    return case


# ---------------------------------------------------------------------------------------------
# The helper, on torch ops only (preallocated buffers, out= forms)
# ---------------------------------------------------------------------------------------------
def _torch_case(dev, plant=None):
    """y = 2 a + b and z = 3 a.  ``plant``: "default" computes 2 a on the default stream whatever stream
    is current; "other" computes z on a side stream of its own that nothing waits for."""
    g = torch.Generator().manual_seed(1)
    sets = [{"a": torch.randn(1 << 16, generator=g).to(dev), "b": torch.randn(1 << 16, generator=g).to(dev)}
            for _ in (0, 1)]
    t, y, z = (torch.empty(1 << 16, device=dev) for _ in range(3))
    other = torch.cuda.Stream()

    def call(b):
        if plant == "default":
            with torch.cuda.stream(torch.cuda.default_stream()):
                torch.mul(b["a"], 2.0, out=t)
        else:
            torch.mul(b["a"], 2.0, out=t)
        torch.add(t, b["b"], out=y)
        if plant == "other":
            with torch.cuda.stream(other):
                torch.mul(b["a"], 3.0, out=z)
        else:
            torch.mul(b["a"], 3.0, out=z)
        return {"y": y, "z": z}

    return ST.Case(f"torch-{plant}", sets, call)


def test_helper_passes_a_stream_ordered_call(dev):
    case = _torch_case(dev)
    ST.run(case)
    want, ms = case.eager
    assert torch.equal(want[0]["y"], 2.0 * case.sets[0]["a"] + case.sets[0]["b"])
    assert torch.equal(want[1]["z"], 3.0 * case.sets[1]["a"]) and not same_bytes(want[0]["y"], want[1]["y"])
    assert ST.delay_ms(ms) >= ST.MIN_DELAY_MS and ST.delay_ms(100.0) == 1000.0


def test_helper_catches_work_on_the_default_stream(dev):
    """Part of the work under ``torch.cuda.stream(torch.cuda.default_stream())``: it reads the poison
    while the side stream still sleeps.  (Eager and side-stream legs only: no legacy-stream launch
    inside a capture.)"""
    case = _torch_case(dev, plant="default")
    ST.run(case, legs=("eager",))
    with pytest.raises(AssertionError, match=r"side-stream leg differs .* output 'y'"):
        ST.run_side(case)
    torch.cuda.synchronize()


def test_helper_catches_work_outside_the_capture(dev):
    """One output computed on another, non-capturing stream: it ran once while capturing, on poison,
    and no replay computes it again."""
    case = _torch_case(dev, plant="other")
    ST.run(case, legs=("eager",))
    with pytest.raises(AssertionError, match=r"replay of the captured call differs .* output 'z'"):
        ST.run_capture(case)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# Every entry point, all three legs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", PLAIN_IDS)
def test_streams(dev, cid):
    ST.run(_get(cid, dev))


@pytest.mark.parametrize("cid", MODULE_IDS)
def test_module_api_side_stream(dev, cid):
    ST.run(_get(cid, dev), legs=SIDE_ONLY)


# the forked plans: eager and side-stream legs here, each capture leg (a graph with parallel
# branches) in a test of its own
@pytest.mark.parametrize("cid", FORKED_IDS)
def test_forked_side_stream(dev, cid):
    case = _get(cid, dev)
    if CASES[cid]["forked"] == "backward":
        assert FORK_B * FORK_H * FORK_W >= 1 << 19 > (FORK_B - 1) * FORK_H * FORK_W
    ST.run(case, legs=SIDE_ONLY)


def _capture_after_warm_up(case):
    if not getattr(case, "warm", False):     # the side-stream leg creates the helper streams and events
        ST.run(case, legs=SIDE_ONLY)
        case.warm = True
    ST.run_capture(case)


def test_forked_rollout_capture(dev):
    _capture_after_warm_up(_get(_rollout_id(SUBS2_ROW), dev))


@pytest.mark.parametrize("cid", [k for k in FORKED_IDS if CASES[k]["forked"] == "chain-trace"])
def test_forked_chain_and_trace_capture(dev, cid):
    _capture_after_warm_up(_get(cid, dev))


@pytest.mark.parametrize("kind", list(FORK_MODELS))
def test_forked_backward_capture(dev, kind):
    _capture_after_warm_up(_get(f"bwd-forked-{kind}", dev))


@pytest.mark.parametrize("kind", list(FORK_MODELS))
def test_forked_backward_matches_oracle(dev, kind):
    """The default-stream result of the forked backward against the float64 VJP oracle, at the bounds of
    tests/test_gpu_grad.py::_check (max |hip - f64| <= 2e-5 max |f64| + 1e-6 per tensor), as
    test_module_backward_72_batch_matches_oracle holds B = 96."""
    from oracle import nca_oracle_vjp as V
    case = _get(f"bwd-forked-{kind}", dev)
    B, H, W = FORK_B, FORK_H, FORK_W
    assert B * H * W >= 1 << 19
    m, seed = case.model, case.seed
    got = ST.run_eager(case)[0][0]
    x64 = LC.build("sparse", seed, B, m["C"], H, W, m["thr"], (24, 24)).x.astype(np.float64)
    fire = np.concatenate([O.hash_fire_mask(seed, 0, b, 1, H, W, 0.5) for b in range(B)])
    rgx, rgr = V.nca_step_vjp(x64, LC.f64(LC.params(m, seed)), LC.oracle_cfg(m), case.gy0.astype(np.float64),
                              chosen=LC.offsets(m), fire_mask=fire)
    ref = dict({"d " + k: v for k, v in rgr.items()}, gx=rgx)
    for k, v in got.items():       # a parameter the reference leaves without a gradient: nothing but zeros
        assert k in ref or float(v.abs().max()) == 0.0, (case.id, k)
    for k, r in ref.items():
        g = got[k].double().cpu().numpy().reshape(np.shape(r))
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        print(f"[streams] {case.id} {k}: err={err:.3e} scale={scale:.3e}")
        assert np.isfinite(g).all(), (case.id, k)
        assert err <= G_RT * scale + G_AT, (case.id, k, f"err={err:.3e} scale={scale:.3e}")


# ---------------------------------------------------------------------------------------------
# Two host threads on the per-device helper streams; a device that is not current
# ---------------------------------------------------------------------------------------------
def test_two_threads_share_the_helper_streams(dev):
    """Two host threads, each with a stream of its own, start together and each make three calls of the
    subs = 2 rollout and of the forked backward (they share the per-device helper streams and their
    mutexes): every result is bitwise the serial one.  One pass."""
    cases = [_get(_rollout_id(SUBS2_ROW), dev), _get("bwd-forked-torus", dev)]
    want = [ST.run_eager(c)[0] for c in cases]
    torch.cuda.synchronize()
    barrier = threading.Barrier(2, timeout=60)
    got, errors = [[], []], []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                barrier.wait()
                for _ in range(3):
                    for c in cases:      # thread i computes on input set #i
                        got[i].append({k: v.clone() for k, v in c.call(c.sets[i]).items()})
            s.synchronize()
        except BaseException as e:      # noqa: BLE001 (reported by the test below)
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for i in (0, 1):
        assert len(got[i]) == 6
        for j, outs in enumerate(got[i]):
            w = want[j % 2][i]
            for k in w:
                assert same_bytes(outs[k], w[k]), (f"thread {i}, call {j} ({cases[j % 2].id}), output '{k}': "
                                                   + diff(w[k], outs[k]))


def _second_gpu():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    return torch.device("cuda:1")


def test_another_device_than_the_current_one(dev):
    """The current device stays cuda:0; the tensors, the weights and a non-default stream are on cuda:1
    (StreamDeviceGuard's non-null branch and the helper-stream caches keyed by the device)."""
    d1 = _second_gpu()
    for cid in (_step_id(STEP_CASES[0]), _rollout_id(SUBS2_ROW), "bwd-forked-torus"):
        case = _get(cid, dev)
        want = ST.run_eager(case)[0][0]
        ins = {k: v.to(d1) for k, v in case.sets[0].items()}
        torch.cuda.synchronize(d1)
        s1 = torch.cuda.Stream(device=d1)
        with torch.cuda.stream(s1), torch.cuda.device(0):
            assert torch.cuda.current_device() == 0 and torch.cuda.current_stream(d1) == s1
            got = {k: v.clone() for k, v in case.call(ins).items()}
            assert torch.cuda.current_device() == 0
        s1.synchronize()
        assert torch.cuda.current_device() == 0
        for k in want:
            assert got[k].device == d1 and same_bytes(got[k], want[k]), (cid, k, diff(want[k], got[k].to(dev)))


def test_wrong_device_default_stream_is_refused(dev):
    """A cuda:1 tensor on cuda:1's default stream while cuda:0 is current: the null stream names no
    device, so the call is refused before anything is launched."""
    from graph_neural_cellular_automata_amd import step as S
    d1 = _second_gpu()
    assert torch.cuda.current_device() == 0 and torch.cuda.current_stream(d1).cuda_stream == 0
    with pytest.raises(ValueError, match=r"cuda:1 .* current device is cuda:0 .*torch\.cuda\.device\(1\)"):
        S.stream_ptr(d1)
    with pytest.raises(ValueError, match="cuda:1"):
        S.perceive(torch.zeros(4, 3, 1, 3, device=d1), torch.zeros(1, 4, 5, 7, device=d1))
    with torch.cuda.device(1):
        assert S.stream_ptr(d1) == 0
    assert S.stream_ptr(dev) == 0 and torch.cuda.current_device() == 0
