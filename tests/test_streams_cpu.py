"""The gate of tests/test_gpu_streams.py: every stream-taking entry point of include/gnca.h is run on
the three legs of tests/streams.py or excluded with a reason, and the case tables reach the plans
they are chosen for (host-only: the planner needs no GPU).  Also the Python layer's refusal of a
default-stream call for a device that is not current, on stand-ins for ``torch.cuda``.
"""
import os
import re

import pytest
import torch

from tests import liveness_cases as LC
from tests import streams as ST
from tests import test_gpu_streams as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stream-taking entry points that are NOT run on the legs, and why (tests/test_poison_cpu.py)
EXCLUDED = {
    "gnca_rollout_stamped_f32": "measurement only: its launches and streams are gnca_rollout_f32's (one "
                                "rollout_impl), plus a stamp buffer that its contract has the caller zero",
    "gnca_step_phases_f32": "measurement hook: skipping a phase leaves its outputs stale by contract; all phases "
                            "is gnca_step_f32",
}


def _entry_points():
    """Every ``int gnca_*(...)`` declaration whose parameter list holds ``void* stream``."""
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    decls = re.findall(r"^int (gnca_\w+)\(([^;]*)\);", src, re.M)
    return sorted(name for name, params in decls if re.search(r"\bvoid\s*\*\s*stream\b", params))


def _need_lib():
    if not os.path.exists(os.path.join(ROOT, "graph_neural_cellular_automata_amd", "libgnca.so")):
        import __graft_entry__
        __graft_entry__.build()


def test_every_stream_taking_entry_point_is_covered_or_excluded_with_a_reason():
    eps = _entry_points()
    assert len(eps) >= 27, eps
    for name in ("gnca_step_f32", "gnca_fire_mask_u8", "gnca_optim_step", "gnca_pool_commit", "gnca_graph_diag",
                 "gnca_rollout_trace_diag", "gnca_damage_f32"):       # the rule sees the names without _f32 too
        assert name in eps, name
    assert "gnca_k1_variant" not in eps and "gnca_abi_version" not in eps
    for e in eps:
        assert (e in G.COVERED) != (e in EXCLUDED), f"{e}: decide whether tests/test_gpu_streams.py covers it"
    for e, why in list(G.COVERED.items()) + list(EXCLUDED.items()):
        assert e in eps, f"{e} is not a stream-taking entry point of include/gnca.h"
        assert isinstance(why, str) and why.strip()
    for e, tests in G.COVERED.items():      # the tests a covered entry names exist
        names = re.findall(r"test_\w+", tests)
        assert names, e
        for name in names:
            assert callable(getattr(G, name, None)), (e, name)
    # every case of a covered entry point runs all three legs; the module API is outside the capture claim
    for cid, v in G.CASES.items():
        assert (v["legs"] == ST.LEGS) == bool(v["eps"]), cid
        assert v["eps"] or cid.startswith("module-"), cid
    assert sorted(G.MODULE_IDS) == ["module-adam", "module-pool-commit", "module-rollout", "module-trace"]
    assert sorted(G.PLAIN_IDS + G.FORKED_IDS + G.MODULE_IDS) == sorted(G.CASES)


def test_tables_hold_the_stream_relevant_rows():
    assert G.pytestmark.name == "gpu"
    named = {(n, B, H, W) for n, B, H, W, _ in LC.PLAN_ROWS}
    assert {r[:4] for r in G.ROLLOUT_ROWS} <= named and G.SUBS2_ROW in named and G.DENSE_ROW in named
    assert G.SUBS2_ROW in {r[:4] for r in G.ROLLOUT_ROWS}
    # both chain kinds; the ALIVE chain on the subs = 2 row
    assert {c[0] for c in G.CHAIN_CASES} == {"alive", "pending"}
    assert [c[1:] for c in G.CHAIN_CASES if c[0] == "alive"] == [G.SUBS2_ROW]
    # steps: a zero-pad row, a classic row, one with attention, every fire mode, the masked step
    fams = {sc[0] for sc in G.STEP_CASES}
    assert fams == {"s8x24", "tiny", "c32"}
    assert {sc[2] for sc in G.STEP_CASES} == {"none", "rand", "mask", "hash"}
    picked = [(sc, G._lc_step_case(sc[0], sc[1])) for sc in G.STEP_CASES]
    assert any(c["m"]["graph"] and c["m"]["zp"] for sc, c in picked)
    assert any(not c["m"]["graph"] for sc, c in picked)
    assert any(sc[3] and c["m"]["graph"] for sc, c in picked) and any(sc[4] for sc in G.STEP_CASES)
    for sc, c in picked:
        assert not sc[4] or c["B"] == len(G.ACTIVE[0]), sc
        assert (c["B"], c["H"], c["W"]) == {"s8x24": (4, 48, 72), "tiny": (4, 5, 7), "c32": (4, 32, 32)}[sc[0]]
    # the forked backward, torus and zero-padded shift, and what shares its plans' capture tests
    assert set(G.FORK_MODELS.values()) == {"graph", "graph_zp"}
    assert G.FORK_B * G.FORK_H * G.FORK_W >= 1 << 19 > (G.FORK_B - 1) * G.FORK_H * G.FORK_W
    forked = {cid: G.CASES[cid]["forked"] for cid in G.FORKED_IDS}
    assert forked == {"rollout-graph-64-48-72": "rollout", "chain-alive-graph-64-48-72": "chain-trace",
                      "trace-subs2": "chain-trace", "bwd-forked-torus": "backward", "bwd-forked-zp": "backward"}
    assert set(G.BPTT_MODES) == {"tape", "recompute", "notape"}
    for ids in (G.PLAIN_IDS, G.FORKED_IDS, G.MODULE_IDS):
        assert len(ids) == len(set(ids))


def test_planned_rows():
    """Host-only: a subs = 2 row, a compact-fold row, a dense-fold row and a zero-pad row."""
    _need_lib()
    plans = {r[:4]: LC.check_plan(*r[:4]) for r in G.ROLLOUT_ROWS}
    assert plans[G.SUBS2_ROW]["subs"] == 2
    assert [p["subs"] for r, p in plans.items() if r != G.SUBS2_ROW] == [1, 1, 1]
    assert any(p["fold"] and p["compact"] for p in plans.values())
    assert any(p["fold"] and not p["compact"] for p in plans.values())
    assert plans[G.DENSE_ROW]["fold"] and not plans[G.DENSE_ROW]["compact"]
    assert any(LC.MODELS[r[0]]["zp"] for r in plans)
    for kind, *row in G.CHAIN_CASES:
        plan = LC.check_plan(*row)
        assert plan["subs"] == 2 if kind == "alive" else (plan["subs"] == 1 and plan["fold"]), (kind, row, plan)


def test_the_fork_threshold_is_the_one_the_forked_shape_was_chosen_for():
    """A change of kSideMinCells fails here: revisit FORK_B in tests/test_gpu_streams.py with it."""
    src = open(os.path.join(ROOT, "graph_neural_cellular_automata_amd", "csrc", "gnca_bwd.hip")).read()
    assert "kSideMinCells = 1L << 19" in src
    assert "cells < kSideMinCells" in src


def test_delay_is_sized_from_the_eager_duration():
    assert ST.delay_ms(0.0) == ST.MIN_DELAY_MS == 5.0 and ST.delay_ms(0.49) == 5.0
    assert ST.delay_ms(2.0) == 20.0 and ST.DELAY_FACTOR == 10.0
    assert ST.LEGS == ("eager", "side", "capture")


# ---------------------------------------------------------------------------------------------
# step.stream_ptr: the wrong-device default-stream call is refused
# ---------------------------------------------------------------------------------------------
class _FakeStream:
    def __init__(self, ptr):
        self.cuda_stream = ptr


@pytest.mark.parametrize("count,current,ptr,refused", [
    (2, 0, 0, True),          # cuda:1 tensor, cuda:0 current, default stream: would launch on cuda:0
    (2, 1, 0, False),         # inside torch.cuda.device(1)
    (2, 0, 0x5EED, False),    # a stream of cuda:1: it names its device
    (1, 0, 0, False),         # one GPU: nothing to confuse
])
def test_stream_ptr_refuses_the_null_stream_of_a_device_that_is_not_current(monkeypatch, count, current, ptr, refused):
    from graph_neural_cellular_automata_amd import step as S
    monkeypatch.setattr(S, "_MULTI_GPU", None)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: count)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: current)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _FakeStream(ptr))
    target = torch.device("cuda", min(1, count - 1))
    if refused:
        with pytest.raises(ValueError) as e:
            S.stream_ptr(target)
        msg = str(e.value)
        assert "cuda:1" in msg and "current device is cuda:0" in msg
        assert "torch.cuda.device(1)" in msg and "torch.cuda.Stream(1)" in msg
    else:
        assert S.stream_ptr(target) == ptr
    assert S.stream_ptr(torch.device("cuda", current)) == ptr       # the current device: never refused
