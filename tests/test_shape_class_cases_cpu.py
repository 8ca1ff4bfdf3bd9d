"""The shape-class case table (tests/shape_class_cases.py) without a GPU: every case plans the
kernels it names (gnca_k1_variant / gnca_bb_variant are host-only), the cases together plan every
runtime-geometry row of ``kVariants`` and every row of ``kBB``, the support set ends where the
messages say it does, and the float64 oracles agree with the fp32 torch CPU reference at channel
counts that are no multiple of 4 (the oracles themselves had only been checked at multiples).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from oracle.torch_cpu_ref import TorchCpuStep
from tests import shape_class_cases as SC


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_table_shape():
    """B <= 3, canvas <= 24x24; zero-pad / torus, GroupNorm on / off, hidden_only, alive_to_alive and
    both fire rates each on at least two padded-channel cases."""
    for n, c in SC.CASES.items():
        assert 1 <= c["B"] <= 3 and c["H"] <= 24 and c["W"] <= 24, n
        assert c["bb"][2] == -(-c["hidden"] // c["bb"][1]), n
    pg = [SC.CASES[n] for n in SC.PADDED_IDS if SC.CASES[n]["graph"]]
    pa = [SC.CASES[n] for n in SC.PADDED_IDS]
    for key, cases in (("zp", pg), ("hidden_only", pg), ("a2a", pg), ("gn", pa)):
        for v in (True, False):
            assert sum(c[key] == v for c in cases) >= 2, (key, v)
    for rate in (1.0, 0.5):
        assert sum(c["fire_rate"] == rate for c in pa) >= 2, rate
    for group in (SC.ANCHOR_IDS, SC.BPTT_IDS, SC.TRACE_IDS):
        assert set(group) <= set(SC.IDS)


@pytest.mark.parametrize("name", SC.IDS)
def test_planned_kernels(lib, name):
    d = SC.desc(name)
    k1, arith = S.k1_variant(d)
    assert k1.startswith(SC.k1_name(name)) and arith == "f32", (name, k1, arith)
    assert S.bb_variant(d) == SC.bb_name(name), (name, S.bb_variant(d))
    # a message-off step (the rollouts') plans the same K1 and a runtime-geometry BB of the same CP (the
    # same one but for p31, whose smaller halo then lets a 64-unit slice fit LDS)
    off = SC.desc(name, message_gain=0.0)
    assert S.k1_variant(off)[0].startswith(SC.k1_name(name)), name
    assert S.bb_variant(off) == (SC.bb_name(name) if name != "p31" else "gnca_b_mlp<32,64,0,0,0,0,0,-1,0>"), name
    assert lib.gnca_workspace_bytes(ctypes.byref(d)) > 0 and lib.gnca_bwd_workspace_bytes(ctypes.byref(d)) > 0


def test_split_kernels_excluded(lib):
    """p13 (whole 8x24 tiles, 8 offsets within radius 4, hidden 128) and p31 (16x16 tiles, 16 offsets
    within radius 5) are the bf16-split K1s' shapes but for C: the same shapes at C = 16 / 32 do plan
    the split K1 and a compile-time BB instance, so it is the channel count that keeps them off."""
    for name, C, k1 in (("p13", 16, "gnca_k1_split<"), ("p31", 32, "gnca_k1_split32<")):
        full = S.k1_variant(SC.desc(name, C=C))
        assert full[0].startswith(k1) and full[1] == "bf16x6", (name, full)
        assert "split" not in S.k1_variant(SC.desc(name))[0]
    # (the compile-time BB instance needs a batch that fills the chip: planned at B = 64 for C = 16)
    assert S.bb_variant(SC.desc("p13", C=16, B=64)) == "gnca_b_mlp<16,128,1,8,24,4,4,8,0>"
    for B in (2, 64):
        assert S.bb_variant(SC.desc("p13", B=B)) == "gnca_b_mlp<16,128,0,0,0,0,0,-1,0>"


def test_cases_cover_both_kernel_tables():
    """A condition, not a measurement: a row added to kVariants or kBB without a case fails here."""
    assert {SC.CASES[n]["k1"] for n in SC.IDS} == SC.K1_ROWS and len(SC.K1_ROWS) == 17
    assert {SC.CASES[n]["bb"][:2] for n in SC.IDS} == SC.BB_ROWS and len(SC.BB_ROWS) == 17
    src = os.path.join(os.path.dirname(L.LIB_PATH), "csrc")
    step = open(os.path.join(src, "gnca_step.hip")).read()
    bwd = open(os.path.join(src, "gnca_bwd.hip")).read()
    rows = lambda text, macro: {(int(a), int(b)) for a, b in re.findall(macro + r"\((\d+), (\d+)\)", text)}
    assert rows(step, "GNCA_GV") == SC.K1_ROWS
    assert rows(bwd, "GNCA_BV") == SC.BB_ROWS


@pytest.mark.parametrize("C,hidden", SC.UNSUPPORTED)
def test_support_set_boundary(lib, C, hidden):
    d = SC.bare_desc(C, hidden)
    assert lib.gnca_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.gnca_bwd_workspace_bytes(ctypes.byref(d)) == 0
    # one step inside: supported
    inside = SC.bare_desc(min(C, 32), {257: 256, 129: 128}.get(hidden, hidden))
    assert lib.gnca_workspace_bytes(ctypes.byref(inside)) > 0 and lib.gnca_bwd_workspace_bytes(ctypes.byref(inside)) > 0


def test_support_set_messages(lib):
    """The status string and the Python layer's messages state the real support set."""
    msg = lib.gnca_status_string(-2).decode()      # GNCA_ERR_UNSUPPORTED
    for text in (msg, S.SUPPORT_SET):
        assert "4 <= C <= 32" in text and "hidden <= 128" in text and "13 <= C <= 16" in text, text


# ---------------------------------------------------------------------------------------------
# The float64 oracles against the fp32 torch CPU reference
# ---------------------------------------------------------------------------------------------
def _torch_ref(name, dtype=torch.float32):
    c = SC.CASES[name]
    step = TorchCpuStep(SC.model(name).state_dict(), graph=c["graph"], update_gain=c["gain"], alpha_thr=c["thr"],
                        message_gain=c["msg"], hidden_only=c["hidden_only"], alive_to_alive=c["a2a"],
                        zero_padded_shift=c["zp"], use_groupnorm=c["gn"])
    step.p = {k: v.detach().to(dtype).clone().requires_grad_(k != "perception.conv.weight" and v.is_floating_point())
              for k, v in step.p.items()}
    return step


def _run_torch_ref(name, dtype):
    c = SC.CASES[name]
    step = _torch_ref(name, dtype)
    x = SC.state(name).to(dtype).requires_grad_(True)
    f = SC.fire_mask(name)
    out = step.step(x, chosen=SC.offsets(name)[0] if c["graph"] else None,
                    fire_mask=None if f is None else f.to(dtype))
    (out * SC.cotangent(name).to(dtype)).sum().backward()
    got = {k: v.grad.numpy() for k, v in step.p.items() if v.grad is not None}
    got["gx"] = x.grad.numpy()
    return out.detach().numpy(), got


@pytest.mark.parametrize("name", SC.ANCHOR_IDS)
def test_oracle_matches_torch_cpu_reference(name):
    """One step and its VJP (autograd) on the torch CPU reference against the float64 oracle and its
    hand-written VJP, elementwise at the bound of tests/test_torch_cpu_ref.py (rtol 1e-5, atol 2e-6).

    The step is compared in the reference's own fp32.  A weight gradient is a sum over B * H * W
    cells: in fp32 its rounding reaches a few ulp of the LARGEST entry on every entry (p13,
    update_net.2.weight: 3.7e-6 at a scale of 8.0, in a summation order that depends on the CPU and
    its thread count), which an elementwise bound with atol 2e-6 cannot grant the small entries.  So
    the elementwise bound is asserted on the same reference run in float64, where it tests the
    oracle's VJP and not the reference's rounding, and the fp32 gradients are held to the project's
    bound for an fp32 gradient against float64, 2e-5 * max|ref| + 1e-6 per tensor
    (tests/test_gpu_grad.py)."""
    ref = SC.reference(name)
    want = dict(ref["grads"], gx=ref["gx"])
    out32, got32 = _run_torch_ref(name, torch.float32)
    print(f"[shape classes] {name}: torch fp32 vs f64 oracle: out {float(np.abs(out32 - ref['out']).max()):.3e}")
    np.testing.assert_allclose(out32, ref["out"], rtol=1e-5, atol=2e-6)
    out64, got64 = _run_torch_ref(name, torch.float64)
    np.testing.assert_allclose(out64, ref["out"], rtol=1e-5, atol=2e-6)
    assert set(got32) == set(want) and set(got64) == set(want), (sorted(got32), sorted(want))
    for k, r in want.items():
        g32, g64 = got32[k].reshape(r.shape), got64[k].reshape(r.shape)
        scale, e32, e64 = float(np.abs(r).max()), float(np.abs(g32 - r).max()), float(np.abs(g64 - r).max())
        print(f"[shape classes] {name}: {k}: fp32 err {e32:.3e} f64 err {e64:.3e} scale {scale:.3e}")
        np.testing.assert_allclose(g64, r, rtol=1e-5, atol=2e-6, err_msg=f"{name} {k}")
        assert e32 <= 2e-5 * scale + 1e-6, (name, k, e32, scale)
    assert float(np.abs(want["update_net.2.weight"]).max()) > 0 and float(np.abs(want["gx"]).max()) > 0
