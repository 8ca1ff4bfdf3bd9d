"""CPU-side checks of the classic objective's ABI (gnca_loss_masked_f32 / gnca_loss_stability_f32 and their
backwards): the ctypes mirror of gnca_masked_loss_desc matches the header, the library exports the new
symbols, bad arguments are rejected before any launch, ``masked_loss`` / ``stability_loss`` validate
before the library is touched, and the float64 oracle (tests/loss_ref.py) agrees with the fixtures the
reference trainers' own functions produced (tests/golden/loss/loss_*.npz).  No GPU needed."""
import ctypes
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from tests import loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss")
NEW_SYMBOLS = ("gnca_loss_masked_f32", "gnca_loss_masked_bwd_f32", "gnca_loss_stability_workspace_bytes",
               "gnca_loss_stability_f32", "gnca_loss_stability_bwd_f32")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "loss_*.npz")))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_masked_loss_desc_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.MaskedLossDesc._fields_]
    assert fields == ["B", "H", "W", "alpha_thr", "lam_area", "lam_bg_alpha", "lam_bg_rgb", "close_thresh",
                      "close_steps"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gnca_masked_loss_desc));', 'printf("abi %d\\n", GNCA_ABI_VERSION);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gnca_masked_loss_desc, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.MaskedLossDesc)
    assert int(got["abi"]) == L.ABI_VERSION == 5       # additions only: the version stays
    for f in fields:
        assert int(got[f]) == getattr(L.MaskedLossDesc, f).offset, f


def test_exports_new_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTS
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert hasattr(lib, n)
    assert lib.gnca_abi_version() == 5


def _desc(B=2, H=8, W=8, K=3):
    d = L.MaskedLossDesc()
    d.B, d.H, d.W, d.alpha_thr, d.lam_area, d.close_thresh, d.close_steps = B, H, W, 0.2, 5e-5, 0.01, K
    return ctypes.byref(d)


# (fake, never dereferenced device addresses: every call below must return before any launch)
P, T, O, A, N, G, GP = 4096, 8192, 12288, 16384, 20480, 24576, 28672


def test_masked_loss_rejects_bad_args_without_touching_gpu(lib):
    f = lib.gnca_loss_masked_f32
    assert f(None, P, 256, T, 0, O, A, N, None) == -1
    for bad in (dict(B=0), dict(H=0), dict(W=-3), dict(B=-1)):
        assert f(_desc(**bad), P, 256, T, 0, O, A, N, None) == -1
    assert f(_desc(), None, 256, T, 0, O, A, N, None) == -1
    assert f(_desc(), P, 256, None, 0, O, A, N, None) == -1
    assert f(_desc(), P, 256, T, 0, None, A, N, None) == -1
    assert f(_desc(), P, 256, T, 0, O, None, N, None) == -1
    assert f(_desc(), P, -1, T, 0, O, A, N, None) == -1
    assert f(_desc(), P, 256, T, -256, O, A, N, None) == -1
    assert f(_desc(K=-1), P, 256, T, 0, O, A, N, None) == -1      # a negative K with nsteps_out set
    b = lib.gnca_loss_masked_bwd_f32
    assert b(None, P, 256, T, 0, A, G, GP, 256, None) == -1
    for bad in (dict(B=0), dict(H=-2), dict(W=0)):
        assert b(_desc(**bad), P, 256, T, 0, A, G, GP, 256, None) == -1
    assert b(_desc(), None, 256, T, 0, A, G, GP, 256, None) == -1
    assert b(_desc(), P, 256, None, 0, A, G, GP, 256, None) == -1
    assert b(_desc(), P, 256, T, 0, None, G, GP, 256, None) == -1
    assert b(_desc(), P, 256, T, 0, A, None, GP, 256, None) == -1
    assert b(_desc(), P, 256, T, 0, A, G, None, 256, None) == -1
    assert b(_desc(), P, -4, T, 0, A, G, GP, 256, None) == -1
    assert b(_desc(), P, 256, T, -4, A, G, GP, 256, None) == -1
    assert b(_desc(), P, 256, T, 0, A, G, GP, -256, None) == -1


def test_stability_loss_rejects_bad_args_without_touching_gpu(lib):
    size = lib.gnca_loss_stability_workspace_bytes
    assert size(0) == 0 and size(-4) == 0
    assert size(16) >= 16 * 8 and size(16) % 8 == 0 and size(1024) >= size(16)
    f = lib.gnca_loss_stability_f32
    big = 1 << 40
    C, LO, SC, WS = 32768, 36864, 40960, 45056
    assert f(0, 8, 8, P, 256, T, 0, C, LO, SC, WS, big, None) == -1
    assert f(2, 0, 8, P, 256, T, 0, C, LO, SC, WS, big, None) == -1
    assert f(2, 8, -1, P, 256, T, 0, C, LO, SC, WS, big, None) == -1
    assert f(2, 8, 8, None, 256, T, 0, C, LO, SC, WS, big, None) == -1
    assert f(2, 8, 8, P, 256, None, 0, C, LO, SC, WS, big, None) == -1
    assert f(2, 8, 8, P, 256, T, 0, None, LO, SC, WS, big, None) == -1
    assert f(2, 8, 8, P, 256, T, 0, C, None, SC, WS, big, None) == -1
    assert f(2, 8, 8, P, 256, T, 0, C, LO, None, WS, big, None) == -1
    assert f(2, 8, 8, P, -256, T, 0, C, LO, SC, WS, big, None) == -1
    assert f(2, 8, 8, P, 256, T, -1, C, LO, SC, WS, big, None) == -1
    assert f(2, 8, 8, P, 256, T, 0, C, LO, SC, WS, size(2) - 1, None) == -3
    assert f(2, 8, 8, P, 256, T, 0, C, LO, SC, None, big, None) == -3
    b = lib.gnca_loss_stability_bwd_f32
    assert b(0, 8, 8, P, 256, T, 0, C, SC, G, GP, 256, None) == -1
    assert b(2, -8, 8, P, 256, T, 0, C, SC, G, GP, 256, None) == -1
    assert b(2, 8, 0, P, 256, T, 0, C, SC, G, GP, 256, None) == -1
    assert b(2, 8, 8, None, 256, T, 0, C, SC, G, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, None, 0, C, SC, G, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, T, 0, None, SC, G, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, T, 0, C, None, G, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, T, 0, C, SC, None, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, T, 0, C, SC, G, None, 256, None) == -1
    assert b(2, 8, 8, P, -1, T, 0, C, SC, G, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, T, -1, C, SC, G, GP, 256, None) == -1
    assert b(2, 8, 8, P, 256, T, 0, C, SC, G, GP, -1, None) == -1


# ---- Python: validation before the library is touched ----
def _no_load(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")
    monkeypatch.setattr(L, "load", no_load)


def test_masked_loss_validates_before_loading_the_library(monkeypatch):
    from graph_neural_cellular_automata_amd.loss import masked_loss
    _no_load(monkeypatch)
    p, t = torch.zeros(2, 4, 8, 8), torch.zeros(4, 8, 8)
    for pred, target in ((torch.zeros(2, 3, 8, 8), t), (torch.zeros(4, 8, 8), t), (torch.zeros(2, 16, 8, 8), t),
                         (p, torch.zeros(4, 8, 9)), (p, torch.zeros(3, 8, 8)), (p, torch.zeros(3, 4, 8, 8)),
                         (p, torch.zeros(1, 1, 4, 8, 8)), (p, None), (torch.zeros(0, 4, 8, 8), t),
                         (torch.zeros(2, 4, 0, 8), torch.zeros(4, 0, 8))):
        with pytest.raises(ValueError):
            masked_loss(pred, target)
    for stab in ((0.01,), (0.01, 24, 1), 0.01, "ab", (0.01, -1), (0.01, 2.5), (0.01, True), ("x", 3),
                 (float("nan"), 3), (0.01, None)):
        with pytest.raises(ValueError):
            masked_loss(p, t, stability=stab)
    for kw in (dict(alpha_thr="a"), dict(lam_area=None), dict(lam_bg_alpha=float("inf")), dict(lam_bg_rgb=[1])):
        with pytest.raises(ValueError):
            masked_loss(p, t, **kw)
    # well-formed arguments on the CPU: no CPU path, and still no library
    with pytest.raises(RuntimeError):
        masked_loss(p, t, 0.2, 5e-5, 1e-3, 2e-4, stability=(0.01, 24))


def test_stability_loss_validates_before_loading_the_library(monkeypatch):
    from graph_neural_cellular_automata_amd.loss import stability_loss
    _no_load(monkeypatch)
    p, t = torch.zeros(2, 4, 8, 8), torch.zeros(4, 8, 8)
    ok = torch.zeros(2, dtype=torch.bool)
    for pred, target in ((torch.zeros(2, 3, 8, 8), t), (torch.zeros(4, 8, 8), t), (p, torch.zeros(4, 8, 9)),
                         (p, torch.zeros(3, 4, 8, 8)), (p, None), (torch.zeros(0, 4, 8, 8), t)):
        with pytest.raises(ValueError):
            stability_loss(pred, target, ok)
    for close in (torch.zeros(3, dtype=torch.bool), torch.zeros(2, 1, dtype=torch.bool), torch.zeros((), dtype=torch.bool),
                  torch.zeros(2), torch.zeros(2, dtype=torch.int32), [True, False], None, True):
        with pytest.raises(ValueError):
            stability_loss(p, t, close)
    with pytest.raises(RuntimeError):
        stability_loss(p, t, ok)
    with pytest.raises(RuntimeError):
        stability_loss(p, t, ok.to(torch.uint8))


# ---- the oracle against the reference's own results ----
def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    knobs = (meta["alpha_thr"], meta["lam_area"], meta["lam_bg_alpha"], meta["lam_bg_rgb"])
    return z, meta, knobs


def test_fixtures_present():
    assert len(FIXTURES) >= 3, FIXTURES
    assert "loss_knobs_b3_9x13" in FIXTURES and "loss_config_b3_9x13" in FIXTURES


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference(name):
    z, meta, knobs = _load(name)
    m = LR.masked_loss(z["pred"], z["target"], *knobs, g=z["g"])
    assert z["value_f64"].dtype == np.float64 and z["grad_f64"].dtype == np.float64
    assert z["value_f32"].dtype == np.float32 and z["grad_f32"].dtype == np.float32
    ev, eg = _rel(m.value, z["value_f64"]), _rel(m.grad, z["grad_f64"])
    e32, g32 = _rel(z["value_f32"], m.value), _rel(z["grad_f32"], m.grad)
    print(f"{name}: oracle vs reference f64: value {ev:.2e} grad {eg:.2e}; reference f32 vs oracle: "
          f"value {e32:.2e} grad {g32:.2e}")
    assert np.abs(m.value - z["value_f64"]).max() <= 1e-12 * np.abs(z["value_f64"]).max()
    assert np.abs(m.grad - z["grad_f64"]).max() <= 1e-12 * np.abs(z["grad_f64"]).max()
    assert (np.abs(z["value_f32"] - m.value) <= 1e-6 * np.abs(m.value)).all()
    assert np.allclose(m.value, m.primary + m.bg_alpha + m.bg_rgb + m.area, rtol=1e-15, atol=0)
    sv, sg = LR.stability_loss(z["pred"], z["target"], z["close"], g=meta["stability_g"])
    assert abs(sv - float(z["stab_f64"])) <= 1e-12 * abs(float(z["stab_f64"]))
    assert np.abs(sg - z["stab_grad_f64"]).max() <= 1e-12 * np.abs(z["stab_grad_f64"]).max()
    assert abs(float(z["stab_f32"]) - sv) <= 1e-6 * abs(sv)
    assert not sg[~z["close"]].any()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_inputs_cover_the_edges(name):
    z, meta, knobs = _load(name)
    pred, target, thr = z["pred"], z["target"], np.float32(meta["alpha_thr"])
    assert pred.shape == (3, 4, 9, 13) and pred.min() < 0 and pred.min() >= -0.2 and pred.max() <= 1.2
    alive = LR.alive_mask(target, meta["alpha_thr"])[:, 0]
    counts = alive.reshape(3, -1).sum(1)
    assert 0 in counts and 9 * 13 in counts and ((counts > 0) & (counts < 9 * 13)).any()
    assert np.array_equal(LR.masked_loss(pred, target, *knobs).alive_count, counts)
    at_thr = target[:, 3] == thr
    assert at_thr.any() and not alive[at_thr].any()           # equal to the threshold: dead
    dead_rgb = pred[:, :3][np.broadcast_to(~alive[:, None], (3, 3, 9, 13))]
    assert (dead_rgb == 0).any() and (dead_rgb < 0).any()


def test_oracle_threshold_is_compared_in_float32():
    """A target alpha equal to float32(0.2) is dead; a float64 comparison against 0.2 would call it alive."""
    z, meta, knobs = _load("loss_knobs_b3_9x13")
    target = z["target"]
    at_thr = target[:, 3] == np.float32(0.2)
    assert at_thr.any() and (target[:, 3].astype(np.float64)[at_thr] > 0.2).all()
    assert not LR.alive_mask(target, 0.2)[:, 0][at_thr].any()


def test_oracle_edges():
    rng = np.random.default_rng(0)
    pred = rng.random((2, 4, 5, 6), dtype=np.float32) - np.float32(0.3)
    target = rng.random((2, 4, 5, 6), dtype=np.float32)
    target[0, 3] = 0                                            # nothing alive in sample 0
    pred[0, 0, 0, 0] = 0
    m = LR.masked_loss(pred, target, 0.2, 0.3, 0.7, 0.4)
    assert m.alive_count[0] == 0 and m.primary[0] == 0.0 and np.isfinite(m.value).all()
    # the gradient of a sample with nothing alive: the penalties only (sign(0) = 0)
    hw = 30.0
    assert np.allclose(m.grad[0, 3], (0.7 + 0.3) / hw, rtol=1e-14)
    assert np.allclose(m.grad[0, :3], 0.4 * np.sign(pred[0, :3].astype(np.float64)) / (3 * hw), rtol=1e-14)
    assert m.grad[0, 0, 0, 0] == 0.0
    # stability: nothing close is the skipped term; all close is the plain mean
    v, g = LR.stability_loss(pred, target, [False, False])
    assert v == 0.0 and not g.any()
    v, g = LR.stability_loss(pred, target, [True, True])
    assert abs(v - ((pred.astype(np.float64) - target) ** 2).mean()) <= 1e-15
