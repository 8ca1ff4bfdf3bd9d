"""CPU-side checks of the device damage policy (gnca_damage_policy, damage.DamagePolicy,
damage.regrow_trace): the config parsing against ``apply_damage_policy_``'s reading of the same dicts,
the descriptor mirror against the header, argument errors before any launch, the numpy restatement
tests/damage_policy_ref.py against the statistical conditions (a check of the yardstick), and
``regrow_trace``'s splitting on a stub model.  No GPU needed."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import damage as D
from graph_neural_cellular_automata_amd.metrics import ImageMetrics
from graph_neural_cellular_automata_amd.modules._stepper import TraceResult
from tests import damage_policy_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000     # a well-formed address that is never dereferenced: every call below is rejected or a no-op


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


# ---------------------------------------------------------------------------------------------
# Config parsing: what apply_damage_policy_ reads from the same dict
# ---------------------------------------------------------------------------------------------
CONFIGS = {
    "empty": {},
    "legacy": {"damage_start_epoch": 7, "damage_prob": 0.25, "damage_patch_size": 5},
    "legacy-shadowed": {"damage_start_epoch": 7, "start_epoch": 3, "damage_prob": 0.25, "prob": 0.5,
                        "damage_patch_size": 5, "size_min": 2, "size_max": 4},
    "big-min": {"prob": 1.0, "start_epoch": 0, "size_min": 20},
    "regeneration": {"start_epoch": 0, "prob": 1.0, "per_sample_prob": 1.0, "size_min": 10, "size_max": 20,
                     "kinds": {"square": 1.0, "circle": 2.0, "stripes": 1.0, "alpha_drop": 0.5, "saltpepper": 0.5,
                               "gaussian": 1.0, "hidden_noise": 1.0},
                     "alpha_thr": 0.2, "alpha_dropout_p": 0.3, "stripe_width": 3, "salt_pepper_p": 0.05,
                     "hidden_noise_sigma": 0.15, "gaussian_softness": 0.5},
}


def _old_reading(cfg, monkeypatch):
    """Run ``apply_damage_policy_`` on ``cfg`` with its draws and launchers replaced by recorders."""
    seen = {}

    def choices(names, weights, k):
        seen["table"] = dict(zip(names, weights))
        return [names[0]]

    def randint(lo, hi):
        seen["size"] = (lo, hi)
        return lo

    monkeypatch.setattr(random, "choices", choices)
    monkeypatch.setattr(random, "randint", randint)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.zeros(1))
    first = next(iter(cfg.get("kinds", {"square": 1.0})))
    monkeypatch.setitem(D._KINDS, first if first in D._KINDS else "square",
                        lambda st, n, k: seen.update(knobs=dict(k), n=n))
    state = torch.zeros(1, 6, 8, 8)
    start = None
    for epoch in range(0, 200):
        seen.clear()
        D.apply_damage_policy_(state, cfg, epoch)
        if seen or float(cfg.get("prob", cfg.get("damage_prob", 0.0))) <= 0:
            start = epoch
            break
    return start, dict(seen)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_parsing_matches_the_host_policy(name, monkeypatch):
    cfg = CONFIGS[name]
    p = D.DamagePolicy(cfg, seed=1)
    start, seen = _old_reading(cfg, monkeypatch)
    assert p.prob == float(cfg.get("prob", cfg.get("damage_prob", 0.0)))
    if p.prob <= 0:
        assert not seen                                      # the host policy returns before any draw
        return
    assert start == p.start_epoch
    assert seen["size"] == (p.size_min, p.size_max)
    table = {D.KIND_CODES[k]: w for k, w in seen["table"].items()}
    assert list(table) == p.kinds
    total = sum(table.values())
    assert p.cum == [float(np.float32(c)) for c in np.cumsum(list(table.values()), dtype=np.float64) / total][:-1] + [1.0]
    k = seen["knobs"]
    assert (k["alpha_thr"], k["alpha_dropout_p"], k["salt_pepper_p"], k["hidden_noise_sigma"], k["gaussian_softness"]) \
        == (p.alpha_thr, p.alpha_dropout_p, p.salt_pepper_p, p.hidden_sigma, p.gaussian_softness)
    assert k["stripe_width"] == (p.stripe_width if p.stripe_width > 0 else seen["n"])
    assert p.per_sample_prob == float(cfg.get("per_sample_prob", 1.0))


def test_defaults():
    p = D.DamagePolicy({}, seed=0)
    assert (p.start_epoch, p.prob, p.per_sample_prob, p.size_min, p.size_max) == (100, 0.0, 1.0, 8, 14)
    assert (p.kinds, p.cum, p.stripe_width) == ([L.DMG_SQUARE], [1.0], 0)
    assert D.DamagePolicy({"size_min": 20}, seed=0).size_max == 20     # max(size_min, 14)


def test_unknown_kinds_fall_back_to_the_square_and_zero_weights_are_dropped():
    p = D.DamagePolicy({"kinds": {"circle": 0.0, "melt": 1.0, "square": 1.0, "gaussian": 2.0, "stripes": 0}}, seed=0)
    assert p.kinds == [L.DMG_SQUARE, L.DMG_GAUSSIAN]            # "melt" is the square, merged with it
    assert p.cum == [0.5, 1.0]
    assert D.DamagePolicy.codes(["melt", None, "stripes", "hidden_noise"]).tolist() == [0, -1, 9, 8]
    assert D.KIND_CODES == {"square": 0, "circle": 1, "stripe_h": 2, "stripe_v": 3, "alpha_drop": 4,
                            "alpha_drop_soft": 5, "saltpepper": 6, "gaussian": 7, "hidden_noise": 8, "stripes": 9}
    # a drawn u never picks a kind whose weight is zero, wherever it stands in the table
    kinds, cum = [1, 0, 7, 9], [np.float32(0.0), np.float32(0.5), np.float32(0.5), np.float32(1.0)]
    picked = {PR.pick_kind(np.float32(u), kinds, cum) for u in np.linspace(0, 1, 257)[:-1]}
    assert picked == {0, 9}


def test_constructor_errors():
    for bad in (dict(cfg={}, seed=-1), dict(cfg={}, seed=1 << 64), dict(cfg={}, seed=1.0), dict(cfg={}, seed=True),
                dict(cfg={}, seed=0, scope="rank"), dict(cfg={"size_min": 5, "size_max": 4}, seed=0),
                dict(cfg={"kinds": {"square": -1.0}}, seed=0), dict(cfg={"kinds": {"square": 0.0}}, seed=0),
                dict(cfg={"kinds": {}}, seed=0), dict(cfg={"kinds": {"square": float("nan")}}, seed=0)):
        with pytest.raises(ValueError):
            D.DamagePolicy(**bad)


@pytest.mark.parametrize("size", [-2, 0, 1, 2, 3, 7, 8])
def test_the_radius_rules_are_the_host_policys(size, monkeypatch):
    """circle: size // 2, or 1 when size <= 1; gaussian: max(1, size // 2); square / stripes: size itself
    (no-ops at size <= 0)."""
    got = {}
    monkeypatch.setattr(D, "cutout_circle_", lambda st, r: got.update(circle=r))
    monkeypatch.setattr(D, "gaussian_hole_", lambda st, radius, softness: got.update(gaussian=radius))
    D._KINDS["circle"](None, size, {})
    D._KINDS["gaussian"](None, size, {"gaussian_softness": 0.35})
    p = dict(scope="sample", prob=1.0, per_sample_prob=1.0, kinds=[0], cum=[1.0], size_min=size, size_max=size,
             stripe_width=0, alpha_dropout_p=0.1, salt_pepper_p=0.1, hidden_sigma=0.1, seed=3)
    assert PR.sample_draws(p, 16, 16, 6, 0, 0, forced=PR.CIRCLE)[1:3] == (PR.CIRCLE, got["circle"])
    assert PR.sample_draws(p, 16, 16, 6, 0, 0, forced=PR.GAUSSIAN)[1:3] == (PR.GAUSSIAN, got["gaussian"])
    for kind in (PR.SQUARE, PR.STRIPE_H, PR.STRIPE_V, PR.STRIPES):
        row = PR.sample_draws(p, 16, 16, 6, 0, 0, forced=kind)
        assert row == PR.NOT_APPLIED if size <= 0 else (row[0], row[2]) == (1, size), (kind, row)


def test_the_early_returns_of_the_noise_kinds():
    p = dict(scope="batch", prob=1.0, per_sample_prob=1.0, kinds=[0], cum=[1.0], size_min=3, size_max=3,
             stripe_width=0, alpha_dropout_p=0.0, salt_pepper_p=0.0, hidden_sigma=0.0, seed=3)
    for kind in (PR.ALPHA_DROP, PR.ALPHA_DROP_SOFT, PR.SALT_PEPPER, PR.HIDDEN_NOISE):
        assert PR.sample_draws(p, 8, 8, 6, 0, 0, forced=kind) == PR.NOT_APPLIED
    p.update(alpha_dropout_p=0.1, salt_pepper_p=0.1, hidden_sigma=0.1)
    assert PR.sample_draws(p, 8, 8, 6, 0, 0, forced=PR.HIDDEN_NOISE)[:2] == (1, PR.HIDDEN_NOISE)
    assert PR.sample_draws(p, 8, 8, 4, 0, 0, forced=PR.HIDDEN_NOISE) == PR.NOT_APPLIED      # no hidden channels
    assert PR.sample_draws(p, 8, 8, 6, 0, 0, forced=-1) == PR.NOT_APPLIED


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_desc_layout_matches_header(tmp_path):
    cname, mirror = "gnca_damage_policy_desc", L.DamagePolicyDesc
    consts = ("GNCA_DMG_STRIPES_AUTO", "GNCA_DMG_MAX_KINDS", "GNCA_DMG_SCOPE_BATCH", "GNCA_DMG_SCOPE_SAMPLE",
              "GNCA_DMG_RNG_GATE", "GNCA_DMG_RNG_SAMPLE_GATE", "GNCA_DMG_RNG_KIND", "GNCA_DMG_RNG_SIZE",
              "GNCA_DMG_RNG_ORIENT", "GNCA_DMG_RNG_Y", "GNCA_DMG_RNG_X", "GNCA_DMG_RNG_CELL",
              "GNCA_DMG_RNG_NORMAL_U1", "GNCA_DMG_RNG_NORMAL_U2")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("abi %d\\n", GNCA_ABI_VERSION);', 'printf("shared %llu\\n", (unsigned long long)GNCA_DMG_SHARED_SAMPLE);']
    lines += [f'printf("{c} %d\\n", {c});' for c in consts]
    lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
    for f, _ in mirror._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["abi"]) == 5 == L.ABI_VERSION
    assert int(got["shared"]) == L.DMG_SHARED_SAMPLE == PR.SHARED
    assert [int(got[c]) for c in consts] == [L.DMG_STRIPES_AUTO, L.DMG_MAX_KINDS, L.DMG_SCOPE_BATCH,
                                             L.DMG_SCOPE_SAMPLE] + list(range(10))
    assert list(range(10)) == [PR.GATE, PR.SAMPLE_GATE, PR.KIND, PR.SIZE, PR.ORIENT, PR.Y, PR.X, PR.CELL,
                               PR.NORMAL_U1, PR.NORMAL_U2] and len(L.DMG_RNG_STREAMS) == 10
    assert int(got[cname]) == ctypes.sizeof(mirror)
    for f, _ in mirror._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(mirror, f).offset, f
    fields = [f for f, _ in mirror._fields_]
    assert fields[:8] == ["B", "C", "H", "W", "scope", "prob", "per_sample_prob", "n_kinds"]


def test_symbol_is_exported(lib):
    assert lib.gnca_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert "gnca_damage_policy" in L.EXPORTS
    assert re.search(r"\bT gnca_damage_policy$", out, re.M)
    assert lib.gnca_damage_policy.argtypes is not None
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    assert re.search(r"^int gnca_damage_policy\(", src, re.M)


def _desc(**kw):
    d = D.DamagePolicy({"prob": 1.0, "start_epoch": 0, "kinds": {"square": 1.0, "stripes": 1.0}}, seed=5).desc(2, 6, 8, 8)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_point_rejects_bad_args_without_a_gpu(lib):
    f = lib.gnca_damage_policy
    assert f(None, PTR, None, None, None, None) == -1
    assert f(ctypes.byref(_desc()), None, None, None, None, None) == -1
    for bad in (dict(B=-1), dict(C=3), dict(H=0), dict(W=0), dict(W=-4), dict(scope=2), dict(scope=-1), dict(n_kinds=0),
                dict(n_kinds=11), dict(size_min=9, size_max=8)):
        assert f(ctypes.byref(_desc(**bad)), PTR, None, None, None, None) == -1, bad
    for code in (-1, 10):
        d = _desc()
        d.kinds[1] = code
        assert f(ctypes.byref(d), PTR, None, None, None, None) == -1, code
    d = _desc()
    d.kinds[5] = 99                                                   # past n_kinds: not read
    d.B = 0
    assert f(ctypes.byref(d), PTR, None, None, None, None) == 0       # an empty batch: nothing to do, no launch


def test_apply_argument_errors_come_before_any_launch(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(L, "load", no_load)
    p = D.DamagePolicy({"prob": 1.0, "start_epoch": 0}, seed=5)
    x = torch.zeros(2, 6, 8, 8)
    for bad in (dict(state=torch.zeros(6, 8, 8)), dict(state=torch.zeros(2, 3, 8, 8)), dict(state=None),
                dict(epoch=1.5), dict(epoch=True), dict(event=0.5), dict(event=True), dict(event=1 << 63),
                dict(event=torch.zeros(2, dtype=torch.int64)), dict(event=torch.zeros(1, dtype=torch.int32)),
                dict(sample_base=-1), dict(sample_base=(1 << 32) - 2), dict(sample_base=0.0),
                dict(kinds=["square"]), dict(kinds=["square", 3]), dict(kinds=torch.zeros(2, dtype=torch.int64)),
                dict(kinds=torch.zeros(3, dtype=torch.int32))):
        kw = dict(state=x, epoch=0, event=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            p.apply_(kw.pop("state"), kw.pop("epoch"), kw.pop("event"), **kw)
    with pytest.raises(RuntimeError):
        p.apply_(x, 0, 0)                                             # a CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        p.apply_(x, 0, 0, kinds=["square", None])


# ---------------------------------------------------------------------------------------------
# The reference RNG alone (fixed seeds, chosen here so that the conditions hold)
# ---------------------------------------------------------------------------------------------
N = 4096
CHI2_12_9999 = 39.1            # the 0.9999 point of chi-square at 12 degrees of freedom


def _chi2_13(d):
    """13-bin chi-square of 24-bit draws."""
    counts = np.bincount((np.asarray(d, np.int64) * 13) >> 24, minlength=13)
    e = len(d) / 13.0
    return float(((counts - e) ** 2 / e).sum())


def test_mix64_and_the_keying_are_the_definition():
    assert PR.mix64(0) == 0 and PR.mix64(1) == 0x5692161D100B05E5       # splitmix64's finaliser
    a = np.array([0, 1, (1 << 64) - 1], np.uint64)
    assert [int(v) for v in PR.mix64(a)] == [PR.mix64(int(v)) for v in a]
    seed, event, sample, stream, index = 11, 3, 70000, PR.CELL, 12345
    k0 = PR.mix64(seed + 0xD6E8FEB86659FD93)
    k1 = PR.mix64(k0 + 0x9E3779B97F4A7C15 * (event + 1))
    k2 = PR.mix64(k1 ^ (sample << 8 | stream))
    assert PR.draw(seed, event, sample, stream, index) == PR.mix64(k2 + index) >> 40
    assert int(PR.draw(seed, event, sample, stream, np.array([index], np.uint64))[0]) == PR.mix64(k2 + index) >> 40
    # the domain constant differs from the fire hash's keying of the same seed
    assert k0 != seed and PR.DOMAIN != PR.GOLDEN
    assert PR.draw(seed, -1, 0, 0) == PR.mix64(PR.mix64(PR.mix64(k0) ^ 0)) >> 40      # event + 1 wraps to 0


@pytest.mark.parametrize("seed", [1, 2024])
def test_reference_scalar_streams_are_uniform(seed):
    for stream in range(7):
        d = [PR.draw(seed, 5, gs, stream) for gs in range(N)]
        assert _chi2_13(d) < CHI2_12_9999, (stream, _chi2_13(d))


@pytest.mark.parametrize("seed", [1, 2024])
def test_reference_kind_frequencies_and_sizes(seed):
    w = np.array([1.0, 2.0, 1.0, 0.5, 0.5, 1.0, 1.0])
    p = PR.policy_fields(D.DamagePolicy(dict(CONFIGS["regeneration"], size_min=4, size_max=16), seed, "sample"))
    rows = np.array([PR.sample_draws(p, 72, 72, 16, 9, gs) for gs in range(N)])
    assert rows[:, 0].all()
    prim = np.where(np.isin(rows[:, 1], (PR.STRIPE_H, PR.STRIPE_V)), PR.STRIPES, rows[:, 1])
    codes = [PR.SQUARE, PR.CIRCLE, PR.STRIPES, PR.ALPHA_DROP, PR.SALT_PEPPER, PR.GAUSSIAN, PR.HIDDEN_NOISE]
    for code, q in zip(codes, w / w.sum()):
        n = int((prim == code).sum())
        assert abs(n - N * q) <= 5 * np.sqrt(N * q * (1 - q)), (code, n, N * q)
    h = int((rows[:, 1] == PR.STRIPE_H).sum())
    nst = int((prim == PR.STRIPES).sum())
    assert abs(h - nst / 2) <= 5 * np.sqrt(nst / 4)
    sizes = np.array([PR.randint(PR.draw(seed, 9, gs, PR.SIZE), 4, 16) for gs in range(N)])
    assert set(sizes) == set(range(4, 17))
    assert _chi2_13([PR.draw(seed, 9, gs, PR.SIZE) for gs in range(N)]) < CHI2_12_9999
    sq = rows[rows[:, 1] == PR.SQUARE]
    assert (sq[:, 2] >= 4).all() and (sq[:, 2] <= 16).all() and len(set(sq[:, 2])) == 13


@pytest.mark.parametrize("H,W,size", [(72, 72, 10), (11, 13, 4), (11, 13, 11), (11, 13, 12), (11, 13, 40), (12, 12, 1)])
def test_reference_positions_stay_in_the_reference_ranges(H, W, size):
    p = dict(scope="sample", prob=1.0, per_sample_prob=1.0, kinds=[0], cum=[1.0], size_min=size, size_max=size,
             stripe_width=0, alpha_dropout_p=0.1, salt_pepper_p=0.1, hidden_sigma=0.1, seed=77)
    n = 1024
    sq = np.array([PR.sample_draws(p, H, W, 6, 2, gs, forced=PR.SQUARE) for gs in range(n)])
    assert sq[:, 3].min() == 0 and sq[:, 3].max() == max(1, H - size + 1) - 1
    assert sq[:, 4].min() == 0 and sq[:, 4].max() == max(1, W - size + 1) - 1
    for kind in (PR.CIRCLE, PR.GAUSSIAN):
        c = np.array([PR.sample_draws(p, H, W, 6, 2, gs, forced=kind) for gs in range(n)])
        r = size // 2 if size > 1 else 1
        assert (c[:, 2] == r).all()
        assert c[:, 3].min() == r and c[:, 3].max() == max(r + 1, H - r) - 1         # r >= H / 2: always r
        assert c[:, 4].min() == r and c[:, 4].max() == max(r + 1, W - r) - 1
    st = np.array([PR.sample_draws(p, H, W, 6, 2, gs, forced=PR.STRIPES) for gs in range(n)])
    hs, vs = st[st[:, 1] == PR.STRIPE_H], st[st[:, 1] == PR.STRIPE_V]
    assert len(hs) and len(vs) and (hs[:, 4] == 0).all() and (vs[:, 3] == 0).all()
    assert hs[:, 3].min() == 0 and hs[:, 3].max() == max(1, H - size + 1) - 1
    assert vs[:, 4].min() == 0 and vs[:, 4].max() == max(1, W - size + 1) - 1


def test_batch_scope_shares_the_scalar_draws_and_not_the_positions():
    p = PR.policy_fields(D.DamagePolicy(dict(CONFIGS["regeneration"], stripe_width=0), 31, "batch"))
    seen = set()
    for event in range(40):
        rows = np.array([PR.sample_draws(p, 72, 72, 16, event, gs) for gs in (0, 1, 5, 1000)])
        assert len(set(map(tuple, rows[:, :3]))) == 1                 # applied, kind and size argument
        if rows[0, 1] in (PR.STRIPE_H, PR.STRIPE_V):
            assert len(set(map(tuple, rows))) == 1                    # the stripe's origin too
        elif rows[0, 1] in (PR.SQUARE, PR.CIRCLE, PR.GAUSSIAN):
            assert len(set(map(tuple, rows[:, 3:5]))) > 1
        seen.add(int(rows[0, 1]))
    assert len(seen) >= 6
    gated = PR.policy_fields(D.DamagePolicy(dict(CONFIGS["regeneration"], prob=0.3), 31, "batch"))
    applied = [PR.sample_draws(gated, 72, 72, 16, e, 0)[0] for e in range(400)]
    assert abs(sum(applied) - 120) <= 5 * np.sqrt(400 * 0.3 * 0.7)
    gated["scope"], gated["prob"], gated["per_sample_prob"] = "sample", 1.0, 0.25
    applied = [PR.sample_draws(gated, 72, 72, 16, 1, gs)[0] for gs in range(N)]
    assert abs(sum(applied) - N / 4) <= 5 * np.sqrt(N * 0.25 * 0.75)


@pytest.mark.parametrize("seed", [1, 2024])
def test_reference_cell_noise(seed):
    H = W = 64
    u = PR.cell_uniforms(seed, 4, 17, H, W).astype(np.float64).reshape(-1)
    n = u.size
    assert u.min() >= 0 and u.max() < 1
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n)
    assert abs(u.var() - 1 / 12) <= 5 * np.sqrt(1 / 180 / n)           # var of (u - 1/2)^2 is 1/180
    lag = np.corrcoef(u[:-1], u[1:])[0, 1]
    assert abs(lag) <= 5 / np.sqrt(n), lag
    other = PR.cell_uniforms(seed, 4, 18, H, W).astype(np.float64).reshape(-1)
    assert abs(np.corrcoef(u, other)[0, 1]) <= 5 / np.sqrt(n)          # the next sample's plane
    z, r = PR.cell_normals(seed, 4, 17, 6, H, W)
    z = z.reshape(-1)
    assert abs(z.mean()) <= 5 / np.sqrt(z.size)
    assert abs(z.std() - 1) <= 5 / np.sqrt(2 * z.size)
    assert r.max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12              # u1 >= 2^-24: |n| <= 5.77


# ---------------------------------------------------------------------------------------------
# regrow_trace on a stub model
# ---------------------------------------------------------------------------------------------
class _StubModel:
    """``trace`` records its arguments and returns tensors that name the call and the recorded step."""

    def __init__(self):
        self.calls = []

    def trace(self, x, steps, **kw):
        self.calls.append((x, steps, dict(kw)))
        rec, k = list(kw["record"]), 100.0 * len(self.calls)
        mk = lambda *shape: torch.tensor([k + r for r in rec]).reshape(-1, *([1] * len(shape))).expand(-1, *shape).clone()
        met = ImageMetrics(mk(2, 4)) if kw.get("target") is not None else None
        return TraceResult(x + steps, mk(2, 4, 3, 3) if kw.get("frames", True) else None, rec,
                           mk(2, 3, 3) if kw.get("return_attention") else None, met, None,
                           rgb_u8=mk(2, 3, 3, 3).to(torch.uint8) if kw.get("render") else None)


class _StubPolicy(D.DamagePolicy):
    def apply_(self, state, epoch, event, **kw):
        self.seen = (state.clone(), epoch, event, dict(kw))
        state.add_(1000.0)


def _policy():
    return _StubPolicy({"prob": 1.0, "start_epoch": 4}, seed=5)


def test_regrow_trace_splits_every_and_offsets():
    m, p = _StubModel(), _policy()
    x = torch.zeros(2, 6, 3, 3)
    offs = [[(t, 0)] for t in range(7)]
    r = D.regrow_trace(m, x, 7, p, 3, event=9, every=2, offsets=offs, first_step=10, target=torch.zeros(4, 3, 3),
                       return_attention=True, render=True, seed=1, sample_base=6)
    (x1, n1, k1), (x2, n2, k2) = m.calls
    assert (n1, n2) == (3, 4) and x1 is x
    assert (k1["record"], k2["record"]) == ([2], [1, 3, 4])            # steps 2 | 4, 6, 7 of the whole run
    assert (k1["first_step"], k2["first_step"]) == (10, 13)
    assert (k1["offsets"], k2["offsets"]) == (offs[:3], offs[3:])
    assert "every" not in k1 and "every" not in k2
    for k in (k1, k2):
        assert (k["seed"], k["sample_base"], k["return_attention"], k["render"]) == (1, 6, True, True)
    st, epoch, event, kw = p.seen
    assert torch.equal(st, x + 3) and (epoch, event) == (4, 9)         # x_final of the first call; start_epoch
    assert kw == dict(sample_base=6, kinds=None)
    assert torch.equal(x2, x + 3 + 1000) and torch.equal(r.x_final, x + 3 + 1000 + 4)
    assert r.steps == [2, 4, 6, 7]
    want = [102.0, 201.0, 203.0, 204.0]
    assert r.frames[:, 0, 0, 0, 0].tolist() == want and tuple(r.frames.shape) == (4, 2, 4, 3, 3)
    assert r.attention[:, 0, 0, 0].tolist() == want
    assert r.metrics.stacked[:, 0, 0].tolist() == want and r.metrics.mse.shape == (4, 2)
    assert r.rgb_u8[:, 0, 0, 0, 0].tolist() == [102, 201, 203, 204] and r.attention_u8 is None
    assert r.diagnostics is None


def test_regrow_trace_splits_record_and_passes_kinds():
    m, p = _StubModel(), _policy()
    x = torch.zeros(2, 6, 3, 3)
    r = D.regrow_trace(m, x, 6, p, 2, record=[2, 3, 6], kinds=["circle", None], epoch=50, frames=False)
    assert [c[2]["record"] for c in m.calls] == [[2], [1, 4]] and r.steps == [2, 3, 6]
    assert [c[2]["offsets"] for c in m.calls] == [None, None] and r.frames is None
    assert p.seen[1] == 50 and p.seen[3]["kinds"].tolist() == [1, -1] and p.seen[3]["kinds"].dtype == torch.int32
    r = D.regrow_trace(m, x, 6, p, 4, record=[5, 6])                    # nothing recorded before the damage
    assert [c[2]["record"] for c in m.calls[2:]] == [[], [1, 2]] and r.steps == [5, 6]
    assert tuple(r.frames.shape) == (2, 2, 4, 3, 3)


def test_regrow_trace_damage_step_zero_damages_a_copy_before_the_first_step():
    m, p = _StubModel(), _policy()
    x = torch.zeros(2, 6, 3, 3)
    r = D.regrow_trace(m, x, 5, p, 0, every=2)
    ((x2, n2, k2),) = m.calls
    assert n2 == 5 and k2["record"] == [2, 4, 5] and k2["first_step"] == 0 and r.steps == [2, 4, 5]
    assert torch.equal(p.seen[0], x) and torch.equal(x2, x + 1000) and float(x.abs().max()) == 0.0


def test_regrow_trace_argument_errors_draw_nothing():
    m, p = _StubModel(), _policy()
    x = torch.zeros(2, 6, 3, 3)
    random.seed(3)
    st = random.getstate()
    for bad in (dict(steps=4, damage_step=4), dict(steps=4, damage_step=9), dict(steps=4, damage_step=-1),
                dict(steps=4, damage_step=1.0), dict(steps=True, damage_step=0), dict(steps=4, damage_step=1, every=0),
                dict(steps=4, damage_step=1, record=[5]), dict(steps=4, damage_step=1, record=[2], every=2),
                dict(steps=4, damage_step=1, offsets=[[(0, 1)]] * 3), dict(steps=4, damage_step=1, first_step=-1),
                dict(steps=4, damage_step=1, kinds=["square"]), dict(steps=4, damage_step=1, policy=object())):
        kw = dict(bad)
        pol = kw.pop("policy", p)
        with pytest.raises(ValueError):
            D.regrow_trace(m, x, kw.pop("steps"), pol, kw.pop("damage_step"), **kw)
    assert not m.calls and not hasattr(p, "seen") and random.getstate() == st
