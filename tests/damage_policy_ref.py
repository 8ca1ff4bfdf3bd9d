"""numpy restatement of the device damage policy (gnca_damage_policy; include/gnca.h holds the
definition): the counter RNG and the draw rules in uint64 / int64 arithmetic, the normals in float64,
the effects through oracle.damage_oracle.damage one sample at a time (tests/test_damage.py pins that
oracle to the reference).  TEST INFRASTRUCTURE ONLY: it shares no code with the package.
"""
from __future__ import annotations

import numpy as np

from oracle import damage_oracle as DO

M64 = (1 << 64) - 1
DOMAIN = 0xD6E8FEB86659FD93
GOLDEN = 0x9E3779B97F4A7C15
SHARED = 0xFFFFFFFF
GATE, SAMPLE_GATE, KIND, SIZE, ORIENT, Y, X, CELL, NORMAL_U1, NORMAL_U2 = range(10)
SQUARE, CIRCLE, STRIPE_H, STRIPE_V, ALPHA_DROP, ALPHA_DROP_SOFT, SALT_PEPPER, GAUSSIAN, HIDDEN_NOISE, STRIPES = range(10)
NOT_APPLIED = (0, -1, 0, 0, 0, 0, 0, 0)


def mix64(z):
    """splitmix64's finaliser on a Python int or a uint64 array (wrapping)."""
    if isinstance(z, np.ndarray):
        z = z.astype(np.uint64)
        with np.errstate(over="ignore"):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key1(seed: int, event: int) -> int:
    k0 = mix64(seed + DOMAIN)
    return mix64(k0 + GOLDEN * ((event + 1) & M64))


def key2(k1: int, sample: int, stream: int) -> int:
    return mix64(k1 ^ (((sample << 8) & M64) | stream))


def draw(seed: int, event: int, sample: int, stream: int, index=0):
    """The 24-bit integer d(seed, event, sample, stream, index); ``index`` an int or an integer array."""
    k2 = key2(key1(seed, event), sample, stream)
    if isinstance(index, np.ndarray):
        with np.errstate(over="ignore"):
            return (mix64(np.uint64(k2) + index.astype(np.uint64)) >> np.uint64(40)).astype(np.int64)
    return mix64(k2 + index) >> 40


def uniform(d):
    """d * 2^-24 as fp32 (exact)."""
    return np.float32(d) * np.float32(2.0 ** -24) if not isinstance(d, np.ndarray) else \
        d.astype(np.float32) * np.float32(2.0 ** -24)


def randint(d: int, lo: int, hi: int) -> int:
    return lo + ((d * (hi - lo + 1)) >> 24)


def normal_f64(d1, d2):
    """The normals in float64 and the radius sqrt(-2 ln u1) (for the bound of the fp32 ones)."""
    u1 = (d1.astype(np.float64) + 1.0) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * (d2.astype(np.float64) * 2.0 ** -24)), r


def pick_kind(u, kinds, cum) -> int:
    for k, c in enumerate(cum):
        if u < np.float32(c):
            return kinds[k]
    return kinds[-1]


def sample_draws(p: dict, H: int, W: int, C: int, event: int, gs: int, forced=None) -> tuple:
    """draws_out's row of global sample ``gs``.  ``p``: the policy's parsed fields (scope "batch" /
    "sample", prob, per_sample_prob, kinds, cum, size_min, size_max, stripe_width, alpha_dropout_p,
    salt_pepper_p, hidden_sigma, seed).  ``forced``: None (draw) or a kind code (-1: untouched)."""
    seed = p["seed"]
    d = lambda sample, stream: draw(seed, event, sample, stream)
    per = p["scope"] == "sample"
    ks = gs if per else SHARED
    if forced is not None:
        kind = int(forced)
        if not 0 <= kind <= 9:
            return NOT_APPLIED
    else:
        if not uniform(d(SHARED, GATE)) <= np.float32(p["prob"]):
            return NOT_APPLIED
        if per and not uniform(d(gs, SAMPLE_GATE)) <= np.float32(p["per_sample_prob"]):
            return NOT_APPLIED
        kind = pick_kind(uniform(d(ks, KIND)), p["kinds"], p["cum"])
    size = randint(d(ks, SIZE), p["size_min"], p["size_max"])
    y = x = arg = 0
    if kind == SQUARE:
        if size <= 0:
            return NOT_APPLIED
        arg = size
        y = randint(d(gs, Y), 0, max(1, H - size + 1) - 1)
        x = randint(d(gs, X), 0, max(1, W - size + 1) - 1)
    elif kind in (CIRCLE, GAUSSIAN):
        arg = r = size // 2 if size > 1 else 1
        y = randint(d(gs, Y), r, max(r + 1, H - r) - 1)
        x = randint(d(gs, X), r, max(r + 1, W - r) - 1)
    elif kind in (STRIPE_H, STRIPE_V, STRIPES):
        arg = p["stripe_width"] if p["stripe_width"] > 0 else size
        if arg <= 0:
            return NOT_APPLIED
        if kind == STRIPES:
            kind = STRIPE_H if d(ks, ORIENT) < (1 << 23) else STRIPE_V
        if kind == STRIPE_H:
            y = randint(d(ks, Y), 0, max(1, H - arg + 1) - 1)
        else:
            x = randint(d(ks, X), 0, max(1, W - arg + 1) - 1)
    elif kind in (ALPHA_DROP, ALPHA_DROP_SOFT):
        if p["alpha_dropout_p"] <= 0:
            return NOT_APPLIED
    elif kind == SALT_PEPPER:
        if p["salt_pepper_p"] <= 0:
            return NOT_APPLIED
    elif kind == HIDDEN_NOISE:
        if C <= 4 or p["hidden_sigma"] <= 0:
            return NOT_APPLIED
    return (1, kind, arg, y, x, 0, 0, 0)


def cell_uniforms(seed: int, event: int, gs: int, H: int, W: int) -> np.ndarray:
    """[H,W] fp32: the uniforms of an alpha kind (plane 0 of noise_out)."""
    return uniform(draw(seed, event, gs, CELL, np.arange(H * W, dtype=np.uint64))).reshape(H, W)


def cell_normals(seed: int, event: int, gs: int, C: int, H: int, W: int):
    """([C-4,H,W] float64 normals, their radii): the hidden-noise planes of noise_out."""
    idx = np.arange((C - 4) * H * W, dtype=np.uint64)
    n, r = normal_f64(draw(seed, event, gs, NORMAL_U1, idx), draw(seed, event, gs, NORMAL_U2, idx))
    return n.reshape(C - 4, H, W), r.reshape(C - 4, H, W)


def policy_fields(policy) -> dict:
    """A ``DamagePolicy``'s parsed fields as the dict the functions here take."""
    return {k: getattr(policy, k) for k in ("scope", "prob", "per_sample_prob", "kinds", "cum", "size_min", "size_max",
                                            "stripe_width", "alpha_thr", "alpha_dropout_p", "salt_pepper_p",
                                            "hidden_sigma", "gaussian_softness", "seed")}


def reference(p: dict, shape, event: int, sample_base: int = 0, forced=None):
    """(draws int32 [B,8], noise {b: planes}) of a batch: noise[b] is the [H,W] fp32 uniforms of an alpha
    sample or the ([C-4,H,W] float64 normals, radii) of a hidden-noise sample."""
    B, C, H, W = shape
    draws = np.zeros((B, 8), np.int32)
    noise = {}
    for b in range(B):
        gs = sample_base + b
        row = sample_draws(p, H, W, C, event, gs, None if forced is None else forced[b])
        draws[b] = row
        if row[0] and row[1] in (ALPHA_DROP, ALPHA_DROP_SOFT, SALT_PEPPER):
            noise[b] = cell_uniforms(p["seed"], event, gs, H, W)
        elif row[0] and row[1] == HIDDEN_NOISE:
            noise[b] = cell_normals(p["seed"], event, gs, C, H, W)
    return draws, noise


def apply_effects(x: np.ndarray, p: dict, draws: np.ndarray, noise: np.ndarray) -> np.ndarray:
    """The state after the draws ``draws`` [B,8] with the noise planes ``noise`` [B,max(1,C-4),H,W]
    (fp32, as dumped or as restated), through the numpy oracle sample by sample."""
    out = x.copy()
    for b in range(x.shape[0]):
        applied, prim, arg, y, x0 = (int(v) for v in draws[b, :5])
        if not applied:
            continue
        xb, pos = out[b:b + 1], [(y, x0)]
        if prim == SQUARE:
            out[b:b + 1] = DO.damage(xb, "square", size=arg, pos=pos)
        elif prim == CIRCLE:
            out[b:b + 1] = DO.damage(xb, "circle", size=arg, pos=pos)
        elif prim in (STRIPE_H, STRIPE_V):
            out[b:b + 1] = DO.damage(xb, "stripe", size=arg, pos=pos, orientation="h" if prim == STRIPE_H else "v")
        elif prim in (ALPHA_DROP, ALPHA_DROP_SOFT):
            out[b:b + 1] = DO.damage(xb, "alpha_drop", noise=noise[b:b + 1, :1], p=np.float32(p["alpha_dropout_p"]),
                                     alpha_thr=np.float32(p["alpha_thr"]), hard=prim == ALPHA_DROP)
        elif prim == SALT_PEPPER:
            out[b:b + 1] = DO.damage(xb, "saltpepper", noise=noise[b:b + 1, :1], p=np.float32(p["salt_pepper_p"]))
        elif prim == GAUSSIAN:
            out[b:b + 1] = DO.damage(xb, "gaussian", size=arg, pos=pos, softness=p["gaussian_softness"])
        elif prim == HIDDEN_NOISE:
            out[b:b + 1] = DO.damage(xb, "hidden_noise", noise=noise[b:b + 1], sigma=p["hidden_sigma"])
        else:
            raise ValueError(prim)
    return out
