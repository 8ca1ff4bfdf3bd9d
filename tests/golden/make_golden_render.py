#!/usr/bin/env python3
"""Record the reference's own uint8 frames: tests/golden/render/render_*.npz (a folder of
their own: tests/golden_io.py takes every .npz directly under tests/golden for a step fixture).

Runs the reference's ``masked_rgb`` / ``attn_to_rgb`` (testing/test_graph_augmented_regeneration.py) and
``save_img`` (testing/test_intermediate_loss.py; its ``plt.imsave`` is replaced by a function that keeps
the array) on small inputs and stores input, arguments and ``(img * 255).astype(np.uint8)``::

    python tests/golden/make_golden_render.py /path/to/reference

Inputs: *dyadic* (multiples of 1/64 in [-0.25, 1.25]: at power-of-two scales every product and sum is
exact in fp32 in any order), *random* (uniform in [-0.2, 1.2]) and *threshold* (alpha cells at exactly
float32(thr) and one ulp above); maps for ``attn_to_rgb``: random non-negative, all-zero, single-peak.
"""
import os
import sys

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render")


def dyadic(rng, shape):
    return (rng.integers(-16, 81, size=shape) / 64.0).astype(np.float32)


def uniform(rng, shape):
    return rng.uniform(-0.2, 1.2, size=shape).astype(np.float32)


def threshold(rng, shape, thr):
    x = uniform(rng, shape)
    x[:, :3] = np.abs(x[:, :3]) + np.float32(0.25)          # visible colours: a wrong mask shows
    t = np.float32(thr)
    a = x[:, 3].copy().reshape(-1)
    a[0::3] = t                                              # at the threshold: dead (strict >)
    a[1::3] = np.nextafter(t, np.float32(2))                 # one ulp above: alive
    a[2::3] = np.nextafter(t, np.float32(-2))                # one ulp below: dead
    x[:, 3] = a.reshape(x[:, 3].shape)
    return x


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    sys.path.insert(0, os.path.join(ref, "src"))
    import matplotlib
    matplotlib.use("Agg")
    import torch
    from testing import test_graph_augmented_regeneration as REG
    from testing import test_intermediate_loss as INT

    kept = []
    INT.plt.imsave = lambda path, arr, **kw: kept.append(np.array(arr, copy=True))

    def u8(img):
        return (np.asarray(img) * 255).astype(np.uint8)

    def rgb_ref(x, thr, s):
        return np.stack([u8(REG.masked_rgb(torch.from_numpy(xi), thr, upscale=s)) for xi in x])

    def rgba_ref(x, s):
        out = []
        for xi in x:
            del kept[:]
            INT.save_img(torch.from_numpy(xi), "unused.png", upscale=s)
            out.append(u8(np.clip(kept[0], 0, 1)))           # (the reference clips only when it upscales)
        return np.stack(out)

    rng = np.random.default_rng(20240607)
    cases = [(7, 9, s, 2) for s in (1, 2, 4)] + [(17, 29, 4, 1)]
    n = 0
    for kind, make in (("dyadic", dyadic), ("random", uniform), ("threshold", None)):
        for H, W, s, B in cases:
            if kind == "threshold" and (H, W) != (7, 9):
                continue
            for mode, thr in (("rgb", 0.1), ("rgb", 0.12), ("rgba", 0.1)):
                if thr == 0.12 and (kind != "threshold" and s != 2):
                    continue
                x = threshold(rng, (B, 4, H, W), thr) if make is None else make(rng, (B, 4, H, W))
                out = rgb_ref(x, thr, s) if mode == "rgb" else rgba_ref(x, s)
                name = f"render_{mode}_{kind}_{H}x{W}_s{s}" + ("_thr012" if thr == 0.12 else "") + ".npz"
                np.savez_compressed(os.path.join(HERE, name), x=x, alpha_thr=np.float64(thr), upscale=np.int64(s),
                                    mode=np.array(mode), kind=np.array(kind), out=out)
                n += 1
    for H, W in ((7, 9), (17, 29)):
        maps = np.abs(rng.normal(size=(4, H, W))).astype(np.float32)
        maps[1] = 0.0
        maps[2] = 0.0
        maps[2, H // 2, W // 3] = 3.5                         # a single peak
        maps[3] *= np.float32(1e-3)                           # a small maximum: 1e-8 matters in fp32
        out = np.stack([u8(REG.attn_to_rgb(m)) for m in maps])
        np.savez_compressed(os.path.join(HERE, f"render_attn_{H}x{W}.npz"), maps=maps, out=out)
        n += 1
    print(f"wrote {n} fixtures to {HERE}")


if __name__ == "__main__":
    main()
