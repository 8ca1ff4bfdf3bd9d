"""The uint8 rendering on the GPU (gnca_render_u8 / gnca_colorize_u8, render.py, ``trace(render=...)``):
against the reference's own recorded frames (tests/golden/render/render_*.npz), against the float32
restatement tests/render_ref.py on the shapes where heads, tails, unaligned image starts and band
edges occur, every byte written and nothing else, per-map normalisation, ``trace(render=...)`` against
the standalone calls, the stream contract on the three legs of tests/streams.py, and determinism.

Tolerances.  Dyadic inputs (multiples of 1/64) at power-of-two scales: every product and sum is exact
in fp32, so the bytes are bitwise.  Random inputs: an fp32 error of 1e-6 moves ``trunc(255 v)`` by at
most one, and only within about 1e-5 of an integer, so every byte is within 1 and at most 0.5 % of a
case's bytes differ at all.  ``s = 3``: only ``|d| <= 1`` (torch's own fp32 weights at a scale that is
no power of two already put flat saturated regions at 254; not a parity claim).
"""
import glob
import os
import random

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests import streams as ST
from tests.poison import same_bytes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render")
FRAME_FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "render_rgb*.npz")))
MAP_FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "render_attn_*.npz")))
MAX_DIFF, MAX_SHARE = 1, 0.005
SHAPES = [(1, 1), (5, 7), (17, 29), (40, 40), (72, 72)]
SCALES = [1, 2, 3, 4, 8]
GUARD, CANARY = 4096, 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from graph_neural_cellular_automata_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def R(dev):
    from graph_neural_cellular_automata_amd import render
    render.lut("viridis", dev)          # the named tables: uploaded once, outside every capture
    render.lut("magma", dev)
    return render


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def dyadic_state(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-16, 81, (B, C, H, W), generator=g).float() / 64


def random_state(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, C, H, W, generator=g) * 1.4 - 0.2


def check(got, want, what, exact, share=True):
    n, worst = RR.count_diff(got.cpu().numpy(), np.asarray(want))
    print(f"{what}: {n} of {got.numel()} bytes differ, max |d| = {worst}")
    if exact:
        assert n == 0, (what, n, worst)
    else:
        assert worst <= MAX_DIFF, (what, n, worst)
        if share:
            assert n <= MAX_SHARE * got.numel(), (what, n, worst)


# ---------------------------------------------------------------------------------------------
# 1. the reference's frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_reference_frames(dev, R, name):
    f = load(name)
    got = R.render_rgb(torch.from_numpy(f["x"]).to(dev), float(f["alpha_thr"]), int(f["upscale"]), str(f["mode"]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == f["out"].shape
    check(got, f["out"], name, exact=str(f["kind"]) in ("dyadic", "threshold"))
    if str(f["kind"]) == "threshold" and int(f["upscale"]) == 1:
        t = np.float32(float(f["alpha_thr"]))
        a = f["x"][:, 3]
        rgb = got.cpu().numpy()[..., :3]
        assert (rgb[a == t] == 0).all()                                       # at float32(thr): black
        assert (rgb[a == np.nextafter(t, np.float32(2))].max(axis=-1) > 0).all()      # one ulp above: shown


# ---------------------------------------------------------------------------------------------
# 2. render_ref on the shapes with heads, tails, unaligned image starts and band edges
# ---------------------------------------------------------------------------------------------
def _against_ref(dev, R, H, W, s, mode, B=3):
    pow2 = s in (1, 2, 4, 8, 16)
    for kind, make in (("dyadic", dyadic_state), ("random", random_state)):
        x = make(B, 16, H, W, seed=H * 1000 + W * 10 + s)
        got = R.render_rgb(x.to(dev)[:, :4], 0.1, s, mode)                    # a channel-slice view, read in place
        want = RR.render_rgb(x[:, :4], 0.1, s, mode)
        assert tuple(got.shape) == (B, H * s, W * s, 3 if mode == "rgb" else 4)
        check(got, want, f"{kind} {H}x{W} s={s} {mode}", exact=pow2 and kind == "dyadic", share=pow2)


@pytest.mark.parametrize("mode", ["rgb", "rgba"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_against_render_ref(dev, R, H, W, s, mode):
    _against_ref(dev, R, H, W, s, mode)


@pytest.mark.parametrize("mode", ["rgb", "rgba"])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_band_edges(dev, R, s, mode):
    """Heights at the band size, one row below and above it, and two bands and a row."""
    b = R.BAND_ROWS
    for H in (b - 1, b, b + 1, 2 * b + 1):
        _against_ref(dev, R, H, 5, s, mode)


@pytest.mark.parametrize("W,mode,s", [(600, "rgba", 2), (1500, "rgb", 1), (1500, "rgb", 2)])
def test_wide_images_use_smaller_bands(dev, R, W, mode, s):
    """A band of 8 rows and its halo would not fit the LDS: 4 rows per workgroup at 600 (rgba), 1 at 1500."""
    _against_ref(dev, R, 5, W, s, mode, B=2)


def test_too_wide_an_image_is_an_error(dev, R):
    from graph_neural_cellular_automata_amd import _lib as L
    with pytest.raises(L.GncaError, match="unsupported"):
        R.render_rgb(torch.zeros(1, 4, 2, 4000, device=dev), 0.1, 1, "rgba")


def test_layouts_and_out(dev, R):
    """Five dimensions, a whole 16-channel state, a layout that has to be copied, and ``out=``."""
    x = dyadic_state(6, 16, 5, 7, seed=5)
    want = RR.render_rgb(x, 0.1, 2, "rgb")
    xd = x.to(dev)
    assert same_bytes(R.render_rgb(xd, 0.1, 2), want)
    assert same_bytes(R.render_rgb(xd.view(2, 3, 16, 5, 7), 0.1, 2), want.view(2, 3, 10, 14, 3))
    assert same_bytes(R.render_rgb(xd[0], 0.1, 2), want[0])
    nc = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)             # channels-last storage
    assert same_bytes(R.render_rgb(nc, 0.1, 2), want)
    assert same_bytes(R.render_rgb(xd[::2], 0.1, 2), want[::2])
    out = torch.zeros(6, 10, 14, 3, dtype=torch.uint8, device=dev)
    assert R.render_rgb(xd, 0.1, 2, out=out) is out and same_bytes(out, want)
    with pytest.raises(ValueError):
        R.render_rgb(xd, 0.1, 2, out=out.cpu())
    with pytest.raises(ValueError):
        R.render_rgb(xd, 0.1, 4, out=out)


# ---------------------------------------------------------------------------------------------
# 3. a region of exactly 1.0
# ---------------------------------------------------------------------------------------------
def test_a_region_of_ones_is_255(dev, R):
    x = torch.full((1, 4, 12, 12), 0.3)
    x[:, 3] = 1.0
    x[:, :3, 3:9, 2:10] = 1.0
    for mode in ("rgb", "rgba"):
        img = R.render_rgb(x.to(dev), 0.1, 4, mode)[0].cpu()
        inner = img[4 * 3 + 2:4 * 9 - 2, 4 * 2 + 2:4 * 10 - 2]                # every tap inside the region
        assert int(inner.min()) == 255
        assert int(img[:4, :4, :3].max()) == int(0.3 * 255)
    full = torch.ones(2, 4, 5, 7)
    assert int(R.render_rgb(full.to(dev), 0.1, 4, "rgba").min()) == 255


# ---------------------------------------------------------------------------------------------
# 4. every byte written, nothing else written
# ---------------------------------------------------------------------------------------------
def _guarded(n, fill, dev):
    block = torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    assert block.data_ptr() % 4 == 0
    block[GUARD:GUARD + n] = fill
    return block, block[GUARD:GUARD + n]


def _guards_intact(block, n):
    return bool((block[:GUARD] == CANARY).all()) and bool((block[GUARD + n:] == CANARY).all())


@pytest.mark.parametrize("what", ["rgb_s1", "rgb_s2", "rgba_s3", "rgb_s4", "colorize"])
def test_every_byte_written_and_nothing_else(dev, R, what):
    B, H, W = 3, 5, 7
    if what == "colorize":
        g = torch.Generator().manual_seed(9)
        a = torch.rand(B, H, W, generator=g)
        shape = (B, H, W, 3)
        want = RR.colorize(a, R.CMAPS["viridis"])
        call = lambda out: R.colorize(a.to(dev), "viridis", out=out)
    else:
        mode, s = what.split("_s")
        s = int(s)
        x = dyadic_state(B, 16, H, W, seed=2)
        shape = (B, H * s, W * s, 3 if mode == "rgb" else 4)
        want = RR.render_rgb(x[:, :4], 0.1, s, mode)
        call = lambda out: R.render_rgb(x.to(dev)[:, :4], 0.1, s, mode, out=out)
    n = int(np.prod(shape))
    got = []
    for fill in (0x00, 0xFF):
        block, body = _guarded(n, fill, dev)
        call(body.view(shape))
        torch.cuda.synchronize()
        assert _guards_intact(block, n), (what, hex(fill))
        got.append(body.view(shape).clone())
    assert same_bytes(got[0], got[1]), what
    check(got[0], want, what, exact=what != "rgba_s3", share=False)


# ---------------------------------------------------------------------------------------------
# 5. colorize
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAP_FIXTURES)
def test_reference_maps(dev, R, name):
    f = load(name)
    got = R.colorize(torch.from_numpy(f["maps"]).to(dev), "viridis", "max")
    assert same_bytes(got, torch.from_numpy(f["out"]))


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (72, 72)])
@pytest.mark.parametrize("cmap,norm", [("viridis", "max"), ("magma", "minmax")])
def test_colorize_against_render_ref(dev, R, H, W, cmap, norm):
    g = torch.Generator().manual_seed(H * 100 + W)
    a = torch.rand(6, H, W, generator=g) * torch.tensor([1e-3, 0.02, 0.5, 1.0, 7.0, 300.0]).view(6, 1, 1)
    if norm == "minmax":
        a = a - torch.tensor([0.0, 0.01, 0.6, -2.0, 3.0, 150.0]).view(6, 1, 1)
    got = R.colorize(a.to(dev), cmap, norm)
    assert same_bytes(got, RR.colorize(a, R.CMAPS[cmap], norm))
    # per map, not per batch: each map alone gives its own bytes
    for i in (0, 5):
        assert same_bytes(R.colorize(a[i].to(dev), cmap, norm), got[i])
    if H * W > 1:
        idx = RR.lut_index(a, norm)
        assert all(int(idx[i].max()) >= 254 for i in range(6))                # every map reaches the top of the table


@pytest.mark.parametrize("norm", ["max", "minmax"])
def test_colorize_zero_and_constant_maps(dev, R, norm):
    a = torch.zeros(4, 5, 7)
    a[1] = 0.37
    a[2] = -1.5
    a[3, 2, 3] = 2.0
    got = R.colorize(a.to(dev), "viridis", norm)
    assert same_bytes(got, RR.colorize(a, R.CMAPS["viridis"], norm))
    first, last = R.CMAPS["viridis"][0], R.CMAPS["viridis"][255]
    assert bool((got[0].cpu() == first).all()) and bool((got[2].cpu() == first).all())
    assert bool((got[1].cpu() == (last if norm == "max" else first)).all())
    assert bool((got[3, 2, 3].cpu() == last).all())


def test_colorize_user_lut(dev, R):
    g = torch.Generator().manual_seed(1)
    table = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g)
    a = torch.rand(2, 17, 29, generator=g)
    want = RR.colorize(a, table)
    assert same_bytes(R.colorize(a.to(dev), table.to(dev)), want)
    assert same_bytes(R.colorize(a.to(dev), table), want)                     # a CPU table is moved


# ---------------------------------------------------------------------------------------------
# 6. trace(render=...)
# ---------------------------------------------------------------------------------------------
def test_trace_render(dev, R):
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph
    torch.manual_seed(0)
    model = NeuralCAGraph(16, 128, update_gain=0.05, alpha_thr=0.12, message_gain=0.25).to(dev).eval()
    with torch.no_grad():
        model.update_net[2].weight.normal_(0, 0.05)
    g = torch.Generator().manual_seed(31)
    x = torch.rand(2, 16, 40, 40, generator=g)
    x[:, 4:] = torch.randn(2, 12, 40, 40, generator=g)
    x = x.to(dev)
    rr = random.Random(17)
    kw = dict(every=2, return_attention=True, fire_rate=0.5, seed=5,
              offsets=[rr.sample(model.graph.offsets, 8) for _ in range(6)])
    base = model.trace(x, 6, **kw)
    assert base.rgb_u8 is None and base.attention_u8 is None
    res = model.trace(x, 6, render=True, **kw)
    assert tuple(res.rgb_u8.shape) == (3, 2, 160, 160, 3) and tuple(res.attention_u8.shape) == (3, 2, 40, 40, 3)
    assert same_bytes(res.rgb_u8, R.render_rgb(res.frames, 0.12, 4, "rgb"))
    assert same_bytes(res.attention_u8, R.colorize(res.attention))
    for name in ("x_final", "frames", "attention"):
        assert same_bytes(getattr(res, name), getattr(base, name)), name
    assert res.steps == base.steps == [2, 4, 6]
    assert int(res.rgb_u8.max()) > 0 and len(torch.unique(res.attention_u8)) > 8
    res = model.trace(x, 6, render=dict(upscale=2, mode="rgba", alpha_thr=0.3, cmap="magma"), channels=16, **kw)
    assert same_bytes(res.rgb_u8, R.render_rgb(res.frames, 0.3, 2, "rgba"))
    check(res.rgb_u8, RR.render_rgb(res.frames.cpu(), 0.3, 2, "rgba"), "trace frames against render_ref", exact=False)
    assert same_bytes(res.attention_u8, R.colorize(res.attention, "magma"))
    res = model.trace(x, 6, render=True, every=3, fire_rate=0.5, seed=5, offsets=kw["offsets"])
    assert res.attention_u8 is None and tuple(res.rgb_u8.shape) == (2, 2, 160, 160, 3)
    classic = NeuralCA(16, 128, alpha_thr=0.12).to(dev).eval()
    res = classic.trace(x, 4, every=2, render=dict(upscale=1))
    assert same_bytes(res.rgb_u8, R.render_rgb(res.frames, 0.12, 1))


# ---------------------------------------------------------------------------------------------
# 7. the stream contract (the stream travels in the descriptor: include/gnca.h)
# ---------------------------------------------------------------------------------------------
def _stream_case(R, dev, which):
    if which == "render":
        sets = tuple({"x": random_state(3, 16, 17, 29, seed=s).to(dev)} for s in (1, 2))
        return ST.Case("gnca_render_u8", sets, lambda b: {"rgb": R.render_rgb(b["x"][:, :4], 0.1, 4, "rgb")})
    sets = tuple({"maps": (random_state(3, 1, 17, 29, seed=s)[:, 0] * s).to(dev).contiguous()} for s in (3, 4))
    return ST.Case("gnca_colorize_u8", sets, lambda b: {"img": R.colorize(b["maps"], "viridis", "max")})


@pytest.mark.parametrize("which", ["render", "colorize"])
def test_stream_contract(dev, R, which):
    case = _stream_case(R, dev, which)
    ST.run(case, ST.LEGS)
    want, _ = case.eager
    assert not same_bytes(want[0][next(iter(want[0]))], want[1][next(iter(want[1]))])   # the two sets differ


# ---------------------------------------------------------------------------------------------
# 8. determinism
# ---------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(dev, R):
    x = random_state(64, 4, 72, 72, seed=8).to(dev)
    assert same_bytes(R.render_rgb(x, 0.1, 4), R.render_rgb(x, 0.1, 4))
    a = x[:, 0].contiguous()
    assert same_bytes(R.colorize(a), R.colorize(a))
