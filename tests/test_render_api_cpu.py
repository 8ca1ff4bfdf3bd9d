"""CPU-side checks of the uint8 rendering (gnca_render_u8 / gnca_colorize_u8, render.py): the float32
restatement tests/render_ref.py against the reference's own recorded frames, the ctypes mirrors
against the header, the exports, the argument checks of both entry points and of the Python layer, and
the shipped colour tables.  No GPU needed."""
import ctypes
import glob
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import render as R
from tests import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render")
FRAME_FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "render_rgb*.npz")))
MAP_FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "render_attn_*.npz")))
SYMBOLS = ("gnca_render_u8", "gnca_colorize_u8")
MAX_DIFF, MAX_SHARE = 1, 0.005     # random inputs: every byte within 1, at most 0.5 % of the bytes differ


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def test_the_fixtures_are_all_there():
    kinds = {(str(load(n)["mode"]), str(load(n)["kind"])) for n in FRAME_FIXTURES}
    assert kinds == {(m, k) for m in ("rgb", "rgba") for k in ("dyadic", "random", "threshold")}
    assert len(MAP_FIXTURES) == 2


# ---------------------------------------------------------------------------------------------
# render_ref against the reference's frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_render_ref_against_the_reference(name):
    f = load(name)
    got = RR.render_rgb(f["x"], float(f["alpha_thr"]), int(f["upscale"]), str(f["mode"])).numpy()
    n, worst = RR.count_diff(got, f["out"])
    print(f"{name}: {n} of {got.size} bytes differ, max |d| = {worst}")
    if str(f["kind"]) in ("dyadic", "threshold"):
        assert n == 0, (name, n, worst)
    else:
        assert worst <= MAX_DIFF and n <= MAX_SHARE * got.size, (name, n, worst)


def test_threshold_fixture_is_strict_on_fp32():
    """A cell at float32(thr) is black, one ulp above is shown (s = 1: a cell is a pixel)."""
    for name in FRAME_FIXTURES:
        f = load(name)
        if str(f["kind"]) != "threshold" or int(f["upscale"]) != 1:
            continue
        t = np.float32(float(f["alpha_thr"]))
        a = f["x"][:, 3]
        at, above = a == t, a == np.nextafter(t, np.float32(2))
        assert at.any() and above.any()
        rgb = f["out"][..., :3]
        assert (rgb[at] == 0).all(), name
        assert (rgb[above].max(axis=-1) > 0).all(), name


@pytest.mark.parametrize("name", MAP_FIXTURES)
def test_attn_fixture_is_the_viridis_lookup(name):
    f = load(name)
    idx = RR.lut_index(f["maps"], "max")
    assert np.array_equal(R.CMAPS["viridis"][idx].numpy(), f["out"])
    assert int(idx[1].max()) == 0 and int(idx[2].max()) == 255        # the all-zero and the single-peak map


def test_render_ref_resampling_is_torchs():
    """The tap-by-tap resampling is F.interpolate's on dyadic values (exact sums), s in {2, 4, 8}."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    v = torch.randint(-16, 81, (2, 3, 5, 7), generator=g).float() / 64
    for s in (2, 4, 8):
        assert torch.equal(RR.resample(v, s), F.interpolate(v, scale_factor=s, mode="bilinear", align_corners=False))
    assert torch.equal(RR.resample(v, 1), v)


def test_cmaps_are_matplotlibs():
    pytest.importorskip("matplotlib")
    from matplotlib import colormaps
    assert set(R.CMAPS) == {"viridis", "magma"}
    for name, t in R.CMAPS.items():
        want = (np.array(colormaps[name].colors) * 255).astype(np.uint8)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 3) and t.device.type == "cpu"
        assert np.array_equal(t.numpy(), want), name


def test_the_package_does_not_import_matplotlib():
    code = "import sys, graph_neural_cellular_automata_amd as g; g.CMAPS; sys.exit('matplotlib' in sys.modules)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ---------------------------------------------------------------------------------------------
# The ABI
# ---------------------------------------------------------------------------------------------
def test_desc_layouts_match_header(tmp_path):
    pairs = (("gnca_render_desc", L.RenderDesc), ("gnca_colorize_desc", L.ColorizeDesc))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){',
             'printf("abi %d\\n", GNCA_ABI_VERSION);', 'printf("band %d\\n", GNCA_RENDER_BAND_ROWS);',
             'printf("consts %d %d %d %d\\n", GNCA_RENDER_RGB, GNCA_RENDER_RGBA, GNCA_NORM_MAX, GNCA_NORM_MINMAX);']
    for cname, mirror in pairs:
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
    assert int(got["band"]) == L.RENDER_BAND_ROWS == R.BAND_ROWS
    assert got["consts"].split() == [str(v) for v in (L.RENDER_RGB, L.RENDER_RGBA, L.NORM_MAX, L.NORM_MINMAX)]
    for cname, mirror in pairs:
        assert int(got[cname]) == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(mirror, f).offset, (cname, f)


def test_symbols_are_exported(lib):
    assert lib.gnca_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for n in SYMBOLS:
        assert n in L.EXPORTS
        assert re.search(rf"\bT {n}$", out, re.M), f"{n} not exported"
        assert getattr(lib, n).argtypes is not None


def test_the_stream_travels_in_the_descriptor():
    """Neither declaration has a trailing ``void* stream`` (the stream gate's table is fixed) nor the
    ``_f32`` suffix (the poison gate's)."""
    src = open(os.path.join(ROOT, "include", "gnca.h")).read()
    for n in SYMBOLS:
        (params,) = re.findall(rf"^int {n}\(([^;]*)\);", src, re.M)
        assert not re.search(r"\bvoid\s*\*\s*stream\b", params) and not n.endswith("_f32")


def _rdesc(**kw):
    d = L.RenderDesc()
    d.N, d.H, d.W, d.upscale, d.mode, d.alpha_thr, d.src_nstride = 2, 5, 7, 2, L.RENDER_RGB, 0.1, 4 * 35
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _cdesc(**kw):
    d = L.ColorizeDesc()
    d.N, d.H, d.W, d.norm = 2, 5, 7, L.NORM_MAX
    for k, v in kw.items():
        setattr(d, k, v)
    return d


PTR = 0x10000     # a well-formed, aligned address that is never dereferenced: every call below is rejected


def test_render_rejects_bad_args_without_a_gpu(lib):
    f = lib.gnca_render_u8
    assert f(None, PTR, PTR) == -1
    assert f(ctypes.byref(_rdesc()), None, PTR) == -1
    assert f(ctypes.byref(_rdesc()), PTR, None) == -1
    assert f(ctypes.byref(_rdesc()), PTR, PTR + 2) == -1          # a misaligned out
    for bad in (dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(W=-3), dict(upscale=0), dict(upscale=17),
                dict(mode=2), dict(mode=-1), dict(src_nstride=4 * 35 - 1), dict(src_nstride=0)):
        assert f(ctypes.byref(_rdesc(**bad)), PTR, PTR) == -1, bad
    # three rows of an image this wide do not fit the LDS: unsupported, not invalid, and no launch
    assert f(ctypes.byref(_rdesc(W=4000, src_nstride=4 * 5 * 4000)), PTR, PTR) == -2


def test_colorize_rejects_bad_args_without_a_gpu(lib):
    f = lib.gnca_colorize_u8
    assert f(None, PTR, PTR, PTR) == -1
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None), (PTR, PTR, PTR + 1)):
        assert f(ctypes.byref(_cdesc()), *args) == -1, args
    for bad in (dict(N=0), dict(H=0), dict(W=-1), dict(norm=2), dict(norm=-1)):
        assert f(ctypes.byref(_cdesc(**bad)), PTR, PTR, PTR) == -1, bad


# ---------------------------------------------------------------------------------------------
# The Python layer
# ---------------------------------------------------------------------------------------------
def test_render_rgb_argument_errors():
    x = torch.zeros(2, 4, 5, 7)
    for bad in (dict(upscale=0), dict(upscale=17), dict(upscale=2.0), dict(upscale=True), dict(mode="bgr"),
                dict(alpha_thr=float("nan")), dict(alpha_thr="0.1")):
        with pytest.raises(ValueError):
            R.render_rgb(x, **bad)
    with pytest.raises(ValueError):
        R.render_rgb(torch.zeros(2, 3, 5, 7))                      # C < 4
    with pytest.raises(ValueError):
        R.render_rgb(torch.zeros(5, 7))
    with pytest.raises(ValueError):
        R.render_rgb(torch.zeros(0, 4, 5, 7))
    with pytest.raises(RuntimeError):
        R.render_rgb(x)                                            # a CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        R.render_rgb(x.double())


def test_colorize_argument_errors():
    m = torch.zeros(2, 5, 7)
    for bad in (dict(cmap="jet"), dict(cmap=torch.zeros(256, 3)), dict(cmap=torch.zeros(255, 3, dtype=torch.uint8)),
                dict(cmap=7), dict(norm="mean")):
        with pytest.raises(ValueError):
            R.colorize(m, **bad)
    with pytest.raises(ValueError):
        R.colorize(torch.zeros(7))
    with pytest.raises(RuntimeError):
        R.colorize(m)
    with pytest.raises(RuntimeError):
        R.colorize(m, cmap=torch.zeros(256, 3, dtype=torch.uint8))


def test_out_is_checked():
    dev = torch.device("cpu")
    ok = torch.zeros(2, 10, 14, 3, dtype=torch.uint8)
    R._check_out(ok, (2, 10, 14, 3), dev)
    for bad in (ok.float(), ok[:, :, :, :2], torch.zeros(2, 10, 14, 4, dtype=torch.uint8), ok.transpose(1, 2),
                torch.zeros(2 * 10 * 14 * 3 + 1, dtype=torch.uint8)[1:].view(2, 10, 14, 3), None):
        with pytest.raises(ValueError):
            R._check_out(bad, (2, 10, 14, 3), dev)


@pytest.mark.parametrize("graph", [True, False])
def test_trace_render_argument_errors_draw_nothing(graph, monkeypatch):
    from graph_neural_cellular_automata_amd import NeuralCA, NeuralCAGraph

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(L, "load", no_load)
    model = NeuralCAGraph(16, 32) if graph else NeuralCA(16, 32)
    x = torch.zeros(1, 16, 8, 8)
    random.seed(11)
    st = random.getstate()
    for kw in (dict(render=3), dict(render="rgb"), dict(render=dict(scale=4)), dict(render=dict(upscale=0)),
               dict(render=dict(upscale=32)), dict(render=dict(mode="bgr")), dict(render=dict(cmap="jet")),
               dict(render=dict(alpha_thr="x")), dict(render=True, frames=False), dict(render=True, channels=3),
               dict(render=dict(upscale=2), channels=1)):
        with pytest.raises(ValueError):
            model.trace(x, 4, **kw)
        assert random.getstate() == st, kw


def test_check_trace_render_defaults():
    assert R.check_trace_render(None, 0.1, 4, True) is None
    assert R.check_trace_render(True, 0.25, 4, True) == dict(upscale=4, mode="rgb", alpha_thr=0.25, cmap="viridis")
    r = R.check_trace_render(dict(upscale=2, mode="rgba", alpha_thr=0.1, cmap="magma"), 0.25, 16, True)
    assert r == dict(upscale=2, mode="rgba", alpha_thr=0.1, cmap="magma")


def test_trace_result_new_fields_are_keyword_only():
    from graph_neural_cellular_automata_amd.modules._stepper import TraceResult
    r = TraceResult(1, 2, [3], 4, 5, 6)
    assert (r.metrics, r.diagnostics, r.rgb_u8, r.attention_u8) == (5, 6, None, None)
    r = TraceResult(1, 2, [3], 4, rgb_u8=7, attention_u8=8)
    assert (r.rgb_u8, r.attention_u8, r.metrics, r.diagnostics) == (7, 8, None, None)
    with pytest.raises(TypeError):
        TraceResult(1, 2, [3], 4, 5, 6, 7)
