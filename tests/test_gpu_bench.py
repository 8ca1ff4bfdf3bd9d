"""bench.py's command line on the GPU: a plain run does the timed rollout only and ``--dump-outputs``
writes what it computed; ``--full`` adds the per-kernel, roofline and provenance objects.

The bench runs as a child of a forkserver child (tests/mr_workers.py): this process has initialised
the GPU and starts no program itself."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_KEYS = ("roofline", "roofline_k2", "device_timeline", "k1_k2_ms_vs_step", "pmc_provenance", "cpu_baseline")
W, K = 1, 3   # warmup and timed steps of the runs below (config c3: graph, B=8, 72x72)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda:0")


def _bench(argv):
    from tests import mr_workers as M
    from tests.test_gpu_multirank import _run_one
    return _run_one(M.bench_cli, (ROOT, argv), timeout=115)


def _c3_rollout(dev):
    """bench.py's c3 rollout restated: its start state (generator seed 1234), its offset draws
    (random.Random(42), one K-sample per step), W warmup steps, then K steps at fire counter W."""
    import bench
    from graph_neural_cellular_automata_amd import step as S
    from graph_neural_cellular_automata_amd.modules.graph_augmentation import GraphAugmentation
    wl = bench.WORKLOADS["c3"]
    B, C, H = wl["B"], wl["C"], wl["H"]
    table = GraphAugmentation._build_offsets(wl["R"])
    w, keep = bench.weight_struct(bench.load_weights(dev, wl), wl)
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.rand(B, C, H, H, device=dev, generator=g)
    x[:, 4:] = torch.randn(B, C - 4, H, H, device=dev, generator=g)
    rr = random.Random(42)
    offs = [rr.sample(table, wl["K"]) for _ in range(W + K)]
    first = table[:wl["K"]]   # the descriptor's own offsets: every step's come with the call
    start = S.rollout(bench.make_desc(wl, B, H, H, first, 0, 0), w, x, W, offs[:W])
    return S.rollout(bench.make_desc(wl, B, H, H, first, 0, W), w, start, K, offs[W:])


def test_plain_run_times_the_steps_only_and_dumps_its_final_state(dev, tmp_path):
    out = tmp_path / "dump"
    res = _bench(["--config", "c3", "--steps", str(K), "--warmup", str(W), "--gpu-warmup-ms", "0",
                  "--dump-outputs", str(out)])
    line = res["line"]
    assert res["lines"] == 1
    assert all(k in line for k in HEADLINE_KEYS) and not any(k in line for k in FULL_KEYS), sorted(line)
    assert line["steps"] == K and line["warmup"] == W and line["full"] is False
    assert line["unit"] == "cell-updates/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(8 * 72 * 72 * K / (line["ms_per_step"] * K / 1e3), rel=1e-9)
    assert sorted(os.listdir(out)) == ["state.npy"]
    state = np.load(out / "state.npy")
    assert state.dtype == np.float32 and state.shape == (8, 16, 72, 72)
    # the dumped array is the timed rollout's result: the line's checksum, and bit for bit this
    # process's rollout of the same inputs
    assert float(state.astype(np.float64).sum()) == pytest.approx(line["rank_state_checksums"][0], rel=1e-12)
    assert np.array_equal(state, _c3_rollout(dev).cpu().numpy())


def test_full_run_adds_the_kernel_and_roofline_objects(dev):
    line = _bench(["--config", "c3", "--steps", str(K), "--warmup", str(W), "--gpu-warmup-ms", "0",
                   "--full", "--no-cpu"])["line"]
    assert all(k in line for k in HEADLINE_KEYS + FULL_KEYS), sorted(line)
    assert line["full"] is True and line["steps"] == K and line["cpu_baseline"] is None
    assert line["roofline"]["k1_ms"] > 0 and line["roofline_k2"]["k2_ms"] > 0
    assert line["device_timeline"]["stamped_rollout_ms_per_step"] > 0
