"""Host-only: ``gnca_k2_variant`` names the finalize kernel each plan launches.  The flat kernel
(``gnca_k2_finalize_flat``) serves the compact update field of a rollout's sub-batch pipeline (K2 beside
the other sub-batch's K1) when W % 4 == 0 and the plan has no fused row sums; everything else keeps the
band kernel ``gnca_k2_finalize<V,COMPACT,CU,ROWS>``: the dense field of single and masked steps, V = 1,
the zero-padded shift's ROWS instance, K2 alone on the chip, the 32-channel K1's one-stream rollouts and
samples with more GroupNorm partials than one wave pass sums."""
import ctypes
import os

import pytest

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import step as S
from tests import liveness_cases as LC

FLAT = "gnca_k2_finalize_flat<4,3>"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _d(model, B, H, W, **kw):
    return LC.make_desc(LC.MODELS[model], B, H, W, **kw)


def test_flat_kernel_beside_k1(lib):
    for model, B, H, W in [("graph", 1024, 72, 72), ("graph", 192, 72, 72), ("classic", 192, 72, 72),
                           ("graph_nogn", 192, 72, 72), ("graph", 64, 48, 72), ("graph", 128, 64, 48),
                           ("graph", 256, 32, 24), ("graph", 128, 40, 40)]:
        d = _d(model, B, H, W)
        assert S.rollout_compact(d) and S.rollout_subs(d) == 2, (model, B, H, W)
        assert S.k2_variant(d, 1) == FLAT, (model, B, H, W)
        # the same shape alone on the chip (a requested fold's last K2) and as a single step
        assert S.k2_variant(d, 0) == "gnca_k2_finalize<4,true,2,false>", (model, B, H, W)
        assert S.k2_variant(d, -1) == "gnca_k2_finalize<4,false,2,false>", (model, B, H, W)
    # the attention flag does not change a rollout's plan (rollouts clear it); a single step keeps it
    d = _d("graph", 192, 72, 72, attention=True)
    assert S.k2_variant(d, 1) == FLAT and S.k2_variant(d, -1) == "gnca_k2_finalize<4,false,2,false>"


def test_band_kernel_everywhere_else(lib):
    # zero-padded shift: the ROWS instance (K2 also writes the next K0's row sums), beside K1 and alone
    d = _d("graph_zp", 192, 72, 72)
    assert S.rollout_subs(d) == 2
    assert S.k2_variant(d, 1) == S.k2_variant(d, 0) == "gnca_k2_finalize<4,true,1,true>"
    # one-stream rollouts: K2 alone on the chip (B=96 at 72^2; C4's 128-sample shard; the 32-channel K1)
    for model, B, H, W in [("graph", 96, 72, 72), ("graph", 128, 72, 72), ("g32", 128, 32, 32), ("g32", 64, 48, 48)]:
        d = _d(model, B, H, W)
        assert S.rollout_compact(d) and S.rollout_subs(d) == 1, (model, B, H, W)
        assert S.k2_variant(d, 0) == "gnca_k2_finalize<4,true,2,false>", (model, B, H, W)
        with pytest.raises(L.GncaError):
            S.k2_variant(d, 1)          # no sub-batch pipeline: no K2 beside a K1
    # small batches: the dense field
    d = _d("graph", 8, 72, 72)
    assert not S.rollout_compact(d) and S.k2_variant(d, 0) == "gnca_k2_finalize<4,false,2,false>"
    # W % 4 != 0: single cells (the runtime-geometry K1, dense field)
    d = _d("graph", 192, 72, 70)
    assert S.k2_variant(d, 0) == S.k2_variant(d, -1) == "gnca_k2_finalize<1,false,2,false>"
    # masked and single steps: the dense field whatever the batch
    assert S.k2_variant(_d("graph", 1024, 72, 72), -1) == "gnca_k2_finalize<4,false,2,false>"
    # more GroupNorm partial pairs per sample than one wave pass (256): 128x72 on 8x24 tiles
    d = _d("graph", 128, 128, 72)
    assert S.rollout_subs(d) == 2 and S.k2_variant(d, 1) == "gnca_k2_finalize<4,true,2,false>"


def test_bad_arguments(lib):
    buf = ctypes.create_string_buffer(64)
    d = _d("graph", 192, 72, 72)
    assert lib.gnca_k2_variant(None, 1, buf, 64) != 0
    assert lib.gnca_k2_variant(ctypes.byref(d), 2, buf, 64) != 0
    assert lib.gnca_k2_variant(ctypes.byref(d), 1, None, 64) != 0
    assert lib.gnca_k2_variant(ctypes.byref(d), 1, buf, 0) != 0
    assert lib.gnca_k2_variant(ctypes.byref(_d("graph", 192, 72, 72).__class__()), 0, buf, 64) != 0   # an empty desc
