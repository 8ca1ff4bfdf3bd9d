"""The float64 reference of the tangent block's QR (tests/tangent_block_ref.py) against numpy and against
its own specification: no GPU."""
import numpy as np

from tests import tangent_block_ref as BR


def _block(n, K, seed):
    return np.random.default_rng(seed).standard_normal((n, K)).astype(np.float32)


def test_full_rank_equals_numpy_qr_up_to_column_signs():
    for n, K, seed in ((140, 1, 0), (140, 3, 1), (140, 8, 2), (500, 16, 3), (17, 16, 4)):
        V = _block(n, K, seed)
        o = BR.qr_sample(V)
        assert o["kept"].all()
        q, r = np.linalg.qr(V.astype(np.float64))
        sgn = np.sign(np.diag(r))
        q, r = q * sgn, r * sgn[:, None]            # numpy's R made non-negative on the diagonal
        scale = np.abs(r).max()
        assert np.abs(o["R"] - r).max() <= 1e-11 * scale, (n, K)
        assert np.abs(o["Q"] - q).max() <= 1e-11, (n, K)
        assert (np.diag(o["R"]) > 0).all() and not np.tril(o["R"], -1).any()
        assert np.abs(o["Q"].T @ o["Q"] - np.eye(K)).max() <= 1e-11
        assert np.abs(o["Rinv"] @ o["R"] - np.eye(K)).max() <= 1e-11
        assert np.array_equal(o["log_diag"], np.log(np.diag(o["R"])))


def test_duplicated_zero_and_nonfinite_columns_drop():
    V = _block(200, 5, 7)
    V[:, 2] = V[:, 0]          # a duplicate
    V[:, 3] = 0.0              # a zero column
    o = BR.qr_sample(V)
    assert o["kept"].tolist() == [True, True, False, False, True]
    assert o["log_diag"][2] == -np.inf and o["log_diag"][3] == -np.inf
    assert not o["Q"][:, 2].any() and not o["Q"][:, 3].any()
    assert not o["R"][2].any() and not o["R"][3].any() and not o["Rinv"][:, 2].any() and not o["Rinv"][2].any()
    kept = [0, 1, 4]
    Qk = o["Q"][:, kept]
    assert np.abs(Qk.T @ Qk - np.eye(3)).max() <= 1e-11
    # the kept columns are the QR of the kept columns alone, and the duplicate is still explained: V_2 = Q R[:, 2]
    alone = BR.qr_sample(np.ascontiguousarray(V[:, kept]))
    assert np.abs(alone["Q"] - Qk).max() <= 1e-13
    assert np.abs(o["Q"] @ o["R"][:, 2] - V[:, 2]).max() <= 1e-6
    W = _block(200, 4, 8)
    W[5, 1] = np.nan
    o = BR.qr_sample(W)
    assert o["kept"].tolist() == [True, False, True, True] and o["log_diag"][1] == -np.inf
    assert np.isfinite(o["Q"]).all() and not o["Q"][:, 1].any()
    Qk = o["Q"][:, [0, 2, 3]]
    assert np.abs(Qk.T @ Qk - np.eye(3)).max() <= 1e-11
    # more columns than rows: the surplus drops
    o = BR.qr_sample(_block(3, 6, 9))
    assert o["kept"].tolist() == [True, True, True, False, False, False]


def test_sum_of_logs_is_half_log_det_and_permutation_invariant():
    V = _block(300, 6, 11)
    base = BR.qr_sample(V)["log_diag"].sum()
    sign, logdet = np.linalg.slogdet(BR.gram(V))
    assert sign == 1.0 and abs(base - 0.5 * logdet) <= 1e-11
    rng = np.random.default_rng(12)
    for _ in range(4):
        perm = rng.permutation(6)
        assert abs(BR.qr_sample(np.ascontiguousarray(V[:, perm]))["log_diag"].sum() - base) <= 1e-11


def test_block_layout_and_carry_rule():
    V = np.random.default_rng(5).standard_normal((3, 2, 4, 5, 7)).astype(np.float32)    # [K,B,C,H,W]
    o = BR.qr_block(V)
    assert o["Q"].shape == (3, 2, 140) and o["R"].shape == (2, 3, 3) and o["log_diag"].shape == (2, 3)
    one = BR.qr_sample(np.ascontiguousarray(V.reshape(3, 2, -1)[:, 1].T))
    assert np.array_equal(o["Q"][:, 1], one["Q"].T) and np.array_equal(o["R"][1], one["R"])
    a = np.array([[0.5, -1.0], [2.0, -np.inf]])
    b = np.array([[0.25, 1.0], [1.0, -np.inf]])
    rec = BR.carry_records([a, b])
    assert np.array_equal(rec[0], a)
    assert np.array_equal(rec[1], np.array([[0.75, 0.0], [3.0, -np.inf]]))
