"""A numpy float64 reference of the tangent block's thin QR exactly as include/gnca.h specifies it
(gnca_tangent_qr): the Gram matrix, the Cholesky columns with the pivot rule and its drops, R^-1 on the
kept rows and columns, Q = V R^-1, and the carry rule of gnca_rollout_tangent_block's records.  Test
infrastructure only.
"""
from __future__ import annotations

import numpy as np

DROP = 2.0 ** -44     # a column is kept iff d_j is positive, finite and > DROP * G_jj


def gram(V: np.ndarray) -> np.ndarray:
    """G = V^T V of one sample: V [n, K] (any float dtype; computed in float64)."""
    V = V.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return V.T @ V


def cholesky_pivot(G: np.ndarray):
    """(R [K,K] upper triangular, kept [K] bool, log_diag [K]) of a Gram matrix, column by column."""
    K = G.shape[0]
    R = np.zeros((K, K), np.float64)
    kept = np.zeros(K, bool)
    log_diag = np.full(K, -np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(K):
            s = 0.0
            for i in range(j):
                s += R[i, j] * R[i, j]
            d = G[j, j] - s
            if d > 0.0 and np.isfinite(d) and d > DROP * G[j, j]:
                kept[j] = True
                R[j, j] = np.sqrt(d)
                log_diag[j] = np.log(R[j, j])
                for k in range(j + 1, K):
                    s = 0.0
                    for i in range(j):
                        s += R[i, j] * R[i, k]
                    R[j, k] = (G[j, k] - s) / R[j, j]
            # a dropped column: row j of R stays zero, so it contributes nothing to later columns
    return R, kept, log_diag


def inverse_kept(R: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """The inverse of R on the kept rows and columns, zero elsewhere (back substitution per column)."""
    K = R.shape[0]
    X = np.zeros((K, K), np.float64)
    for m in range(K):
        if not kept[m]:
            continue
        X[m, m] = 1.0 / R[m, m]
        for i in range(m - 1, -1, -1):
            if not kept[i]:
                continue
            s = 0.0
            for l in range(i + 1, m + 1):
                if kept[l]:
                    s += R[i, l] * X[l, m]
            X[i, m] = -s / R[i, i]
    return X


def qr_sample(V: np.ndarray):
    """One sample: V [n, K] float32 -> dict(G, R, kept, log_diag, Rinv, Q float64 before the rounding)."""
    G = gram(V)
    R, kept, log_diag = cholesky_pivot(G)
    X = inverse_kept(R, kept)
    V64 = V.astype(np.float64)
    Q = np.zeros_like(V64)
    for j in range(V.shape[1]):
        for i in range(j + 1):
            if kept[i] and X[i, j] != 0.0:
                Q[:, j] += V64[:, i] * X[i, j]
    return dict(G=G, R=R, kept=kept, log_diag=log_diag, Rinv=X, Q=Q)


def qr_block(V: np.ndarray):
    """The block V [K, B, ...] as the library takes it: dict of Q [K,B,n] float64, R [B,K,K], log_diag [B,K],
    G [B,K,K], kept [B,K]."""
    K, B = V.shape[:2]
    Vf = V.reshape(K, B, -1)
    out = [qr_sample(np.ascontiguousarray(Vf[:, b].T)) for b in range(B)]
    return dict(Q=np.stack([o["Q"].T for o in out], axis=1), R=np.stack([o["R"] for o in out]),
                log_diag=np.stack([o["log_diag"] for o in out]), G=np.stack([o["G"] for o in out]),
                kept=np.stack([o["kept"] for o in out]))


def carry_records(log_diags):
    """The rollout's records from the per-record log_diag [B,K] arrays, in record order:
    log_r[r] = log_diag_r + carry, then carry += log_diag_r where the column was kept (finite)."""
    carry = np.zeros_like(np.asarray(log_diags[0], np.float64))
    out = []
    for ld in log_diags:
        ld = np.asarray(ld, np.float64)
        out.append(ld + carry)
        carry = np.where(np.isfinite(ld), carry + ld, carry)
    return np.stack(out)
