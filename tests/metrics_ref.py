"""Float64 numpy oracle of the image metrics (include/gnca.h, gnca_image_metrics_f32).

It restates the reference trainer's per-iteration figures (train_graph_augmented_nca.py:405-422) and
skimage's defaults: ``P``, ``X`` and ``Y`` are built in float32 as the trainer builds them, everything
after that is float64.  SSIM takes skimage's own path, ``scipy.ndimage.uniform_filter(size=7)``
followed by a crop of 3; ``ssim_windows`` is the direct valid-window restatement that a CPU test pins
it against.
"""
import numpy as np

WIN, C1, C2, COV = 7, 1e-4, 9e-4, 49.0 / 48.0


def premultiply(pred: np.ndarray) -> np.ndarray:
    """P = (pred_rgb * pred_alpha, pred_alpha) of a float32 [..., >=4, H, W] array, in float32."""
    pred = np.asarray(pred, dtype=np.float32)
    a = pred[..., 3:4, :, :]
    return np.concatenate([pred[..., :3, :, :] * a, a], axis=-3)


def _s_map(mx, my, mxx, myy, mxy):
    vx, vy, vxy = COV * (mxx - mx * mx), COV * (myy - my * my), COV * (mxy - mx * my)
    return ((2 * mx * my + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def ssim_filter(X: np.ndarray, Y: np.ndarray) -> float:
    """Mean SSIM of one [3,H,W] pair: skimage's uniform filter and crop, per channel."""
    from scipy.ndimage import uniform_filter
    H, W = X.shape[-2:]
    if H < WIN or W < WIN:
        return float("nan")
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    per = []
    for x, y in zip(X, Y):
        f = lambda a: uniform_filter(a, size=WIN)
        S = _s_map(f(x), f(y), f(x * x), f(y * y), f(x * y))
        per.append(S[3:H - 3, 3:W - 3].mean())
    return float(np.mean(per))


def ssim_windows(X: np.ndarray, Y: np.ndarray) -> float:
    """The same, as plain means over every full 7x7 window."""
    H, W = X.shape[-2:]
    if H < WIN or W < WIN:
        return float("nan")
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    per = []
    for x, y in zip(X, Y):
        S = np.empty((H - WIN + 1, W - WIN + 1))
        for i in range(S.shape[0]):
            for j in range(S.shape[1]):
                wx, wy = x[i:i + WIN, j:j + WIN], y[i:i + WIN, j:j + WIN]
                S[i, j] = _s_map(wx.mean(), wy.mean(), (wx * wx).mean(), (wy * wy).mean(), (wx * wy).mean())
        per.append(S.mean())
    return float(np.mean(per))


def pixel_perfect_count(P: np.ndarray, T: np.ndarray) -> int:
    """Cells of one float32 [4,H,W] pair with |P_c - T_c| < 0.05 in all four channels (float32)."""
    d = np.abs(P.astype(np.float32) - T.astype(np.float32))
    return int((d < np.float32(0.05)).all(axis=0).sum())


def image_metrics(pred: np.ndarray, target: np.ndarray, ssim=ssim_filter) -> np.ndarray:
    """[N,4] float64 (mse, pixel_perfect, psnr, ssim) of pred [N,>=4,H,W] against target [4,H,W],
    [1,4,H,W] or [N,4,H,W] (premultiplied RGBA)."""
    P = premultiply(pred)
    T = np.asarray(target, dtype=np.float32)
    if T.ndim == 3:
        T = T[None]
    N, _, H, W = P.shape
    T = np.broadcast_to(T, (N, 4, H, W))
    out = np.empty((N, 4))
    for n in range(N):
        d = P[n].astype(np.float64) - T[n].astype(np.float64)
        out[n, 0] = (d * d).mean()
        out[n, 1] = pixel_perfect_count(P[n], T[n]) / float(H * W)
        X, Y = np.clip(P[n, :3], 0, 1), np.clip(T[n, :3], 0, 1)   # float32, as the trainer's
        e = X.astype(np.float64) - Y.astype(np.float64)
        m = (e * e).mean()
        out[n, 2] = np.inf if m == 0 else 10.0 * np.log10(1.0 / m)
        out[n, 3] = ssim(X, Y)
    return out
