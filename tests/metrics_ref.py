"""The image-metric definitions of DESIGN.md §17 / include/mli_metrics.h restated in numpy
float64: the preparation of NeuralLumen/scripts/compute_metrics.py:40-57 and skimage's
mean_squared_error, peak_signal_noise_ratio and structural_similarity(channel_axis=-1,
data_range=1.0), the latter with ``scipy.ndimage.uniform_filter``, the function skimage itself
calls.  skimage is not a dependency: both the kernel and this file implement the restatement.

Arrays are [B, C, H, W] (or [C, H, W]); an alpha is [B, H, W] (or [H, W]).
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
K1, K2 = 0.01, 0.03


def plane(v, quantize=True):
    """uint8 -> / 255; float32 with ``quantize`` -> clamp, x255 in fp32, truncated to uint8 (what
    relight.save_image writes), / 255; float32 without -> the value."""
    v = np.asarray(v)
    if v.dtype == np.uint8:
        return v.astype(np.float64) / 255.0
    assert v.dtype == np.float32, v.dtype
    if quantize:
        q = (np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
        return q.astype(np.float64) / 255.0
    return v.astype(np.float64)


def prepare(pred, target, alpha=None, quantize=True, mask_pred=False, gamma_corr=False, gamma=2.2):
    """The prepared (prediction, target) in float64, shaped as the inputs."""
    p, t = plane(pred, quantize), plane(target, quantize)
    if alpha is not None:
        a = np.asarray(alpha)
        a = a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)
        a = a.reshape(p.shape[:-3] + (1,) + p.shape[-2:])
        t = t * a + 1.0 * (1 - a)
        if mask_pred:
            p = p * a + 1.0 * (1 - a)
    if gamma_corr:
        t = np.power(t, 1 / gamma)
    return p, t


def ssim_plane(x, y):
    """skimage.metrics.structural_similarity of two [H, W] float64 planes, data_range 1, uniform
    7 x 7 window, sample covariance; the mean over the centres whose window lies in the image."""
    assert x.shape == y.shape and min(x.shape) >= WIN
    NP = WIN * WIN
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = K1 ** 2, K2 ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (WIN - 1) // 2
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64)


def metrics_prepared(p, t):
    """mse, psnr, ssim [B] and ssim_channels [B, C] of prepared float64 arrays [B, C, H, W]."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    assert p.shape == t.shape and p.ndim == 4
    B, C = p.shape[:2]
    mse = np.array([np.mean((p[b] - t[b]) ** 2, dtype=np.float64) for b in range(B)])
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(1.0 / mse)
    ch = np.array([[ssim_plane(p[b, c], t[b, c]) for c in range(C)] for b in range(B)])
    return {"mse": mse, "psnr": psnr, "ssim": ch.mean(axis=1), "ssim_channels": ch}


def metrics(pred, target, alpha=None, quantize=True, mask_pred=False, gamma_corr=False, gamma=2.2):
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 3:
        pred, target = pred[None], target[None]
        alpha = None if alpha is None else np.asarray(alpha)[None]
    p, t = prepare(pred, target, alpha, quantize, mask_pred, gamma_corr, gamma)
    out = metrics_prepared(p, t)
    out["prepared_pred"], out["prepared_target"] = p, t
    return out
