"""CPU restatement of the NVS evaluation's image metrics, for the `image_metrics` kernel tests.

SSIM: skimage.metrics.structural_similarity(gt, pred, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0), the call of
third_party_model/anysplat/src/evaluation/metrics.py:44-55, restated in float32 on scipy.ndimage.gaussian_filter (sigma 1.5,
truncate 3.5, mode 'reflect'), the filter skimage uses; scikit-image itself is not needed.  PSNR: metrics.py:11-19 (compute_psnr).
Pixels are uint8 / 255 in float32, as ToTensor makes them of a PNG."""
from __future__ import annotations

import numpy as np
from scipy.ndimage import gaussian_filter


def to_float(u8: np.ndarray) -> np.ndarray:
    return u8.astype(np.float32) / np.float32(255)


def ssim_channel(x: np.ndarray, y: np.ndarray) -> float:
    """one channel, float32 [H, W] -> mean S over the interior crop (float64), skimage's arithmetic"""
    if min(x.shape) < 11:
        raise ValueError("win_size exceeds image extent")
    f = lambda im: gaussian_filter(im, sigma=1.5, truncate=3.5, mode="reflect")
    cov_norm = 121 / 120                      # use_sample_covariance: NP / (NP - 1)
    ux, uy = f(x), f(y)
    uxx, uyy, uxy = f(x * x), f(y * y), f(x * y)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    return float(S[5:-5, 5:-5].mean(dtype=np.float64))


def ssim(a_u8: np.ndarray, b_u8: np.ndarray) -> float:
    """one image pair, uint8 [H, W, C]: mean over channels"""
    x, y = to_float(a_u8), to_float(b_u8)
    return float(np.mean([ssim_channel(x[..., c], y[..., c]) for c in range(x.shape[-1])]))


def mse(a_u8: np.ndarray, b_u8: np.ndarray) -> float:
    d = to_float(a_u8) - to_float(b_u8)
    return float((d.astype(np.float64) ** 2).mean())


def psnr(a_u8: np.ndarray, b_u8: np.ndarray) -> float:
    m = mse(a_u8, b_u8)
    return float("inf") if m == 0 else float(-10 * np.log10(m))
