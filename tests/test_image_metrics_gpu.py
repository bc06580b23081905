"""GPU: the NVS evaluation's metric kernel (csrc/image_metrics.hip) through the C ABI against the CPU restatement of skimage SSIM /
compute_psnr (tests/ssim_oracle.py) on seeded uint8 pairs: noisy, shifted and identical, batched."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ssim_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
SSIM_TOL, PSNR_TOL = 1e-5, 1e-4


def _pairs(N, H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    # a smooth image (what renders look like) plus noise, shifted copies and exact copies
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = (127 + 100 * np.sin(xx / 7.0 + 0.3 * np.arange(3)[:, None, None]) * np.cos(yy / 11.0)).transpose(1, 2, 0)
    b = np.empty_like(a)
    kinds = []
    for i in range(N):
        k = i % 3
        base = np.clip(smooth + rng.normal(0, 20, smooth.shape), 0, 255).astype(np.uint8)
        if k == 0:      # noisy
            a[i] = base
            b[i] = np.clip(base.astype(np.int16) + rng.integers(-30, 31, base.shape), 0, 255).astype(np.uint8)
        elif k == 1:    # shifted
            a[i] = base
            b[i] = np.roll(base, (2, -3), axis=(0, 1))
        else:           # identical
            b[i] = a[i]
        kinds.append(("noisy", "shifted", "identical")[k])
    return a, b, kinds


@pytest.mark.parametrize("N,H,W", [(1, 448, 448), (4, 448, 448), (8, 512, 512), (4, 37, 53), (8, 11, 11), (1, 11, 11)])
def test_image_metrics_vs_oracle(hip_lib, parity, N, H, W):
    from vist3a_amd import ops
    a, b, kinds = _pairs(N, H, W, seed=N * 1000 + H + W)
    ssim, mse = ops.image_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    ssim, mse = ssim.cpu().numpy(), mse.cpu().numpy()
    worst_s = worst_p = 0.0
    for i in range(N):
        want_s, want_p = SO.ssim(a[i], b[i]), SO.psnr(a[i], b[i])
        got_p = math.inf if mse[i] == 0 else -10 * math.log10(mse[i])
        if kinds[i] == "identical":
            assert ssim[i] == 1.0 and got_p == math.inf
            continue
        worst_s = max(worst_s, abs(ssim[i] - want_s))
        worst_p = max(worst_p, abs(got_p - want_p))
        assert abs(ssim[i] - want_s) <= SSIM_TOL, (i, kinds[i], ssim[i], want_s)
        assert abs(got_p - want_p) <= PSNR_TOL, (i, kinds[i], got_p, want_p)
    parity(f"image_metrics N={N} {H}x{W}", max_abs_dssim=worst_s, max_abs_dpsnr_db=worst_p, tol_ssim=SSIM_TOL, tol_psnr_db=PSNR_TOL)


def test_image_metrics_bit_identical_between_launches(hip_lib):
    from vist3a_amd import ops
    a, b, _ = _pairs(4, 448, 448, seed=3)
    a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    s1, m1 = ops.image_metrics(a, b)
    s2, m2 = ops.image_metrics(a, b)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)


def test_image_metrics_unaligned_views_and_channels(hip_lib):
    """rows that start at any byte offset (W * C odd, an offset base pointer) and 1 / 4 channels"""
    from vist3a_amd import ops
    rng = np.random.default_rng(9)
    for C in (1, 3, 4):
        flat = torch.from_numpy(rng.integers(0, 256, 2 * 23 * 29 * C + 1, dtype=np.uint8)).cuda()
        a = flat[1:].view(2, 23, 29, C)                  # base pointer off by one byte
        b = torch.from_numpy(rng.integers(0, 256, (2, 23, 29, C), dtype=np.uint8)).cuda()
        s, m = ops.image_metrics(a, b)
        for i in range(2):
            an, bn = a[i].cpu().numpy(), b[i].cpu().numpy()
            assert abs(s[i].item() - SO.ssim(an, bn)) <= SSIM_TOL
            assert abs(-10 * math.log10(m[i].item()) - SO.psnr(an, bn)) <= PSNR_TOL


def test_image_metrics_rejects_small_images(hip_lib):
    from vist3a_amd import ops
    x = torch.zeros(1, 10, 20, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
        ops.image_metrics(x, x)
