"""Plain-torch restatement of the photometric loss of csrc/ssim_loss.hip, for shapes outside tests/golden/ssim_loss_ref.safetensors:
loss = (1 - lambda) * mean|x - y| + lambda * (1 - ssim(x, y)), ssim = the reference's loss_ssim.py::ssim(data_range=1.0,
size_average=True): 11-tap Gaussian (sigma 1.5) built in float32 as the reference builds it and then cast to the working dtype,
separable valid filtering of x, y, x^2, y^2, xy, population variances, C1 = 1e-4, C2 = 9e-4, mean over the valid map, all channels
and images.  Differentiable by autograd in whatever dtype x has; images are [N,H,W,C] (the rasteriser's layout).
tests/test_ssim_loss_host.py pins it to the fixture in fp64, value and gradient."""
import torch
import torch.nn.functional as F


def taps(dtype=torch.float64):
    c = torch.arange(11, dtype=torch.float)
    c -= 11 // 2
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    return g.to(dtype)


def _blur(t, w):
    C = t.shape[1]
    t = F.conv2d(t, w.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(t, w.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)


def ssim(x, y):
    if x.shape[1] < 11 or x.shape[2] < 11:
        raise ValueError("ssim: H and W must be at least 11")
    X, Y = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    w = taps(x.dtype).to(x.device)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = _blur(X, w), _blur(Y, w)
    s1, s2, s12 = _blur(X * X, w) - mu1 * mu1, _blur(Y * Y, w) - mu2 * mu2, _blur(X * Y, w) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return (((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs).flatten(2).mean(-1).mean()


def photometric_loss(x, y, ssim_lambda=0.2):
    """-> (loss, l1, ssim), scalars of x's dtype"""
    l1 = (x - y).abs().mean()
    s = ssim(x, y)
    return (1 - ssim_lambda) * l1 + ssim_lambda * (1 - s), l1, s
