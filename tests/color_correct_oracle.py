"""Plain-torch restatement of the reference's colour correction (third_party_model/anysplat/src/post_opt/lib_bilagrid.py:56-126,
color_correct) with the dtype as a parameter and every image of a batch fitted on its own: the oracle of csrc/color_correct.hip.
tests/test_color_correct_host.py pins it to tensors recorded from the reference's own function
(tests/golden/color_correct_ref.safetensors).

color_correct        the reference's arithmetic: masked rows zeroed, torch.linalg.lstsq
color_correct_normal what the kernel does instead: fp64 normal equations, and the identity warp for a channel with fewer than 10
                     usable rows or a failed pivot (the package's stated deviation; the reference asserts or is undefined there)"""
import math

import torch

EPS = 0.5 / 255
PIVOT_TOL = 1e-12

# name: ((N, H, W), num_iters) - the cases recorded from the reference (tests/golden/make_golden_color_correct.py)
GOLDEN_CASES = {"1x5x7.it1": ((1, 5, 7), 1), "1x5x7.it5": ((1, 5, 7), 5), "2x13x37.it5": ((2, 13, 37), 5), "1x45x70.it5": ((1, 45, 70), 5)}


def features(x):
    """x [P,3] -> [P,10]: r^2, rg, rb, g^2, gb, b^2, r, g, b, 1 (the reference's a_mat)"""
    r, g, b = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    return torch.cat([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, torch.ones_like(r)], -1)


def unclipped(z, eps):
    return (z >= eps) & (z <= 1 - eps)


def _fit_lstsq(a, b, mask):
    return torch.linalg.lstsq(torch.where(mask[:, None], a, torch.zeros_like(a)), torch.where(mask, b, torch.zeros_like(b)), rcond=-1)[0]


def _fit_normal(a, b, mask, c):
    """-> (w, flag): elimination without row exchanges on the Gram matrix, as the kernel; flag 1 = under 10 rows, 2 = a pivot failed"""
    ident = torch.zeros(10, dtype=a.dtype)
    ident[6 + c] = 1.0
    flag = 1 if int(mask.sum()) < 10 else 0
    am = a[mask]
    G = torch.cat([am.T @ am, (am.T @ b[mask])[:, None]], 1)
    d0 = torch.diagonal(G[:, :10]).clone()
    for k in range(10):
        piv = G[k, k]
        if not (d0[k] > 0 and piv > PIVOT_TOL * d0[k]):
            flag |= 2
            break
        G[k + 1:, k + 1:] -= (G[k + 1:, k:k + 1] / piv) * G[k:k + 1, k + 1:]
    if flag:
        return ident, flag
    w = torch.zeros(10, dtype=a.dtype)
    for r in range(9, -1, -1):
        w[r] = (G[r, 10] - (G[r, r + 1:10] * w[r + 1:]).sum()) / G[r, r]
    if not bool(torch.isfinite(w).all()):
        return ident, flag | 2
    return w, 0


def _run(img, ref, num_iters, eps, dtype, normal, masks):
    N = img.shape[0]
    out = torch.empty(img.shape, dtype=dtype)
    status = torch.zeros(N, 3, dtype=torch.int32)
    for n in range(N):
        x, r = img[n].reshape(-1, 3).to(dtype), ref[n].reshape(-1, 3).to(dtype)
        mask0 = unclipped(x, eps)
        for it in range(num_iters):
            a = features(x)
            warp = []
            for c in range(3):
                mask = mask0[:, c] & unclipped(x[:, c], eps) & unclipped(r[:, c], eps)
                if masks is not None:
                    masks.append(mask.clone())
                if normal:
                    w, flag = _fit_normal(a, r[:, c], mask, c)
                    status[n, c] |= flag
                else:
                    w = _fit_lstsq(a, r[:, c], mask)
                warp.append(w)
            x = torch.clip(a @ torch.stack(warp, -1), 0, 1)
        out[n] = x.reshape(img.shape[1:])
    return out, status


def color_correct(img, ref, num_iters=5, eps=EPS, dtype=torch.float64, masks=None):
    """img, ref [N,H,W,3] -> corrected [N,H,W,3] in `dtype`, each image on its own; `masks` (a list) collects every round's row masks"""
    return _run(img, ref, num_iters, eps, dtype, False, masks)[0]


def color_correct_normal(img, ref, num_iters=5, eps=EPS, dtype=torch.float64):
    """-> (corrected, status int32 [N,3]) with the kernel's solve and its rule for rank-deficient channels"""
    return _run(img, ref, num_iters, eps, dtype, True, None)


def mse(a, b):
    """per-image mean squared error in fp64 -> [N]"""
    return ((a.double() - b.double()) ** 2).flatten(1).mean(1)


def psnr(m):
    return -10.0 * torch.log10(m)


def make_inputs(N, H, W, seed=0):
    """fp32 CPU (img, ref) [N,H,W,3] of one case: ref is a smooth colour field with noise, img is ref seen through a gain, a bias and
    a quadratic cast that differ per image and channel, with noise of its own; then about 5 % of ref's and 10 % of img's pixels are
    put at exactly 0 or 1 (half each), so that all three terms of the mask matter."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * N + 5 * H + 3 * W)
    y, x = torch.meshgrid((torch.arange(H) + 0.5) / H, (torch.arange(W) + 0.5) / W, indexing="ij")
    img, ref = torch.empty(N, H, W, 3), torch.empty(N, H, W, 3)
    for n in range(N):
        chans = []
        for c in range(3):
            fx, fy, ph = (torch.rand(3, generator=g) * torch.tensor([2.0, 2.0, 2 * math.pi])).tolist()
            chans.append(0.5 + 0.3 * torch.sin(2 * math.pi * ((0.5 + fx) * x + (0.5 + fy) * y) + ph))
        base = torch.stack(chans, -1)
        r = (base + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0.02, 0.98)
        gain = 0.75 + 0.4 * torch.rand(3, generator=g)
        bias = 0.06 * (torch.rand(3, generator=g) - 0.5)
        quad = 0.1 * (torch.rand(3, generator=g) - 0.5)
        i = (gain * r + bias + quad * r * r.roll(1, -1) + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
        u = torch.rand(H, W, generator=g)
        r[u < 0.025], r[(u >= 0.025) & (u < 0.05)] = 0.0, 1.0
        u = torch.rand(H, W, generator=g)
        i[u < 0.05], i[(u >= 0.05) & (u < 0.1)] = 0.0, 1.0
        img[n], ref[n] = i, r
    return img.contiguous(), ref.contiguous()
