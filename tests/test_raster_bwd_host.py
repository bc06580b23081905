"""Host-side checks for the rasteriser's backward pass (csrc/raster_bwd.hip), no GPU needed.

  * the two new C entry points validate their arguments before any launch, and the workspace query grows with the capacity;
  * the YARDSTICK of tests/test_raster_bwd_gpu.py is trustworthy: torch.autograd through oracle/gsplat_raster.py
    (project -> sh_colors -> rasterize, composite order fixed beforehand in fp32) gives the same gradients in fp32 and fp64, and
    the fp64 gradients agree with central finite differences, for each of means, covars, sh and opacities.

Bounds (reasoned, not fitted): fp32 against fp64, relative L2 per tensor < 1e-4 - a gradient entry is a sum of at most a few
thousand pixel-Gaussian terms, each a product of ~10 fp32-rounded factors, so eps_fp32 (6e-8) x ~2000 is the worst linear growth
(measured here: 3e-7 .. 2.3e-6).  Finite differences: central, fp64, h = 1e-6 along random directions.  The smallest parameter
scale is a covariance entry (~0.05), so the relative step is ~2e-5 and the truncation term ~(2e-5)^2 = 4e-10 times a modest
derivative ratio; rounding is |loss| x 2^-53 / h ~ 1e3 x 1e-16 / 1e-6 = 1e-7 against directional derivatives of order 1 .. 10.
The bound is 1e-6 relative (absolute below 1): above both terms, two digits below anything an fp32 effect or a wrong term in
the oracle's graph would produce.  (h = 1e-5 leaves 2.5e-6 of truncation on the covariances: measured, which is why h is 1e-6.)"""
import ctypes
import math

import pytest
import torch

from oracle import gsplat_raster as G


def _scene(U, seed, spread=1.5, scale=0.15, z0=4.0, K=25):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(U, 3, generator=g) * torch.tensor([spread, spread, 1.0]) + torch.tensor([0.0, 0.0, z0])
    A = torch.randn(U, 3, 3, generator=g) * scale
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)
    sh = torch.randn(U, 3, 25, generator=g)[:, :, :K] * 0.3
    op = torch.rand(U, generator=g)
    return means, cov, sh, op


def _camera(W, H, f, yaw=0.2, t=(0.1, -0.2, 0.3)):
    c, s = math.cos(yaw), math.sin(yaw)
    view = torch.eye(4)
    view[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    view[:3, 3] = torch.tensor(t)
    K = torch.tensor([[f, 0, W / 2], [0, f * 1.1, H / 2], [0, 0, 1.0]])
    return view, K


def test_backward_entry_points_validate_without_gpu():
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_gs_rasterize_backward(None, None) == -1
    assert L.v3a_gs_project_backward(None, None) == -1
    a = lib.GsRasterizeBackwardArgs()
    assert L.v3a_gs_rasterize_backward(ctypes.byref(a), None) == -1          # null pointers
    for f in ("radii", "means2d", "conics", "colors", "opacities", "tile_offsets", "flatten_ids", "d_color", "d_depth", "d_alpha",
              "d_means2d", "d_conics", "d_colors", "d_opacity_partial", "workspace"):
        setattr(a, f, 1)
    a.U, a.C, a.width, a.height, a.n_isect = 10, 1, 0, 16, 5
    assert L.v3a_gs_rasterize_backward(ctypes.byref(a), None) == -2          # width 0
    a.width, a.n_isect = 16, -1
    assert L.v3a_gs_rasterize_backward(ctypes.byref(a), None) == -1          # negative count
    a.n_isect, a.workspace_bytes = 5, 16
    assert L.v3a_gs_rasterize_backward(ctypes.byref(a), None) == -4          # workspace too small
    a.flatten_ids = None
    assert L.v3a_gs_rasterize_backward(ctypes.byref(a), None) == -1          # intersections without their list
    p = lib.GsProjectBackwardArgs()
    assert L.v3a_gs_project_backward(ctypes.byref(p), None) == -1
    for f in ("means", "covars", "sh", "viewmat", "campos", "K", "radii", "d_means2d", "d_conics", "d_colors", "d_opacity_partial",
              "d_means", "d_covars", "d_sh", "d_opacities"):
        setattr(p, f, 1)
    p.U, p.C, p.width, p.height, p.sh_k, p.sh_degree, p.sh_layout = 10, 1, 16, 16, 25, 5, 1
    assert L.v3a_gs_project_backward(ctypes.byref(p), None) == -2            # degree 5
    p.sh_degree, p.sh_k = 4, 16
    assert L.v3a_gs_project_backward(ctypes.byref(p), None) == -2            # 16 coefficients cannot hold degree 4
    p.sh_k, p.sh_layout = 25, 2
    assert L.v3a_gs_project_backward(ctypes.byref(p), None) == -1            # unknown layout
    p.sh_layout, p.C = 1, 0
    assert L.v3a_gs_project_backward(ctypes.byref(p), None) == -2
    p.C, p.U = 1, 0
    assert L.v3a_gs_project_backward(ctypes.byref(p), None) == 0             # nothing to do, nothing launched


def test_backward_workspace_query():
    from vist3a_amd import lib
    L = lib.load()
    q = L.v3a_gs_rasterize_backward_workspace_bytes
    a, b = q(1000, 2, 64, 48, 1000), q(1000, 2, 64, 48, 100000)
    assert a > 0 and b - a >= 48 * (100000 - 1000) - 512                     # one 48-byte row per intersection
    assert q(2000, 2, 64, 48, 1000) > a                                      # two counters per entry
    assert q(0, 1, 64, 48, 10) == -2 and q(10, 1, 64, 48, 0) == -2 and q(10, 1, 0, 48, 10) == -2


def _oracle_loss(dtype, leaves, view, K, W, H, deg, mask, offs, ids, wimg, walpha, monkeypatch):
    """Random linear functional of the clamped white-background render, computed by the oracle in `dtype` with a fixed order."""
    means, cov, sh, op = leaves
    with monkeypatch.context() as m:
        m.setattr(G, "f32", dtype)
        pr = G.project(means, cov, view.to(dtype), K.to(dtype), W, H)
        campos = torch.linalg.inv(view.double())[:3, 3].to(dtype)
        col = G.sh_colors(means, campos, sh.permute(0, 2, 1), deg) * mask[:, None]
        col4 = torch.cat([col, pr["depths"][:, None]], -1)
        img, alpha = G.rasterize(pr["means2d"], pr["conics"], col4, op, W, H, offs, ids, torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=dtype))
    return (img[..., :3].clamp(0, 1) * wimg[..., :3].to(dtype)).sum() + (img[..., 3] * wimg[..., 3].to(dtype)).sum() + \
        (alpha * walpha.to(dtype)).sum()


def _fixed_order(means, cov, view, K, W, H):
    pr = G.project(means, cov, view, K, W, H)
    offs, ids = G.bin_and_sort(pr["means2d"], pr["radii"], pr["depths"], W, H)   # fp32: reinterprets depth bits
    return pr["radii"] > 0, offs, ids


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("U,W,H,deg", [(300, 64, 48, 4), (120, 40, 33, 2)])
def test_oracle_autograd_fp32_matches_fp64(monkeypatch, U, W, H, deg):
    means, cov, sh, op = _scene(U, 1, scale=0.25, K=(deg + 1) ** 2)
    view, K = _camera(W, H, 60.0)
    mask, offs, ids = _fixed_order(means, cov, view, K, W, H)
    assert int(mask.sum()) > U // 2 and len(ids) > U
    g = torch.Generator().manual_seed(5)
    wimg, walpha = torch.randn(H, W, 4, generator=g), torch.randn(H, W, generator=g)
    grads = {}
    for dt in (torch.float32, torch.float64):
        leaves = [t.detach().clone().to(dt).requires_grad_(True) for t in (means, cov, sh, op)]
        _oracle_loss(dt, leaves, view, K, W, H, deg, mask, offs, ids, wimg, walpha, monkeypatch).backward()
        grads[dt] = [t.grad for t in leaves]
    for name, a, b in zip(("means", "covars", "sh", "opacities"), grads[torch.float32], grads[torch.float64]):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        e = _rel(a, b)
        print(f"oracle fp32 vs fp64 d_{name}: {e:.2e}")
        assert e < 1e-4, (name, e)
    # the covariance gradient follows "the upper triangle is used"
    assert float(grads[torch.float64][1][:, [1, 2, 2], [0, 0, 1]].abs().max()) == 0


def test_oracle_autograd_matches_finite_differences(monkeypatch):
    U, W, H, deg = 6, 32, 32, 4
    means, cov, sh, op = _scene(U, 3, spread=0.4, scale=0.3)
    op = 0.2 + 0.6 * op
    view, K = _camera(W, H, 40.0)
    mask, offs, ids = _fixed_order(means, cov, view, K, W, H)
    assert int(mask.sum()) == U
    g = torch.Generator().manual_seed(7)
    wimg, walpha = torch.randn(H, W, 4, generator=g), torch.randn(H, W, generator=g)
    base = [t.double() for t in (means, cov, sh, op)]
    f = lambda xs: _oracle_loss(torch.float64, xs, view, K, W, H, deg, mask, offs, ids, wimg, walpha, monkeypatch)
    leaves = [t.clone().requires_grad_(True) for t in base]
    f(leaves).backward()
    h = 1e-6
    for i, name in enumerate(("means", "covars", "sh", "opacities")):
        for trial in range(3):
            d = torch.randn(base[i].shape, generator=g, dtype=torch.float64)
            if name == "covars":
                d = torch.triu(d)          # only the upper triangle is an input
            plus = [t if j != i else t + h * d for j, t in enumerate(base)]
            minus = [t if j != i else t - h * d for j, t in enumerate(base)]
            with torch.no_grad():
                fd = float(f(plus) - f(minus)) / (2 * h)
            an = float((leaves[i].grad * d).sum())
            print(f"finite differences d_{name} [{trial}]: analytic {an:+.9e} numeric {fd:+.9e}")
            assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (name, trial, an, fd)
