"""Host-side checks of the post-optimisation's depth term (no GPU): the plain-torch oracle of tests/depth_loss_oracle.py against plain
indexing, single-pixel closed forms and finite differences, the new config fields, and the argument errors of ops.depth_loss and
post_optimize that fire before any device call."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import depth_loss_oracle as DO  # noqa: E402


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (13, 37), (45, 70)])
def test_oracle_at_integer_points_is_plain_indexing(shape):
    """grid_sample(align_corners=True) at the integer coordinates returns the pixels, exactly, and its gradient is one per point"""
    H, W = shape
    g = torch.Generator().manual_seed(H * W)
    ed = torch.rand(H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    ys, xs = torch.nonzero(torch.rand(H, W, generator=g) < 0.7, as_tuple=True)
    if len(ys) == 0:
        ys, xs = torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    got = DO.sample(ed, torch.stack([xs, ys], -1).double())
    assert torch.equal(got.detach(), ed.detach()[ys, xs])
    w = torch.rand(len(ys), generator=g, dtype=torch.float64)
    grad, = torch.autograd.grad((got * w).sum(), ed)
    want = torch.zeros(H, W, dtype=torch.float64)
    want[ys, xs] = w
    assert torch.equal(grad, want)
    # the whole loss against the same formula by indexing
    depth = torch.rand(2, H, W, generator=g, dtype=torch.float64) * 5
    alpha = torch.rand(2, H, W, generator=g, dtype=torch.float64)
    gt = 0.5 + 9.5 * torch.rand(2, H, W, generator=g, dtype=torch.float64)
    gt[0, 0, 0] = 0.0
    mask = torch.rand(2, H, W, generator=g) < 0.7
    loss, count = DO.depth_loss(depth, alpha, gt, mask, scale=1.5)
    used = mask & (gt > 0)
    e = depth / alpha.clamp(min=1e-10)
    disp = torch.where(e > 0, 1 / e, torch.zeros_like(e))
    assert count == int(used.sum())
    if count:
        want = (disp - 1 / gt)[used].abs().sum() / count * 1.5
        assert abs(float(loss) - float(want)) <= 1e-14 * abs(float(want))
    else:
        assert float(loss) == 0.0


def test_single_pixel_closed_forms():
    t = lambda v: torch.tensor([[[v]]], dtype=torch.float64)
    depth, alpha = t(2.0).requires_grad_(True), t(0.5).requires_grad_(True)
    loss, count = DO.depth_loss(depth, alpha, t(2.0))
    gd, ga = torch.autograd.grad(loss, (depth, alpha))
    assert count == 1 and float(DO.expected_depth(depth, alpha).detach()) == 4.0
    assert float(loss.detach()) == 0.25 and float(gd) == 0.125 and float(ga) == -0.5
    # scale multiplies, an unused pixel contributes nothing, an empty selection is (0, zero gradients)
    assert float(DO.depth_loss(depth, alpha, t(2.0), scale=3.0)[0].detach()) == 0.75
    for gt, mask in ((t(0.0), None), (t(-1.0), None), (t(float("inf")), None), (t(float("nan")), None), (t(2.0), torch.zeros(1, 1, 1, dtype=torch.bool))):
        loss, count = DO.depth_loss(depth, alpha, gt, mask)
        gd, ga = torch.autograd.grad(loss, (depth, alpha))
        assert count == 0 and float(loss) == 0.0 and float(gd) == 0.0 and float(ga) == 0.0
    # E <= 0: disparity 0, the term is 1 / gt and carries no gradient
    d0 = t(0.0).requires_grad_(True)
    loss, count = DO.depth_loss(d0, alpha, t(2.0))
    assert count == 1 and float(loss) == 0.5 and float(torch.autograd.grad(loss, d0)[0]) == 0.0
    # alpha under the clamp: E = depth / 1e-10, no gradient for alpha
    a0 = t(1e-12).requires_grad_(True)
    loss, _ = DO.depth_loss(depth, a0, t(2.0))
    gd, ga = torch.autograd.grad(loss, (depth, a0))
    assert float(ga) == 0.0 and float(gd) != 0.0 and float(loss) == pytest.approx(0.5 - 1e-10 / 2.0, rel=1e-12)


def test_oracle_autograd_matches_finite_differences():
    """fp64, 5 x 7, every pixel at least 1e-2 away from the kink disp == 1 / gt, central differences with h = 1e-6"""
    g = torch.Generator().manual_seed(11)
    H, W = 5, 7
    alpha = 0.2 + 0.8 * torch.rand(1, H, W, generator=g, dtype=torch.float64)
    e = 0.5 + 4 * torch.rand(1, H, W, generator=g, dtype=torch.float64)
    depth = e * alpha
    gt = 1 / (1 / e + torch.where(torch.rand(1, H, W, generator=g) < 0.5, -1.0, 1.0) * (0.02 + 0.05 * torch.rand(1, H, W, generator=g, dtype=torch.float64)))
    mask = torch.rand(1, H, W, generator=g) < 0.7
    assert bool((gt > 0).all()) and float(((1 / e - 1 / gt).abs()).min()) > 1e-2
    dl, al = depth.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    loss, count = DO.depth_loss(dl, al, gt, mask, scale=2.0)
    gd, ga = torch.autograd.grad(loss, (dl, al))
    assert 0 < count < H * W
    h = 1e-6
    for name, base, grad in (("depth", depth, gd), ("alpha", alpha, ga)):
        fd = torch.zeros_like(base)
        for i in range(base.numel()):
            p, m = base.clone().reshape(-1), base.clone().reshape(-1)
            p[i] += h
            m[i] -= h
            args = lambda x: (x.reshape(base.shape), alpha) if name == "depth" else (depth, x.reshape(base.shape))
            fd.reshape(-1)[i] = (DO.depth_loss(*args(p), gt, mask, scale=2.0)[0] - DO.depth_loss(*args(m), gt, mask, scale=2.0)[0]) / (2 * h)
        # truncation h^2 f''' / 6 ~ 1e-12 and rounding 1e-16 / h ~ 1e-10 of a loss of order 0.05
        assert float((fd - grad).abs().max()) <= 1e-8, name
        assert bool((grad[~mask] == 0).all()) and float(grad.abs().max()) > 0


def test_config_depth_fields_are_the_reference_names_and_defaults():
    from dataclasses import fields
    from vist3a_amd.post_opt import PostOptConfig
    c = PostOptConfig()
    assert (c.depth_loss, c.depth_lambda, c.scene_scale) == (False, 1e-2, 1.0)
    assert {"depth_loss", "depth_lambda", "scene_scale"} <= {f.name for f in fields(PostOptConfig)}
    assert PostOptConfig(depth_loss=True, depth_lambda=0.1).depth_lambda == 0.1


def test_depth_loss_argument_errors():
    from vist3a_amd import ops
    z = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="device"):
        ops.depth_loss(z, z, z)
    with pytest.raises(NotImplementedError, match="depth_gt"):
        ops.depth_loss(z, z, z.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"\[C,H,W\]"):
        ops.depth_loss(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError):
        ops.depth_loss(z.double(), z, z)


def _gaussians(U=20):
    from vist3a_amd.models.types import Gaussians
    return Gaussians(means=torch.zeros(1, U, 3), covariances=torch.zeros(1, U, 3, 3), harmonics=torch.zeros(1, U, 3, 4),
                     opacities=torch.full((1, U), 0.5), scales=torch.ones(1, U, 3), rotations=torch.ones(1, U, 4))


def test_post_optimize_depth_argument_errors():
    from vist3a_amd.post_opt import PostOptConfig, post_optimize
    img, ext, K = torch.zeros(2, 16, 16, 3), torch.eye(4).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1)
    on = PostOptConfig(depth_loss=True)
    with pytest.raises(ValueError, match="depths"):
        post_optimize(_gaussians(), img, ext, K, on, steps=1)
    for bad in (torch.zeros(2, 16, 15), torch.zeros(1, 16, 16), torch.zeros(2, 16, 16, 1), torch.zeros(2, 16, 16, dtype=torch.float64)):
        with pytest.raises(ValueError, match="depths"):
            post_optimize(_gaussians(), img, ext, K, on, steps=1, depths=bad)
    for bad in (torch.zeros(2, 16, 15, dtype=torch.bool), torch.zeros(2, 16, 16)):
        with pytest.raises(ValueError, match="depth_masks"):
            post_optimize(_gaussians(), img, ext, K, on, steps=1, depths=torch.ones(2, 16, 16), depth_masks=bad)
