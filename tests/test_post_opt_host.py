"""Host-side checks of the post-optimisation feature (no GPU): the plain-torch loss oracle against the reference's own numbers in
tests/golden/ssim_loss_ref.safetensors, the closed-form activation backward against autograd, the config, the view order and
post_optimize's argument errors."""
import sys
from pathlib import Path

import pytest
import torch
from safetensors.torch import load_file

sys.path.insert(0, str(Path(__file__).resolve().parent))
import post_opt_oracle as PO  # noqa: E402
import ssim_loss_oracle as SO  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden" / "ssim_loss_ref.safetensors"
CASES = [f"{s}.{k}" for s in ("11x11", "13x37", "45x70") for k in ("smooth", "noise")]


@pytest.mark.parametrize("case", CASES)
def test_loss_oracle_is_the_reference_in_fp64(case):
    """Both sides are fp64 and the same formula (same float32-built taps): only the summation order separates them -> 1e-12 relative."""
    t = load_file(str(GOLD))
    x = (t[case + ".x"].float() / 255).double().requires_grad_(True)
    y = (t[case + ".y"].float() / 255).double()
    loss, l1, s = SO.photometric_loss(x, y, 1.0)
    g, = torch.autograd.grad(s, x)
    loss, l1, s = loss.detach(), l1.detach(), s.detach()
    assert abs(float(s) - float(t[case + ".ssim64"])) <= 1e-12 * max(1.0, abs(float(t[case + ".ssim64"])))
    assert abs(float(l1) - float(t[case + ".l164"])) <= 1e-12
    assert float(loss) == pytest.approx(1 - float(s), abs=1e-15)
    ref = t[case + ".g_ssim64"]
    assert float((g - ref).norm() / ref.norm()) < 1e-12
    with pytest.raises(ValueError):
        SO.ssim(x[:, :10], y[:, :10])


def test_activation_backward_closed_form_matches_autograd():
    ls, q, lg, G, Gu, d_op = PO.activation_case(400, 5)
    for Gin in (G, Gu):
        lv = [t.clone().requires_grad_(True) for t in (ls, q, lg)]
        cov, op = PO.splat_activate(*lv)
        want = torch.autograd.grad((cov * Gin).sum() + (op * d_op).sum(), lv)
        got = PO.splat_activate_backward(ls, q, lg, Gin, d_op)
        for name, a, b in zip(("log_scales", "quats", "logits"), got, want):
            assert float((a - b).norm() / b.norm()) < 1e-12, name
    # the upper-triangle convention: an upper entry carrying both symmetric positions gives the gradient of the symmetric one
    sym = G + G.transpose(-1, -2)
    up = torch.triu(sym, 1) + torch.diag_embed(torch.diagonal(G, dim1=-2, dim2=-1))
    a = PO.splat_activate_backward(ls, q, lg, up, d_op)
    lv = [t.clone().requires_grad_(True) for t in (ls, q, lg)]
    cov, op = PO.splat_activate(*lv)
    want = torch.autograd.grad((torch.triu(cov) * up).sum() + (op * d_op).sum(), lv)
    for x_, w_ in zip(a, want):
        assert float((x_ - w_).norm() / w_.norm()) < 1e-12


def test_config_defaults_are_the_reference_numbers():
    from vist3a_amd.post_opt import PostOptConfig
    c = PostOptConfig()
    assert (c.max_steps, c.ssim_lambda) == (3000, 0.2)
    assert (c.lr_means, c.lr_scales, c.lr_quats, c.lr_opacities, c.lr_sh) == (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3)
    assert tuple(c.betas) == (0.9, 0.999) and c.eps == 1e-15 and c.min_opacity == 0.01
    assert set(c.params) == {"means", "scales", "quats", "opacities", "sh0", "shN"} and c.seed == 0
    assert c.trained() == ("means", "scales", "quats", "opacities", "sh")
    assert PostOptConfig(params=("opacities", "sh")).trained() == ("opacities", "sh")
    with pytest.raises(ValueError):
        PostOptConfig(params=("sh0",)).trained()
    with pytest.raises(ValueError):
        PostOptConfig(params=("poses",)).trained()


def test_view_order_is_a_seeded_permutation_per_epoch():
    from vist3a_amd.post_opt import view_order
    a, b, c = view_order(5, 13, 7), view_order(5, 13, 7), view_order(5, 13, 8)
    assert a == b and a != c and len(a) == 13
    assert sorted(a[:5]) == sorted(a[5:10]) == list(range(5)) and set(a[10:]) <= set(range(5)) and len(set(a[10:])) == 3
    g = torch.Generator().manual_seed(7)
    assert a[:5] == torch.randperm(5, generator=g).tolist()


def _gaussians(B, U=20):
    from vist3a_amd.models.types import Gaussians
    return Gaussians(means=torch.zeros(B, U, 3), covariances=torch.zeros(B, U, 3, 3), harmonics=torch.zeros(B, U, 3, 4),
                     opacities=torch.full((B, U), 0.5), scales=torch.ones(B, U, 3), rotations=torch.ones(B, U, 4))


def test_post_optimize_argument_errors():
    from vist3a_amd.post_opt import PostOptConfig, post_optimize
    img, ext, K = torch.zeros(2, 16, 16, 3), torch.eye(4).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="batch dimension 1"):
        post_optimize(_gaussians(2), img, ext, K, PostOptConfig(), steps=1)
    with pytest.raises(NotImplementedError, match="extrinsics"):
        post_optimize(_gaussians(1), img, ext.clone().requires_grad_(True), K, PostOptConfig(), steps=1)
    with pytest.raises(NotImplementedError, match="intrinsics"):
        post_optimize(_gaussians(1), img, ext, K.clone().requires_grad_(True), PostOptConfig(), steps=1)
    for bad in (torch.zeros(2, 3, 16, 16), torch.zeros(16, 16, 3), torch.zeros(2, 16, 16, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="images"):
            post_optimize(_gaussians(1), bad, ext, K, PostOptConfig(), steps=1)
    with pytest.raises(ValueError, match="match"):
        post_optimize(_gaussians(1), img, ext[:1], K, PostOptConfig(), steps=1)
