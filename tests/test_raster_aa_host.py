"""Host-side checks for the rasteriser's antialiased mode and the post-optimisation options that came with it; no GPU needed.

The closed-form compensation gradient the HIP backward uses (tests/raster_aa_oracle.py::dcomp_dcov2d, the formula of
include/vist3a_hip.h) against fp64 autograd of the definition; the oracle's own 2D covariance against oracle/gsplat_raster.py;
argument validation of the C ABI through the loaded library (no launch happens); PostOptConfig, the CLI and the log's columns."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

from oracle import gsplat_raster as G

sys.path.insert(0, str(Path(__file__).resolve().parent))
import raster_aa_oracle as AO  # noqa: E402

ERR_ARG = -1


def _spd(n, seed, scale):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(n, 2, 2, generator=g, dtype=torch.float64) * scale
    return A @ A.transpose(1, 2) + 1e-6 * torch.eye(2, dtype=torch.float64)


@pytest.mark.parametrize("scale", [3.0, 0.5, 0.05])
def test_closed_form_gradient_matches_autograd(scale):
    """d comp / d Sigma2 = ((1 - r) B^-1 - eps det(B^-1) I) / (2 comp) against autograd of sqrt(det S / det(S + eps I)) in fp64, on
    random SPD matrices from well above the blur (comp ~ 1) to well below it (comp ~ 0.01): within 1e-12."""
    S = _spd(200, 7, scale).requires_grad_(True)
    comp = AO.compensation(S)
    (auto,) = torch.autograd.grad(comp.sum(), S)
    closed = AO.dcomp_dcov2d(S.detach())
    err = float((auto - closed).abs().max() / auto.abs().max())
    print(f"[aa closed form, scale {scale}] comp {float(comp.min()):.3e} .. {float(comp.max()):.3e}, max abs err / max {err:.3e}")
    assert float(comp.min()) > 0 and float(comp.max()) < 1
    assert err < 1e-12


def test_compensation_range_and_zero_matrix():
    S = torch.cat([_spd(100, 8, 1.0), _spd(100, 9, 0.01), torch.zeros(1, 2, 2, dtype=torch.float64)]).requires_grad_(True)
    comp = AO.compensation(S)
    assert bool(((comp >= 0) & (comp <= 1)).all())
    assert float(comp[-1]) == 0.0
    (g,) = torch.autograd.grad(comp.sum(), S)
    assert bool(torch.isfinite(g).all()) and float(g[-1].abs().max()) == 0.0
    assert float(AO.dcomp_dcov2d(S.detach())[-1].abs().max()) == 0.0


def test_oracle_cov2d_is_the_projection_s(monkeypatch):
    """raster_aa_oracle.cov2d restates oracle/gsplat_raster.py::project up to the blur: the inverse of its S + eps2d I is project's conic."""
    g = torch.Generator().manual_seed(3)
    U, W, H = 50, 64, 48
    means = torch.randn(U, 3, generator=g, dtype=torch.float64) * torch.tensor([1.5, 1.5, 1.0]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(U, 3, 3, generator=g, dtype=torch.float64) * 0.2
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3, dtype=torch.float64)
    view = torch.eye(4, dtype=torch.float64)
    view[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    K = torch.tensor([[60.0, 0, W / 2], [0, 66.0, H / 2], [0, 0, 1.0]], dtype=torch.float64)
    monkeypatch.setattr(G, "f32", torch.float64)
    pr = G.project(means, cov, view, K, W, H)
    S = AO.cov2d(means, cov, view, K, W, H)
    B = S + 0.3 * torch.eye(2, dtype=torch.float64)
    X = torch.linalg.inv(B)
    vis = pr["radii"] > 0
    assert int(vis.sum()) > 10
    got = torch.stack([X[:, 0, 0], X[:, 0, 1], X[:, 1, 1]], -1)
    assert torch.allclose(got[vis], pr["conics"][vis], rtol=1e-12, atol=0)


def _project_args(lib):
    a = lib.GsProjectArgs()
    for f in ("means", "covars", "sh", "viewmat", "campos", "K", "radii", "means2d", "depths", "conics", "colors"):
        setattr(a, f, 1)          # non-null, never dereferenced: validation returns before any launch
    a.sh_layout, a.sh_k, a.sh_degree = 1, 25, 4
    a.U, a.C, a.width, a.height = 10, 1, 16, 16
    return a


def test_argument_validation_without_gpu():
    """The struct tails: zero means classic; a mode other than 0 / 1 and mode 1 without its array are refused before any launch."""
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_abi_version() == lib.EXPECTED_ABI >= 30
    a = _project_args(lib)
    a.rasterize_mode = 2
    assert L.v3a_gs_project(C.byref(a), None) == ERR_ARG
    a.rasterize_mode, a.compensations = 1, None
    assert L.v3a_gs_project(C.byref(a), None) == ERR_ARG
    b = lib.GsProjectBackwardArgs()
    for f in ("means", "covars", "sh", "viewmat", "campos", "K", "radii", "d_means2d", "d_conics", "d_colors", "d_opacity_partial", "d_means",
              "d_covars", "d_sh", "d_opacities"):
        setattr(b, f, 1)
    b.sh_layout, b.sh_k, b.sh_degree = 1, 25, 4
    b.U, b.C, b.width, b.height = 10, 1, 16, 16
    b.rasterize_mode = 2
    assert L.v3a_gs_project_backward(C.byref(b), None) == ERR_ARG
    b.rasterize_mode, b.opacities = 1, None
    assert L.v3a_gs_project_backward(C.byref(b), None) == ERR_ARG
    # the new reduction: null pointers, bad sizes, a workspace that is too small or misaligned
    assert L.v3a_splat_reg(None, None, 4, None, None, 0, None) == ERR_ARG
    assert L.v3a_splat_reg_backward(None, None, 4, None, None, None, None) == ERR_ARG
    assert L.v3a_splat_reg_workspace_bytes(0) == -2 and L.v3a_splat_reg_workspace_bytes(1 << 30) == -2
    assert L.v3a_splat_reg_workspace_bytes(1) == 16
    assert L.v3a_splat_reg(8, 8, 4, 8, 8, 8, None) == -4 and L.v3a_splat_reg(8, 8, 4, 8, 4, 1024, None) == -4
    assert L.v3a_splat_reg(8, 8, 0, 8, 8, 1024, None) == -2


def test_unknown_mode_raises_value_error():
    from vist3a_amd import ops
    from vist3a_amd.models.decoder_splatting import DecoderSplattingCUDA
    t = torch.zeros(1, 3)
    with pytest.raises(ValueError, match="rasterize_mode"):
        ops.gs_project(t, t, t, t, t, t, 16, 16, rasterize_mode="mip")
    with pytest.raises(ValueError, match="rasterize_mode"):
        ops.gs_render(t, t, t, t, t, t, t, 16, 16, rasterize_mode="Antialiased")
    with pytest.raises(ValueError, match="rasterize_mode"):
        ops.gs_project_backward(t, t, t, t, t, t, 16, 16, t, {}, rasterize_mode="")
    with pytest.raises(ValueError, match="rasterize_mode"):
        DecoderSplattingCUDA(device="cpu", rasterize_mode="mip")


def test_config_cli_and_log_columns():
    from vist3a_amd.post_opt import PostOptConfig, log_columns, random_backgrounds, view_order
    from vist3a_amd.utils.argument import inference_vist3a_argument
    cfg = PostOptConfig()
    assert (cfg.antialiased, cfg.random_bkgd, cfg.opacity_reg, cfg.scale_reg) == (False, False, 0.0, 0.0)
    assert log_columns(cfg) == ["loss", "l1", "ssim"]
    assert log_columns(PostOptConfig(opacity_reg=0.01)) == ["loss", "l1", "ssim", "opacity_mean"]
    assert log_columns(PostOptConfig(scale_reg=0.01)) == ["loss", "l1", "ssim", "scale_mean"]
    assert log_columns(PostOptConfig(depth_loss=True, use_bilateral_grid=True, opacity_reg=0.01, scale_reg=0.01)) == [
        "loss", "l1", "ssim", "depth_term", "bilagrid_tv", "opacity_mean", "scale_mean"]
    req = ["--checkpoint_path", "c", "--transformer_lora_path", "l", "--input_texts_path", "t"]
    ns = inference_vist3a_argument().parse_args(req)
    assert (ns.post_opt_antialiased, ns.post_opt_random_bkgd, ns.post_opt_opacity_reg, ns.post_opt_scale_reg) == (False, False, 0.0, 0.0)
    ns = inference_vist3a_argument().parse_args(req + ["--post_opt_antialiased", "--post_opt_random_bkgd", "--post_opt_opacity_reg", "0.01",
                                                 "--post_opt_scale_reg", "0.02"])
    assert (ns.post_opt_antialiased, ns.post_opt_random_bkgd, ns.post_opt_opacity_reg, ns.post_opt_scale_reg) == (True, True, 0.01, 0.02)
    # the backgrounds: reproducible, in [0, 1), from a generator of their own (the view order of a seed does not depend on them)
    b = random_backgrounds(7, 5)
    assert b.shape == (7, 3) and b.dtype == torch.float32 and torch.equal(b, random_backgrounds(7, 5))
    assert torch.equal(b[:4], random_backgrounds(4, 5)) and not torch.equal(b, random_backgrounds(7, 6))
    assert bool(((b >= 0) & (b < 1)).all())
    g = torch.Generator().manual_seed(6)
    assert torch.equal(b[0], torch.rand(3, generator=g))
    assert view_order(3, 7, 5) == view_order(3, 7, 5)
