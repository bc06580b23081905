"""Evaluation of a scene on views with known images: the reference's third_party_model/anysplat/src/post_opt/simple_trainer.py::eval
(:1177-1270) on the HIP rasteriser and metric kernels.  Each view is rendered on a black background and clamped to [0,1]; the keys
of the result are the reference's:

  psnr          mean over the views of -10 log10(MSE), the MSE of the f32 render against the f32 image (ops.image_mse, fp64 sums)
  ssim          mean of the valid-map SSIM of ops.photometric_loss (the loss kernel's own: fused_ssim(padding="valid"); the
                reference's eval uses torchmetrics' StructuralSimilarityIndexMeasure, whose padding differs)
  lpips         only with an evaluation.lpips.LPIPS: mean LPIPS(VGG)
  cc_psnr       only with color_correct=True: the PSNR after ops.color_correct has fitted the render to the image (the reference
                reports it when bilateral grids are on: a grid absorbs a view's exposure and white balance and is not exported, so a
                held-out view's raw render is off by a smooth colour transform that plain PSNR punishes)
  num_GS        the number of Gaussians
  ellipse_time  seconds per image of the render alone, the device synchronised before and after (the reference's name)
  per_view      one dict per view with the same metric keys (and cc_status, the three status words of the fit)"""
from __future__ import annotations

import time
from math import isqrt

import torch

from .. import ops
from ..models.types import Gaussians
from .trainer import _cameras, _single


def evaluate_views(gaussians: Gaussians, images: torch.Tensor, extrinsics: torch.Tensor, intrinsics: torch.Tensor, *,
                   color_correct: bool = False, lpips=None, antialiased: bool = False) -> dict:
    """`images` f32 [V,H,W,3] in [0,1] on the device, `extrinsics` camera-to-world [V,4,4], `intrinsics` normalised [V,3,3], as
    post_optimize takes them (H, W >= 11 for the SSIM window).  `antialiased`: render in the rasteriser's antialiased mode, as a
    scene fitted with PostOptConfig.antialiased wants to be seen.  Nothing here has a gradient."""
    _single(gaussians)
    if images.dim() != 4 or images.shape[-1] != 3 or images.dtype != torch.float32:
        raise ValueError(f"images must be float32 [V,H,W,3], got {images.dtype} {tuple(images.shape)}")
    V, H, W, _ = images.shape
    if V < 1:
        raise ValueError("evaluate_views: no view to evaluate")
    if tuple(extrinsics.shape) != (V, 4, 4) or tuple(intrinsics.shape) != (V, 3, 3):
        raise ValueError(f"extrinsics [V,4,4] and intrinsics [V,3,3] must match the {V} images, got {tuple(extrinsics.shape)} and "
                         f"{tuple(intrinsics.shape)}")
    if not images.is_cuda or not gaussians.means.is_cuda:
        raise ValueError("images and gaussians must be on the device (the HIP path has no CPU fallback)")
    dev = images.device
    with torch.no_grad():
        means, cov = gaussians.means[0].float().contiguous(), gaussians.covariances[0].float().contiguous()
        sh, op = gaussians.harmonics[0].float().contiguous(), gaussians.opacities[0].reshape(-1).float().contiguous()
        sh_degree = isqrt(sh.shape[-1]) - 1
        view, campos, Kpix = _cameras(extrinsics.detach(), intrinsics.detach(), W, H, dev)
        images = images.detach().contiguous()
        background = torch.zeros(3, device=dev, dtype=torch.float32)
        ws = ops.GsWorkspace()
        renders, seconds = [], 0.0
        for j in range(V):
            torch.cuda.synchronize(dev)
            tic = time.perf_counter()
            color, _, _ = ops.gs_render(means, cov, sh, op, view[j:j + 1], campos[j:j + 1], Kpix[j:j + 1], W, H, sh_degree=sh_degree,
                                        sh_layout=1, background=background, clamp_rgb=True, workspace=ws,
                                        rasterize_mode="antialiased" if antialiased else "classic")
            torch.cuda.synchronize(dev)
            seconds += time.perf_counter() - tic
            renders.append(color.clamp(0, 1))
        render = torch.cat(renders)
        cols = dict(psnr=-10.0 * torch.log10(ops.image_mse(render, images)),
                    ssim=torch.stack([ops.photometric_loss(render[j:j + 1], images[j:j + 1], 0.2)[2] for j in range(V)]))
        if lpips is not None:
            cols["lpips"] = lpips(render.permute(0, 3, 1, 2).contiguous(), images.permute(0, 3, 1, 2).contiguous()).to(dev)
        status = None
        if color_correct:
            _, cc_mse, status = ops.color_correct(render, images)
            cols["cc_psnr"] = -10.0 * torch.log10(cc_mse)
        host = {k: v.double().cpu().tolist() for k, v in cols.items()}
        status = None if status is None else status.cpu().tolist()
    out = {k: sum(v) / V for k, v in host.items()}
    out["num_GS"] = int(means.shape[0])
    out["ellipse_time"] = seconds / V
    out["per_view"] = [dict({k: host[k][j] for k in host}, **({} if status is None else {"cc_status": status[j]})) for j in range(V)]
    return out
