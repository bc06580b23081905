"""Post-optimisation: losses, bilateral grids, parameter activation, Adam and the two strategies."""
import ctypes as C
from typing import Optional

import torch

from .. import lib as L
from .common import _f32_dev, _i32_dev, _ptr, _stream, _tensor, _workspace, f32
from .scene import SPLAT_TENSORS, _splat_dicts


# ------------------------------------------------------------------------------------------------ post-optimisation (csrc/ssim_loss.hip, csrc/post_opt.hip)
class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, ssim_lambda):
        N, H, W, Cc = pred.shape
        lib = L.load()
        dev = pred.device
        ws, ws_bytes = _workspace(lib.v3a_photometric_loss_workspace_bytes(N, H, W, Cc),
                                  f"v3a_photometric_loss_workspace_bytes (shape {tuple(pred.shape)}; H, W >= 11 and C <= 4 required)", dev)
        planes = None
        if ctx.needs_input_grad[0]:
            planes = torch.empty(int(lib.v3a_photometric_loss_planes_bytes(N, H, W, Cc)) // 8, device=dev, dtype=torch.float64)
        out = torch.empty(3, device=dev, dtype=torch.float64)
        args = L.PhotometricLossArgs(_ptr(pred), _ptr(target), N, H, W, Cc, float(ssim_lambda), _ptr(out), _ptr(ws), ws_bytes,
                                     _ptr(planes), planes.numel() * 8 if planes is not None else 0)
        L.check(lib.v3a_photometric_loss_forward(C.byref(args), _stream()), "v3a_photometric_loss_forward")
        if planes is not None:
            ctx.save_for_backward(pred, target, planes)
        ctx.ssim_lambda = float(ssim_lambda)
        return out[0], out[1], out[2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, d_l1, d_ssim):
        pred, target, planes = ctx.saved_tensors
        N, H, W, Cc = pred.shape
        z = torch.zeros((), device=pred.device, dtype=torch.float64)
        d_out = torch.stack([z if g is None else g.to(torch.float64).reshape(()) for g in (d_loss, d_l1, d_ssim)])
        d_pred = torch.empty_like(pred)
        args = L.PhotometricLossArgs(_ptr(pred), _ptr(target), N, H, W, Cc, ctx.ssim_lambda, None, None, 0, _ptr(planes), planes.numel() * 8)
        L.check(L.load().v3a_photometric_loss_backward(C.byref(args), _ptr(d_out), _ptr(d_pred), _stream()), "v3a_photometric_loss_backward")
        return d_pred, None, None


def photometric_loss(pred: torch.Tensor, target: torch.Tensor, ssim_lambda: float = 0.2):
    """(1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM) of f32 images [N,H,W,C] (C <= 4, H, W >= 11; the layout gs_render emits),
    SSIM as the reference's loss_ssim.py::ssim(data_range=1.0) on the valid map = fused_ssim(padding="valid") (csrc/ssim_loss.hip).
    -> (loss, l1, ssim): float64 scalars on the device, differentiable with respect to `pred` (HIP backward, first order only).
    `target` is a constant: one that requires grad is refused."""
    if target.requires_grad:
        raise NotImplementedError("photometric_loss: no gradient for target (it is a constant of the loss); detach it")
    if pred.dim() != 4:
        raise ValueError(f"photometric_loss: pred must be [N,H,W,C], got {tuple(pred.shape)}")
    _f32_dev(pred, "pred")
    _f32_dev(target, "target", pred.shape)
    return _PhotometricLoss.apply(pred, target, float(ssim_lambda))


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, depth_gt, mask, scale):
        Cc, H, W = depth.shape
        lib = L.load()
        dev = depth.device
        ws, ws_bytes = _workspace(lib.v3a_depth_loss_workspace_bytes(Cc, H, W), f"v3a_depth_loss_workspace_bytes (shape {tuple(depth.shape)})", dev)
        out = torch.empty(2, device=dev, dtype=torch.float64)
        args = L.DepthLossArgs(_ptr(depth), _ptr(alpha), _ptr(depth_gt), _ptr(mask), Cc, H, W, float(scale), _ptr(out), _ptr(ws), ws_bytes)
        L.check(lib.v3a_depth_loss_forward(C.byref(args), _stream()), "v3a_depth_loss_forward")
        ctx.save_for_backward(depth, alpha, depth_gt, mask, out)
        ctx.scale = float(scale)
        loss, count = out[0], out[1]
        ctx.mark_non_differentiable(count)
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, _d_count):
        depth, alpha, depth_gt, mask, out = ctx.saved_tensors
        Cc, H, W = depth.shape
        d_out = d_loss.to(torch.float64).reshape(1).contiguous()
        d_depth, d_alpha = torch.empty_like(depth), torch.empty_like(alpha)
        args = L.DepthLossArgs(_ptr(depth), _ptr(alpha), _ptr(depth_gt), _ptr(mask), Cc, H, W, ctx.scale, _ptr(out), None, 0)
        L.check(L.load().v3a_depth_loss_backward(C.byref(args), _ptr(d_out), _ptr(d_depth), _ptr(d_alpha), _stream()), "v3a_depth_loss_backward")
        return d_depth, d_alpha, None, None, None


def depth_loss(depth: torch.Tensor, alpha: torch.Tensor, depth_gt: torch.Tensor, mask: Optional[torch.Tensor] = None, scale: float = 1.0):
    """The reference loop's depth term (simple_trainer.py:943-961) on dense maps (csrc/depth_loss.hip): `depth`, `alpha` f32 [C,H,W]
    as gs_render returns them (depth = the alpha-weighted z), `depth_gt` f32 [C,H,W], `mask` bool / uint8 [C,H,W] (nonzero = use the
    pixel) or None.  loss = scale * mean over the used pixels of |disp - 1 / depth_gt|, disp = 1 / E where E = depth /
    max(alpha, 1e-10) > 0, else 0; a pixel is used where the mask is set and depth_gt is positive and finite.
    -> (loss, count): float64 scalars on the device, count = the number of used pixels (0 gives loss 0 and zero gradients).
    Differentiable with respect to `depth` and `alpha` (HIP backward, first order only); `depth_gt` and `mask` are constants."""
    if depth_gt.requires_grad or (mask is not None and mask.requires_grad):
        raise NotImplementedError("depth_loss: no gradient for depth_gt / mask (they are constants of the loss); detach them")
    if depth.dim() != 3:
        raise ValueError(f"depth_loss: depth must be [C,H,W], got {tuple(depth.shape)}")
    _f32_dev(depth, "depth")
    _f32_dev(alpha, "alpha", depth.shape)
    _f32_dev(depth_gt, "depth_gt", depth.shape)
    if mask is not None:
        _tensor(mask, "mask", (torch.bool, torch.uint8), depth.shape)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)   # the same bytes (a bool is stored as 0 / 1), no copy
    return _DepthLoss.apply(depth, alpha, depth_gt, mask, float(scale))


class _BilagridSlice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, grids):
        N, H, W, _ = rgb.shape
        _, Lz, GY, GX, _ = grids.shape
        out = torch.empty_like(rgb)
        args = L.BilagridSliceArgs(_ptr(rgb), _ptr(grids), N, H, W, GX, GY, Lz)
        L.check(L.load().v3a_bilagrid_slice_forward(C.byref(args), _ptr(out), _stream()),
                f"v3a_bilagrid_slice_forward (rgb {tuple(rgb.shape)}, grids {tuple(grids.shape)})")
        ctx.save_for_backward(rgb, grids)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        rgb, grids = ctx.saved_tensors
        N, H, W, _ = rgb.shape
        _, Lz, GY, GX, _ = grids.shape
        d_out = d_out.float().contiguous()
        d_rgb = torch.empty_like(rgb) if ctx.needs_input_grad[0] else None
        d_grids = torch.empty_like(grids) if ctx.needs_input_grad[1] else None
        args = L.BilagridSliceArgs(_ptr(rgb), _ptr(grids), N, H, W, GX, GY, Lz)
        L.check(L.load().v3a_bilagrid_slice_backward(C.byref(args), _ptr(d_out), _ptr(d_rgb), _ptr(d_grids), _stream()),
                "v3a_bilagrid_slice_backward")
        return d_rgb, d_grids


def _bilagrid_check(grids: torch.Tensor, what: str) -> None:
    if grids.dim() != 5 or grids.shape[-1] != 12:
        raise ValueError(f"{what}: grids must be [V,L,GY,GX,12], got {tuple(grids.shape)}")
    _f32_dev(grids, "grids")


def bilagrid_slice(rgb: torch.Tensor, grids: torch.Tensor) -> torch.Tensor:
    """The reference's bilateral-grid slice (lib_bilagrid.py::slice, one grid per image) on csrc/bilagrid.hip: `rgb` f32 [N,H,W,3]
    as gs_render emits it, `grids` f32 [N,L,GY,GX,12] (coefficient 4c + k = row c, column k of the 3x4 matrix; GX, GY, L >= 2).
    Pixel (i, j) samples its image's grid at ((j + 0.5) / W, (i + 0.5) / H, gray(rgb)) - trilinear, align_corners=True, border -
    and the 3x4 affine matrix it gets is applied to its colour.  -> f32 [N,H,W,3], differentiable with respect to both inputs
    (HIP backward, first order only; deterministic, no atomics)."""
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"bilagrid_slice: rgb must be [N,H,W,3], got {tuple(rgb.shape)}")
    _f32_dev(rgb, "rgb")
    _bilagrid_check(grids, "bilagrid_slice")
    if grids.shape[0] != rgb.shape[0]:
        raise ValueError(f"bilagrid_slice: one grid per image: grids must have shape [{rgb.shape[0]},L,GY,GX,12], got {tuple(grids.shape)}")
    return _BilagridSlice.apply(rgb, grids)


class _BilagridTv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        V, Lz, GY, GX, _ = grids.shape
        lib = L.load()
        ws, ws_bytes = _workspace(lib.v3a_bilagrid_tv_workspace_bytes(V, GX, GY, Lz),
                                  f"v3a_bilagrid_tv_workspace_bytes (grids {tuple(grids.shape)})", grids.device)
        out = torch.empty(1, device=grids.device, dtype=torch.float64)
        args = L.BilagridTvArgs(_ptr(grids), V, GX, GY, Lz, _ptr(out), _ptr(ws), ws_bytes)
        L.check(lib.v3a_bilagrid_tv_forward(C.byref(args), _stream()), "v3a_bilagrid_tv_forward")
        ctx.save_for_backward(grids)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_tv):
        grids, = ctx.saved_tensors
        V, Lz, GY, GX, _ = grids.shape
        d_out = d_tv.to(torch.float64).reshape(1).contiguous()
        d_grids = torch.empty_like(grids)
        args = L.BilagridTvArgs(_ptr(grids), V, GX, GY, Lz, None, None, 0)
        L.check(L.load().v3a_bilagrid_tv_backward(C.byref(args), _ptr(d_out), _ptr(d_grids), _stream()), "v3a_bilagrid_tv_backward")
        return d_grids


def bilagrid_tv(grids: torch.Tensor) -> torch.Tensor:
    """lib_bilagrid.py::total_variation_loss of `grids` f32 [V,L,GY,GX,12] (csrc/bilagrid.hip): per axis L, GY, GX the sum of squared
    forward differences over the number of differences, added and divided by V.  -> a float64 scalar on the device, differentiable
    (HIP backward, first order only)."""
    _bilagrid_check(grids, "bilagrid_tv")
    return _BilagridTv.apply(grids)


def bilagrid_identity(V: int, GX: int, GY: int, L: int, device) -> torch.Tensor:
    """V identity grids f32 [V,L,GY,GX,12]: every vertex holds the 3x4 matrix [I | 0]"""
    if V < 1 or min(GX, GY, L) < 2:
        raise ValueError(f"bilagrid_identity: V >= 1 and GX, GY, L >= 2 required, got V={V}, (GX, GY, L)={(GX, GY, L)}")
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=f32, device=device)
    return eye.repeat(V, L, GY, GX, 1).contiguous()


def bilagrid_from_reference(t: torch.Tensor) -> torch.Tensor:
    """the reference's BilateralGrid.grids [V,12,L,GY,GX] -> this package's [V,L,GY,GX,12] (a copy)"""
    if t.dim() != 5 or t.shape[1] != 12:
        raise ValueError(f"bilagrid_from_reference: expected [V,12,L,GY,GX], got {tuple(t.shape)}")
    return t.permute(0, 2, 3, 4, 1).contiguous()


def bilagrid_to_reference(t: torch.Tensor) -> torch.Tensor:
    """this package's [V,L,GY,GX,12] -> the reference's [V,12,L,GY,GX] (a copy)"""
    if t.dim() != 5 or t.shape[-1] != 12:
        raise ValueError(f"bilagrid_to_reference: expected [V,L,GY,GX,12], got {tuple(t.shape)}")
    return t.permute(0, 4, 1, 2, 3).contiguous()


class _SplatActivate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_scales, quats, logits):
        U = logits.shape[0]
        cov = torch.empty(U, 3, 3, device=logits.device, dtype=f32)
        op = torch.empty(U, device=logits.device, dtype=f32)
        L.check(L.load().v3a_splat_activate(_ptr(log_scales), _ptr(quats), _ptr(logits), U, _ptr(cov), _ptr(op), _stream()), "v3a_splat_activate")
        ctx.save_for_backward(log_scales, quats, logits)
        return cov, op

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_cov, d_op):
        log_scales, quats, logits = ctx.saved_tensors
        U = logits.shape[0]
        d_cov = torch.zeros(U, 3, 3, device=logits.device, dtype=f32) if d_cov is None else d_cov.float().contiguous()
        d_op = torch.zeros(U, device=logits.device, dtype=f32) if d_op is None else d_op.float().contiguous()
        d_ls, d_q, d_lg = torch.empty_like(log_scales), torch.empty_like(quats), torch.empty_like(logits)
        L.check(L.load().v3a_splat_activate_backward(_ptr(log_scales), _ptr(quats), _ptr(logits), _ptr(d_cov), _ptr(d_op), U, _ptr(d_ls),
                                                     _ptr(d_q), _ptr(d_lg), _stream()), "v3a_splat_activate_backward")
        return d_ls, d_q, d_lg


def splat_activate(log_scales: torch.Tensor, quats: torch.Tensor, logits: torch.Tensor):
    """(log-scales [U,3], raw quaternions [U,4] xyzw, opacity logits [U]) -> (covariances [U,3,3], opacities [U]), the inverse of
    (log g.scales, g.rotations, logit g.opacities) of gaussian_adapter's output; differentiable (closed-form HIP backward)."""
    U = logits.shape[0]
    if U < 1:
        raise ValueError("splat_activate: no Gaussians")
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(quats, "quats", (U, 4))
    _f32_dev(logits, "logits", (U,))
    return _SplatActivate.apply(log_scales, quats, logits)


class _SplatRegularisers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_scales, logits):
        U = logits.shape[0]
        lib = L.load()
        ws, ws_bytes = _workspace(lib.v3a_splat_reg_workspace_bytes(U), f"v3a_splat_reg_workspace_bytes (U = {U})", logits.device)
        out = torch.empty(2, device=logits.device, dtype=torch.float64)
        L.check(lib.v3a_splat_reg(_ptr(logits), _ptr(log_scales), U, _ptr(out), _ptr(ws), ws_bytes, _stream()), "v3a_splat_reg")
        ctx.save_for_backward(log_scales, logits)
        return out[0], out[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_opacity, d_scale):
        log_scales, logits = ctx.saved_tensors
        z = torch.zeros((), device=logits.device, dtype=torch.float64)
        d_out = torch.stack([z if g is None else g.to(torch.float64).reshape(()) for g in (d_opacity, d_scale)])
        d_ls, d_lg = torch.empty_like(log_scales), torch.empty_like(logits)
        L.check(L.load().v3a_splat_reg_backward(_ptr(logits), _ptr(log_scales), logits.shape[0], _ptr(d_out), _ptr(d_lg), _ptr(d_ls),
                                                _stream()), "v3a_splat_reg_backward")
        return d_ls, d_lg


def splat_regularisers(log_scales: torch.Tensor, logits: torch.Tensor):
    """The reference loop's two regularisers (simple_trainer.py:966-977; csrc/splat_reg.hip) of log-scales [U,3] and opacity logits
    [U] -> (opacity_mean, scale_mean) = (sigmoid(logits).mean(), exp(log_scales).mean()): float64 scalars on the device, summed in
    fp64 in a fixed order (bit-identical run to run), differentiable with respect to both inputs (HIP backward, first order only)."""
    U = logits.shape[0]
    if U < 1:
        raise ValueError("splat_regularisers: no Gaussians")
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(logits, "logits", (U,))
    return _SplatRegularisers.apply(log_scales, logits)


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, step: int, betas=(0.9, 0.999),
              eps: float = 1e-8, lr2: Optional[float] = None, period: int = 0) -> None:
    """One torch.optim.Adam update of p (f32, any shape), in place on p, m, v, reading the gradient g; `step` counts from 1 and
    sets the bias corrections (computed here in double).  period > 0 with lr2: flat element e uses lr where e % period == 0 and lr2
    elsewhere - the harmonics [U,3,K] with period K are the reference's sh0 / shN optimisers in one launch."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _f32_dev(t, name, p.shape)
    if step < 1:
        raise ValueError("adam_step: step counts from 1")
    b1, b2 = float(betas[0]), float(betas[1])
    a = L.AdamArgs(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(lr if lr2 is None else lr2), int(period), b1, b2, float(eps),
                   1.0 - b1 ** step, 1.0 - b2 ** step)
    L.check(L.load().v3a_adam_step(C.byref(a), _stream()), "v3a_adam_step")


def gs_visibility(radii: torch.Tensor) -> torch.Tensor:
    """The step's visibility mask (simple_trainer.py:1111): radii int32 [C,U] as gs_render's info_out holds them -> uint8 [U], 1
    where radii[c,g] > 0 for some camera c: (radii > 0).any(0) in one launch (v3a_gs_visibility), every byte written once."""
    if radii.dim() != 2 or radii.shape[0] < 1:
        raise ValueError(f"gs_visibility: radii [C,U] with C >= 1 required, got {tuple(radii.shape)}")
    Cn, U = radii.shape
    _i32_dev(radii, "radii", (Cn, U))
    visible = torch.empty(U, device=radii.device, dtype=torch.uint8)
    if U > 0:
        L.check(L.load().v3a_gs_visibility(_ptr(radii), Cn, U, _ptr(visible), _stream()), "v3a_gs_visibility")
    return visible


def adam_step_visible(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, visible: torch.Tensor, *, lr: float,
                      betas=(0.9, 0.999), eps: float = 1e-8, lr2: Optional[float] = None, period: int = 0) -> None:
    """gsplat's SelectiveAdam (the reference's visible_adam, simple_trainer.py:449-450) on p, g, m, v f32 [U, ...] and the mask
    `visible` uint8 [U] (gs_visibility), in place on p, m, v: every element of a row with visible != 0 gets
    m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr m / (sqrt(v) + eps) - no bias correction, hence no step argument.  A
    row with visible == 0 keeps the bits of p, m, v, and its g is not loaded (a NaN there reaches nothing).  period / lr2 as in
    adam_step, the element index taken within the whole tensor."""
    if p.dim() < 1 or p.shape[0] < 1 or p.numel() < 1:
        raise ValueError(f"adam_step_visible: p [U, ...] with at least one element required, got {tuple(p.shape)}")
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _f32_dev(t, name, p.shape)
    U = p.shape[0]
    _tensor(visible, "visible", torch.uint8, (U,))
    if visible.device != p.device:
        raise ValueError(f"visible is on {visible.device}, p on {p.device}")
    a = L.AdamVisibleArgs(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(visible), U, p.numel() // U, float(lr), float(lr if lr2 is None else lr2),
                          int(period), float(betas[0]), float(betas[1]), float(eps))
    L.check(L.load().v3a_adam_step_visible(C.byref(a), _stream()), "v3a_adam_step_visible")


# the random streams of the strategies' Philox draws: the sampler's two (2 and 3 are the noise's draws), and the first of the two
# consecutive streams of each split child of the densification (z0, z1 of stream s, z2 = z0 of stream s + 1)
MCMC_STREAMS = dict(relocate=0, grow=1, split0=4, split1=6)


def _mcmc_key(seed: int, step: int, what: str):
    seed, step = int(seed), int(step)
    if not 0 <= seed < 2 ** 64 or not 0 <= step < 2 ** 32:
        raise ValueError(f"{what}: seed must fit 64 bits and step 32 bits, both unsigned, got {seed} and {step}")
    return seed, step


def mcmc_sample(weights: torch.Tensor, *, min_weight: float, alive_only: bool, n_slots: int, seed: int, stream: int, step: int):
    """The MCMC strategy's weighted sampler (csrc/mcmc.hip, v3a_mcmc_sample) over opacities `weights` f32 [U] -> (src int32 [n_slots],
    counts int32 [U]).  alive_only (relocation, n_slots == U): slot s draws iff weights[s] <= min_weight, among the Gaussians above
    it; otherwise (growth) every slot draws among all.  src is the drawn row or -1, counts how often each row was drawn.  Philox
    counter (slot, 0, stream, step) under the key `seed`; fp64 sums in a fixed order: bit-identical run to run and reproducible on
    the host (tests/mcmc_oracle.py).  An empty pool, or no slot that draws, is a no-op (all -1, all 0)."""
    U = weights.shape[0] if weights.dim() == 1 else 0
    if U < 1:
        raise ValueError("mcmc_sample: no Gaussians")
    _f32_dev(weights, "weights", (U,))
    n_slots = int(n_slots)
    if n_slots < 1 or (alive_only and n_slots != U):
        raise ValueError(f"mcmc_sample: n_slots must be positive, and U = {U} with alive_only, got {n_slots}")
    if stream not in (0, 1):
        raise ValueError(f"mcmc_sample: stream is 0 (relocation) or 1 (growth), got {stream!r}")
    seed, step = _mcmc_key(seed, step, "mcmc_sample")
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_mcmc_sample_workspace_bytes(U), f"v3a_mcmc_sample_workspace_bytes (U = {U})", weights.device)
    src = torch.empty(n_slots, device=weights.device, dtype=torch.int32)
    counts = torch.empty(U, device=weights.device, dtype=torch.int32)
    L.check(lib.v3a_mcmc_sample(_ptr(weights), U, float(min_weight), int(bool(alive_only)), n_slots, seed, int(stream), step, _ptr(src),
                                _ptr(counts), _ptr(ws), ws_bytes, _stream()), "v3a_mcmc_sample")
    return src, counts


def mcmc_relocate(src: torch.Tensor, counts: torch.Tensor, params: dict, m: dict, v: dict, *, dst_offset: int, min_opacity: float) -> None:
    """Relocation (dst_offset = 0) or growth (dst_offset = U) from mcmc_sample's (src, counts), in place on `params` and Adam's
    moments `m`, `v`: dicts of means [R,3], scales (logs) [R,3], quats [R,4], opacities (logits) [R], sh [R,3,K], f32, with R = U
    rows (relocation, src [U]) or R = U + n rows filled up to U (growth, src [n]).  Every drawn row j and its copies get
    compute_relocation's opacity and scales for counts[j] + 1 copies (fp64, csrc/mcmc.hip); copies take means, quats and sh of j.
    Relocation zeroes the moments of j and leaves the dead row's; growth zeroes the new row's and leaves j's."""
    U, n = counts.shape[0], src.shape[0]
    dst_offset = int(dst_offset)
    if dst_offset not in (0, U) or (dst_offset == 0 and n != U):
        raise ValueError(f"mcmc_relocate: dst_offset is 0 with src [U] (relocation) or U (growth), got {dst_offset} with U = {U}, src [{n}]")
    rows = U if dst_offset == 0 else U + n
    _i32_dev(src, "mcmc_relocate: src", (n,))
    _i32_dev(counts, "mcmc_relocate: counts", (U,))
    K = _splat_dicts("mcmc_relocate", params, m, v, rows)
    if not 0.0 < float(min_opacity) < 1.0:
        raise ValueError(f"mcmc_relocate: min_opacity must lie in (0, 1), got {min_opacity!r}")
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_mcmc_relocate_workspace_bytes(U), f"v3a_mcmc_relocate_workspace_bytes (U = {U})", src.device)
    a = L.McmcRelocateArgs(_ptr(src), _ptr(counts), *(_ptr(d[name]) for d in (params, m, v) for name in SPLAT_TENSORS), U, n, dst_offset, K,
                           float(min_opacity), _ptr(ws), ws_bytes)
    L.check(lib.v3a_mcmc_relocate(C.byref(a), _stream()), "v3a_mcmc_relocate")


def mcmc_noise(means: torch.Tensor, log_scales: torch.Tensor, quats: torch.Tensor, logits: torch.Tensor, *, scaler: float, seed: int,
               step: int) -> None:
    """The MCMC strategy's per-step noise, in place on means [U,3]: means += cov . (xi * gate * scaler), cov from (log_scales [U,3],
    raw quats [U,4]) as splat_activate forms it, gate = sigmoid(-100 (opacity - 0.005)) of logits [U], xi three standard normals of
    (seed, step, row) (csrc/mcmc.hip, v3a_mcmc_noise: fp64 after the loads, one rounding at the store)."""
    U = logits.shape[0] if logits.dim() == 1 else 0
    if U < 1:
        raise ValueError("mcmc_noise: no Gaussians")
    _f32_dev(means, "means", (U, 3))
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(quats, "quats", (U, 4))
    _f32_dev(logits, "logits", (U,))
    seed, step = _mcmc_key(seed, step, "mcmc_noise")
    L.check(L.load().v3a_mcmc_noise(_ptr(means), _ptr(log_scales), _ptr(quats), _ptr(logits), U, float(scaler), seed, step, _stream()),
            "v3a_mcmc_noise")


# ------------------------------------------------------------------------------------------------ densification (csrc/densify.hip)
def densify_accumulate(grad2d: torch.Tensor, count: torch.Tensor, d_means2d: torch.Tensor, radii: torch.Tensor, width: int,
                       height: int) -> None:
    """The densification strategy's per-step statistics, in place on grad2d f32 [U] and count int32 [U]: for every camera c (index
    order) with radii[c,g] > 0, grad2d[g] += sqrt((gx W/2 C)^2 + (gy H/2 C)^2) with (gx, gy) = d_means2d[c,g], count[g] += 1
    (v3a_densify_accumulate: fp64 norm and sum, one rounding per call).  d_means2d f32 [C,U,2] and radii int32 [C,U] as
    gs_render's info_out holds them."""
    U = grad2d.shape[0] if grad2d.dim() == 1 else -1
    if U < 0 or d_means2d.dim() != 3 or d_means2d.shape[0] < 1:
        raise ValueError("densify_accumulate: grad2d [U] and d_means2d [C,U,2] required")
    Cn = d_means2d.shape[0]
    _f32_dev(grad2d, "grad2d", (U,))
    _i32_dev(count, "count", (U,))
    _f32_dev(d_means2d, "d_means2d", (Cn, U, 2))
    _i32_dev(radii, "radii", (Cn, U))
    if width < 1 or height < 1:
        raise ValueError(f"densify_accumulate: width and height must be positive, got {width} x {height}")
    if U == 0:
        return
    L.check(L.load().v3a_densify_accumulate(_ptr(d_means2d), _ptr(radii), U, Cn, int(width), int(height), _ptr(grad2d), _ptr(count), _stream()),
            "v3a_densify_accumulate")


def densify_classify(grad2d: torch.Tensor, count: torch.Tensor, log_scales: torch.Tensor, logits: torch.Tensor, *, grow_grad2d: float,
                     grow_scale3d: float, prune_opa: float, prune_scale3d: float, grow: bool = True, prune_big: bool = False,
                     revised_opacity: bool = False) -> dict:
    """The fate of every Gaussian at a refine (v3a_densify_classify; fp64 decisions on exactly converted values; the two scale
    thresholds come multiplied by the scene scale) -> dict(fates uint8 [U]: 0 keep, 1 clone, 2 split, + 4 when the rows it leaves
    are pruned; counts int32 [3,U]: the rows it leaves in segment A (the original), B (the clone), C = D (each split child);
    offsets int32 [3,U]: their exclusive prefix sums; totals int64 [3] on the device).  grow=False forces every fate to keep
    (prune only); prune_big adds the scale criterion to the opacity criterion."""
    U = grad2d.shape[0] if grad2d.dim() == 1 else -1
    if U < 0:
        raise ValueError("densify_classify: grad2d [U] required")
    _f32_dev(grad2d, "grad2d", (U,))
    _i32_dev(count, "count", (U,))
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(logits, "logits", (U,))
    dev = grad2d.device
    out = dict(fates=torch.empty(U, device=dev, dtype=torch.uint8), counts=torch.empty(3, U, device=dev, dtype=torch.int32),
               offsets=torch.empty(3, U, device=dev, dtype=torch.int32), totals=torch.zeros(3, device=dev, dtype=torch.int64))
    if U == 0:
        return out
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_densify_classify_workspace_bytes(U), f"v3a_densify_classify_workspace_bytes (U = {U})", dev)
    a = L.DensifyClassifyArgs(_ptr(grad2d), _ptr(count), _ptr(log_scales), _ptr(logits), U, float(grow_grad2d), float(grow_scale3d),
                              float(prune_opa), float(prune_scale3d), int(bool(grow)), int(bool(prune_big)), int(bool(revised_opacity)),
                              _ptr(out["fates"]), _ptr(out["counts"]), _ptr(out["offsets"]), _ptr(out["totals"]), _ptr(ws), ws_bytes)
    L.check(lib.v3a_densify_classify(C.byref(a), _stream()), "v3a_densify_classify")
    return out


def densify_apply(cls: dict, params: dict, m: dict, v: dict, *, seed: int, step: int, revised_opacity: bool = False,
                  totals: Optional[list] = None):
    """The refined scene from densify_classify's `cls` and the old tensors (dicts of means [U,3], scales (logs) [U,3], quats [U,4],
    opacities (logits) [U], sh [U,3,K], f32) -> (params, m, v): NEW dicts of tensors with U_out = A + B + 2 C rows in the order
    A surviving non-split originals, B surviving clones, C first children, D second children (v3a_densify_apply; include/vist3a_hip.h
    states a child's values).  The old tensors are read only.  `totals` = cls["totals"].tolist() if the caller has read it already;
    otherwise it is read here: the refine's one read-back, which sizes the new tensors."""
    U = cls["fates"].shape[0]
    K = _splat_dicts("densify_apply", params, m, v, U)
    _tensor(cls["fates"], "densify_apply: cls['fates']", torch.uint8, (U,))
    _i32_dev(cls["offsets"], "cls['offsets']", (3, U))
    _tensor(cls["totals"], "densify_apply: cls['totals']", torch.int64, (3,))
    seed, step = _mcmc_key(seed, step, "densify_apply")
    nA, nB, nC = (int(x) for x in (cls["totals"].tolist() if totals is None else totals))
    U_out = nA + nB + 2 * nC
    if min(nA, nB, nC) < 0 or nA + nB > 2 * U or nC > U or U_out >= 2 ** 31:
        raise ValueError(f"densify_apply: segment totals {(nA, nB, nC)} do not belong to {U} Gaussians")
    dev = params["sh"].device
    new = [{name: torch.empty((U_out,) + tuple(params[name].shape[1:]), device=dev, dtype=f32) for name in SPLAT_TENSORS} for _ in range(3)]
    if U == 0 or U_out == 0:
        return tuple(new)
    a = L.DensifyApplyArgs(*(_ptr(d[name]) for d in (params, m, v, *new) for name in SPLAT_TENSORS), _ptr(cls["fates"]), _ptr(cls["offsets"]),
                           _ptr(cls["totals"]), U, U_out, K, seed, step, int(bool(revised_opacity)))
    L.check(L.load().v3a_densify_apply(C.byref(a), _stream()), "v3a_densify_apply")
    return tuple(new)


def densify_reset_opacity(logits: torch.Tensor, m: torch.Tensor, v: torch.Tensor, max_opacity: float) -> None:
    """The strategy's opacity reset, in place: logits = min(logits, logit(max_opacity)), Adam's moments m and v of the logits = 0
    (v3a_densify_reset_opacity)."""
    U = logits.shape[0] if logits.dim() == 1 else -1
    if U < 0:
        raise ValueError("densify_reset_opacity: logits [U] required")
    for name, t in (("logits", logits), ("m", m), ("v", v)):
        _f32_dev(t, name, (U,))
    if not 0.0 < float(max_opacity) < 1.0:
        raise ValueError(f"densify_reset_opacity: max_opacity must lie in (0, 1), got {max_opacity!r}")
    if U == 0:
        return
    L.check(L.load().v3a_densify_reset_opacity(_ptr(logits), _ptr(m), _ptr(v), U, float(max_opacity), _stream()), "v3a_densify_reset_opacity")
