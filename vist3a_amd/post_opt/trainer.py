"""The reference's post-optimisation loop (third_party_model/anysplat/src/post_opt/simple_trainer.py) on this package's kernels.

`create_splats` is create_splats_with_optimizers (:402-462): a `Gaussians` object becomes the parameters means, log-scales,
quaternions, opacity logits and harmonics, each with its Adam moments.  `post_optimize` is train() (:804-1152) with the features the
reference switches off, or that need what this package does not have, left out (DESIGN.md section 7f lists them): one view per step,
loss = 0.8 L1 + 0.2 (1 - SSIM) (:938-942), one Adam (eps 1e-15) per tensor, the means' rate decaying to 1 % over max_steps, no
densification (:389-392), optionally the depth term (:943-961, cfg.depth_loss: ops.depth_loss on the rasteriser's depth and alpha
against a dense depth map per view).  Every step is ops.splat_activate -> ops.gs_render -> ops.photometric_loss (+ cfg.depth_lambda *
ops.depth_loss with cfg.depth_loss) -> backward -> ops.adam_step per trained tensor: HIP kernels throughout, torch only carries the
autograd graph.  Nothing in the loop reads a value back to the host (apart from the rasteriser's own intersection count); the
per-step loss, L1, SSIM and, with cfg.depth_loss, the depth term stay in a device tensor.

cfg.use_bilateral_grid adds the reference's per-view bilateral grids (:352-355, :697-710, :831-846, :916-923, :962-964;
lib_bilagrid.py): the render goes through ops.bilagrid_slice with the view's grid before the photometric loss, the loss gains
cfg.bilagrid_tv_lambda * ops.bilagrid_tv(all grids), and the grids [V,L,GY,GX,12] train with an Adam and a warm-up schedule of their
own.  They absorb per-view exposure and white balance so that the scene does not; they stay in `splats` and are not exported.

Four more switches of the reference's Config, all off by default: cfg.antialiased (:323-324, :769-770) renders every step in the
rasteriser's antialiased mode; cfg.random_bkgd (:326-327, :925-927) draws a fresh RGB background per step; cfg.opacity_reg and
cfg.scale_reg (:329-332, :966-977) add weight * mean sigmoid(logit) and weight * mean exp(log-scale), both from
ops.splat_regularisers (one HIP reduction), only when the weight is above 0.

cfg.strategy = "mcmc" is the reference's `mcmc` configuration (:1485-1501), gsplat's MCMCStrategy called at :1142-1150, restated in
DESIGN.md section 7f (that text is the contract: gsplat is not in the reference tree).  After the Adam updates of a step, every
cfg.mcmc_refine_every steps, Gaussians at or below cfg.mcmc_min_opacity are relocated onto live ones drawn by opacity
(ops.mcmc_sample, ops.mcmc_relocate) and the scene grows by 5 % up to cfg.mcmc_cap_max; after every step ops.mcmc_noise adds
opacity-gated, covariance-shaped noise to the means.  All of it is csrc/mcmc.hip with counter-based random numbers keyed by
cfg.seed and the step, so two runs are bit-identical; nothing is read back.  With the default "none" the loop is as it was.

cfg.pose_opt is the reference's camera pose optimisation (:335-339, :653-663, :824-829, :891-892, :1120-1122; utils.py:12-48
CameraOptModule): 9 deltas per training view (translation + 6D rotation, zero at the start) adjust the view's camera through
ops.camera_adjust, the render takes ops.gs_render(camera_grad=True), and the deltas train with an Adam of their own (weight decay
pose_opt_reg, torch's default eps 1e-8, rate decaying to 1 % over max_steps).  The reference runs it BY DEFAULT (pose_opt = True);
here it is off by default so that no existing call changes - a stated deviation.  The deltas stay in
`splats["pose_deltas"]`; adjusted_extrinsics turns them into cameras.

cfg.strategy = "densify" is the reference's `default` configuration with its densification running (:1486-1491; the reference
parks the schedule at :389-392; the value "default" stays refused, as it always was: in this package the reference's `default`
as it runs is "none"): gsplat's DefaultStrategy, the classic 3DGS adaptive density control, restated in DESIGN.md section
7f (again the contract).  After the Adam updates of a step the screen-space gradient of every visible Gaussian joins a running sum
(ops.densify_accumulate, from gs_render's info_out); every cfg.densify_refine_every steps Gaussians whose average exceeds
cfg.densify_grow_grad2d are cloned (small ones) or split in two (large ones), transparent and oversized ones are pruned
(ops.densify_classify, ops.densify_apply: csrc/densify.hip), and every cfg.densify_reset_every steps the opacities are capped
(ops.densify_reset_opacity).  One read-back per refine - the three segment sizes, which size the new tensors (gsplat syncs there
too) - and a second one only when cfg.densify_cap_max turns a refine into prune-only.

cfg.batch_size = B > 1 is the reference's batch_size (:268, :848-855): every step shows a batch of up to B distinct views
(train_batch_order) to ONE render, loss and backward - every op of the step takes a leading camera or image dimension - and updates
once, with the optimisers scaled as the reference scales them (batch_hyperparameters; :441-461, :660, :707).  cfg.visible_adam is
its visible_adam (:322, :449-450, :1103-1116; gsplat's SelectiveAdam, restated in DESIGN.md section 7f): ops.gs_visibility turns the
render's radii into the step's mask and ops.adam_step_visible updates only the Gaussians some view of the step saw, without bias
correction; the others keep parameters and moments.  With both at their defaults the loop is what it was.

The harmonics stay ONE [U,3,K] tensor: the reference's sh0 / shN optimisers (rates lr_sh and lr_sh / 20) are one ops.adam_step with
a period of K, which is the same arithmetic because Adam is elementwise."""
from __future__ import annotations

from dataclasses import dataclass
from math import isqrt, sqrt
from typing import Optional, Tuple

import torch

from .. import ops
from ..models.types import Gaussians

PARAM_NAMES = ops.SPLAT_TENSORS   # "sh" = the reference's sh0 and shN


@dataclass
class PostOptConfig:
    # the reference's Config fields and defaults (simple_trainer.py:52-180, 442-460)
    max_steps: int = 3000
    ssim_lambda: float = 0.2
    lr_means: float = 1.6e-4
    lr_scales: float = 5e-3
    lr_quats: float = 1e-3
    lr_opacities: float = 5e-2
    lr_sh: float = 2.5e-3            # sh0; shN trains at lr_sh / 20
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15
    min_opacity: float = 0.01        # Gaussians at or below it are dropped at creation (:427)
    depth_loss: bool = False         # :358-360; the term itself :943-961, here on dense maps (ops.depth_loss)
    depth_lambda: float = 1e-2
    scene_scale: float = 1.0         # multiplies the depth term (:426, :960)
    use_bilateral_grid: bool = False                        # :352-355
    bilateral_grid_shape: Tuple[int, int, int] = (16, 16, 8)   # (X, Y, W = the guidance axis L), as the reference spells it
    bilagrid_lr: float = 2e-3        # :707, times sqrt(batch_size)
    bilagrid_warmup_steps: int = 1000   # :839: LinearLR(0.01 -> 1) chained with the decay to 1 % over max_steps
    bilagrid_tv_lambda: float = 10.0    # :963
    antialiased: bool = False        # :323-324: rasterize_mode="antialiased" (the loop's renders; evaluation and export follow it)
    random_bkgd: bool = False        # :326-327: a random background per step, to discourage transparency
    opacity_reg: float = 0.0         # :329-330: weight of mean sigmoid(logit), added when > 0
    scale_reg: float = 0.0           # :331-332: weight of mean exp(log-scale), added when > 0
    strategy: str = "none"           # "none" (the reference's `default` as it runs: densification parked, :389-392), "mcmc" (:1485-1501) or
                                     # "densify" (the reference's `default` with gsplat's DefaultStrategy running, :1486-1491)
    mcmc_cap_max: int = 1_000_000    # gsplat MCMCStrategy's defaults from here on: the scene stops growing at this many Gaussians
    mcmc_noise_lr: float = 5e5       # the noise is scaled by mcmc_noise_lr * (the means' current learning rate)
    mcmc_refine_start_iter: int = 500
    mcmc_refine_stop_iter: int = 25_000
    mcmc_refine_every: int = 100
    mcmc_min_opacity: float = 0.005  # at or below it a Gaussian is dead: relocated at the next refine
    densify_prune_opa: float = 0.005       # gsplat DefaultStrategy's defaults from here on: rows below this opacity are pruned
    densify_grow_grad2d: float = 2e-4      # average screen-space gradient above which a Gaussian is cloned or split
    densify_grow_scale3d: float = 0.01     # (x scene_scale) largest scale up to which it is cloned, above which it is split
    densify_prune_scale3d: float = 0.1     # (x scene_scale) largest scale above which a row is pruned, once i > densify_reset_every
    densify_refine_start_iter: int = 500
    densify_refine_stop_iter: int = 15_000
    densify_reset_every: int = 3000
    densify_refine_every: int = 100
    densify_pause_refine_after_reset: int = 0
    densify_absgrad: bool = False          # accumulate gsplat's absgrad (sum of absolute per-pixel gradients) instead of the gradient
    densify_revised_opacity: bool = False  # split children get opacity 1 - sqrt(1 - o) (arXiv:2404.06109) instead of o
    densify_cap_max: int = 0               # ours: > 0, a refine that would pass this many Gaussians prunes only
    test_every: int = 0              # k > 0: the views with index % k == 0 are held out of the loop (the reference's dataset split, test_every)
    pose_opt: bool = False           # :335-336; True in the reference - off here so that existing calls keep their bits (a stated deviation)
    pose_opt_lr: float = 1e-5        # :337
    pose_opt_reg: float = 1e-6       # :338: the pose Adam's weight decay
    batch_size: int = 1              # :268: views per step (1 .. 9); rates, eps and betas scale with it (batch_hyperparameters)
    visible_adam: bool = False       # :322: gsplat's SelectiveAdam - only the Gaussians some view of the step saw are updated
    # ours
    params: Tuple[str, ...] = ("means", "scales", "quats", "opacities", "sh0", "shN")
    seed: int = 0

    def trained(self) -> Tuple[str, ...]:
        names = set(self.params)
        bad = names - {"means", "scales", "quats", "opacities", "sh0", "shN", "sh"}
        if bad:
            raise ValueError(f"PostOptConfig.params: unknown parameter names {sorted(bad)}")
        if ("sh0" in names) != ("shN" in names):
            raise ValueError("PostOptConfig.params: sh0 and shN are one tensor here and train together (name both, or 'sh')")
        if names & {"sh0", "shN"}:
            names = (names - {"sh0", "shN"}) | {"sh"}
        return tuple(n for n in PARAM_NAMES if n in names)

    def check_strategy(self) -> None:
        if self.strategy not in ("none", "mcmc", "densify"):
            raise ValueError(f"PostOptConfig.strategy must be 'none', 'mcmc' or 'densify' (the reference's `default` configuration is 'none' as it runs there, 'densify' with its DefaultStrategy running), got {self.strategy!r}")
        if self.strategy == "none":
            return
        if isinstance(self.seed, bool) or not isinstance(self.seed, int) or not 0 <= self.seed < 2 ** 64:
            raise ValueError(f"PostOptConfig.seed keys the strategy's random numbers: an integer in [0, 2^64), got {self.seed!r}")
        if self.strategy == "densify":
            ints = {n: getattr(self, n) for n in ("densify_refine_start_iter", "densify_refine_stop_iter", "densify_reset_every",
                                                  "densify_refine_every", "densify_pause_refine_after_reset", "densify_cap_max")}
            for name, n in ints.items():
                if not isinstance(n, int) or isinstance(n, bool) or n < 0:
                    raise ValueError(f"PostOptConfig.{name} must be a non-negative integer, got {n!r}")
            if self.densify_refine_every < 1 or self.densify_reset_every < 1:
                raise ValueError(f"PostOptConfig.densify_refine_every and densify_reset_every must be positive, got "
                                 f"{self.densify_refine_every!r} and {self.densify_reset_every!r}")
            if not 0.0 < self.densify_prune_opa < 0.5:
                raise ValueError(f"PostOptConfig.densify_prune_opa must lie in (0, 0.5) (the reset caps opacities at twice it), got "
                                 f"{self.densify_prune_opa!r}")
            for name in ("densify_grow_grad2d", "densify_grow_scale3d", "densify_prune_scale3d", "scene_scale"):
                if not getattr(self, name) > 0:
                    raise ValueError(f"PostOptConfig.{name} must be positive, got {getattr(self, name)!r}")
            for name in ("densify_absgrad", "densify_revised_opacity"):
                if not isinstance(getattr(self, name), bool):
                    raise ValueError(f"PostOptConfig.{name} must be a bool, got {getattr(self, name)!r}")
            return
        ints = dict(mcmc_cap_max=self.mcmc_cap_max, mcmc_refine_start_iter=self.mcmc_refine_start_iter,
                    mcmc_refine_stop_iter=self.mcmc_refine_stop_iter, mcmc_refine_every=self.mcmc_refine_every)
        for name, n in ints.items():
            if not isinstance(n, int) or isinstance(n, bool):
                raise ValueError(f"PostOptConfig.{name} must be an integer, got {n!r}")
        if self.mcmc_cap_max < 1 or self.mcmc_refine_every < 1:
            raise ValueError(f"PostOptConfig.mcmc_cap_max and mcmc_refine_every must be positive, got {self.mcmc_cap_max!r} and "
                             f"{self.mcmc_refine_every!r}")
        if not self.mcmc_noise_lr >= 0 or not 0.0 < self.mcmc_min_opacity < 1.0:
            raise ValueError(f"PostOptConfig.mcmc_noise_lr must be non-negative and mcmc_min_opacity in (0, 1), got "
                             f"{self.mcmc_noise_lr!r} and {self.mcmc_min_opacity!r}")

    def check_pose(self) -> None:
        if not isinstance(self.pose_opt, bool):
            raise ValueError(f"PostOptConfig.pose_opt must be a bool, got {self.pose_opt!r}")
        if not self.pose_opt:
            return
        if not self.pose_opt_lr > 0 or not self.pose_opt_reg >= 0:
            raise ValueError(f"PostOptConfig.pose_opt_lr must be positive and pose_opt_reg non-negative, got {self.pose_opt_lr!r} and "
                             f"{self.pose_opt_reg!r}")
        if not isinstance(self.max_steps, int) or self.max_steps < 1:
            raise ValueError(f"PostOptConfig.max_steps must be a positive integer (the pose rate decays over it), got {self.max_steps!r}")

    def check_batch(self) -> None:
        B = self.batch_size
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError(f"PostOptConfig.batch_size must be an integer >= 1, got {B!r}")
        if B >= 10:
            raise ValueError(f"PostOptConfig.batch_size must be at most 9, got {B!r}: the reference sets beta1 = 1 - batch_size * (1 - 0.9), "
                             "which is 0 at 10 and negative beyond - a case the reference itself leaves unresolved")
        if not isinstance(self.visible_adam, bool):
            raise ValueError(f"PostOptConfig.visible_adam must be a bool, got {self.visible_adam!r}")
        if B > 1 and not all(0.0 <= 1.0 - B * (1.0 - b) < 1.0 for b in self.betas):
            raise ValueError(f"PostOptConfig.betas = {tuple(self.betas)!r} leave [0, 1) at batch_size = {B}: 1 - batch_size * (1 - beta)")

    def check_bilagrid(self) -> None:
        if not self.use_bilateral_grid:
            return
        shape = tuple(self.bilateral_grid_shape)
        if len(shape) != 3 or any(not isinstance(n, int) or isinstance(n, bool) or n < 2 for n in shape):
            raise ValueError(f"PostOptConfig.bilateral_grid_shape must be three integers (X, Y, W) >= 2, got {self.bilateral_grid_shape!r}")
        if not isinstance(self.bilagrid_warmup_steps, int) or self.bilagrid_warmup_steps < 1:
            raise ValueError(f"PostOptConfig.bilagrid_warmup_steps must be a positive integer, got {self.bilagrid_warmup_steps!r}")
        if not self.bilagrid_lr > 0 or not self.bilagrid_tv_lambda >= 0:
            raise ValueError(f"PostOptConfig.bilagrid_lr must be positive and bilagrid_tv_lambda non-negative, got {self.bilagrid_lr!r} "
                             f"and {self.bilagrid_tv_lambda!r}")


def bilagrid_learning_rate(cfg: PostOptConfig, s: int) -> float:
    """The grid Adam's rate at the step with `s` earlier steps: the closed form of the reference's ChainedScheduler(LinearLR(0.01,
    warmup), ExponentialLR(0.01 ** (1 / max_steps))) (:831-846)."""
    w = cfg.bilagrid_warmup_steps
    return cfg.bilagrid_lr * (0.01 + 0.99 * min(s, w) / w) * (0.01 ** (s / cfg.max_steps))


def pose_learning_rate(cfg: PostOptConfig, s: int) -> float:
    """The pose Adam's rate at the step with `s` earlier steps: ExponentialLR(0.01 ** (1 / max_steps)) in closed form (:824-829)."""
    return cfg.pose_opt_lr * (0.01 ** (s / cfg.max_steps))


def batch_hyperparameters(cfg: PostOptConfig) -> dict:
    """The reference's scaling of the optimisers with B = cfg.batch_size (:441-461, :660, :707) -> dict(lr = {tensor: its rate times
    sqrt(B)} for the five splat tensors (the means' decay multiplies it per step), eps = cfg.eps / sqrt(B), betas = (1 - B (1 - b1),
    1 - B (1 - b2)), lr_scale = sqrt(B): what the bilateral-grid and pose rates are multiplied by, their eps and betas staying).
    B is the configured size, never the length of an epoch's short last batch.  At B = 1 nothing is multiplied or divided: the
    values are cfg's own, lr_scale is 1.0."""
    B = cfg.batch_size
    lr = dict(means=cfg.lr_means, scales=cfg.lr_scales, quats=cfg.lr_quats, opacities=cfg.lr_opacities, sh=cfg.lr_sh)
    if B == 1:
        return dict(lr=lr, eps=cfg.eps, betas=(cfg.betas[0], cfg.betas[1]), lr_scale=1.0)
    r = sqrt(B)
    return dict(lr={n: x * r for n, x in lr.items()}, eps=cfg.eps / r,
                betas=(1.0 - B * (1.0 - cfg.betas[0]), 1.0 - B * (1.0 - cfg.betas[1])), lr_scale=r)


def view_order(n_views: int, steps: int, seed: int) -> list:
    """The view of every step: one permutation of the views per epoch from a CPU generator seeded with `seed`."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    while len(out) < steps:
        out += torch.randperm(n_views, generator=g).tolist()
    return out[:steps]


def random_backgrounds(steps: int, seed: int) -> torch.Tensor:
    """cfg.random_bkgd's background of every step, f32 [steps,3] in [0,1): one torch.rand(3) per step from a CPU generator seeded
    `seed` + 1, a generator of its own so that switching the option on leaves view_order where it was."""
    g = torch.Generator().manual_seed(int(seed) + 1)
    return torch.stack([torch.rand(3, generator=g) for _ in range(steps)]) if steps > 0 else torch.zeros(0, 3)


def log_columns(cfg: "PostOptConfig") -> list:
    """The names of post_optimize's log columns for `cfg`, in order."""
    cols = ["loss", "l1", "ssim"]
    if cfg.depth_loss:
        cols.append("depth_term")
    if cfg.use_bilateral_grid:
        cols.append("bilagrid_tv")
    if cfg.opacity_reg > 0.0:
        cols.append("opacity_mean")
    if cfg.scale_reg > 0.0:
        cols.append("scale_mean")
    return cols


def mcmc_refines_at(cfg: PostOptConfig, i: int) -> bool:
    """Whether the strategy refines (relocates and grows) after the Adam updates of 0-based step `i`: gsplat's
    step > refine_start_iter and step < refine_stop_iter and step % refine_every == 0."""
    return cfg.mcmc_refine_start_iter < i < cfg.mcmc_refine_stop_iter and i % cfg.mcmc_refine_every == 0


def mcmc_growth(cfg: PostOptConfig, U: int) -> int:
    """The Gaussians a refine adds to a scene of U: up to 5 %, never past cfg.mcmc_cap_max (a scene already above the cap only
    relocates)."""
    return max(0, min(cfg.mcmc_cap_max, int(1.05 * U)) - U)


def mcmc_refine(splats: dict, cfg: PostOptConfig, t: int) -> None:
    """One refine with `t` optimiser steps done: relocation (random stream 0), then growth (stream 1), in place on `splats`; the
    tensors of params / m / v are REPLACED by longer ones when the scene grows.  Appends (relocated, added) to splats["mcmc_counts"],
    int64 [refines,2] on the device."""
    p, m, v = splats["params"], splats["m"], splats["v"]
    U, dev = p["means"].shape[0], p["means"].device
    with torch.no_grad():
        _, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        src, counts = ops.mcmc_sample(op, min_weight=cfg.mcmc_min_opacity, alive_only=True, n_slots=U, seed=cfg.seed,
                                      stream=ops.MCMC_STREAMS["relocate"], step=t)
        ops.mcmc_relocate(src, counts, p, m, v, dst_offset=0, min_opacity=cfg.mcmc_min_opacity)
        relocated = (src >= 0).sum()
        n = mcmc_growth(cfg, U)
        if n > 0:
            _, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])      # of the relocated state
            src, counts = ops.mcmc_sample(op, min_weight=cfg.mcmc_min_opacity, alive_only=False, n_slots=n, seed=cfg.seed,
                                          stream=ops.MCMC_STREAMS["grow"], step=t)
            for d in (p, m, v):
                for name in PARAM_NAMES:
                    old = d[name].detach()
                    d[name] = torch.zeros((U + n,) + tuple(old.shape[1:]), device=dev, dtype=old.dtype)
                    d[name][:U].copy_(old)
            ops.mcmc_relocate(src, counts, p, m, v, dst_offset=U, min_opacity=cfg.mcmc_min_opacity)
        row = torch.stack([relocated, torch.full((), n, device=dev, dtype=torch.int64)])[None]
        splats["mcmc_counts"] = torch.cat([splats["mcmc_counts"], row]) if "mcmc_counts" in splats else row


def densify_active_at(cfg: PostOptConfig, i: int) -> bool:
    """Whether the densification strategy does anything after the Adam updates of 0-based step `i`: gsplat returns at once when
    step >= refine_stop_iter (no statistics, no refine, no reset)."""
    return i < cfg.densify_refine_stop_iter


def densify_refines_at(cfg: PostOptConfig, i: int) -> bool:
    """Whether it refines after step `i`: gsplat's step > refine_start_iter and step % refine_every == 0 and
    step % reset_every >= pause_refine_after_reset."""
    return (densify_active_at(cfg, i) and i > cfg.densify_refine_start_iter and i % cfg.densify_refine_every == 0
            and i % cfg.densify_reset_every >= cfg.densify_pause_refine_after_reset)


def densify_resets_at(cfg: PostOptConfig, i: int) -> bool:
    """Whether it resets the opacities after step `i`: gsplat's step % reset_every == 0, and i > 0 (ours: gsplat also resets after
    the very first step, which would cap the predicted opacities before anything was learnt)."""
    return densify_active_at(cfg, i) and i > 0 and i % cfg.densify_reset_every == 0


def densify_state(splats: dict) -> dict:
    """splats["densify"] = {"grad2d": f32 [U], "count": int32 [U]}, the running statistics, created as zeros when missing"""
    U, dev = splats["params"]["means"].shape[0], splats["params"]["means"].device
    st = splats.get("densify")
    if st is None:
        st = splats["densify"] = dict(grad2d=torch.zeros(U, device=dev, dtype=torch.float32), count=torch.zeros(U, device=dev, dtype=torch.int32))
    if tuple(st["grad2d"].shape) != (U,) or tuple(st["count"].shape) != (U,):
        raise ValueError(f"splats['densify'] holds statistics of {tuple(st['grad2d'].shape)} Gaussians, the scene has {U}")
    return st


def densify_refine(splats: dict, cfg: PostOptConfig, i: int) -> None:
    """One refine after the Adam updates of 0-based step `i`, on the updated parameters: classify (clone / split / keep, then the
    prune verdict of the rows each parent leaves), read the three segment sizes back, and REPLACE the fifteen tensors of params / m / v
    by new ones in gsplat's row order (surviving originals, clones, first children, second children; new rows start with zero
    moments).  The split children's offsets are drawn from Philox streams 4-7 at counter (parent, 0, stream, i + 1) under cfg.seed.
    With cfg.densify_cap_max > 0, a refine that would exceed it is classified again with growth off (one more read-back) and prunes
    only.  The statistics restart as zeros at the new length.  Appends (cloned, split, pruned, U_after) to splats["densify_counts"],
    int64 [refines,4] on the device: surviving clones, split parents whose children survive, parents whose rows were pruned.
    A refine that leaves no Gaussian raises RuntimeError."""
    p, m, v = splats["params"], splats["m"], splats["v"]
    U, dev = p["means"].shape[0], p["means"].device
    st = densify_state(splats)
    with torch.no_grad():
        kw = dict(grow_grad2d=cfg.densify_grow_grad2d, grow_scale3d=cfg.densify_grow_scale3d * cfg.scene_scale,
                  prune_opa=cfg.densify_prune_opa, prune_scale3d=cfg.densify_prune_scale3d * cfg.scene_scale,
                  prune_big=i > cfg.densify_reset_every, revised_opacity=cfg.densify_revised_opacity)
        cls = ops.densify_classify(st["grad2d"], st["count"], p["scales"].detach(), p["opacities"].detach(), grow=True, **kw)
        nA, nB, nC = cls["totals"].tolist()                    # the refine's read-back
        if cfg.densify_cap_max > 0 and nA + nB + 2 * nC > cfg.densify_cap_max:
            cls = ops.densify_classify(st["grad2d"], st["count"], p["scales"].detach(), p["opacities"].detach(), grow=False, **kw)
            nA, nB, nC = cls["totals"].tolist()
        U_out = nA + nB + 2 * nC
        if U_out == 0:
            raise RuntimeError(f"densification pruned all {U} Gaussians at step {i} (densify_prune_opa = {cfg.densify_prune_opa}, "
                               f"densify_prune_scale3d = {cfg.densify_prune_scale3d})")
        new = ops.densify_apply(cls, {k: t.detach() for k, t in p.items()}, m, v, seed=cfg.seed, step=i + 1,
                                revised_opacity=cfg.densify_revised_opacity, totals=(nA, nB, nC))
        for d, nd in zip((p, m, v), new):
            d.update(nd)
        splats["densify"] = dict(grad2d=torch.zeros(U_out, device=dev, dtype=torch.float32), count=torch.zeros(U_out, device=dev, dtype=torch.int32))
        row = torch.tensor([[nB, nC, U + nB + nC - U_out, U_out]], device=dev, dtype=torch.int64)
        splats["densify_counts"] = torch.cat([splats["densify_counts"], row]) if "densify_counts" in splats else row


def train_views(n_views: int, test_every: int) -> list:
    """The views the loop may show: all of them, or with test_every = k > 0 those with index % k != 0 (the others are held out for
    post_opt.evaluate_views, as the reference's parser splits its dataset)."""
    k = int(test_every)
    if k < 0:
        raise ValueError(f"PostOptConfig.test_every must be >= 0, got {test_every!r}")
    train = [i for i in range(n_views) if k == 0 or i % k != 0]
    if not train:
        raise ValueError(f"test_every = {k} holds out all {n_views} views: no view is left to train on (use a value >= 2 with at "
                         "least 2 views)")
    return train


def train_view_order(n_views: int, steps: int, seed: int, test_every: int = 0) -> list:
    """The view of every step of post_optimize: view_order over the training views.  With test_every = 0 it is view_order itself."""
    if int(test_every) == 0:
        return view_order(n_views, steps, seed)
    train = train_views(n_views, test_every)
    return [train[j] for j in view_order(len(train), steps, seed)]


def train_batch_order(n_views: int, steps: int, seed: int, test_every: int = 0, batch_size: int = 1) -> list:
    """The views of every step of post_optimize, a list of `steps` lists: view_order's per-epoch permutations of the training views
    (same generator, same seed), each cut into consecutive chunks of batch_size; an epoch's last chunk is short when batch_size does
    not divide the number of training views (DataLoader(shuffle=True, drop_last=False), :848-855).  The views of a batch are
    distinct.  With batch_size = 1 it is [[j] for j in train_view_order(...)]."""
    B = int(batch_size)
    if B < 1:
        raise ValueError(f"train_batch_order: batch_size must be >= 1, got {batch_size!r}")
    train = train_views(n_views, test_every)
    g = torch.Generator().manual_seed(int(seed))
    out = []
    while len(out) < steps:
        perm = torch.randperm(len(train), generator=g).tolist()
        out += [[train[j] for j in perm[k:k + B]] for k in range(0, len(perm), B)]
    return out[:steps]


def _single(gaussians: Gaussians) -> None:
    if gaussians.means.dim() != 3 or gaussians.means.shape[0] != 1:
        raise ValueError(f"post-optimisation takes one scene (batch dimension 1), got means of shape {tuple(gaussians.means.shape)}")


def create_splats(gaussians: Gaussians, cfg: PostOptConfig, n_views: Optional[int] = None) -> dict:
    """-> {"params": {name: f32 tensor}, "m": {...}, "v": {...}, "step": 0, "keep": bool [U] (the rows kept)}.  "keep" describes
    creation only: which of the input's Gaussians became rows; the MCMC strategy later moves and adds rows and leaves it alone.  scales are stored as
    logs, opacities as logits (clamped to 1 - 1e-6 so that the logit is finite), quaternions as they come (xyzw, as `Gaussians` keeps them).
    With cfg.use_bilateral_grid and `n_views`, also "bil_grids" (identity, f32 [n_views,L,GY,GX,12]) and its moments "bil_m", "bil_v"."""
    _single(gaussians)
    if not gaussians.means.is_cuda:
        raise ValueError("post-optimisation runs on the device (the HIP path has no CPU fallback)")
    with torch.no_grad():
        op = gaussians.opacities[0].reshape(-1).float()
        keep = op > cfg.min_opacity
        sel = lambda t: t[0].float()[keep].contiguous()
        p = dict(means=sel(gaussians.means), scales=torch.log(sel(gaussians.scales)), quats=sel(gaussians.rotations),
                 opacities=torch.logit(op[keep].clamp(max=1 - 1e-6)).contiguous(), sh=sel(gaussians.harmonics))
    if p["means"].shape[0] == 0:
        raise ValueError(f"no Gaussian has an opacity above min_opacity = {cfg.min_opacity}")
    splats = dict(params=p, m={k: torch.zeros_like(t) for k, t in p.items()}, v={k: torch.zeros_like(t) for k, t in p.items()}, step=0, keep=keep)
    if cfg.use_bilateral_grid and n_views is not None:
        add_bilateral_grids(splats, cfg, n_views)
    return splats


def add_bilateral_grids(splats: dict, cfg: PostOptConfig, n_views: int) -> None:
    """splats["bil_grids"]: one identity grid per training view, with its Adam moments (the reference's BilateralGrid(len(trainset), ...))"""
    cfg.check_bilagrid()
    GX, GY, L = cfg.bilateral_grid_shape
    g = ops.bilagrid_identity(n_views, GX, GY, L, splats["params"]["means"].device)
    splats.update(bil_grids=g, bil_m=torch.zeros_like(g), bil_v=torch.zeros_like(g))


def add_pose_deltas(splats: dict, n_views: int) -> None:
    """splats["pose_deltas"]: zeros f32 [n_views,9], one row per training view, with its Adam moments (CameraOptModule.zero_init)"""
    d = torch.zeros(n_views, 9, device=splats["params"]["means"].device, dtype=torch.float32)
    splats.update(pose_deltas=d, pose_m=torch.zeros_like(d), pose_v=torch.zeros_like(d))


def _camera_bases(extrinsics, dev):
    # the full matrices behind _cameras' view and campos (the same two host inversions): what ops.camera_adjust starts from
    w2c = torch.linalg.inv(extrinsics.detach().float().cpu())
    c2w = torch.linalg.inv(w2c)
    return w2c.contiguous().to(dev), c2w.contiguous().to(dev)


def pose_transforms(deltas: torch.Tensor) -> torch.Tensor:
    """deltas [...,9] -> the rigid transforms [Rd | dx] as fp64 [...,4,4] (CameraOptModule's `transform`): a1 = drot[:3] + (1,0,0),
    a2 = drot[3:] + (0,1,0), Gram-Schmidt with F.normalize's clamp at 1e-12, rows b1, b2, b3 = b1 x b2.  The same few lines stand in
    tests/pose_opt_oracle.py, which is what is pinned to the reference's module; the tests hold this copy to that one."""
    d = deltas.detach().double()
    a1 = d[..., 3:6] + torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=d.device)
    a2 = d[..., 6:9] + torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=d.device)
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    b3 = torch.linalg.cross(b1, b2, dim=-1)
    T = torch.zeros(*d.shape[:-1], 4, 4, dtype=torch.float64, device=d.device)
    T[..., :3, :3] = torch.stack((b1, b2, b3), dim=-2)
    T[..., :3, 3] = d[..., :3]
    T[..., 3, 3] = 1.0
    return T


def adjusted_extrinsics(extrinsics: torch.Tensor, splats: dict, cfg: PostOptConfig) -> torch.Tensor:
    """The cameras after pose optimisation: camera-to-world f32 [V,4,4] like `extrinsics`, the training views multiplied by their
    deltas' transform (c2w [Rd | dx], in fp64, rounded once), held-out views (cfg.test_every) unchanged - the reference does not
    adjust its validation cameras either.  Without "pose_deltas" in `splats` it is `extrinsics` itself."""
    if tuple(extrinsics.shape[1:]) != (4, 4) or extrinsics.dim() != 3:
        raise ValueError(f"adjusted_extrinsics: extrinsics [V,4,4] required, got {tuple(extrinsics.shape)}")
    out = extrinsics.detach().float().clone()
    if "pose_deltas" not in splats:
        return out
    train = train_views(extrinsics.shape[0], cfg.test_every)
    deltas = splats["pose_deltas"]
    if tuple(deltas.shape) != (len(train), 9):
        raise ValueError(f"splats['pose_deltas'] has shape {tuple(deltas.shape)}, the {len(train)} training views want {(len(train), 9)}")
    idx = torch.tensor(train, device=out.device)
    out[idx] = (out[idx].double() @ pose_transforms(deltas).to(out.device)).float()
    return out


def _cameras(extrinsics, intrinsics, W, H, dev):
    # tiny per-camera matrices on the host, exactly as DecoderSplattingCUDA derives them
    w2c = torch.linalg.inv(extrinsics.float().cpu())
    c2w = torch.linalg.inv(w2c)
    K = intrinsics.float().cpu().clone()
    K[:, 0] = K[:, 0] * W
    K[:, 1] = K[:, 1] * H
    return w2c.contiguous().to(dev), c2w[:, :3, 3].contiguous().to(dev), K.contiguous().to(dev)


def splats_to_gaussians(splats: dict) -> Gaussians:
    """All six fields consistent: scales = exp, opacities = sigmoid, covariances rebuilt from them, rotations normalised."""
    p = splats["params"]
    with torch.no_grad():
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        return Gaussians(means=p["means"].detach().clone()[None], covariances=cov[None], harmonics=p["sh"].detach().clone()[None],
                         opacities=op[None], scales=torch.exp(p["scales"])[None],
                         rotations=torch.nn.functional.normalize(p["quats"], dim=-1)[None])


def post_optimize(gaussians: Gaussians, images: torch.Tensor, extrinsics: torch.Tensor, intrinsics: torch.Tensor,
                  cfg: Optional[PostOptConfig] = None, steps: Optional[int] = None, splats: Optional[dict] = None,
                  depths: Optional[torch.Tensor] = None, depth_masks: Optional[torch.Tensor] = None):
    """Refine one scene's Gaussians against `images` (f32 [V,H,W,3] in [0,1], on the device) seen from `extrinsics` (camera-to-world
    [V,4,4]) with `intrinsics` (normalised [V,3,3]) - the decoder's conventions.  `steps` (default cfg.max_steps) steps of one view
    each; the means' learning-rate schedule always spans cfg.max_steps.  -> (Gaussians, log): the refined scene (rows at or below
    cfg.min_opacity dropped) and a float64 device tensor of per-step (loss, l1, ssim), [steps,3], or with cfg.depth_loss
    (loss, l1, ssim, depth_term), [steps,4]: loss is the total, depth_term the unweighted term.  With cfg.use_bilateral_grid a
    last column holds the unweighted total variation of the grids; the returned Gaussians are the raw scene (no grid applied) and
    the trained grids stay in `splats["bil_grids"]` (pass `splats` to keep them).

    With cfg.depth_loss the step's loss is photometric + cfg.depth_lambda * ops.depth_loss(rendered depth, alpha, depths[j],
    depth_masks[j], cfg.scene_scale): `depths` f32 [V,H,W] on the device are z along the camera axis in the units of `extrinsics`,
    `depth_masks` bool / uint8 [V,H,W] (or None: every pixel with a positive finite depth).  Without cfg.depth_loss `depths` is ignored.

    With cfg.test_every = k > 0 the views with index % k == 0 are never shown (train_view_order); their images and depths
    are not read, and there is one bilateral grid per TRAINING view, in their order.  post_opt.evaluate_views scores them.

    cfg.antialiased renders in the rasteriser's antialiased mode.  cfg.random_bkgd replaces the black background of step i by
    random_backgrounds(steps, cfg.seed)[i]; the target image is not composited over it (as in the reference), and the render is
    clamped to [0,1] AFTER the background went in (the reference adds it to an unclamped render: a deviation).  cfg.opacity_reg /
    cfg.scale_reg > 0 add weight * ops.splat_regularisers(...) terms to the loss and, each, one last log column with the unweighted
    mean, opacity before scale, after every other column (log_columns(cfg) names them all).

    With cfg.strategy = "mcmc", after the Adam updates of the step with i steps done before it: if mcmc_refines_at(cfg, i),
    mcmc_refine (relocation, then growth by mcmc_growth rows: the tensors in `splats` are replaced by longer ones and the returned
    Gaussians follow the new count); then, on every step, ops.mcmc_noise on the means with scaler = cfg.mcmc_noise_lr * the means'
    rate after the step.  The random numbers are keyed by cfg.seed and the steps done, so with `splats` carried through several calls
    the STRATEGY continues where one call would be: its random numbers, the timing of its refines and the grown tensors.  The view
    order and the random backgrounds restart with every call, as they always did, so several calls equal one call only where
    those repeat.  splats["mcmc_counts"], int64 [refines,2] on the device, holds (relocated, added) of every refine;
    nothing is read back.  The reference pairs the strategy with opacity_reg = scale_reg = 0.01; neither default changes here.

    With cfg.pose_opt, `splats["pose_deltas"]` (zeros f32 [Vt,9] at the start, one row per TRAINING view in their order, moments
    "pose_m" / "pose_v"; a wrong shape raises) adjusts the step's camera: ops.camera_adjust -> ops.gs_render(camera_grad=True), the
    deltas being one more leaf of the step's single autograd.grad (the depth term reaches the camera through the rendered depth).
    Update: ops.adam_step(deltas, grad + cfg.pose_opt_reg * deltas, lr = pose_learning_rate(cfg, steps done), betas (0.9, 0.999),
    eps 1e-8) - torch.optim.Adam(weight_decay) restated; every row moves each step.  cfg.params may then be empty (a pose-only fit).
    `extrinsics` that require grad are still refused: the deltas are the loop's own state.  adjusted_extrinsics(extrinsics, splats,
    cfg) returns the refined cameras; held-out views keep their given poses.  The log has no column of its own for it.

    With cfg.batch_size = B > 1 a step shows the views train_batch_order(V, steps, cfg.seed, cfg.test_every, B)[i] - up to B distinct
    views, fewer in an epoch's last batch - to one render, one loss (the means run over the batch), one backward and one update with
    batch_hyperparameters(cfg); one random background per step; the log keeps one row per step and splats["step"] counts steps.
    With cfg.visible_adam the five splat tensors update through ops.adam_step_visible under ops.gs_visibility(the step's radii):
    rows no view of the step saw keep parameters and moments; grids and pose deltas keep ops.adam_step.

    With cfg.strategy = "densify", after the Adam updates of 0-based step i (while densify_active_at(cfg, i)): ops.densify_accumulate
    adds the step's screen-space gradients (gs_render's info_out; the absolute ones with cfg.densify_absgrad) to splats["densify"] =
    {"grad2d": f32 [U], "count": int32 [U]}; if densify_refines_at(cfg, i), densify_refine (the tensors in `splats` are replaced, the
    returned Gaussians follow the new count; splats["densify_counts"], int64 [refines,4], holds (cloned, split, pruned, U_after));
    if densify_resets_at(cfg, i), ops.densify_reset_opacity caps the opacities at 2 cfg.densify_prune_opa and zeroes their moments.
    A `splats` carried through several calls continues where it was, as MCMC's state does.  Each refine reads the three segment
    sizes back to the host (they size the new tensors; gsplat synchronises there too) - beside the rasteriser's intersection count
    the loop's only read-back."""
    cfg = cfg or PostOptConfig()
    cfg.check_bilagrid()
    cfg.check_strategy()
    cfg.check_pose()
    cfg.check_batch()
    _single(gaussians)
    for t, n in ((extrinsics, "extrinsics"), (intrinsics, "intrinsics")):
        if t.requires_grad:
            raise NotImplementedError(f"post_optimize: no gradient for {n} (the given cameras are constants; cfg.pose_opt trains pose "
                                      "deltas of the loop's own)")
    if images.dim() != 4 or images.shape[-1] != 3 or images.dtype != torch.float32:
        raise ValueError(f"images must be float32 [V,H,W,3], got {images.dtype} {tuple(images.shape)}")
    V, H, W, _ = images.shape
    if tuple(extrinsics.shape) != (V, 4, 4) or tuple(intrinsics.shape) != (V, 3, 3):
        raise ValueError(f"extrinsics [V,4,4] and intrinsics [V,3,3] must match the {V} images, got {tuple(extrinsics.shape)} and "
                         f"{tuple(intrinsics.shape)}")
    if cfg.depth_loss:
        if depths is None:
            raise ValueError("post_optimize: cfg.depth_loss needs `depths` (f32 [V,H,W])")
        if tuple(depths.shape) != (V, H, W) or depths.dtype != torch.float32:
            raise ValueError(f"depths must be float32 [V,H,W] = {(V, H, W)} like the images, got {depths.dtype} {tuple(depths.shape)}")
        if depth_masks is not None and (tuple(depth_masks.shape) != (V, H, W) or depth_masks.dtype not in (torch.bool, torch.uint8)):
            raise ValueError(f"depth_masks must be bool or uint8 [V,H,W] = {(V, H, W)}, got {depth_masks.dtype} {tuple(depth_masks.shape)}")
        if not depths.is_cuda or (depth_masks is not None and not depth_masks.is_cuda):
            raise ValueError("depths and depth_masks must be on the device (the HIP path has no CPU fallback)")
        depths = depths.detach().contiguous()
        depth_masks = None if depth_masks is None else depth_masks.detach().contiguous()
    if not images.is_cuda:
        raise ValueError("images must be on the device (the HIP path has no CPU fallback)")
    steps = cfg.max_steps if steps is None else int(steps)
    trained = cfg.trained()
    train = train_views(V, cfg.test_every)
    grid_of = {j: g for g, j in enumerate(train)}     # the identity when nothing is held out
    Vt = len(train)
    splats = splats if splats is not None else create_splats(gaussians, cfg, Vt)
    p, m, v = splats["params"], splats["m"], splats["v"]
    bil = cfg.use_bilateral_grid
    if bil:
        if "bil_grids" not in splats:
            add_bilateral_grids(splats, cfg, Vt)
        GX, GY, Lz = cfg.bilateral_grid_shape
        if tuple(splats["bil_grids"].shape) != (Vt, Lz, GY, GX, 12):
            raise ValueError(f"splats['bil_grids'] has shape {tuple(splats['bil_grids'].shape)}, the {Vt} training views and "
                             f"cfg.bilateral_grid_shape want {(Vt, Lz, GY, GX, 12)}")
    pose = cfg.pose_opt
    if pose:
        if "pose_deltas" not in splats:
            add_pose_deltas(splats, Vt)
        if tuple(splats["pose_deltas"].shape) != (Vt, 9):
            raise ValueError(f"splats['pose_deltas'] has shape {tuple(splats['pose_deltas'].shape)}, the {Vt} training views want {(Vt, 9)}")
    dev = p["means"].device
    Ksh = p["sh"].shape[-1]
    sh_degree = isqrt(Ksh) - 1
    view, campos, Kpix = _cameras(extrinsics, intrinsics, W, H, dev)
    if pose:
        w2c_base, c2w_base = _camera_bases(extrinsics, dev)
    images = images.contiguous()
    background = torch.zeros(3, device=dev, dtype=torch.float32)
    bkgds = random_backgrounds(steps, cfg.seed).to(dev) if cfg.random_bkgd else None
    mode = "antialiased" if cfg.antialiased else "classic"
    reg_op, reg_sc = cfg.opacity_reg > 0.0, cfg.scale_reg > 0.0
    log = torch.zeros(steps, len(log_columns(cfg)), device=dev, dtype=torch.float64)
    hyp = batch_hyperparameters(cfg)
    lrs, lr_scale = hyp["lr"], hyp["lr_scale"]
    vis_adam = cfg.visible_adam
    decay = 0.01 ** (1.0 / cfg.max_steps)
    ws = ops.GsWorkspace()
    mcmc = cfg.strategy == "mcmc"
    densify = cfg.strategy == "densify"
    if densify:
        densify_state(splats)
    # what the densification and the visibility mask read of every render
    extra = dict(info_out={}, absgrad=cfg.densify_absgrad) if densify else dict(info_out={}) if vis_adam else {}
    leaves = [p[n].requires_grad_(True) for n in trained]
    if bil:
        leaves.append(splats["bil_grids"].requires_grad_(True))
    if pose:   # the last leaf; its gradient is dense [Vt,9] with zero rows for the other views, as nn.Embedding's is
        leaves.append(splats["pose_deltas"].requires_grad_(True))
    try:
        for i, js in enumerate(train_batch_order(V, steps, cfg.seed, cfg.test_every, cfg.batch_size)):
            if len(js) == 1:     # one view: slices (views of the tensors, no copy)
                j = slice(js[0], js[0] + 1)
                gj = slice(grid_of[js[0]], grid_of[js[0]] + 1)
            else:                # b distinct views: gathered rows; the gradient's scatter back is order-free
                j = torch.tensor(js, device=dev)
                gj = torch.tensor([grid_of[x] for x in js], device=dev)
            cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
            if pose:
                view_j, campos_j = ops.camera_adjust(w2c_base[j], c2w_base[j], splats["pose_deltas"][gj])
            else:
                view_j, campos_j = view[j], campos[j]
            color, depth, alpha = ops.gs_render(p["means"], cov, p["sh"], op, view_j, campos_j, Kpix[j], W, H,
                                                sh_degree=sh_degree, sh_layout=1, background=background if bkgds is None else bkgds[i],
                                                clamp_rgb=True, workspace=ws, rasterize_mode=mode, camera_grad=pose, **extra)
            if bil:
                color = ops.bilagrid_slice(color, splats["bil_grids"][gj])
            loss, l1, ssim = ops.photometric_loss(color, images[j], cfg.ssim_lambda)
            if cfg.depth_loss:
                dterm, _ = ops.depth_loss(depth, alpha, depths[j], None if depth_masks is None else depth_masks[j], cfg.scene_scale)
                loss = loss + cfg.depth_lambda * dterm
                rec = [loss.detach(), l1.detach(), ssim.detach(), dterm.detach()]
            else:
                rec = [loss.detach(), l1.detach(), ssim.detach()]
            if bil:
                tv = ops.bilagrid_tv(splats["bil_grids"])
                loss = loss + cfg.bilagrid_tv_lambda * tv
                rec = [loss.detach()] + rec[1:] + [tv.detach()]
            if reg_op or reg_sc:
                op_mean, sc_mean = ops.splat_regularisers(p["scales"], p["opacities"])
                if reg_op:
                    loss = loss + cfg.opacity_reg * op_mean
                    rec.append(op_mean.detach())
                if reg_sc:
                    loss = loss + cfg.scale_reg * sc_mean
                    rec.append(sc_mean.detach())
                rec[0] = loss.detach()
            grads = torch.autograd.grad(loss, leaves)
            log[i].copy_(torch.stack(rec))
            t = splats["step"] + 1
            with torch.no_grad():
                if vis_adam:   # the Gaussians some view of this step saw (:1111)
                    visible = ops.gs_visibility(extra["info_out"]["radii"])
                for n, g in zip(trained, grads):
                    lr = lrs[n] * (decay ** (t - 1) if n == "means" else 1.0)
                    sh = n == "sh"
                    if vis_adam:
                        ops.adam_step_visible(p[n], g.contiguous(), m[n], v[n], visible, lr=lr, betas=hyp["betas"], eps=hyp["eps"],
                                              lr2=lr / 20 if sh else None, period=Ksh if sh and Ksh > 1 else 0)
                    else:
                        ops.adam_step(p[n], g.contiguous(), m[n], v[n], lr=lr, step=t, betas=hyp["betas"], eps=hyp["eps"],
                                      lr2=lr / 20 if sh else None, period=Ksh if sh and Ksh > 1 else 0)
                if bil:   # every view's grid moves each step through the TV term, as in the reference
                    lr = bilagrid_learning_rate(cfg, t - 1)
                    ops.adam_step(splats["bil_grids"], grads[len(trained)].contiguous(), splats["bil_m"], splats["bil_v"],
                                  lr=lr * lr_scale if lr_scale != 1.0 else lr, step=t, betas=cfg.betas, eps=1e-15, period=0)
                if pose:  # torch.optim.Adam(weight_decay=reg): the decay joins the gradient; momentum and decay move every row each step
                    d = splats["pose_deltas"]
                    lr = pose_learning_rate(cfg, t - 1)
                    ops.adam_step(d, (grads[-1] + cfg.pose_opt_reg * d).contiguous(), splats["pose_m"], splats["pose_v"],
                                  lr=lr * lr_scale if lr_scale != 1.0 else lr, step=t, betas=(0.9, 0.999), eps=1e-8, period=0)
                if mcmc:
                    if mcmc_refines_at(cfg, t - 1):
                        mcmc_refine(splats, cfg, t)
                        leaves = [p[n].requires_grad_(True) for n in trained] + leaves[len(trained):]    # a grown scene has new tensors
                    ops.mcmc_noise(p["means"], p["scales"], p["quats"], p["opacities"], scaler=cfg.mcmc_noise_lr * (lrs["means"] * decay ** t),
                                   seed=cfg.seed, step=t)
                if densify and densify_active_at(cfg, t - 1):
                    info, st = extra["info_out"], densify_state(splats)
                    ops.densify_accumulate(st["grad2d"], st["count"], info["d_means2d_abs" if cfg.densify_absgrad else "d_means2d"],
                                           info["radii"], W, H)
                    if densify_refines_at(cfg, t - 1):
                        densify_refine(splats, cfg, t - 1)
                        leaves = [p[n].requires_grad_(True) for n in trained] + leaves[len(trained):]    # new tensors
                    if densify_resets_at(cfg, t - 1):
                        ops.densify_reset_opacity(p["opacities"].detach(), m["opacities"], v["opacities"], 2.0 * cfg.densify_prune_opa)
            splats["step"] = t
    finally:
        for n in trained:
            p[n].requires_grad_(False)
        if bil:
            splats["bil_grids"].requires_grad_(False)
        if pose:
            splats["pose_deltas"].requires_grad_(False)
    return splats_to_gaussians(splats), log
