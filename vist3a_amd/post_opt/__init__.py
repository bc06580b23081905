"""Post-optimisation of predicted Gaussians against their input views (the reference's
third_party_model/anysplat/src/post_opt/simple_trainer.py), on the HIP rasteriser, loss and optimiser."""
from .trainer import (PARAM_NAMES, PostOptConfig, adjusted_extrinsics, batch_hyperparameters, bilagrid_learning_rate, create_splats, densify_active_at,  # noqa: F401
                      densify_refine, densify_refines_at, densify_resets_at, densify_state, log_columns, mcmc_growth, mcmc_refine, mcmc_refines_at, pose_learning_rate, pose_transforms, post_optimize, random_backgrounds,
                      train_batch_order, train_view_order, train_views, view_order)
from .evaluate import evaluate_views  # noqa: F401


def export_splats_from(splats: dict, format: str = "ply", save_to=None, sh_rest: bool = True) -> bytes:
    """A trainer state (create_splats / post_optimize's `splats`) as a scene file: the reference trainer's save_ply step
    (simple_trainer.py calls its exporter's export_splats).  `format` is "ply", "splat" or "ply_compressed"; the parameters are
    read where they are (logs, logits, xyzw quaternions, one harmonics tensor); sh_rest=False writes the DC colour only."""
    from ..utils.splat_export import export_scene
    p = dict(splats["params"])
    p = {k: p[k].detach() for k in PARAM_NAMES}
    if not sh_rest:
        p["sh"] = p["sh"][..., :1].contiguous()
    return export_scene(p, format, save_to, quats_xyzw=True)


def load_splats_into(path, cfg: PostOptConfig, n_views=None, **load_kw) -> dict:
    """The inverse of export_splats_from: a stored scene (`ply`, `ply_compressed` or `splat`; a path or the file's bytes) as a fresh
    trainer state - create_splats' dict with every row of the file kept, zero Adam moments and step 0 - so that post_optimize(...,
    splats=...) refines it further.  load_kw: utils.splat_import.load_scene's `opacity` and `strict`.  With cfg.use_bilateral_grid
    and `n_views`, identity grids are added as create_splats adds them."""
    import torch
    from .trainer import add_bilateral_grids
    from ..utils.splat_import import load_scene
    p = load_scene(path, quats_xyzw=True, **load_kw)
    if p["means"].shape[0] == 0:
        raise ValueError("load_splats_into: the file holds no splat")
    splats = dict(params=p, m={k: torch.zeros_like(t) for k, t in p.items()}, v={k: torch.zeros_like(t) for k, t in p.items()}, step=0,
                  keep=torch.ones(p["means"].shape[0], dtype=torch.bool, device=p["means"].device))
    if cfg.use_bilateral_grid and n_views is not None:
        add_bilateral_grids(splats, cfg, n_views)
    return splats
