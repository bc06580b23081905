"""Post-optimisation of predicted Gaussians against their input views (the reference's
third_party_model/anysplat/src/post_opt/simple_trainer.py), on the HIP rasteriser, loss and optimiser."""
from .trainer import (PARAM_NAMES, PostOptConfig, adjusted_extrinsics, bilagrid_learning_rate, create_splats, densify_active_at,  # noqa: F401
                      densify_refine, densify_refines_at, densify_resets_at, densify_state, log_columns, mcmc_growth, mcmc_refine, mcmc_refines_at, pose_learning_rate, pose_transforms, post_optimize, random_backgrounds,
                      train_view_order, train_views, view_order)
from .evaluate import evaluate_views  # noqa: F401
