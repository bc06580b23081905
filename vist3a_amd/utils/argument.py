"""CLI contract of the text->3DGS driver: every flag of `inference_vist3a_argument()` in /root/reference/utils/argument.py:392-443
(built there from add_model_selection_args :58-78, add_stitching_args :234-270, add_common_data_args :140-160) with the same
names, types and defaults, plus MI355X-specific extras that default to the reference's behaviour."""
from __future__ import annotations

import argparse

from ..models.stitching_layer_builder import parse_conv_spec


def inference_vist3a_argument() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Inference on VIST3A argument", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = p.add_argument_group("Model selection")
    g.add_argument("--feedforward_model", type=str, default="anysplat", choices=["anysplat"], help="Feedforward model to use")
    g.add_argument("--video_model", type=str, default="wan", choices=["wan"], help="Video model to use")
    g = p.add_argument_group("Stitching")
    g.add_argument("--stitching_layer_location", type=str, default="enc_blocks_2", help="Location of the stitching layer in the feedforward model")
    g.add_argument("--initialization_weight_path", type=str, default=None, help="Path to the initialization weight for the stitching layer")
    g.add_argument("--stitching_layer_config", type=parse_conv_spec, default="conv3d_k5x3x3_o1024_s1x2x2_p2x1x1", metavar="CONV_SPEC")
    g.add_argument("--lora_config", type=str, default="r8,a16,d0.05,f0", help="r<rank>,a<alpha>,d<dropout>,b<bias>,t<targets>,f<0/1>")
    g = p.add_argument_group("Data (common)")
    g.add_argument("--resolution", type=int, default=512, help="Image resolution")
    g.add_argument("--feedforward_resolution", type=int, default=448, help="Image resolution for feedforward model")
    g = p.add_argument_group("Inference")
    g.add_argument("--model_id", default="Wan-AI/Wan2.1-T2V-1.3B-Diffusers", type=str)
    g.add_argument("--checkpoint_path", type=str, required=True, help="Path to the trained stitching model ('synthetic' = seeded random weights)")
    g.add_argument("--transformer_lora_path", type=str, required=True, help="Path to the LoRA weights for the transformer ('none' to skip)")
    g.add_argument("--input_texts_path", type=str, required=True, help="Path to input texts for inference")
    g.add_argument("--output_dir", type=str, default="inference_vist3a_results", help="Path to save inference results")
    g.add_argument("--num_frames", type=int, default=13, help="Number of frames to generate for each input text")
    g.add_argument("--flow_shift", type=float, default=5, help="Flow shift value for timesteps")
    g.add_argument("--cfg_scale", type=str, default="7.5", help="Classifier-free guidance scale(s)")
    g = p.add_argument_group("MI355X extras (not in the reference)")
    g.add_argument("--num_inference_steps", type=int, default=50, help="denoise steps (the reference hard-codes 50)")
    g.add_argument("--anysplat_weights", type=str, default=None, help="local AnySplat .safetensors (no HF hub access offline)")
    g.add_argument("--text_embeds_path", type=str, default=None,
                   help="torch file {prompt: [512,4096] embedding, '__negative__': ...}; UMT5-XXL itself is outside this path (SURVEY §8f)")
    g.add_argument("--synthetic_text", action="store_true", help="seeded synthetic text embeddings (weights-free smoke runs)")
    g.add_argument("--scene_parallel", action="store_true",
                   help="all ranks cooperate on each prompt (CFG-parallel x sequence-parallel DiT over RCCL) instead of striding prompts")
    g.add_argument("--no_video", action="store_true", help="skip the interpolated orbit render (gs.avi / depth.avi)")
    g.add_argument("--overwrite", action="store_true", help="reuse an existing output directory (the reference raises)")
    g.add_argument("--post_opt_steps", type=int, default=0,
                   help="refine the predicted Gaussians for N steps against the frames the reconstruction was fed (AnySplat's post-optimisation, "
                        "vist3a_amd/post_opt) before gaussians.ply and the videos are written; 0 = off")
    g.add_argument("--post_opt_depth_lambda", type=float, default=0.0,
                   help="weight of the post-optimisation's depth term (the reference's depth_loss / depth_lambda, there 1e-2): an L1 in "
                        "disparity between the rendered expected depth and the depth head's map of each view, on its confident pixels; "
                        "0 = off")
    g.add_argument("--post_opt_bilateral_grid", action="store_true",
                   help="post-optimisation with one bilateral grid per view (the reference's use_bilateral_grid): the grids absorb the "
                        "frames' exposure and white-balance drift instead of the scene; they are not exported")
    g.add_argument("--post_opt_antialiased", action="store_true",
                   help="post-optimisation in the rasteriser's antialiased mode (the reference's antialiased; gsplat "
                        "rasterize_mode=\"antialiased\"): a Gaussian thinner than a pixel is dimmed as well as widened, so the scene "
                        "holds up at other resolutions; the evaluation and the videos then render in that mode too")
    g.add_argument("--post_opt_random_bkgd", action="store_true",
                   help="post-optimisation against a random background per step (the reference's random_bkgd), to discourage transparency")
    g.add_argument("--post_opt_opacity_reg", type=float, default=0.0, metavar="X",
                   help="weight of the mean opacity in the post-optimisation loss (the reference's opacity_reg); 0 = off")
    g.add_argument("--post_opt_scale_reg", type=float, default=0.0, metavar="X",
                   help="weight of the mean scale in the post-optimisation loss (the reference's scale_reg); 0 = off")
    g.add_argument("--post_opt_mcmc", action="store_true",
                   help="post-optimise with the MCMC strategy (the reference's `mcmc` configuration): dead Gaussians are relocated onto live "
                        "ones and the scene grows by 5 %% at every refine, opacity-gated noise moves the means after every step.  The "
                        "reference pairs it with --post_opt_opacity_reg 0.01 --post_opt_scale_reg 0.01; this switch does not set them")
    g.add_argument("--post_opt_mcmc_cap_max", type=int, default=1_000_000, metavar="N",
                   help="the MCMC strategy stops adding Gaussians at N (a scene already above N only relocates)")
    g.add_argument("--post_opt_mcmc_refine", type=str, default="500,25000,100", metavar="START,STOP,EVERY",
                   help="the MCMC strategy refines after the steps i with START < i < STOP and i %% EVERY == 0 (counted from 0)")
    g.add_argument("--post_opt_densify", action="store_true",
                   help="post-optimise with adaptive density control (the reference's `default` configuration with gsplat's "
                        "DefaultStrategy running): where the screen-space gradient is high small Gaussians are cloned and large ones "
                        "split, transparent and oversized ones are pruned, the opacities are reset periodically.  Not with --post_opt_mcmc")
    g.add_argument("--post_opt_densify_refine", type=str, default="500,15000,100,3000", metavar="START,STOP,EVERY,RESET",
                   help="densification refines after the steps i with START < i < STOP and i %% EVERY == 0 (counted from 0) and resets "
                        "the opacities every RESET steps")
    g.add_argument("--post_opt_densify_grad", type=float, default=2e-4, metavar="X",
                   help="average screen-space gradient above which a Gaussian is cloned or split (gsplat's grow_grad2d)")
    g.add_argument("--post_opt_densify_absgrad", action="store_true",
                   help="densify on the sum of absolute per-pixel gradients (gsplat's absgrad; wants a larger --post_opt_densify_grad, "
                        "gsplat suggests 8e-4)")
    g.add_argument("--post_opt_densify_cap_max", type=int, default=0, metavar="N",
                   help="a refine that would pass N Gaussians only prunes; 0 = no cap")
    g.add_argument("--post_opt_pose_opt", action="store_true",
                   help="refine the predicted camera poses together with the scene (the reference's pose_opt, on by default there): 9 "
                        "deltas per training view train through the rasteriser's camera gradients; the adjusted cameras are written to "
                        "post_opt_cameras.json next to gaussians.ply (the videos keep the predicted path)")
    g.add_argument("--post_opt_pose_lr", type=float, default=None, metavar="X",
                   help="with --post_opt_pose_opt: the pose optimiser's learning rate (the reference's pose_opt_lr, 1e-5)")
    g.add_argument("--post_opt_batch_size", type=int, default=1, metavar="B",
                   help="views per post-optimisation step (the reference's batch_size), 1 to 9: one render, loss and backward over B views, "
                        "one optimiser step; the rates are multiplied by sqrt(B), eps divided by it, the betas become 1 - B (1 - beta)")
    g.add_argument("--post_opt_visible_adam", action="store_true",
                   help="update only the Gaussians some view of the step saw (the reference's visible_adam, gsplat's SelectiveAdam: no "
                        "bias correction; rows outside every view keep parameters and moments)")
    g.add_argument("--post_opt_eval_every", type=int, default=0, metavar="K",
                   help="hold the views with index %% K == 0 out of the post-optimisation (the reference's test_every) and evaluate them "
                        "before and after it: PSNR, SSIM, the number of Gaussians and a time per image - with --post_opt_bilateral_grid "
                        "also the colour-corrected cc_psnr - into post_opt_stats.json next to gaussians.ply; 0 = off")
    g.add_argument("--export_format", type=str, default="", metavar="FMT[,FMT]",
                   help="extra scene files next to gaussians.ply, packed on the GPU: a comma list of ply_compressed "
                        "(gaussians.compressed.ply, SuperSplat's 16 bytes per splat) and splat (gaussians.splat, 32 bytes per splat); "
                        "empty = none")
    g.add_argument("--export_sh_rest", action="store_true",
                   help="with --export_format: write the higher-order harmonics into gaussians.compressed.ply too (default: DC colour "
                        "only, like gaussians.ply)")
    g.add_argument("--export_frame", type=str, default="camera", choices=("camera", "normalized"),
                   help="the frame of gaussians.ply and of every --export_format file: camera (the first camera's OpenCV frame, as "
                        "predicted) or normalized (upright, centred, unit-sized: world_normalisation of the predicted or pose-refined "
                        "cameras and the means, moved on the GPU, harmonics rotated; writes world_transform.json; the videos keep the camera frame)")
    g.add_argument("--lpips_vgg_weights", type=str, default=None, metavar="PATH",
                   help="with --post_opt_eval_every: torchvision's VGG-16 state dict (vgg16-397923af.pth); with --lpips_lin_weights adds "
                        "LPIPS to post_opt_stats.json")
    g.add_argument("--lpips_lin_weights", type=str, default=None, metavar="PATH",
                   help="with --post_opt_eval_every: the lpips package's weights/v0.1/vgg.pth (lin0..lin4)")
    return p


def parse_lora_mode(spec: str):
    """'r64,a32,d0.0,f0' -> (r, alpha): the two numbers the merged-at-load LoRA needs.  Grammar and defaults (r=8, alpha=32) of
    /root/reference/utils/lora_util/utils.py:57-117 (`LoraConfig`, `parse_lora_mode`); pinned by tests/golden/lora_tiny.safetensors."""
    import re
    r, alpha = 8, 32
    pat = re.compile(r"(?P<key>[radbf t])(?:(?P<num>[\d.]+)|(?P<str>[^,]+))")
    for chunk in spec.split(","):
        c = chunk.strip().lower()
        if c in ("enc", "fix_head", "fixhead"):
            continue
        m = pat.fullmatch(c)
        if not m:
            raise ValueError(f"Bad LoRA chunk: {c!r}")
        k = m["key"]
        if k in "radf" and m["num"] is None:
            raise ValueError(f"Bad LoRA chunk: {c!r}")
        if k == "r":
            r = int(m["num"])
        elif k == "a":
            alpha = int(m["num"])
        elif k == "d":
            float(m["num"])
        elif k == "b":
            if m["str"] not in {"none", "all", "lora_only"}:
                raise ValueError("b chunk must be none|all|lora_only")
        elif k == "f":
            if bool(int(m["num"])):
                raise NotImplementedError("fan_in_fan_out LoRA layers (f1) are not supported by the merged-at-load path")
    return r, alpha
