"""Text -> 3DGS inference CLI — drop-in for /root/reference/inference_t23d.py (same flags, same output layout
`<output_dir>/<prompt[:100] sans '/'>/{prompt.txt, gaussians.ply, gs.mp4, depth.mp4}` — H.264 mp4 like the reference when imageio-ffmpeg
or OpenCV is importable; in this image neither exists and the same frames are written as Motion-JPEG gs.avi / depth.avi).

    python -m torch.distributed.run --nproc_per_node=K --master-addr 127.0.0.1 inference_t23d.py --checkpoint_path ... \
        --transformer_lora_path ... --input_texts_path prompts.txt

One process per GPU; prompts are strided over ranks (no inter-GPU traffic), exactly like the reference (:53-62)."""
from __future__ import annotations

import json
import os
import sys
import zlib
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from vist3a_amd.models.loading import load_stitching_model  # noqa: E402
from vist3a_amd.misc.image_io import save_interpolated_video  # noqa: E402
from vist3a_amd.t23d import Text23DGS, synthetic_text_embeddings  # noqa: E402
from vist3a_amd.utils.argument import inference_vist3a_argument  # noqa: E402
from vist3a_amd.utils.dist_util import setup_dist, shard_prompts  # noqa: E402
from vist3a_amd.utils.ply_export import export_ply  # noqa: E402
from vist3a_amd.utils.splat_export import FILE_NAMES as EXPORT_FILE_NAMES, export_gaussians, parse_formats as parse_export_formats  # noqa: E402
from vist3a_amd.utils.splat_transform import transform_gaussians, world_normalisation, write_world_transform  # noqa: E402
from vist3a_amd.wan.dit import WAN_1_3B, WAN_14B, WanDiT  # noqa: E402
from vist3a_amd.wan.weights import load_dit_config, load_dit_state_dict, load_peft_lora, random_dit_state_dict  # noqa: E402

PROMPT_TEMPLATE = "The camera rotates around the scene, maintaining constant distance: `{}`. The orbiting trajectory captures 3D structure and consistency."
NEGATIVE_PROMPT = ("Background blur, Blurred background, Blurred scene, Artifacts, not aesthetic, not realistic, rendered noise, low quality movement, "
                   "low quality video, low quality image, deformed, disfigured, distorted, extra limbs, cloned face, skinny, glitchy, double torso, "
                   "extra arms, extra hands, mangled fingers, missing lips, ugly face, distorted legs, fused fingers, too many fingers, long neck")


def build_transformer(args, device):
    cfg = WAN_14B if "14B" in args.model_id else WAN_1_3B
    if args.checkpoint_path == "synthetic" and not os.path.isdir(args.model_id):
        sd = random_dit_state_dict(cfg, seed=0, device=str(device))
    else:
        cfg = load_dit_config(args.model_id, cfg)   # <model_id>/transformer/config.json, as diffusers' from_pretrained
        sd = load_dit_state_dict(args.model_id)
    if args.transformer_lora_path not in ("none", "", None):
        load_peft_lora(args.transformer_lora_path, sd)  # merged at load: W += (alpha/r) B A
    return WanDiT(cfg, sd, device=device)


def build_text_encoder(args, device):
    """(prompts, max_len) -> embeddings from `<model_id>/text_encoder` + `<model_id>/tokenizer` (the folders diffusers' WanPipeline
    loads, /root/reference/inference_t23d.py:71-83), or None when they are not on disk (no hub access here)."""
    te, tk = os.path.join(args.model_id, "text_encoder"), os.path.join(args.model_id, "tokenizer")
    if not (os.path.isdir(te) and os.path.isdir(tk)):
        return None
    import glob
    from safetensors.torch import load_file
    from transformers import AutoTokenizer
    from vist3a_amd.wan.text_encoder import UMT5Config, UMT5TextEncoder, make_pipeline_text_encoder
    sd = {}
    for f in sorted(glob.glob(os.path.join(te, "*.safetensors"))):
        sd.update(load_file(f))
    return make_pipeline_text_encoder(UMT5TextEncoder(UMT5Config(), sd, device=device), AutoTokenizer.from_pretrained(tk))


def refine(gaussians, clip_cl, pose, res, steps, depth_dict=None, depth_lambda=0.0, bilateral_grid=False, eval_every=0, lpips=None,
           antialiased=False, random_bkgd=False, opacity_reg=0.0, scale_reg=0.0, mcmc=None, pose_opt=False, pose_lr=None,
           cameras_out=None, densify=None, batch_size=1, visible_adam=False):
    """-> (refined Gaussians, stats or None).  With eval_every = K > 0 the views with index % K == 0 are held out of the loop and
    scored before and after it: stats = {"before": {...}, "after": {...}, "held_out": [...]} (vist3a_amd.post_opt.evaluate_views).
    antialiased / random_bkgd / opacity_reg / scale_reg: the PostOptConfig fields of those names; the evaluation renders in the
    loop's rasterize mode.  mcmc: None, or (cap_max, (start, stop, every)) to run the loop with cfg.strategy = "mcmc"; the refined
    scene then has as many Gaussians as the strategy left it with.  pose_opt / pose_lr: cfg.pose_opt and cfg.pose_opt_lr (None: its
    default) - scene and cameras are refined together, and the dict `cameras_out` (if given) receives "extrinsics" (the adjusted
    camera-to-world matrix of every view, held-out views as given), "deltas" [Vt,9] and "train_views", as lists.
    densify: None, or densify_options' dict of PostOptConfig fields to run the loop with cfg.strategy = "densify" (adaptive density
    control: clone / split / prune); the refined scene has as many Gaussians as it left.
    batch_size / visible_adam: the PostOptConfig fields of those names (views per step; the masked Adam update)."""
    from vist3a_amd import ops
    from vist3a_amd.post_opt import PostOptConfig, adjusted_extrinsics, create_splats, evaluate_views, post_optimize, train_views
    with torch.no_grad():
        ff = ops.bilinear_cl(clip_cl, (res, res), align_corners=False)          # what Text23DGS.generate fed the reconstruction
        frames = ((ff[..., :3].float() + 1) / 2).clamp(0, 1).contiguous()       # [V,res,res,3] in [0,1]
    cfg, extra = PostOptConfig(), {}
    if depth_lambda > 0:
        if not depth_dict or "depth" not in depth_dict or "conf_valid_mask" not in depth_dict:
            raise ValueError("--post_opt_depth_lambda needs the reconstruction's depth_dict (depth, conf_valid_mask); this output has none")
        # the depth head's map is z along the camera axis in the units of pose["extrinsic"]: what the
        # rasteriser's depth channel accumulates, so it is the target as it stands
        depths, masks = depth_dict["depth"][0, ..., 0].detach().float().contiguous(), depth_dict["conf_valid_mask"][0].detach().contiguous()
        if tuple(depths.shape[-2:]) != tuple(frames.shape[1:3]) or tuple(masks.shape[-2:]) != tuple(frames.shape[1:3]):
            raise ValueError(f"depth maps {tuple(depths.shape)} / masks {tuple(masks.shape)} do not match the frames {tuple(frames.shape)}")
        cfg = PostOptConfig(depth_loss=True, depth_lambda=float(depth_lambda))
        extra = dict(depths=depths, depth_masks=masks)
    cfg.use_bilateral_grid = bool(bilateral_grid)
    cfg.test_every = int(eval_every)
    cfg.antialiased, cfg.random_bkgd = bool(antialiased), bool(random_bkgd)
    cfg.opacity_reg, cfg.scale_reg = float(opacity_reg), float(scale_reg)
    if mcmc is not None:
        cfg.strategy, cfg.mcmc_cap_max = "mcmc", int(mcmc[0])
        cfg.mcmc_refine_start_iter, cfg.mcmc_refine_stop_iter, cfg.mcmc_refine_every = (int(x) for x in mcmc[1])
    if densify is not None:
        cfg.strategy = "densify"
        for k, x in densify.items():
            setattr(cfg, k, x)
    cfg.pose_opt = bool(pose_opt)
    cfg.batch_size, cfg.visible_adam = batch_size, bool(visible_adam)
    if pose_lr is not None:
        cfg.pose_opt_lr = float(pose_lr)
    ext, intr = pose["extrinsic"][0].detach(), pose["intrinsic"][0].detach()
    stats = None
    if cfg.test_every > 0:
        train = set(train_views(frames.shape[0], cfg.test_every))      # raises when K leaves no view to train on
        held = [i for i in range(frames.shape[0]) if i not in train]
        score = lambda gs: evaluate_views(gs, frames[held].contiguous(), ext[held], intr[held], color_correct=cfg.use_bilateral_grid,
                                          lpips=lpips, antialiased=cfg.antialiased)
        stats = dict(before=score(gaussians), held_out=held)
    if cfg.pose_opt:   # the loop's state is kept: the trained deltas are in it
        tv = train_views(frames.shape[0], cfg.test_every)
        splats = create_splats(gaussians, cfg, len(tv))
        g, _ = post_optimize(gaussians, frames, ext, intr, cfg, steps=steps, splats=splats, **extra)
        if cameras_out is not None:
            cameras_out.update(extrinsics=adjusted_extrinsics(ext, splats, cfg).cpu().tolist(), deltas=splats["pose_deltas"].cpu().tolist(),
                               train_views=tv)
    else:
        g, _ = post_optimize(gaussians, frames, ext, intr, cfg, steps=steps, **extra)
    if stats is not None:
        stats = dict(before=stats["before"], after=score(g), held_out=stats["held_out"])
    return g, stats


def mcmc_options(args):
    """--post_opt_mcmc* -> None (off) or (cap_max, (start, stop, every)) for refine()"""
    if not args.post_opt_mcmc:
        return None
    if args.post_opt_steps <= 0:
        raise ValueError("--post_opt_mcmc needs --post_opt_steps > 0 (it is a strategy of the post-optimisation)")
    try:
        refine_at = tuple(int(x) for x in args.post_opt_mcmc_refine.split(","))
    except ValueError:
        refine_at = ()
    if len(refine_at) != 3 or refine_at[2] < 1:
        raise ValueError(f"--post_opt_mcmc_refine wants three integers START,STOP,EVERY with EVERY >= 1, got {args.post_opt_mcmc_refine!r}")
    if args.post_opt_mcmc_cap_max < 1:
        raise ValueError("--post_opt_mcmc_cap_max must be positive")
    return args.post_opt_mcmc_cap_max, refine_at


def batch_options(args):
    """--post_opt_batch_size / --post_opt_visible_adam -> (batch_size, visible_adam) for refine(), validated as PostOptConfig does"""
    from vist3a_amd.post_opt import PostOptConfig
    if (args.post_opt_batch_size != 1 or args.post_opt_visible_adam) and args.post_opt_steps <= 0:
        raise ValueError("--post_opt_batch_size / --post_opt_visible_adam need --post_opt_steps > 0 (they are options of the post-optimisation)")
    try:
        PostOptConfig(batch_size=args.post_opt_batch_size, visible_adam=bool(args.post_opt_visible_adam)).check_batch()
    except ValueError as e:
        raise ValueError(f"--post_opt_batch_size: {e}") from None
    return args.post_opt_batch_size, bool(args.post_opt_visible_adam)


def densify_options(args):
    """--post_opt_densify* -> None (off) or the PostOptConfig fields of the "densify" strategy for refine()"""
    if not args.post_opt_densify:
        return None
    if args.post_opt_mcmc:
        raise ValueError("--post_opt_densify and --post_opt_mcmc are two strategies of the post-optimisation: choose one")
    if args.post_opt_steps <= 0:
        raise ValueError("--post_opt_densify needs --post_opt_steps > 0 (it is a strategy of the post-optimisation)")
    try:
        at = tuple(int(x) for x in args.post_opt_densify_refine.split(","))
    except ValueError:
        at = ()
    if len(at) != 4 or min(at) < 0 or at[2] < 1 or at[3] < 1:
        raise ValueError("--post_opt_densify_refine wants four integers START,STOP,EVERY,RESET >= 0 with EVERY, RESET >= 1, got "
                         f"{args.post_opt_densify_refine!r}")
    if not args.post_opt_densify_grad > 0:
        raise ValueError("--post_opt_densify_grad must be positive")
    if args.post_opt_densify_cap_max < 0:
        raise ValueError("--post_opt_densify_cap_max must be >= 0 (0 = no cap)")
    return dict(densify_refine_start_iter=at[0], densify_refine_stop_iter=at[1], densify_refine_every=at[2], densify_reset_every=at[3],
                densify_grow_grad2d=float(args.post_opt_densify_grad), densify_absgrad=bool(args.post_opt_densify_absgrad),
                densify_cap_max=int(args.post_opt_densify_cap_max))


def main(args):
    batch_size, visible_adam = batch_options(args)   # before anything is loaded: a refused batch size costs nothing
    setup_dist()
    rank, world = dist.get_rank(), dist.get_world_size()
    device = torch.device(f"cuda:{rank % torch.cuda.device_count()}")
    torch.cuda.set_device(device)
    with open(args.input_texts_path, "r") as f:
        prompts = [line.strip() for line in f.readlines()]
    coop = args.scene_parallel and world > 1
    if not coop:  # the reference's split: whole prompts per rank, no collective
        prompts = shard_prompts(prompts, rank, world)
    gen = torch.Generator().manual_seed(12413)  # seed_everything(12413): one stream per process, consumed in prompt order
    transformer = build_transformer(args, device)
    stitched = load_stitching_model(args)
    scene = Text23DGS(transformer, stitched.diffusion_vae, stitched, flow_shift=args.flow_shift,
                      feedforward_resolution=args.feedforward_resolution, device=device)
    if coop:  # every rank works on the same prompt: CFG-parallel x sequence-parallel denoise, rank 0 writes
        from vist3a_amd.wan.seqpar import DenoisePlan
        scene.pipe.plan = DenoisePlan.from_dist()
        stitched.recon_group = scene.pipe.plan.world      # the reconstruction of the scene split by views over the same ranks
    embeds = torch.load(args.text_embeds_path, map_location="cpu") if args.text_embeds_path else None
    if args.post_opt_eval_every < 0 or (args.post_opt_eval_every > 0 and args.post_opt_steps <= 0):
        raise ValueError("--post_opt_eval_every K needs K >= 0 and --post_opt_steps > 0 (it evaluates the views held out of the refinement)")
    if args.post_opt_opacity_reg < 0 or args.post_opt_scale_reg < 0:
        raise ValueError("--post_opt_opacity_reg and --post_opt_scale_reg are weights >= 0")
    mcmc = mcmc_options(args)
    densify = densify_options(args)
    export_formats = parse_export_formats(args.export_format)
    if args.export_sh_rest and not export_formats:
        raise ValueError("--export_sh_rest needs --export_format (it is an option of the extra scene files)")
    if (args.post_opt_pose_opt or args.post_opt_pose_lr is not None) and args.post_opt_steps <= 0:
        raise ValueError("--post_opt_pose_opt / --post_opt_pose_lr need --post_opt_steps > 0 (the poses are refined by the post-optimisation)")
    if args.post_opt_pose_lr is not None and not args.post_opt_pose_lr > 0:
        raise ValueError("--post_opt_pose_lr must be positive")
    if (args.lpips_vgg_weights is None) != (args.lpips_lin_weights is None):
        raise ValueError("--lpips_vgg_weights and --lpips_lin_weights go together: give both or neither")
    lpips = None
    if args.post_opt_eval_every > 0 and args.lpips_vgg_weights is not None:
        from vist3a_amd.evaluation.lpips import get_lpips
        lpips = get_lpips(args.lpips_vgg_weights, args.lpips_lin_weights, device)
    encode = None if (embeds is not None or args.synthetic_text) else build_text_encoder(args, device)
    for prompt in prompts:
        if encode is not None:  # the reference's own route: WanPipeline.encode_prompt(prompt, negative_prompt), 512 tokens, zero padded
            pe, ne = encode([PROMPT_TEMPLATE.format(prompt)], 512), encode([NEGATIVE_PROMPT], 512)
        elif embeds is not None:
            pe, ne = embeds[PROMPT_TEMPLATE.format(prompt)][None].to(device), embeds["__negative__"][None].to(device)
        elif args.synthetic_text:
            pe, ne = synthetic_text_embeddings(device, seed=zlib.crc32(prompt.encode()) % (2 ** 31))
        else:
            raise RuntimeError(f"no text encoder: {args.model_id}/text_encoder + /tokenizer are not on disk (no hub access here); pass "
                               "--text_embeds_path (precomputed UMT5 embeddings) or --synthetic_text")
        out, _, clip_cl = scene.generate(pe, ne, generator=gen, num_frames=args.num_frames, num_inference_steps=args.num_inference_steps,
                                   guidance_scale=float(args.cfg_scale), height=args.resolution, width=args.resolution)
        if coop and rank != 0:
            continue
        save = Path(args.output_dir) / prompt[:100].replace("/", "")
        os.makedirs(save, exist_ok=args.overwrite)  # the reference raises when the directory exists (inference_t23d.py:126)
        (save / "prompt.txt").write_text(prompt)
        g = out.gaussians
        cameras = {}
        if args.post_opt_steps > 0:   # against the frames the reconstruction saw, at the predicted context poses and intrinsics
            g, stats = refine(g, clip_cl, out.pred_context_pose, args.feedforward_resolution, args.post_opt_steps, out.depth_dict,
                              args.post_opt_depth_lambda, args.post_opt_bilateral_grid, args.post_opt_eval_every, lpips,
                              antialiased=args.post_opt_antialiased, random_bkgd=args.post_opt_random_bkgd,
                              opacity_reg=args.post_opt_opacity_reg, scale_reg=args.post_opt_scale_reg, mcmc=mcmc,
                              pose_opt=args.post_opt_pose_opt, pose_lr=args.post_opt_pose_lr, cameras_out=cameras, densify=densify,
                              batch_size=batch_size, visible_adam=visible_adam)
            if stats is not None:
                (save / "post_opt_stats.json").write_text(json.dumps(stats, indent=1))
            if args.post_opt_pose_opt:   # the refined cameras; the videos below keep the predicted path, as the reference's trajectory does
                (save / "post_opt_cameras.json").write_text(json.dumps(cameras, indent=1))
        if not args.no_video:  # orbit video through the predicted context poses (reference :144-154)
            decoder = stitched.stitched_3d_model.decoder
            mode = decoder.rasterize_mode
            if args.post_opt_steps > 0 and args.post_opt_antialiased:   # a scene fitted in the antialiased mode is shown in it
                decoder.rasterize_mode = "antialiased"
            try:
                save_interpolated_video(out.pred_context_pose["extrinsic"], out.pred_context_pose["intrinsic"], 1, args.feedforward_resolution,
                                        args.feedforward_resolution, g, str(save), decoder)
            finally:
                decoder.rasterize_mode = mode
        if args.export_frame == "normalized":   # the files below in the normalised world frame; the videos above kept the camera frame
            ext = torch.tensor(cameras["extrinsics"], dtype=torch.float64) if "extrinsics" in cameras else out.pred_context_pose["extrinsic"][0]
            T = world_normalisation(ext, g.means[0].detach().float().contiguous())
            g = transform_gaussians(g, T)
            write_world_transform(save / "world_transform.json", T, ext)
        export_ply(g.means[0], g.scales[0], g.rotations[0], g.harmonics[0], g.opacities[0], save / "gaussians.ply", save_sh_dc_only=True)
        for fmt in export_formats:   # extra files only: gaussians.ply above is written as without the flag
            export_gaussians(g, save / EXPORT_FILE_NAMES[fmt], fmt, sh_rest=args.export_sh_rest)
        print(f"[rank {rank}] {save}: {g.means.shape[1]} gaussians", flush=True)
    if world > 1:
        dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(inference_vist3a_argument().parse_args())
