"""Novel-view rendering of the RE10K protocol: the reference's evaluation/novel_view_synthesis_bench/nvs_eval.py:82-192
(`inference_nvs`, `main`).

Per sequence: the last four views (reversed) are the targets, the rest are the context, with the last context view duplicated
(1 + 4k views for the VAE encoder).  One full `StitchVAE3D.forward` on the context gives the Gaussians and the context poses; a
poses-only pass (`predict_poses`) on context + targets gives the target poses, whose translations are rescaled by
mean(first-pass context translations) / mean(pose-pass context translations); the targets are rendered at the feed-forward size
and, like the ground truth, written as PNGs quantised by `prep_image` (clip, * 255, truncated)."""
from __future__ import annotations

import json
import time
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch

N_TARGET = 4


def split_views(n: int) -> Tuple[List[int], List[int]]:
    """-> (target_view_index, source_index): target = reversed(range(n))[:4], source = the rest in order"""
    target = list(range(n))[::-1][:N_TARGET]
    source = [i for i in range(n) if i not in target]
    # the context pass sees len(source) + 1 views, the pose pass that + 4: the VAE encoder needs 1 + 4k frames
    if len(target) != N_TARGET or len(source) % 4 != 0 or not source:
        raise ValueError(f"{n} views: the NVS split needs 4 targets and 4k context views (+1 duplicated) so that both passes see "
                         f"1 + 4k views for the VAE encoder (e.g. 12 views -> 9 + 13)")
    return target, source


def align_target_poses(ctx_extrinsic: torch.Tensor, all_extrinsic: torch.Tensor, all_intrinsic: torch.Tensor, num_context_view: int):
    """nvs_eval.py:109-132: scale the pose pass's translations to the first pass's scene scale.
    -> (target extrinsics [1,4,4,4], target intrinsics [1,4,3,3], scale_factor, context extrinsics)"""
    ctx_all = all_extrinsic[:, :num_context_view].clone()
    tgt = all_extrinsic[:, num_context_view:].clone()
    tgt_K = all_intrinsic[:, num_context_view:]
    scale_factor = ctx_extrinsic[:, :, :3, 3].mean() / ctx_all[:, :, :3, 3].mean()
    tgt[..., :3, 3] = tgt[..., :3, 3] * scale_factor
    ctx_all[..., :3, 3] = ctx_all[..., :3, 3] * scale_factor
    return tgt, tgt_K, scale_factor, ctx_all


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def inference_nvs(images: torch.Tensor, vae_images: torch.Tensor, model, target_view_index: List[int],
                  generator: Optional[torch.Generator] = None, timings: Optional[dict] = None, device="cuda", record: Optional[dict] = None):
    """images [n,3,h,w], vae_images [n,3,H,W] in [0,1] -> rendered targets [4,3,h,w] in [0,1].
    timings: filled with encode_forward_ms / pose_ms / render_ms.  record: filled with the intermediate poses (tests)."""
    n = images.shape[0]
    source_index = [i for i in range(n) if i not in target_view_index]
    ctx = images[None].to(device)[:, source_index]
    ctx = torch.cat((ctx, ctx[:, -1:]), 1)
    ctx_vae = vae_images[None].to(device)[:, source_index]
    ctx_vae = torch.cat((ctx_vae, ctx_vae[:, -1:]), 1)
    num_context_view = ctx.shape[1]
    mark = _event if timings is not None else (lambda: None)     # (device events only when timing: the split runs on CPU in tests)
    e0 = mark()
    out = model(images=ctx_vae.permute(0, 2, 1, 3, 4) * 2 - 1, feedforward_image=ctx.permute(0, 2, 1, 3, 4) * 2 - 1, train=False,
                generator=generator)
    gaussians, ctx_pose = out.gaussians, out.pred_context_pose
    e1 = mark()
    tgt = images[None].to(device)[:, target_view_index]
    tgt_vae = vae_images[None].to(device)[:, target_view_index]
    allv = torch.cat((ctx, tgt), 1)
    allv_vae = torch.cat((ctx_vae, tgt_vae), 1)
    poses = model.predict_poses(images=allv_vae.permute(0, 2, 1, 3, 4) * 2 - 1, feedforward_image=allv.permute(0, 2, 1, 3, 4) * 2 - 1,
                                generator=generator)
    e2 = mark()
    tgt_ext, tgt_K, scale_factor, _ = align_target_poses(ctx_pose["extrinsic"], poses["extrinsic"], poses["intrinsic"], num_context_view)
    v = tgt.shape[1]
    h, w = images.shape[-2:]
    dev = tgt_ext.device
    render = model.stitched_3d_model.decoder.forward(gaussians, tgt_ext, tgt_K.float(), torch.ones(1, v, device=dev) * 0.01,
                                                     torch.ones(1, v, device=dev) * 100, (h, w))
    e3 = mark()
    if timings is not None:
        e3.synchronize()
        timings.update(encode_forward_ms=e0.elapsed_time(e1), pose_ms=e1.elapsed_time(e2), render_ms=e2.elapsed_time(e3))
    if record is not None:
        record.update(gaussians=gaussians, target_extrinsic=tgt_ext, target_intrinsic=tgt_K.float(), scale_factor=scale_factor)
    return render.color[0]


def quantize(image: torch.Tensor) -> np.ndarray:
    """prep_image (anysplat/src/misc/image_io.py:41-57): [3,H,W] in [0,1] -> uint8 [H,W,3], clip(x, 0, 1) * 255 truncated"""
    return (image.detach().clip(min=0, max=1) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()


def save_png(image: torch.Tensor, path: Path) -> None:
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(quantize(image)).save(path)


def load_nvs_model(args):
    """load_stitching_model (models/loading.py) with a VAE that can encode: with `--checkpoint_path synthetic` and no local Wan
    folder, the VAE gets seeded encoder weights next to the seeded decoder."""
    import os
    from ..models.loading import load_stitching_model
    vae = None
    if getattr(args, "checkpoint_path", None) == "synthetic" and not os.path.isdir(os.path.join(str(args.model_id or ""), "vae")):
        from ..t23d import random_vae_decoder_state_dict, random_vae_encoder_state_dict
        from ..wan.vae import WanVAEConfig, WanVAEDecoder
        cfg = WanVAEConfig()
        sd = {**random_vae_decoder_state_dict(cfg, 1, "cuda"), **random_vae_encoder_state_dict(cfg, 4, "cuda")}
        vae = WanVAEDecoder(cfg, sd, device=torch.device("cuda"))
    return load_stitching_model(args, vae=vae)


def main(args) -> List[dict]:
    """nvs_eval.py main: render every sequence's targets into <output_dir>/images/<seq>/{gt,pred}/NNNNNN.png"""
    from .re10k import Re10KNVSDataset, load_seq_id_map
    if len(args.dataset) > 1:
        raise NotImplementedError("Currently only single dataset evaluation is supported.")
    name, root = args.dataset[0]
    if name != "re10k":
        raise NotImplementedError(f"NVS evaluation dataset {name} is not implemented.")
    seq_id_map = load_seq_id_map(args.seq_id_map)
    dataset = Re10KNVSDataset(root, seq_id_map, load_img_size=args.resolution, feedforward_img_size=args.feedforward_resolution,
                              seq_file=args.seq_file)
    t0 = time.time()
    model = load_nvs_model(args)
    print(f"[nvs] model loaded in {time.time() - t0:.1f} s; {len(dataset)} sequences")
    seqs = dataset.sequence_list[: args.max_sequences] if args.max_sequences else dataset.sequence_list
    rows = []
    for seq in seqs:
        batch = dataset.get_data(sequence_name=seq, ids=seq_id_map[seq])
        images, vae_images = batch["images"], batch["vae_images"]
        target_view_index, _ = split_views(images.shape[0])
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        t = {}
        with torch.no_grad():
            pred = inference_nvs(images, vae_images, model, target_view_index, generator=gen, timings=t)
        save = Path(args.output_dir) / "images" / seq
        for i, (g, p) in enumerate(zip(images[target_view_index], pred)):
            save_png(g, save / "gt" / f"{i:0>6}.png")
            save_png(p, save / "pred" / f"{i:0>6}.png")
        print(f"[nvs] {seq}: encode+forward {t['encode_forward_ms']:.1f} ms, pose pass {t['pose_ms']:.1f} ms, "
              f"render {t['render_ms']:.1f} ms")
        rows.append(dict(seq=seq, **t))
    Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    (Path(args.output_dir) / "nvs_timings.json").write_text(json.dumps(rows, indent=1))
    return rows
