"""CLI contract of the two NVS evaluation scripts: every flag of `stitching_nvs_evaluation_argument()` in
the reference's utils/argument.py:315-331 (built there from add_model_selection_args :58-78, add_stitching_args :234-270,
add_eval_data_args :203-231 with add_common_data_args :140-160) with the same names, types, defaults and required flags, plus
MI355X-specific extras that default to the reference's behaviour."""
from __future__ import annotations

import argparse
import pathlib

from ..models.stitching_layer_builder import parse_conv_spec


def parse_dataset(arg: str):
    """NAME:ROOT -> (name, root) (argument.py:16-32)"""
    try:
        name, root = arg.split(":", 1)
    except ValueError:
        raise argparse.ArgumentTypeError("Dataset must be NAME:PATH, e.g. dl3dv:/data/dl3dv")
    root_path = pathlib.Path(root).expanduser()
    if not root_path.exists():
        raise argparse.ArgumentTypeError(f"Path does not exist: {root_path}")
    return name, root_path


def stitching_nvs_evaluation_argument() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Stitching NVS evaluation argument", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
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
    g = p.add_argument_group("Data (evaluation)")
    g.add_argument("--dataset", type=parse_dataset, action="append", metavar="NAME:ROOT", required=True,
                   help="Provide a dataset as NAME:ROOT, e.g. --dataset re10k:/data/re10k")
    g.add_argument("--seq_id_map", type=str, required=True, help="Path to the JSON file mapping sequence names to frame IDs for evaluation")
    g = p.add_argument_group("Evaluation")
    g.add_argument("--checkpoint_path", type=str, help="Path to the trained stitching model ('synthetic' = seeded random weights)")
    g.add_argument("--output_dir", type=str, default="nvs_evaluation_results", help="Path to save evaluation results")
    g = p.add_argument_group("MI355X extras (not in the reference)")
    g.add_argument("--anysplat_weights", type=str, default=None, help="local AnySplat .safetensors (no HF hub access offline)")
    g.add_argument("--model_id", default="Wan-AI/Wan2.1-T2V-1.3B-Diffusers", type=str, help="local Wan folder whose vae/ holds the VAE")
    g.add_argument("--seq_file", type=str, default=None,
                   help="sequence list, one per line (the reference's re10k_test.txt); default: the keys of --seq_id_map in file order")
    g.add_argument("--seed", type=int, default=0, help="seed of each sequence's posterior-sampling generator (the reference uses the global RNG)")
    g.add_argument("--max_sequences", type=int, default=None, help="evaluate at most this many sequences")
    g.add_argument("--save_suffix", type=str, default=None, help="calculate_metric.py: write overall-metric-<suffix>.csv")
    return p


class _MetricParser(argparse.ArgumentParser):
    """rejects one LPIPS weight file without the other"""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if (ns.lpips_vgg_weights is None) != (ns.lpips_lin_weights is None):
            self.error("--lpips_vgg_weights and --lpips_lin_weights go together: give both or neither")
        return ns, rest


def calculate_metric_argument() -> argparse.ArgumentParser:
    """calculate_metric.py's command line: stitching_nvs_evaluation_argument() plus the two LPIPS weight files (not in the reference,
    whose lpips package finds its own).  Without them LPIPS is not computed."""
    p = _MetricParser(description="Stitching NVS evaluation argument", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                      parents=[stitching_nvs_evaluation_argument()], add_help=False)
    g = p.add_argument_group("LPIPS (not in the reference)")
    g.add_argument("--lpips_vgg_weights", type=str, default=None, metavar="PATH",
                   help="torchvision's VGG-16 state dict (vgg16-397923af.pth, or a .safetensors of it)")
    g.add_argument("--lpips_lin_weights", type=str, default=None, metavar="PATH",
                   help="the lpips package's weights/v0.1/vgg.pth (lin0..lin4)")
    return p
