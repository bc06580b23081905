"""Generation quality evaluation (the reference's evaluation/gen_eval/t3_scene_evaluation.py), CLIP scores on the MI355X.

    python evaluation/gen_eval/t3_scene_evaluation.py --folder_path <results> --eval_save_path eval_results.json \
        --clip_model <local openai/clip-vit-base-patch16 folder> --longclip_model <local zer0int/LongCLIP-L-Diffusers folder>

<results>/<sequence>/{gs.avi|gs.mp4, prompt.txt} as written by inference_t23d.py.  Either model may be omitted; metrics that are not
computed (aesthetic, MUSIQ, UnifiedReward) are left out of the JSON."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def make_clip_scorer(model_dir):
    """f(frames uint8 [n,H,W,3], prompt) -> float for one local Hugging Face CLIPModel folder (weights + tokenizer files)"""
    import torch
    from transformers import CLIPTokenizerFast

    from vist3a_amd.evaluation.clip import ClipScorer, ClipWeights
    scorer = ClipScorer(ClipWeights.from_pretrained(model_dir, device="cuda"))
    tok = CLIPTokenizerFast.from_pretrained(str(model_dir), local_files_only=True)

    def fn(frames, prompt):
        enc = tok([prompt], padding=True, return_tensors="pt")
        return scorer.prompt_score(torch.from_numpy(frames), enc["input_ids"], enc["attention_mask"])
    return fn


def main(args, make_scorer=make_clip_scorer):
    from vist3a_amd.evaluation import gen_eval
    models = {"clip_score": args.clip_model, "longclip_score": args.longclip_model}
    models = {k: v for k, v in models.items() if v}
    if not models:
        raise SystemExit("nothing to compute: pass --clip_model and / or --longclip_model (local Hugging Face CLIPModel folders)")
    for name, d in models.items():
        if not Path(d).is_dir() or not (Path(d) / "config.json").exists():
            raise SystemExit(f"--{name.replace('_score', '')}_model: {d} is not a local Hugging Face model folder (no config.json)")
    if not Path(args.folder_path).is_dir():
        raise SystemExit(f"--folder_path: {args.folder_path} is not a directory")
    scorers = {name: make_scorer(d) for name, d in models.items()}
    return gen_eval.evaluate_folder(args.folder_path, scorers, args.eval_save_path)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Generation quality evaluation.")
    parser.add_argument("--folder_path", type=str, required=True, help="Path to the folder containing generated results.")
    parser.add_argument("--eval_save_path", type=str, default="eval_results.json", help="Path to save the evaluation results JSON.")
    parser.add_argument("--cache_folder", type=str, default=None, help="Accepted for compatibility with the reference; unused.")
    parser.add_argument("--clip_model", type=str, default=None, help="Local folder of openai/clip-vit-base-patch16 (clip_score).")
    parser.add_argument("--longclip_model", type=str, default=None, help="Local folder of zer0int/LongCLIP-L-Diffusers (longclip_score).")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
