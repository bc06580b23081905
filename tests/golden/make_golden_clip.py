"""Golden vectors for the CLIP score, produced by transformers.CLIPModel itself on seeded random weights (offline; no checkpoint).

    python tests/golden/make_golden_clip.py   ->  tests/golden/clip_tiny.safetensors

Two configurations with head size 64, keys prefixed a. and b.:
  a  patch 16 at image 64 (17 tokens), one vision layer; a 2-layer text tower with eos_token_id = 2 (pooling at argmax(input_ids))
  b  patch 14 at image 56 (17 tokens, K = 588 is not a multiple of 8), two vision layers; eos_token_id = 59 (pooling at its first
     position), prompts padded AFTER the EOS token, one of them with the pad token equal to the EOS token
Per configuration: w.<state-dict key> (bf16-exact values stored as bf16, to keep the file under the size limit; LayerNorm weights and
all biases are randomised), frames (uint8), pixel_values (CLIPImageProcessorPil's own output), input_ids, attention_mask, image_embeds,
text_embeds, logits_per_image, vision_hidden.N, text_hidden.N (output_hidden_states) and meta = the config numbers."""
from __future__ import annotations

import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np
import torch
from safetensors.torch import save_file

CONFIGS = {
    "a": dict(vision=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1, image_size=64, patch_size=16),
              text=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=1, vocab_size=60,
                        max_position_embeddings=16, eos_token_id=2, bos_token_id=0, pad_token_id=1),
              proj=32, seed=31, frame_hw=(80, 112),
              ids=[[5, 9, 33, 41, 58, 3, 1, 1, 1, 1], [7, 8, 9, 10, 11, 12, 13, 14, 15, 59]],
              mask=[[1, 1, 1, 1, 1, 1, 0, 0, 0, 0], [1] * 10]),
    "b": dict(vision=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=1, image_size=56, patch_size=14),
              text=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1, vocab_size=60,
                        max_position_embeddings=12, eos_token_id=59, bos_token_id=58, pad_token_id=0),
              proj=32, seed=47, frame_hw=(90, 70),
              ids=[[58, 4, 17, 59, 0, 0, 0, 0, 0], [58, 21, 22, 23, 24, 25, 59, 59, 59]],
              mask=[[1, 1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0, 0]]),
}


def frames_for(hw, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    smooth = torch.stack([0.5 + 0.4 * torch.sin(0.07 * (c + 1) * x + 0.05 * y + c) for c in range(3)], -1)
    noisy = torch.rand(H, W, 3, generator=g, dtype=torch.float64)
    return (torch.stack([smooth, noisy]).clamp(0, 1) * 255).round().to(torch.uint8)


def make(tag, c, out):
    from transformers import CLIPConfig, CLIPModel
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    torch.manual_seed(c["seed"])
    cfg = CLIPConfig(text_config=dict(c["text"], hidden_act="quick_gelu"), vision_config=dict(c["vision"], hidden_act="quick_gelu"),
                     projection_dim=c["proj"])
    m = CLIPModel(cfg).eval()
    g = torch.Generator().manual_seed(c["seed"] + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif "norm" in k and k.endswith(".weight"):
                p.copy_(1 + torch.randn(p.shape, generator=g) * 0.1)
            elif "embedding" in k:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5))
            p.copy_(p.to(torch.bfloat16).float())
    frames = frames_for(c["frame_hw"], c["seed"])
    S = c["vision"]["image_size"]
    proc = CLIPImageProcessorPil(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
    pv = proc(images=[f.numpy() for f in frames], return_tensors="pt")["pixel_values"]
    ids, mask = torch.tensor(c["ids"]), torch.tensor(c["mask"])
    with torch.no_grad():
        o = m(input_ids=ids, attention_mask=mask, pixel_values=pv, output_hidden_states=True)
        ie, te = m.get_image_features(pixel_values=pv), m.get_text_features(input_ids=ids, attention_mask=mask)
    ie = getattr(ie, "pooler_output", ie)
    te = getattr(te, "pooler_output", te)
    for k, v in m.state_dict().items():
        out[f"{tag}.w.{k}"] = v.to(torch.bfloat16) if v.is_floating_point() and v.dim() > 0 else v
    out[f"{tag}.frames"], out[f"{tag}.pixel_values"] = frames, pv
    out[f"{tag}.input_ids"], out[f"{tag}.attention_mask"] = ids, mask
    out[f"{tag}.image_embeds"], out[f"{tag}.text_embeds"], out[f"{tag}.logits_per_image"] = ie, te, o.logits_per_image
    for i, h in enumerate(o.vision_model_output.hidden_states):
        out[f"{tag}.vision_hidden.{i}"] = h
    for i, h in enumerate(o.text_model_output.hidden_states):
        out[f"{tag}.text_hidden.{i}"] = h
    out[f"{tag}.meta"] = torch.tensor([c["vision"]["num_attention_heads"], c["text"]["num_attention_heads"], c["text"]["eos_token_id"], S,
                                       c["vision"]["patch_size"]])


if __name__ == "__main__":
    out = {}
    for tag, c in CONFIGS.items():
        make(tag, c, out)
    path = HERE / "clip_tiny.safetensors"
    save_file({k: v.contiguous() for k, v in out.items()}, str(path))
    print(f"wrote {path} ({path.stat().st_size / 1024:.0f} KiB)")
