"""CPU restatement of the CLIP score (vist3a_amd.evaluation.clip) in plain torch, in float64 or float32: Hugging Face CLIPModel's
get_image_features / get_text_features (modeling_clip.py) on its state dict, the torchmetrics score, and the Pillow-path preprocessing.
Pinned to tests/golden/clip_tiny.safetensors (made by transformers.CLIPModel itself) in tests/test_clip_host.py."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def preprocess(frames_u8: np.ndarray, image_size: int) -> np.ndarray:
    """CLIPImageProcessor's Pillow path on uint8 [N,H,W,3] -> f32 [N,3,S,S] (PIL resize; the arithmetic of transformers' rescale and
    normalize restated)"""
    from PIL import Image
    out = []
    for f in frames_u8:
        H, W = f.shape[:2]
        short, long = (W, H) if W <= H else (H, W)
        ns, nl = image_size, int(image_size * long / short)
        oh, ow = (nl, ns) if W <= H else (ns, nl)
        r = np.asarray(Image.fromarray(f).resize((ow, oh), resample=Image.BICUBIC))
        top, left = (oh - image_size) // 2, (ow - image_size) // 2
        r = r[top: top + image_size, left: left + image_size]
        x = (r.astype(np.float64) * (1 / 255)).astype(np.float32)
        x = (x - np.array(CLIP_MEAN, dtype=np.float32)) / np.array(CLIP_STD, dtype=np.float32)
        out.append(x.transpose(2, 0, 1))
    return np.stack(out)


def _ln(x, sd, p, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _blocks(x, sd, prefix, heads, eps, mask):
    """x [B,S,d] -> list of hidden states (input first), pre-LN CLIPEncoderLayer with quick_gelu"""
    hidden = [x]
    B, S, d = x.shape
    hd = d // heads
    i = 0
    while f"{prefix}.encoder.layers.{i}.layer_norm1.weight" in sd:
        p = f"{prefix}.encoder.layers.{i}"
        h = _ln(x, sd, p + ".layer_norm1", eps)
        q, k, v = (F.linear(h, sd[f"{p}.self_attn.{n}_proj.weight"], sd[f"{p}.self_attn.{n}_proj.bias"]).view(B, S, heads, hd).transpose(1, 2)
                   for n in "qkv")
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        if mask is not None:
            s = s + mask
        a = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, S, d)
        x = x + F.linear(a, sd[p + ".self_attn.out_proj.weight"], sd[p + ".self_attn.out_proj.bias"])
        h = _ln(x, sd, p + ".layer_norm2", eps)
        u = F.linear(h, sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"])
        u = u * torch.sigmoid(1.702 * u)
        x = x + F.linear(u, sd[p + ".mlp.fc2.weight"], sd[p + ".mlp.fc2.bias"])
        hidden.append(x)
        i += 1
    return hidden


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def image_features(sd, pixel_values, heads, eps=1e-5, dtype=torch.float64):
    """-> (embeddings [N, proj], hidden states: after pre_layrnorm, then after every block)"""
    sd = cast(sd, dtype)
    x = torch.as_tensor(pixel_values).to(dtype)
    w = sd["vision_model.embeddings.patch_embedding.weight"]
    P = w.shape[-1]
    pe = F.conv2d(x, w, stride=P).flatten(2).transpose(1, 2)
    cls = sd["vision_model.embeddings.class_embedding"].expand(x.shape[0], 1, -1)
    x = torch.cat([cls, pe], 1) + sd["vision_model.embeddings.position_embedding.weight"]
    x = _ln(x, sd, "vision_model.pre_layrnorm", eps)
    hidden = _blocks(x, sd, "vision_model", heads, eps, None)
    pooled = _ln(hidden[-1][:, 0], sd, "vision_model.post_layernorm", eps)
    return F.linear(pooled, sd["visual_projection.weight"]), hidden


def text_features(sd, input_ids, attention_mask, heads, eos_token_id, eps=1e-5, dtype=torch.float64):
    sd = cast(sd, dtype)
    ids = torch.as_tensor(input_ids).long()
    ids = ids[:, : sd["text_model.embeddings.position_embedding.weight"].shape[0]]
    B, S = ids.shape
    x = sd["text_model.embeddings.token_embedding.weight"][ids] + sd["text_model.embeddings.position_embedding.weight"][:S]
    keep = torch.ones(S, S, dtype=torch.bool).tril()[None, None]
    if attention_mask is not None:
        keep = keep & (torch.as_tensor(attention_mask)[:, None, None, :S] != 0)
    mask = torch.zeros(keep.shape, dtype=dtype).masked_fill(~keep, float("-inf"))
    hidden = _blocks(x, sd, "text_model", heads, eps, mask)
    last = _ln(hidden[-1], sd, "text_model.final_layer_norm", eps)
    if eos_token_id == 2:
        pos = ids.argmax(-1)
    else:
        pos = (ids == eos_token_id).int().argmax(-1)
    pooled = last[torch.arange(B), pos]
    return F.linear(pooled, sd["text_projection.weight"]), hidden


def clip_scores(image_emb, text_emb):
    """torchmetrics CLIPScore per frame against one text embedding [D]: max(100 cos, 0), in the inputs' dtype"""
    i = image_emb / image_emb.norm(p=2, dim=-1, keepdim=True)
    t = text_emb / text_emb.norm(p=2, dim=-1, keepdim=True)
    return (100 * (i * t).sum(-1)).clamp(min=0)


def seeded_state_dict(vision: dict, text: dict, proj: int, seed: int):
    """a CLIPModel-shaped state dict without transformers: vision / text = dict(width, layers, inter, [patch, image | vocab, positions]);
    weights N(0, 1/fan_in)-scaled, LayerNorm weights 1 + 0.1 N, biases 0.05 N - full fp32 values"""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std
    sd = {}

    def tower(prefix, d, layers, inter):
        for i in range(layers):
            p = f"{prefix}.encoder.layers.{i}"
            for n in "qkv":
                sd[f"{p}.self_attn.{n}_proj.weight"] = rn(d, d, std=d ** -0.5)
                sd[f"{p}.self_attn.{n}_proj.bias"] = rn(d, std=0.05)
            sd[f"{p}.self_attn.out_proj.weight"] = rn(d, d, std=d ** -0.5)
            sd[f"{p}.self_attn.out_proj.bias"] = rn(d, std=0.05)
            for n in ("layer_norm1", "layer_norm2"):
                sd[f"{p}.{n}.weight"] = 1 + rn(d, std=0.1)
                sd[f"{p}.{n}.bias"] = rn(d, std=0.05)
            sd[f"{p}.mlp.fc1.weight"] = rn(inter, d, std=d ** -0.5)
            sd[f"{p}.mlp.fc1.bias"] = rn(inter, std=0.05)
            sd[f"{p}.mlp.fc2.weight"] = rn(d, inter, std=inter ** -0.5)
            sd[f"{p}.mlp.fc2.bias"] = rn(d, std=0.05)
    dv, P = vision["width"], vision["patch"]
    G = vision["image"] // P
    sd["vision_model.embeddings.class_embedding"] = rn(dv, std=0.5)
    sd["vision_model.embeddings.patch_embedding.weight"] = rn(dv, 3, P, P, std=(3 * P * P) ** -0.5)
    sd["vision_model.embeddings.position_embedding.weight"] = rn(G * G + 1, dv, std=0.3)
    for n in ("pre_layrnorm", "post_layernorm"):
        sd[f"vision_model.{n}.weight"] = 1 + rn(dv, std=0.1)
        sd[f"vision_model.{n}.bias"] = rn(dv, std=0.05)
    tower("vision_model", dv, vision["layers"], vision["inter"])
    dt = text["width"]
    sd["text_model.embeddings.token_embedding.weight"] = rn(text["vocab"], dt, std=0.5)
    sd["text_model.embeddings.position_embedding.weight"] = rn(text["positions"], dt, std=0.3)
    sd["text_model.final_layer_norm.weight"] = 1 + rn(dt, std=0.1)
    sd["text_model.final_layer_norm.bias"] = rn(dt, std=0.05)
    tower("text_model", dt, text["layers"], text["inter"])
    sd["visual_projection.weight"] = rn(proj, dv, std=dv ** -0.5)
    sd["text_projection.weight"] = rn(proj, dt, std=dt ** -0.5)
    sd["logit_scale"] = torch.tensor(2.6592)
    return sd
