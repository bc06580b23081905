"""CLIP score of the generated-scene evaluation on the MI355X: the reference's evaluation/gen_eval/t3_scene_evaluation.py:97-120
(`clip_score`: torchmetrics `CLIPScore("openai/clip-vit-base-patch16")`, `longclip_score`: the same with `zer0int/LongCLIP-L-Diffusers`)
called per frame by evaluation/gen_eval/gen_metrics/clip_score.py:18-29.  Both checkpoints are the Hugging Face `CLIPModel` architecture.

Metric (what the reference computes):
  frames    8 frames of `gs.*` at indices int(i * total_frames / 8), i = 0..7, RGB uint8 [H,W,3] (t3_scene_evaluation.py:28-47).
  pixels    CLIPImageProcessor, Pillow path: resize so that the shorter edge is `image_size` (long edge int(image_size * long / short)),
            Pillow BICUBIC (antialiased, 8-bit, horizontal then vertical pass, each rounded and clipped to uint8), centre crop to
            image_size^2, x * (1/255), (x - mean) / std in fp32.
  image     CLIPModel.get_image_features: patch convolution (no bias), class token + position embeddings, pre_layrnorm, pre-LN blocks
            (q/k/v/out with bias, scale hd^-0.5, MLP with quick_gelu = x sigmoid(1.702 x)), post_layernorm on the class token,
            visual_projection.
  text      CLIPModel.get_text_features: token + position embeddings, the same blocks under a causal mask, final_layer_norm, the row of
            the EOS token (CLIPTextTransformer's rule: argmax(input_ids) when eos_token_id == 2, else the first position of eos_token_id),
            text_projection.  Prompts longer than max_position_embeddings are cut to it (torchmetrics).
  score     per frame max(100 cos(image, text), 0); per prompt the mean over its frames; `all_average` the mean over prompts.

On the device (csrc/clip.hip, include/vist3a_hip.h): v3a_clip_preprocess (integer Pillow resize from host-built fixed-point tables, crop,
table normalise, patch matrix as a bf16 pair) -> the towers: every linear layer is v3a_conv_split as a 1x1 convolution (split bf16:
operands carried as (hi, lo) pairs of 16 significand bits, fp32 accumulation - about 5e-6 per block against fp64, ten times fp32's own
error, no 8-bit bf16 rounding anywhere; fc1 with the QUICK_GELU epilogue; out / fc2 with the f32 residual), LayerNorms v3a_layernorm /
v3a_layernorm_pair, attention v3a_attention_f32 (fp32, causal + valid length for text; only the tokens up to the last EOS of the batch
are computed) -> v3a_clip_score
(fp64).  No weights ship with this repository: `ClipWeights.from_pretrained` reads a local Hugging Face folder; tokenisation is the
caller's (the CLI builds transformers.CLIPTokenizerFast from the same folder)."""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import lib as L
from .. import ops

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22          # Pillow Resample.c: 32 - 8 - 2
UNUSED_KEYS = ("vision_model.embeddings.position_ids", "text_model.embeddings.position_ids", "logit_scale")
HEAD_DIM = 64
# transformers' CLIPTextConfig / CLIPVisionConfig defaults, for the fields a saved config.json leaves out
TEXT_DEFAULTS = dict(num_attention_heads=8, layer_norm_eps=1e-5, hidden_act="quick_gelu", eos_token_id=49407)
VISION_DEFAULTS = dict(num_attention_heads=12, layer_norm_eps=1e-5, hidden_act="quick_gelu", image_size=224, patch_size=32)


# ------------------------------------------------------------------------------------------------ host: Pillow's coefficient tables
def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pillow_bicubic_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) for BICUBIC over the whole axis, in float64 with
    the same operation order -> (bounds int32 [out, 2] = first input sample and tap count, coefficients int32 [out, ksize], fixed point
    with 22 fractional bits, rounded half away from zero)."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ws = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        for x, w in enumerate(ws):
            if ww != 0.0:
                w = w / ww
            kk[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def resize_geometry(H: int, W: int, image_size: int) -> Tuple[int, int, int, int]:
    """CLIPImageProcessor's shorter-edge resize and centre crop: -> (resized height, resized width, crop top, crop left)"""
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = image_size, int(image_size * long / short)
    oh, ow = (new_long, new_short) if W <= H else (new_short, new_long)
    return oh, ow, (oh - image_size) // 2, (ow - image_size) // 2


def resize_tables_host(H: int, W: int, image_size: int) -> dict:
    """the tables v3a_clip_preprocess reads, for the crop's columns and rows only (numpy), and the input rows the vertical taps touch"""
    oh, ow, top, left = resize_geometry(H, W, image_size)
    xb, xk = pillow_bicubic_coeffs(W, ow)
    yb, yk = pillow_bicubic_coeffs(H, oh)
    xb, xk = xb[left: left + image_size], xk[left: left + image_size]
    yb, yk = yb[top: top + image_size], yk[top: top + image_size]
    row0 = int(yb[:, 0].min())
    rows = int((yb[:, 0] + yb[:, 1]).max()) - row0
    assert (xb[:, 0] >= 0).all() and (xb[:, 0] + xb[:, 1] <= W).all() and row0 >= 0 and row0 + rows <= H
    return dict(x_bounds=np.ascontiguousarray(xb), x_coeffs=np.ascontiguousarray(xk), y_bounds=np.ascontiguousarray(yb),
                y_coeffs=np.ascontiguousarray(yk), row0=row0, rows=rows, size=(H, W, image_size))


def resample_numpy(img: np.ndarray, bounds_x, kx, bounds_y, ky) -> np.ndarray:
    """the integer resampler the kernel implements, in numpy (tests; uint8 [H,W,C] -> uint8 [len(bounds_y), len(bounds_x), C])"""
    def one_pass(a, bounds, kk):   # along axis 1
        out = np.empty((a.shape[0], len(bounds), a.shape[2]), np.uint8)
        a = a.astype(np.int64)
        for i, (lo, n) in enumerate(bounds):
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(a[:, lo: lo + n], kk[i, :n].astype(np.int64), axes=([1], [0]))
            out[:, i] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return out
    h = one_pass(img, bounds_x, kx)
    return one_pass(h.transpose(1, 0, 2), bounds_y, ky).transpose(1, 0, 2)


def normalize_lut(mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """f32 [3,256]: transformers' rescale (float64 product with 1/255, cast to fp32) and normalize ((x - mean) / std in fp32) of every
    uint8 value"""
    r = (np.arange(256, dtype=np.uint8).astype(np.float64) * (1 / 255)).astype(np.float32)
    m, s = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32)
    return np.ascontiguousarray(((r[:, None] - m) / s).T.astype(np.float32))


# ------------------------------------------------------------------------------------------------ weights
def _read_folder(folder) -> Tuple[dict, Dict[str, torch.Tensor]]:
    folder = Path(folder)
    if not folder.is_dir():
        raise FileNotFoundError(f"CLIP model folder {folder} does not exist")
    cfg_path = folder / "config.json"
    if not cfg_path.exists():
        raise FileNotFoundError(f"{folder}: no config.json (expected a local Hugging Face CLIPModel folder)")
    cfg = json.loads(cfg_path.read_text())
    if (folder / "model.safetensors").exists():
        from safetensors.torch import load_file
        sd = load_file(str(folder / "model.safetensors"), device="cpu")
    elif (folder / "pytorch_model.bin").exists():
        sd = torch.load(str(folder / "pytorch_model.bin"), map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{folder}: neither model.safetensors nor pytorch_model.bin")
    pp = folder / "preprocessor_config.json"
    if pp.exists():
        cfg["_preprocessor"] = json.loads(pp.read_text())
    return cfg, sd


class _Taker:
    def __init__(self, sd: Dict[str, torch.Tensor], name: str):
        self.sd, self.name, self.used = sd, name, set()

    def __call__(self, key: str, shape: Optional[tuple] = None) -> torch.Tensor:
        if key not in self.sd:
            raise ValueError(f"{self.name}: missing key {key!r}")
        t = self.sd[key]
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{self.name}: key {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        self.used.add(key)
        return t.detach().float()


class TowerWeights:
    """one transformer stack: per layer the fused q|k|v, out, fc1, fc2 as ops.ConvWeightSplit and the two LayerNorms (f32)"""

    def __init__(self, take: _Taker, prefix: str, d: int, heads: int, eps: float, act: str, device):
        if act != "quick_gelu":
            raise ValueError(f"{take.name}: hidden_act {act!r} is not supported (CLIP's quick_gelu only)")
        if d != heads * HEAD_DIM:
            raise ValueError(f"{take.name}: {prefix} has head size {d / heads:g}; only {HEAD_DIM} is supported")
        self.d, self.heads, self.eps = d, heads, eps
        self.layers: List[dict] = []
        i = 0
        while f"{prefix}.encoder.layers.{i}.layer_norm1.weight" in take.sd:
            p = f"{prefix}.encoder.layers.{i}"
            qkv_w = torch.cat([take(f"{p}.self_attn.{n}_proj.weight", (d, d)) for n in "qkv"], 0)
            qkv_b = torch.cat([take(f"{p}.self_attn.{n}_proj.bias", (d,)) for n in "qkv"], 0)
            inter = take.sd[f"{p}.mlp.fc1.weight"].shape[0]
            self.layers.append(dict(
                ln1=(take(f"{p}.layer_norm1.weight", (d,)).to(device), take(f"{p}.layer_norm1.bias", (d,)).to(device)),
                ln2=(take(f"{p}.layer_norm2.weight", (d,)).to(device), take(f"{p}.layer_norm2.bias", (d,)).to(device)),
                qkv=ops.ConvWeightSplit(qkv_w[:, :, None, None], qkv_b, device=device),
                out=ops.ConvWeightSplit(take(f"{p}.self_attn.out_proj.weight", (d, d))[:, :, None, None],
                                        take(f"{p}.self_attn.out_proj.bias", (d,)), device=device),
                fc1=ops.ConvWeightSplit(take(f"{p}.mlp.fc1.weight", (inter, d))[:, :, None, None], take(f"{p}.mlp.fc1.bias", (inter,)),
                                        device=device),
                fc2=ops.ConvWeightSplit(take(f"{p}.mlp.fc2.weight", (d, inter))[:, :, None, None], take(f"{p}.mlp.fc2.bias", (d,)),
                                        device=device),
            ))
            i += 1
        if not self.layers:
            raise ValueError(f"{take.name}: no {prefix}.encoder.layers.*")


class ClipWeights:
    """A Hugging Face CLIPModel packed for the HIP path.  `unused` lists the state-dict keys that were not consumed (all of them must be
    in UNUSED_KEYS, else from_state_dict raises)."""

    @classmethod
    def from_pretrained(cls, folder, device="cuda") -> "ClipWeights":
        cfg, sd = _read_folder(folder)
        return cls.from_state_dict(cfg, sd, device=device, name=str(folder))

    @classmethod
    def from_state_dict(cls, config: dict, sd: Dict[str, torch.Tensor], device="cuda", name="CLIP") -> "ClipWeights":
        self = cls()
        tc = {**TEXT_DEFAULTS, **(config.get("text_config") or {})}
        vc = {**VISION_DEFAULTS, **(config.get("vision_config") or {})}
        take = _Taker(sd, name)
        # vision
        pw = take("vision_model.embeddings.patch_embedding.weight")
        dv, _, P, _ = pw.shape
        if tuple(pw.shape) != (dv, 3, P, P):
            raise ValueError(f"{name}: patch embedding has shape {tuple(pw.shape)}")
        self.patch, self.vision_width = P, dv
        pos = take("vision_model.embeddings.position_embedding.weight")
        G = int(round(math.sqrt(pos.shape[0] - 1)))
        if G * G + 1 != pos.shape[0] or tuple(pos.shape) != (G * G + 1, dv):
            raise ValueError(f"{name}: vision position embedding has shape {tuple(pos.shape)}")
        self.image_size, self.grid = G * P, G
        for key, have in (("image_size", self.image_size), ("patch_size", P)):   # only what config.json itself states
            said = (config.get("vision_config") or {}).get(key)
            if said is not None and int(said) != have:
                raise ValueError(f"{name}: vision_config.{key} = {said} disagrees with the weights ({have})")
        self.patch_w = ops.ConvWeightSplit(pw.reshape(dv, 3 * P * P)[:, :, None, None], None, device=device)
        self.vision_pos = pos.contiguous().to(device)
        self.cls = take("vision_model.embeddings.class_embedding", (dv,)).contiguous().to(device)
        self.pre_ln = tuple(take(f"vision_model.pre_layrnorm.{n}", (dv,)).to(device) for n in ("weight", "bias"))
        self.post_ln = tuple(take(f"vision_model.post_layernorm.{n}", (dv,)).to(device) for n in ("weight", "bias"))
        self.vision = TowerWeights(take, "vision_model", dv, int(vc["num_attention_heads"]), float(vc["layer_norm_eps"]), vc["hidden_act"],
                                   device)
        vp = take("visual_projection.weight")
        self.proj_dim = vp.shape[0]
        self.visual_projection = ops.ConvWeightSplit(vp[:, :, None, None], None, device=device)
        # text
        tok = take("text_model.embeddings.token_embedding.weight")
        self.vocab, dt = tok.shape
        self.text_width = dt
        self.tok = tok.contiguous().to(device)
        tpos = take("text_model.embeddings.position_embedding.weight")
        self.max_positions = tpos.shape[0]
        self.text_pos = tpos.contiguous().to(device)
        self.final_ln = tuple(take(f"text_model.final_layer_norm.{n}", (dt,)).to(device) for n in ("weight", "bias"))
        self.text = TowerWeights(take, "text_model", dt, int(tc["num_attention_heads"]), float(tc["layer_norm_eps"]), tc["hidden_act"], device)
        self.text_projection = ops.ConvWeightSplit(take("text_projection.weight", (self.proj_dim, dt))[:, :, None, None], None, device=device)
        self.eos_token_id = int(tc["eos_token_id"])
        self.unused = sorted(set(sd) - take.used)
        extra = [k for k in self.unused if k not in UNUSED_KEYS]
        if extra:
            raise ValueError(f"{name}: state-dict keys this CLIPModel implementation does not know: {extra[:8]}")
        pre = config.get("_preprocessor") or {}
        self.mean = tuple(pre.get("image_mean", CLIP_MEAN))
        self.std = tuple(pre.get("image_std", CLIP_STD))
        self.lut = torch.from_numpy(normalize_lut(self.mean, self.std)).to(device)
        self.device = torch.device(device)
        return self


def eos_positions(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """CLIPTextTransformer's pooling row per prompt (modeling_clip.py): argmax(input_ids) when eos_token_id == 2 (the openai checkpoints'
    config), else the first position of eos_token_id (0 when it is absent, as argmax of an all-zero row)"""
    ids = input_ids.to(torch.int64)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


# ------------------------------------------------------------------------------------------------ the scorer
class ClipScorer:
    """encode_images(uint8 frames [N,H,W,3]) -> f32 [N, proj]; encode_text(input_ids [B,L], attention_mask) -> f32 [B, proj];
    score(frames, input_ids, attention_mask) -> f64 [F] per-frame CLIP scores of ONE prompt (its mean: `prompt_score`)."""

    def __init__(self, weights: ClipWeights, max_frames: int = 64):
        self.w = weights
        self.device = weights.device
        self.max_frames = max_frames
        self._tables: Dict[tuple, dict] = {}

    # -- pieces
    def tables(self, H: int, W: int) -> dict:
        key = (H, W)
        if key not in self._tables:
            t = resize_tables_host(H, W, self.w.image_size)
            self._tables[key] = {k: (torch.from_numpy(v).to(self.device) if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        return self._tables[key]

    def preprocess(self, frames: torch.Tensor, want_u8: bool = False, want_f32: bool = False):
        if frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[-1] != 3:
            raise ValueError(f"frames must be uint8 [N,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
        frames = frames.to(self.device).contiguous()
        return ops.clip_preprocess(frames, self.tables(frames.shape[1], frames.shape[2]), self.w.lut, self.w.image_size, self.w.patch,
                                   want_u8=want_u8, want_f32=want_f32)

    @staticmethod
    def _linear(x: torch.Tensor, cw: ops.ConvWeightSplit, **kw) -> torch.Tensor:
        """x pair [2, M, Cin] -> f32 [M, Cout] (out_f32) or pair [2, M, Cout]"""
        M = x.shape[1]
        res = kw.pop("residual", None)
        y = ops.conv_split(x.view(2, 1, 1, M, x.shape[2]), cw, residual=None if res is None else res.view(1, 1, M, -1), **kw)
        return y.view(M, cw.CoutP) if kw.get("out_f32") else y.view(2, M, cw.CoutP)

    def block(self, x: torch.Tensor, lw: dict, tw: TowerWeights, B: int, S: int, causal: bool, lens: Optional[torch.Tensor]) -> torch.Tensor:
        """one pre-LN CLIPEncoderLayer on the f32 residual stream x [B S, d]"""
        d = tw.d
        h = ops.layernorm_pair(x, weight=lw["ln1"][0], bias=lw["ln1"][1], eps=tw.eps)
        qkv = self._linear(h, lw["qkv"], out_f32=True)
        a = ops.attention_f32(qkv[:, :d], qkv[:, d: 2 * d], qkv[:, 2 * d:], B=B, S=S, H=tw.heads, causal=causal, lens=lens)
        x = self._linear(a, lw["out"], residual=x, out_f32=True)
        h = ops.layernorm_pair(x, weight=lw["ln2"][0], bias=lw["ln2"][1], eps=tw.eps)
        u = self._linear(h, lw["fc1"], act=L.ACT_QUICK_GELU)
        return self._linear(u, lw["fc2"], residual=x, out_f32=True)

    # -- towers
    def encode_images(self, frames: torch.Tensor, return_hidden: bool = False):
        outs, hidden = [], None
        for s in range(0, frames.shape[0], self.max_frames):
            e, h = self._encode_images(frames[s: s + self.max_frames], return_hidden)
            outs.append(e)
            hidden = h if hidden is None else [torch.cat([a, b], 0) for a, b in zip(hidden, h)]
        e = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
        return (e, hidden) if return_hidden else e

    def _encode_images(self, frames: torch.Tensor, return_hidden: bool):
        patches, _, _ = self.preprocess(frames)
        return self.encode_patches(patches, frames.shape[0], return_hidden)

    def encode_patches(self, patches: torch.Tensor, N: int, return_hidden: bool = False):
        """patch pair [2, N G^2, ldk] (v3a_clip_preprocess's output) -> image embeddings"""
        w = self.w
        S = w.grid * w.grid + 1
        pe = self._linear(patches, w.patch_w, out_f32=True)                       # [N G^2, d]
        x = ops.clip_rows(pe, cls=w.cls, pos=w.vision_pos, S=S)                   # [N S, d]
        x = ops.layernorm(x, weight=w.pre_ln[0], bias=w.pre_ln[1], eps=w.vision.eps, out_dtype=torch.float32)
        hidden = [x.view(N, S, -1)] if return_hidden else None
        for lw in w.vision.layers:
            x = self.block(x, lw, w.vision, N, S, False, None)
            if return_hidden:
                hidden.append(x.view(N, S, -1))
        pooled = ops.layernorm_pair(x, weight=w.post_ln[0], bias=w.post_ln[1], eps=w.vision.eps, M=N, in_rows=(1, S - 1, 0))
        return self._linear(pooled, w.visual_projection, out_f32=True)[:, : w.proj_dim], hidden

    def encode_text(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, return_hidden: bool = False):
        """input_ids int [B, L] (or [L]); attention_mask [B, L] of ones followed by zeros, or None.  hidden states cover the first
        max(EOS position) + 1 tokens only - the causal mask makes the rest irrelevant to the embedding."""
        w = self.w
        ids = input_ids.detach().cpu().to(torch.int64)
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.shape[1] < 1:
            raise ValueError(f"input_ids must be [B, L], got {tuple(ids.shape)}")
        ids = ids[:, : w.max_positions]                                           # torchmetrics: cut to max_position_embeddings
        if ids.min() < 0 or ids.max() >= w.vocab:
            raise ValueError(f"input_ids outside the vocabulary [0, {w.vocab})")
        B = ids.shape[0]
        eos = eos_positions(ids, w.eos_token_id)
        S = int(eos.max()) + 1
        lens = None
        if attention_mask is not None:
            m = attention_mask.detach().cpu().to(torch.int64)
            if m.dim() == 1:
                m = m[None]
            m = m[:, : w.max_positions]
            if m.shape != ids.shape:
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_ids {tuple(input_ids.shape)}")
            n = m.sum(1)
            if ((m != 0) != (torch.arange(m.shape[1])[None] < n[:, None])).any() or (n < 1).any():
                raise ValueError("attention_mask must be ones followed by zeros (right padding), with at least one token")
            lens = n.clamp(max=S).to(torch.int32).to(self.device)
        idd = ids[:, :S].contiguous().to(torch.int32).to(self.device).view(-1)
        x = ops.clip_rows(w.tok, ids=idd, pos=w.text_pos, S=S)                    # [B S, d]
        hidden = [x.view(B, S, -1)] if return_hidden else None
        for lw in w.text.layers:
            x = self.block(x, lw, w.text, B, S, True, lens)
            if return_hidden:
                hidden.append(x.view(B, S, -1))
        rows = (torch.arange(B) * S + eos).to(torch.int32).to(self.device)
        pooled = ops.layernorm_pair(ops.clip_rows(x, ids=rows), weight=w.final_ln[0], bias=w.final_ln[1], eps=w.text.eps)
        e = self._linear(pooled, w.text_projection, out_f32=True)[:, : w.proj_dim]
        return (e, hidden) if return_hidden else e

    # -- score
    def _score(self, frames, input_ids, attention_mask):
        ids = input_ids if input_ids.dim() == 2 else input_ids[None]
        if ids.shape[0] != 1:
            raise ValueError("score() takes one prompt; call it per prompt")
        img = self.encode_images(frames).contiguous()
        txt = self.encode_text(ids, attention_mask).contiguous()
        return ops.clip_score(img, txt[0].contiguous())

    def score(self, frames: torch.Tensor, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._score(frames, input_ids, attention_mask)[0]

    def prompt_score(self, frames: torch.Tensor, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> float:
        """the mean of the per-frame scores, summed in frame order on the device"""
        return float(self._score(frames, input_ids, attention_mask)[1].item())
