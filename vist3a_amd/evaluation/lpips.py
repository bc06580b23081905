"""LPIPS (VGG) of the novel-view-synthesis evaluation on the MI355X: the reference's
third_party_model/anysplat/src/evaluation/metrics.py:22-34 (`compute_lpips`: lpips 0.1 `LPIPS(net="vgg")`, `normalize=True`).

The network reads two files every user of the reference already has - torchvision's VGG-16 state dict (`vgg16-397923af.pth`, or a
.safetensors of it) and the lpips package's `weights/v0.1/vgg.pth` - from paths the caller passes; no weights ship with this repository.

Per pair, on the device (csrc/lpips.hip, include/vist3a_hip.h: v3a_lpips_*):
  input transform (u8 / 255, 2 x - 1, ScalingLayer) -> VGG-16 `features` (13 fp32-equivalent split convolutions with ReLU, four exact
  2x2 max-pools on pairs) -> at relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 the head (channel-normalise, squared difference, learned
  1x1 weighting, spatial mean; fp64) -> the sum of the five layer means, f64.
Each layer's convolution form (halo tile or implicit GEMM, and the GEMM tile) depends on the layer's shape only, and the head's
reduction order on (h, w, C) only, so a pair's score is bit-identical whether it is scored alone or inside a batch."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional

import torch

from .. import lib as L
from .. import ops

# torchvision vgg16().features: the conv indices, stage by stage (a 2x2 max-pool precedes stages 2-5: features.4 / 9 / 16 / 23)
VGG_STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
VGG_CHANNELS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
                17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
LIN_CHANNELS = (64, 128, 256, 512, 512)   # lin0..lin4 of lpips' vgg.pth: relu1_2 .. relu5_3
MIN_SIZE = 16                             # the fifth stage (after four pools) must keep at least one pixel
# The form of each convolution is chosen as for a launch of this many frames (four pairs), whatever the launch really holds.
FORM_FRAMES = 8


def _read_state_dict(path) -> Dict[str, torch.Tensor]:
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"LPIPS weights: {path} does not exist")
    if path.suffix == ".safetensors":
        from safetensors.torch import load_file
        return load_file(str(path), device="cpu")
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def _take(sd: Dict[str, torch.Tensor], key: str, shape: tuple, path) -> torch.Tensor:
    if key not in sd:
        raise ValueError(f"{path}: missing key {key!r}")
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{path}: key {key!r} has shape {got}, expected {shape}")
    return t.float()


def _conv_tile(cw: ops.ConvWeightSplit, h: int, w: int) -> int:
    """v3a_conv_split's `tile` for this layer at an h x w feature map, from the shape alone: the halo-tile form where the layer has it
    and FORM_FRAMES frames would fill half the chip with it (the library's own rule), else an explicit implicit-GEMM tile - the one
    the library's rule picks for FORM_FRAMES frames (small tiles where big ones cannot fill the chip, 256 x 128 otherwise)."""
    if cw.w_halo is not None and h % 16 == 0 and w % 32 == 0:
        bn = L.load().v3a_conv_split_halo_bn(cw.CoutP)
        if FORM_FRAMES * (h // 16) * (w // 32) * (cw.CoutP // bn) >= 128:
            return -2
    M, N = FORM_FRAMES * h * w, cw.CoutP
    if ((M + 255) // 256) * ((N + 255) // 256) < 128:
        return 11 if (M <= 4096 and N <= 256) else 9
    return 10 if N <= 64 else 4


class LPIPSWeights:
    """The 13 VGG-16 convolutions packed as ops.ConvWeightSplit (conv1_1's 3 input channels padded to `cin_pad`: 16 lets it take the
    halo-tile form, 8 is ConvWeightSplit's own padding) and the five f32 lin vectors."""

    def __init__(self, convs: List[ops.ConvWeightSplit], lins: List[torch.Tensor], cin_pad: int):
        self.convs, self.lins, self.cin_pad = convs, lins, cin_pad

    @classmethod
    def from_state_dicts(cls, vgg: Dict[str, torch.Tensor], lin: Dict[str, torch.Tensor], device="cuda", cin_pad: int = 16,
                         vgg_name="vgg", lin_name="lin") -> "LPIPSWeights":
        if cin_pad not in (8, 16):
            raise ValueError("cin_pad must be 8 or 16")
        convs = []
        for i, (ci, co) in VGG_CHANNELS.items():
            wt = _take(vgg, f"features.{i}.weight", (co, ci, 3, 3), vgg_name)
            b = _take(vgg, f"features.{i}.bias", (co,), vgg_name)
            if i == 0 and cin_pad == 16:
                wt = torch.cat([wt, wt.new_zeros(co, 13, 3, 3)], 1)
            convs.append(ops.ConvWeightSplit(wt, b, device=device))
        lins = [_take(lin, f"lin{k}.model.1.weight", (1, c, 1, 1), lin_name).reshape(c).contiguous().to(device)
                for k, c in enumerate(LIN_CHANNELS)]
        return cls(convs, lins, cin_pad)

    @classmethod
    def load(cls, vgg_path, lin_path, device="cuda", cin_pad: int = 16) -> "LPIPSWeights":
        """vgg_path: torchvision's VGG-16 state dict (.pth or .safetensors; `features.N.weight/bias`, `classifier.*` ignored);
        lin_path: lpips' weights/v0.1/vgg.pth (`lin0..lin4.model.1.weight`).  ValueError naming the key for a missing or misshaped one."""
        return cls.from_state_dicts(_read_state_dict(vgg_path), _read_state_dict(lin_path), device, cin_pad,
                                    vgg_name=str(vgg_path), lin_name=str(lin_path))


class LPIPS:
    """LPIPS(net="vgg", version="0.1") of image pairs; `__call__(pred, gt)` -> f64 [N] on the device.

    pred / gt: uint8 [N,H,W,3] (PNG bytes) or f32 [N,3,H,W] in [0,1] (what ToTensor gives), H, W >= 16; host tensors are copied to the
    weights' device.  Pairs are scored in chunks whose activations stay under `max_bytes` (at least one pair per chunk)."""

    def __init__(self, weights: LPIPSWeights, max_bytes: int = 2 << 30):
        self.w = weights
        self.max_bytes = max_bytes
        self.device = weights.lins[0].device

    @staticmethod
    def pair_bytes(H: int, W: int) -> int:
        """device bytes one pair needs at the widest layer: the 64-channel pair of both images, in and out of a convolution, plus the
        next layer's output (conservative)"""
        return 3 * 2 * 2 * H * W * 64 * 2

    def _check(self, pred: torch.Tensor, gt: torch.Tensor):
        if pred.dtype != gt.dtype or pred.shape != gt.shape:
            raise ValueError(f"pred and gt differ: {pred.dtype} {tuple(pred.shape)} vs {gt.dtype} {tuple(gt.shape)}")
        if pred.dim() != 4:
            raise ValueError(f"images must be 4-D, got shape {tuple(pred.shape)}")
        if pred.dtype == torch.uint8:
            N, H, W, Cc = pred.shape
        elif pred.dtype == torch.float32:
            N, Cc, H, W = pred.shape
        else:
            raise ValueError(f"images must be uint8 [N,H,W,3] or float32 [N,3,H,W], got {pred.dtype}")
        if Cc != 3:
            raise ValueError(f"LPIPS(VGG) takes 3-channel RGB images, got {Cc} channels")
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS(VGG) needs images of at least {MIN_SIZE}x{MIN_SIZE}, got {H}x{W}")
        return N, H, W

    def __call__(self, pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        N, H, W = self._check(pred, gt)
        pred = pred.to(self.device).contiguous()
        gt = gt.to(self.device).contiguous()
        out = torch.empty(N, device=self.device, dtype=torch.float64)
        step = max(1, self.max_bytes // self.pair_bytes(H, W))
        for s in range(0, N, step):
            self.forward_chunk(pred[s: s + step], gt[s: s + step], out[s: s + step])
        return out

    def forward_chunk(self, pred: torch.Tensor, gt: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """one launch sequence over all pairs of the chunk: out f64 [n] (a contiguous slice) = LPIPS"""
        x = ops.lpips_input(pred.contiguous(), gt.contiguous(), self.w.cin_pad)
        k = 0
        for s, idx in enumerate(VGG_STAGES):
            if s > 0:
                x = ops.lpips_pool(x)
            for _ in idx:
                cw = self.w.convs[k]
                k += 1
                x = ops.conv_split(x, cw, pad=(0, 1, 1), act=L.ACT_RELU, tile=_conv_tile(cw, x.shape[2], x.shape[3]))
            ops.lpips_head(x, self.w.lins[s], out, accumulate=s > 0)
        return out


_cache: Dict[tuple, LPIPS] = {}
_default_paths: Optional[tuple] = None


def configure(vgg_path, lin_path) -> None:
    """the weight files compute_lpips uses when it is not given any"""
    global _default_paths
    _default_paths = (vgg_path, lin_path)


def get_lpips(vgg_path, lin_path, device="cuda") -> LPIPS:
    """one LPIPS per (files, device), like the reference's @cache get_lpips"""
    key = (str(vgg_path), str(lin_path), str(device))
    if key not in _cache:
        _cache[key] = LPIPS(LPIPSWeights.load(vgg_path, lin_path, device))
    return _cache[key]


def compute_lpips(ground_truth: torch.Tensor, predicted: torch.Tensor, *, vgg_path=None, lin_path=None) -> torch.Tensor:
    """metrics.py:28-34: f32 [B,3,H,W] pairs in [0,1] -> f64 [B] (`value[:, 0, 0, 0]`), on the device of `predicted` (the GPU when it
    is a host tensor).  The weight files come from the keyword arguments or from `configure` (the reference's lpips package finds its
    own)."""
    if vgg_path is None or lin_path is None:
        if _default_paths is None:
            raise ValueError("compute_lpips needs the VGG-16 and lpips lin weight files: pass vgg_path / lin_path or call configure()")
        vgg_path, lin_path = _default_paths
    dev = predicted.device if predicted.is_cuda else torch.device("cuda")
    return get_lpips(vgg_path, lin_path, dev)(ground_truth.float(), predicted.float())
