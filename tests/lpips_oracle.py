"""CPU restatement of LPIPS(VGG) in float64, for the `evaluation.lpips` tests.

The algorithm of lpips 0.1.x (`lpips.LPIPS(net="vgg", version="0.1")`, `forward(in0, in1, normalize=True)`), as the reference calls it in
third_party_model/anysplat/src/evaluation/metrics.py:22-34:
  1. in = 2 * in - 1 (normalize=True), then ScalingLayer: (in - shift) / scale, shift = [-.030, -.088, -.188], scale = [.458, .448, .450]
     (fp32 tensors).  Pixels are u8 / 255 in float32, as ToTensor makes them of a PNG.
  2. torchvision's vgg16().features, split at relu1_2 / relu2_2 / relu3_3 / relu4_3 / relu5_3 (slices [0:4], [4:9], [9:16], [16:23],
     [23:30]: 3x3 convolutions with padding 1 and ReLU, 2x2 / stride-2 max-pools at features.4 / 9 / 16 / 23).
  3. per tapped layer: normalize_tensor (f / (sqrt(sum_c f^2) + 1e-10)), squared difference, NetLinLayer (1x1 conv lin{l}.model.1,
     no bias), spatial_average (mean over H, W).
  4. the sum of the five layer values.
Step 1 is kept in float32 with torch's rounding points (the GPU reproduces them exactly); steps 2-4 run in float64.  The lpips package
and torchvision are not installed here, so this restatement is written from the package's algorithm and cannot be pinned against the
package itself."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHANNELS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
            17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
LIN = (64, 128, 256, 512, 512)


def make_weights(seed: int = 0, classifier: bool = True):
    """seeded state dicts in torchvision's vgg16 and lpips' vgg.pth key layouts: He-scaled convolutions, small biases, non-negative
    lin weights (lpips clamps its own to >= 0); a dummy classifier.* tensor stands in for the part LPIPS ignores"""
    g = torch.Generator().manual_seed(seed)
    vgg: Dict[str, torch.Tensor] = {}
    for i, (ci, co) in CHANNELS.items():
        vgg[f"features.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        vgg[f"features.{i}.bias"] = torch.randn(co, generator=g) * 0.01
    if classifier:
        vgg["classifier.0.weight"] = torch.randn(8, 16, generator=g)
        vgg["classifier.0.bias"] = torch.zeros(8)
    lin = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) * (8.0 / c) for k, c in enumerate(LIN)}
    return vgg, lin


def to_input(img: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H,W,3] or f32 [N,3,H,W] in [0,1] -> the scaled f32 network input [N,3,H,W] (step 1, float32)"""
    x = img.permute(0, 3, 1, 2).float() / 255 if img.dtype == torch.uint8 else img.float()
    x = 2 * x - 1
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=torch.float32).view(1, 3, 1, 1)
    return (x - shift) / scale


def features(vgg: Dict[str, torch.Tensor], x: torch.Tensor):
    """the five tapped ReLU outputs in float64"""
    h = x.double()
    out = []
    for s, idx in enumerate(STAGES):
        if s > 0:
            h = F.max_pool2d(h, 2, 2)
        for i in idx:
            h = F.relu(F.conv2d(h, vgg[f"features.{i}.weight"].double(), vgg[f"features.{i}.bias"].double(), padding=1))
        out.append(h)
    return out


def layer_values(vgg, lin, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
    """[5, N] float64: the spatial mean of each tapped layer's weighted squared difference"""
    f0, f1 = features(vgg, to_input(in0)), features(vgg, to_input(in1))
    vals = []
    for k, (a, b) in enumerate(zip(f0, f1)):
        na = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        w = lin[f"lin{k}.model.1.weight"].double()
        vals.append(((na - nb) ** 2 * w).sum(1).mean((1, 2)))
    return torch.stack(vals)


def lpips(vgg, lin, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
    """LPIPS of N pairs -> float64 [N]"""
    return layer_values(vgg, lin, in0, in1).sum(0)
