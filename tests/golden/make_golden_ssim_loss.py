"""Golden vectors for the photometric loss (csrc/ssim_loss.hip), produced by the reference's own SSIM
(third_party_model/anysplat/src/loss/loss_ssim.py::ssim, data_range=1.0, size_average=True) and torch's L1.

    python tests/golden/make_golden_ssim_loss.py   ->  tests/golden/ssim_loss_ref.safetensors

Cases, each [2,H,W,3] (the rasteriser's NHWC layout; the reference is fed the NCHW permutation):
  11x11   one map position per channel: every input pixel has exactly one contributor
  13x37   ragged, smaller than any tile
  45x70   several tiles with partial edges in both directions
and per shape two pairs: `smooth` (the smooth frame of make_golden_clip.py::frames_for plus noise, against the smooth frame) and
`noise` (two uniform-noise images).  Inputs are 8-bit like frames_for's and stored as uint8: both sides read float32(u8) / 255.
Per case <shape>.<pair>.:
  x, y                  uint8 inputs
  ssim64, l164          float64 values of the reference run in float64 (l1 = torch's mean |x - y|)
  g_ssim64              d ssim / dx of that run (float64, NHWC); the L1 gradient is sign(x - y) / numel and is not stored
  ssim32, l132, g_ssim32    the same from the reference run in float32 (its own rounding spread: the comparison figure)"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))

import torch
from safetensors.torch import save_file

SHAPES = ((11, 11), (13, 37), (45, 70))


def _ref_ssim():
    sys.path.insert(0, str(HERE))
    import _ref_import
    spec = importlib.util.spec_from_file_location("ref_loss_ssim", _ref_import.REF + "/third_party_model/anysplat/src/loss/loss_ssim.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.ssim


def pair_for(hw, kind, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    if kind == "noise":
        x, y = torch.rand(2, H, W, 3, generator=g, dtype=torch.float64), torch.rand(2, H, W, 3, generator=g, dtype=torch.float64)
    else:
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        y = torch.stack([torch.stack([0.5 + 0.4 * torch.sin(0.07 * (c + 1) * xx + 0.05 * yy + c + n) for c in range(3)], -1) for n in range(2)])
        x = (y + 0.1 * (torch.rand(2, H, W, 3, generator=g, dtype=torch.float64) - 0.5)).clamp(0, 1)
    return (x * 255).round().to(torch.uint8), (y * 255).round().to(torch.uint8)


def run(ssim, x, y, dt):
    out = {}
    for name, fn in (("ssim", lambda a, b: ssim(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), data_range=1.0, size_average=True)[0]),
                     ("l1", lambda a, b: (a - b).abs().mean())):
        a = x.to(dt).clone().requires_grad_(True)
        v = fn(a, y.to(dt))
        v.backward()
        out[name] = v.detach().reshape(1)
        out["g_" + name] = a.grad.contiguous()
    return out


def main():
    ssim = _ref_ssim()
    out = {}
    for i, hw in enumerate(SHAPES):
        for j, kind in enumerate(("smooth", "noise")):
            xu, yu = pair_for(hw, kind, 100 + 10 * i + j)
            p = f"{hw[0]}x{hw[1]}.{kind}."
            out[p + "x"], out[p + "y"] = xu.contiguous(), yu.contiguous()
            x, y = xu.float() / 255, yu.float() / 255
            r64, r32 = run(ssim, x, y, torch.float64), run(ssim, x, y, torch.float32)
            for k in ("ssim", "l1"):
                out[p + k + "64"], out[p + k + "32"] = r64[k], r32[k]
            out[p + "g_ssim64"], out[p + "g_ssim32"] = r64["g_ssim"], r32["g_ssim"]
            dv = abs(float(r32["ssim"]) - float(r64["ssim"]))
            dg = float((r32["g_ssim"].double() - r64["g_ssim"]).norm() / r64["g_ssim"].norm())
            print(f"{p} ssim {float(r64['ssim']):.6f}  fp32 vs fp64: value {dv:.2e}  grad rel {dg:.2e}")
    dst = HERE / "ssim_loss_ref.safetensors"
    save_file(out, str(dst))
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
