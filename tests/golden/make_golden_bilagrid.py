"""Golden vectors for the bilateral grid (csrc/bilagrid.hip, tests/bilagrid_oracle.py), produced by the reference's own module
(third_party_model/anysplat/src/post_opt/lib_bilagrid.py: slice, BilateralGrid, total_variation_loss), loaded by file path.

    python tests/golden/make_golden_bilagrid.py   ->  tests/golden/bilagrid_ref.safetensors

The module imports `tensorly` (not installed; only its CP-decomposed 4-D grid uses it): a stub whose set_backend does nothing goes
into sys.modules first.  Cases (bilagrid_oracle.GOLDEN_CASES): rgb [1,1,1] on (GX,GY,L) = (2,2,2), [1,5,7] on (4,3,5), [2,13,37] on
(5,3,4), inputs of bilagrid_oracle.make_inputs.  Per case <NxHxW>.:
  rgb, grids, d_out                    float32 inputs (grids in the reference layout [N,12,L,GY,GX]; d_out = the gradient fed to `rgb_out`)
  out64, d_rgb64, d_grids64            slice(...)["rgb"] and its gradients, the module run in float64
  tv64, d_tv64                         total_variation_loss(grids) and its gradient, float64
  out32, d_rgb32, d_grids32, tv32, d_tv32    the same from the module run in float32 (its own rounding spread: the comparison figure)"""
from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch
from safetensors.torch import save_file

import bilagrid_oracle as BO


def _ref_module():
    sys.path.insert(0, str(HERE))
    import _ref_import
    stub = types.ModuleType("tensorly")
    stub.set_backend = lambda *a, **k: None
    sys.modules.setdefault("tensorly", stub)
    spec = importlib.util.spec_from_file_location("ref_lib_bilagrid", _ref_import.REF + "/third_party_model/anysplat/src/post_opt/lib_bilagrid.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(m, rgb, grids, d_out, dt):
    N, H, W, _ = rgb.shape
    _, _, L, GY, GX = grids.shape
    bg = m.BilateralGrid(N, grid_X=GX, grid_Y=GY, grid_W=L).to(dt)
    with torch.no_grad():
        bg.grids.copy_(grids.to(dt))
    r = rgb.to(dt).requires_grad_(True)
    xy = BO.pixel_centres(H, W, dt).expand(N, H, W, 2).contiguous()
    idx = torch.arange(N)[:, None, None, None].expand(N, H, W, 1)
    out = m.slice(bg, xy, r, idx)["rgb"]
    d_rgb, d_grids = torch.autograd.grad(out, (r, bg.grids), d_out.to(dt))
    tv = m.total_variation_loss(bg.grids)
    d_tv, = torch.autograd.grad(tv, bg.grids)
    return dict(out=out.detach().contiguous(), d_rgb=d_rgb.contiguous(), d_grids=d_grids.contiguous(), tv=tv.detach().reshape(1),
                d_tv=d_tv.contiguous())


def main():
    m = _ref_module()
    out = {}
    for (N, H, W), (GX, GY, L) in BO.GOLDEN_CASES:
        rgb, grids, d_out = BO.make_inputs(N, H, W, GX, GY, L)
        p = f"{N}x{H}x{W}."
        out[p + "rgb"], out[p + "grids"], out[p + "d_out"] = rgb.contiguous(), grids.contiguous(), d_out.contiguous()
        r64, r32 = run(m, rgb, grids, d_out, torch.float64), run(m, rgb, grids, d_out, torch.float32)
        for k in r64:
            out[p + k + "64"], out[p + k + "32"] = r64[k], r32[k]
        rel = lambda a, b: float((a.double() - b).norm() / b.norm().clamp_min(1e-300))
        print(p, "fp32 vs fp64:", "  ".join(f"{k} {rel(r32[k], r64[k]):.2e}" for k in r64))
    dst = HERE / "bilagrid_ref.safetensors"
    save_file(out, str(dst))
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
