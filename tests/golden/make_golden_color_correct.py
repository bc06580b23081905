"""Golden vectors for the colour correction (csrc/color_correct.hip, tests/color_correct_oracle.py), produced by the reference's own
function (third_party_model/anysplat/src/post_opt/lib_bilagrid.py: color_correct), loaded by file path.

    python tests/golden/make_golden_color_correct.py   ->  tests/golden/color_correct_ref.safetensors

The module imports `tensorly` (not installed; only its CP-decomposed 4-D grid uses it): a stub whose set_backend does nothing goes
into sys.modules first.  The function flattens its whole input into one system, so it is called once per image.
Cases (color_correct_oracle.GOLDEN_CASES, inputs of color_correct_oracle.make_inputs).  Per case <name>.:
  img, ref        float32 inputs [N,H,W,3]
  out64, mse64    color_correct(img, ref, num_iters) with the inputs widened to float64, and its per-image MSE against ref
  out32           the same from the function run in float32 (its own rounding spread: the comparison figure)
  rows            int32 [N, num_iters, 3]: the rows each fit used;  seed: the make_inputs seed
The row masks of every round are captured at the function's lstsq calls (a used row has a_mat's constant column = 1) and the
float32 and float64 runs must select the same rows in every round; the case is re-seeded until they do, so that no threshold flip
hides inside a tolerance."""
from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch
from safetensors.torch import save_file

import color_correct_oracle as CO


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


def run(m, img, ref, num_iters, dt):
    """-> (out [N,H,W,3] in dt, masks: per image a list of num_iters * 3 bool rows)"""
    real = torch.linalg.lstsq
    outs, masks = [], []
    for n in range(img.shape[0]):
        seen = []

        def spy(a, b, *args, **kw):
            seen.append(a[:, -1] != 0)
            return real(a, b, *args, **kw)

        torch.linalg.lstsq = spy
        try:
            outs.append(m.color_correct(img[n].to(dt), ref[n].to(dt), num_iters=num_iters))
        finally:
            torch.linalg.lstsq = real
        assert len(seen) == 3 * num_iters
        masks.append(seen)
    return torch.stack(outs), masks


def main():
    m = _ref_module()
    out = {}
    for name, ((N, H, W), iters) in CO.GOLDEN_CASES.items():
        for seed in range(100):
            img, ref = CO.make_inputs(N, H, W, seed)
            o64, m64 = run(m, img, ref, iters, torch.float64)
            o32, m32 = run(m, img, ref, iters, torch.float32)
            if all(torch.equal(a, b) for x, y in zip(m64, m32) for a, b in zip(x, y)):
                break
            print(name, "seed", seed, "float32 and float64 select different rows: re-seeding")
        else:
            raise SystemExit(f"{name}: no seed with equal masks")
        p = name + "."
        rows = torch.tensor([[[int(im[it * 3 + c].sum()) for c in range(3)] for it in range(iters)] for im in m64], dtype=torch.int32)
        out[p + "img"], out[p + "ref"] = img, ref
        out[p + "out64"], out[p + "out32"], out[p + "mse64"], out[p + "rows"] = o64.contiguous(), o32.contiguous(), CO.mse(o64, ref), rows
        out[p + "seed"] = torch.tensor([seed], dtype=torch.int32)
        rel = float((o32.double() - o64).norm() / o64.norm())
        print(f"{name}: pixels {H * W}, rows used {rows.min().item()}..{rows.max().item()}, fp32 vs fp64 {rel:.3e}, "
              f"psnr {CO.psnr(CO.mse(img, ref)).tolist()} -> cc {CO.psnr(CO.mse(o64, ref)).tolist()}")
    dst = HERE / "color_correct_ref.safetensors"
    save_file(out, str(dst))
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
