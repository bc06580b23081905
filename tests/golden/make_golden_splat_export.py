"""Golden vectors for the scene exporters (csrc/splat_export.hip, tests/splat_export_oracle.py), produced by the reference's own
module (third_party_model/anysplat/src/post_opt/exporter.py: export_splats), loaded by file path.

    python tests/golden/make_golden_splat_export.py   ->  tests/golden/splat_export_ref.safetensors

Cases (splat_export_oracle.CASES / make_inputs): A N = 700, K = 24 (three chunks, the last with 188 splats); B N = 257, K = 3 (a last
chunk of one splat: max == min); C N = 256, K = 0 (one full chunk, an empty `element sh`); D N = 300, K = 8 with Morton ties, five
rows carrying a NaN / Inf and logits on both sides of the opacity threshold; E N = 1.  Per case <case>.:
  means, scales, quats, opacities, sh0, shN     float32 inputs in the reference's signature
  ply, splat, ply_compressed                    export_splats' bytes, uint8

For D only the reference runs with torch.argsort wrapped to stable=True: its own call leaves the order of equal Morton keys
unspecified, and the fixture defines the order this project promises.  Every logit keeps 1e-2 from logit(1/255)."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch
from safetensors.torch import save_file

import splat_export_oracle as SO


def _ref_module():
    sys.path.insert(0, str(HERE))
    import _ref_import
    _ref_import.install()
    spec = importlib.util.spec_from_file_location("ref_exporter", _ref_import.REF + "/third_party_model/anysplat/src/post_opt/exporter.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    m = _ref_module()
    out = {}
    plain_argsort = torch.argsort
    for case in SO.CASES:
        x = SO.make_inputs(case)
        assert float((x["opacities"][torch.isfinite(x["opacities"])] - SO.LOGIT_EDGE).abs().min()) >= 1e-2
        for k, v in x.items():
            out[f"{case}.{k}"] = v.contiguous()
        if case == "D":
            torch.argsort = lambda t, *a, **k: plain_argsort(t, *a, **{**k, "stable": True})
        try:
            for fmt in SO.FORMATS:
                data = m.export_splats(**{k: v.clone() for k, v in x.items()}, format=fmt)
                out[f"{case}.{fmt}"] = torch.frombuffer(bytearray(data), dtype=torch.uint8).clone()
                same = data == SO.export(fmt, **x)
                print(f"{case} {fmt}: {len(data)} bytes, restatement {'identical' if same else 'DIFFERS'}")
        finally:
            torch.argsort = plain_argsort
    dst = HERE / "splat_export_ref.safetensors"
    save_file(out, str(dst))
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
