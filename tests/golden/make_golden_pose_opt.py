"""Golden vectors for the pose parametrisation (csrc/post_opt.hip: v3a_camera_adjust; tests/pose_opt_oracle.py), produced by the
reference's own module (third_party_model/anysplat/src/post_opt/utils.py: CameraOptModule), loaded by file path.

    python tests/golden/make_golden_pose_opt.py   ->  tests/golden/pose_opt_ref.safetensors

The module imports `sklearn` and `matplotlib` at its top (neither is used by CameraOptModule): stubs go into sys.modules first
where they are absent.  The module is run in float64 with its embedding set to the case's deltas.
Cases (pose_opt_oracle.GOLDEN_CASES), V = 3 cameras each.  Per case <name>.:
  c2w      float64 [3,4,4]  the input cameras (pose_opt_oracle.cameras)
  deltas   float64 [3,9]    the embedding's rows (pose_opt_oracle.deltas)
  out      float64 [3,4,4]  CameraOptModule.forward(c2w, ids)
  viewmat  float64 [3,4,4]  torch.linalg.inv(out);   campos  float64 [3,3]  out[:, :3, 3]
The file holds data only."""
from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch
from safetensors.torch import save_file

import pose_opt_oracle as PO


def _ref_module():
    sys.path.insert(0, str(HERE))
    import _ref_import
    for name, subs in (("sklearn", ("neighbors",)), ("matplotlib", ("pyplot",))):
        try:
            __import__(name)
            continue
        except Exception:
            pass
        root = types.ModuleType(name)
        root.__path__ = []
        sys.modules[name] = root
        for sub in subs:
            m = types.ModuleType(f"{name}.{sub}")
            setattr(root, sub, m)
            sys.modules[f"{name}.{sub}"] = m
        if name == "sklearn":
            sys.modules["sklearn.neighbors"].NearestNeighbors = object
        else:
            root.colormaps = {}
    spec = importlib.util.spec_from_file_location("ref_post_opt_utils", _ref_import.REF + "/third_party_model/anysplat/src/post_opt/utils.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    m = _ref_module()
    out = {}
    for i, (name, size) in enumerate(PO.GOLDEN_CASES.items()):
        V = 3
        c2w, d = PO.cameras(V, 100 + i), PO.deltas(V, 200 + i, size)
        mod = m.CameraOptModule(V).double()
        with torch.no_grad():
            mod.embeds.weight.copy_(d)
            # the module builds its transform with torch.eye's default dtype: run it under a float64 default
            torch.set_default_dtype(torch.float64)
            try:
                o = mod(c2w, torch.arange(V))
            finally:
                torch.set_default_dtype(torch.float32)
        assert o.dtype == torch.float64
        p = name + "."
        out[p + "c2w"], out[p + "deltas"], out[p + "out"] = c2w.contiguous(), d.contiguous(), o.contiguous()
        out[p + "viewmat"], out[p + "campos"] = torch.linalg.inv(o).contiguous(), o[:, :3, 3].contiguous()
        mine = PO.adjust(c2w, d)
        print(f"{name}: |deltas| {size}, oracle vs the reference's module {float((mine - o).abs().max()):.3e}")
    dst = HERE / "pose_opt_ref.safetensors"
    save_file(out, str(dst))
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
