"""Scene export in the formats of the reference's post_opt/exporter.py (export_splats): `ply` (float properties, every viewer),
`splat` (32 bytes per splat, antimatter15's viewer) and `ply_compressed` (16 bytes per splat + 72 per 256-splat chunk + one byte per
higher-order SH coefficient, SuperSplat).  Filtering, Morton sort and packing run on the device (csrc/splat_export.hip, DESIGN.md
section 7g); the host assembles the text header, reads the survivor count once and copies the packed bytes back once."""
from __future__ import annotations

from pathlib import Path
from typing import Optional

import torch

from .. import ops

FORMATS = ("ply", "splat", "ply_compressed")
FILE_NAMES = {"ply_compressed": "gaussians.compressed.ply", "splat": "gaussians.splat"}   # the CLI's extra files
OPACITY_THRESHOLD = 1 / 255     # ply_compressed drops splats at or below it (exporter.py:221)
CHUNK_PROPERTIES = ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
                    "max_scale_x", "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b")
VERTEX_PROPERTIES = ("packed_position", "packed_rotation", "packed_scale", "packed_color")


def parse_formats(spec: str) -> tuple:
    """'ply_compressed,splat' -> ('ply_compressed', 'splat'): the CLI's --export_format (extra files; '' = none)."""
    out = []
    for name in (s.strip() for s in (spec or "").split(",")):
        if not name:
            continue
        if name not in FILE_NAMES:
            raise ValueError(f"--export_format: unknown format {name!r}, expected a comma list of {sorted(FILE_NAMES)}")
        if name not in out:
            out.append(name)
    return tuple(out)


def header(fmt: str, n: int, K: int) -> bytes:
    """The text in front of the payload: n splats, K higher-order coefficients per channel ('' for `splat`)."""
    if fmt == "splat":
        return b""
    lines = ["ply", "format binary_little_endian 1.0"]
    if fmt == "ply":
        names = ["x", "y", "z"] + [f"f_dc_{j}" for j in range(3)] + [f"f_rest_{j}" for j in range(3 * K)] + ["opacity"]
        names += [f"scale_{j}" for j in range(3)] + [f"rot_{j}" for j in range(4)]
        lines += [f"element vertex {n}"] + [f"property float {p}" for p in names]
    elif fmt == "ply_compressed":
        lines += [f"element chunk {(n + 255) // 256}"] + [f"property float {p}" for p in CHUNK_PROPERTIES]
        lines += [f"element vertex {n}"] + [f"property uint {p}" for p in VERTEX_PROPERTIES]
        lines += [f"element sh {n}"] + [f"property uchar f_rest_{j}" for j in range(3 * K)]
    else:
        raise ValueError(f"Unsupported format: {fmt}")
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


def export_scene(scene: dict, format: str = "ply", save_to: Optional[str] = None, *, quats_xyzw: bool) -> bytes:
    """The file's bytes from dict(means [U,3], scales (logs) [U,3], quats [U,4], opacities (logits) [U], sh [U,3,K+1]; float32 on
    the device, the trainer's storage).  Rows with a NaN or Inf are left out; `ply_compressed` also leaves out the splats whose
    opacity is at most 1/255; `splat` and `ply_compressed` are in Morton order (equal keys in row order)."""
    if format not in FORMATS:
        raise ValueError(f"Unsupported format: {format}")
    K = scene["sh"].shape[2] - 1 if scene["sh"].dim() == 3 else -1
    rows, count = ops.splat_export_filter(scene, quats_xyzw=quats_xyzw, opacity_threshold=OPACITY_THRESHOLD if format == "ply_compressed" else None)
    n = int(count.item())          # the one synchronisation before the copy: it sizes the file
    if format == "ply":
        parts = [ops.splat_export_pack_ply(scene, rows, n, quats_xyzw=quats_xyzw)]
    else:
        order = ops.splat_export_sort(scene, rows, n, quats_xyzw=quats_xyzw)
        if format == "splat":
            parts = [ops.splat_export_pack_splat(scene, order, n, quats_xyzw=quats_xyzw)]
        else:
            parts = list(ops.splat_export_pack_compressed(scene, order, n, quats_xyzw=quats_xyzw))
    payload = torch.cat([p.reshape(-1).view(torch.uint8) for p in parts]) if len(parts) > 1 else parts[0].reshape(-1).view(torch.uint8)
    data = header(format, n, K) + payload.cpu().numpy().tobytes()
    if save_to:
        Path(save_to).parent.mkdir(exist_ok=True, parents=True)
        with open(save_to, "wb") as f:
            f.write(data)
    return data


def export_splats(means: torch.Tensor, scales: torch.Tensor, quats: torch.Tensor, opacities: torch.Tensor, sh0: torch.Tensor,
                  shN: torch.Tensor, format: str = "ply", save_to: Optional[str] = None) -> bytes:
    """The reference's export_splats (exporter.py:475-553), signature and meaning: means [N,3], log-scales [N,3], quaternions
    w x y z [N,4], opacity logits [N], sh0 [N,1,3], shN [N,K,3]; float32 device tensors.  One torch call brings the harmonics into
    the kernels' [N,3,K+1] layout; everything per splat and per chunk happens in the kernels."""
    N = means.shape[0]
    if tuple(means.shape) != (N, 3) or tuple(scales.shape) != (N, 3) or tuple(quats.shape) != (N, 4) or tuple(opacities.shape) != (N,):
        raise ValueError("export_splats: means [N,3], scales [N,3], quats [N,4] and opacities [N] required")
    if tuple(sh0.shape) != (N, 1, 3) or shN.dim() != 3 or shN.shape[0] != N or shN.shape[2] != 3:
        raise ValueError(f"export_splats: sh0 [N,1,3] and shN [N,K,3] required, got {tuple(sh0.shape)} and {tuple(shN.shape)}")
    for name, t in (("means", means), ("scales", scales), ("quats", quats), ("opacities", opacities), ("sh0", sh0), ("shN", shN)):
        if not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"export_splats: {name} must be a float32 device tensor (the HIP path has no CPU fallback), got {t.dtype} on {t.device}")
    sh = torch.cat([sh0, shN], dim=1).permute(0, 2, 1).contiguous()
    return export_scene(dict(means=means, scales=scales, quats=quats, opacities=opacities, sh=sh), format, save_to, quats_xyzw=False)


def export_gaussians(gaussians, path, format: str = "ply_compressed", sh_rest: bool = False) -> bytes:
    """A `Gaussians` object of one scene (x y z w rotations, linear scales and opacities, as export_ply takes them) to `path`.
    sh_rest=False writes the DC colour only, like gaussians.ply.  The logs and logits are one elementwise torch call each."""
    if gaussians.means.dim() != 3 or gaussians.means.shape[0] != 1:
        raise ValueError(f"export_gaussians takes one scene (batch dimension 1), got means of shape {tuple(gaussians.means.shape)}")
    with torch.no_grad():
        sh = gaussians.harmonics[0].float()
        scene = dict(means=gaussians.means[0].float(), scales=torch.log(gaussians.scales[0].float()), quats=gaussians.rotations[0].float(),
                     opacities=torch.logit(gaussians.opacities[0].reshape(-1).float().clamp(1e-6, 1 - 1e-6)),
                     sh=sh if sh_rest else sh[..., :1].contiguous())
        return export_scene(scene, format, str(path), quats_xyzw=True)
