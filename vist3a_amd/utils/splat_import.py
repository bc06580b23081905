"""Scene import: the files of vist3a_amd/utils/splat_export.py - `ply` (float properties; also any trainer's standard 3DGS PLY and
this package's own gaussians.ply), `ply_compressed` (SuperSplat) and `splat` (antimatter15) - read back into the trainer's storage.
The host parses the text header into a column table and uploads the payload once; every value is decoded on the device
(csrc/splat_import.hip); the number of rows that decoded to a NaN or Inf is the one value read back.

    python -m vist3a_amd.utils.splat_import IN --out OUT --to {ply,splat,ply_compressed} [--opacity linear|logit] [--dc_only]
                                            [--transform FILE.json] [--align_principal_axes]"""
from __future__ import annotations

import argparse
import os
from pathlib import Path
from typing import Union

import numpy as np
import torch

from .. import ops
from .splat_export import CHUNK_PROPERTIES, FORMATS, VERTEX_PROPERTIES, export_scene

MAX_K = 63                          # higher-order coefficients per channel the kernels take (degree 7)
MAX_ROW_FLOATS = 4096               # floats per vertex row of a float PLY
FLOAT_TYPES = ("float", "float32")
END = b"end_header\n"


def _elements(head: str):
    """[(name, count, [(type, property name)])] of a PLY header; refuses what the loaders do not read"""
    lines = [l.strip() for l in head.split("\n")]
    if len(lines) < 2 or not lines[1].startswith("format "):
        raise ValueError("PLY header: the second line must be the format line")
    fmt = lines[1].split()
    if fmt[1:2] != ["binary_little_endian"]:
        raise ValueError(f"PLY format {' '.join(fmt[1:])!r} is not supported: only binary_little_endian files are read (no ASCII, no big-endian)")
    elements = []
    for l in lines[2:]:
        w = l.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        if w[0] == "element" and len(w) == 3 and w[2].isdigit():
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) == 3:
            elements[-1][2].append((w[1], w[2]))
        elif w[0] == "property" and w[1:2] == ["list"]:
            raise ValueError(f"PLY header: list properties are not supported ({l!r})")
        else:
            raise ValueError(f"PLY header: cannot read the line {l!r}")
    return elements


def _payload_size(have: int, want: int, what: str) -> None:
    if have < want:
        raise ValueError(f"{what}: the payload is truncated, {have} bytes where the header promises {want}")
    if have > want:
        raise ValueError(f"{what}: the payload is over-long, {have} bytes where the header promises {want}")


def _rest_count(names, what: str) -> int:
    """f_rest_0 .. f_rest_{3K-1} must follow each other in this order -> 3K"""
    rest = [i for i, p in enumerate(names) if p.startswith("f_rest_")]
    for j, i in enumerate(rest):
        if names[i] != f"f_rest_{j}" or i != rest[0] + j:
            raise ValueError(f"{what}: the f_rest_* properties must be f_rest_0 .. f_rest_{len(rest) - 1}, consecutive and in this order")
    if len(rest) % 3 or len(rest) // 3 > MAX_K:
        raise ValueError(f"{what}: {len(rest)} f_rest_* properties; a multiple of 3, at most {3 * MAX_K}, is required")
    return len(rest)


def parse_header(data: bytes):
    """-> (format, n, K, table, payload_offset).  `format` is "ply", "ply_compressed" or "splat"; n splats with K higher-order
    coefficients per channel; the payload is data[payload_offset:].  table (ply only): {"P": floats per vertex row, and the column
    of each of ops.PLY_COLUMNS} - the properties may stand in any order and other float properties (nx ny nz) are skipped.
    Without the `ply` magic, a length divisible by 32 is a `.splat`.  Refuses, naming the problem: ASCII and big-endian files,
    list properties, a non-float vertex property of a float PLY, a missing property, a payload shorter or longer than the header
    promises, a compressed PLY whose chunk count is not ceil(n / 256)."""
    if not (data[:4] == b"ply\n" or data[:5] == b"ply\r\n"):
        if len(data) % 32:
            raise ValueError(f"neither a PLY (no `ply` magic) nor a .splat: {len(data)} bytes are not a multiple of 32")
        return "splat", len(data) // 32, 0, {}, 0
    end = data.find(END)
    if end < 0:
        raise ValueError("PLY header: no end_header line")
    off = end + len(END)
    elements = _elements(data[:off].decode("ascii", errors="replace").replace("\r\n", "\n"))
    by_name = {e[0]: e for e in elements}
    if "vertex" not in by_name:
        raise ValueError("PLY header: no vertex element")
    n = by_name["vertex"][1]
    names = [p for _, p in by_name["vertex"][2]]
    if "chunk" in by_name or "packed_position" in names:
        what = "compressed PLY"
        order = [e[0] for e in elements]
        if order not in (["chunk", "vertex"], ["chunk", "vertex", "sh"]):
            raise ValueError(f"{what}: elements {order}; chunk, vertex and (optionally) sh are required, in this order")
        _, nch, cprops = by_name["chunk"]
        if [p for _, p in cprops] != list(CHUNK_PROPERTIES) or any(t not in FLOAT_TYPES for t, _ in cprops):
            missing = [p for p in CHUNK_PROPERTIES if p not in [q for _, q in cprops]]
            raise ValueError(f"{what}: the chunk element must hold the 18 float properties {CHUNK_PROPERTIES[0]} .. {CHUNK_PROPERTIES[-1]} (missing property: {missing})")
        if names != list(VERTEX_PROPERTIES) or any(t not in ("uint", "uint32") for t, _ in by_name["vertex"][2]):
            missing = [p for p in VERTEX_PROPERTIES if p not in names]
            raise ValueError(f"{what}: the vertex element must hold the 4 uint properties {VERTEX_PROPERTIES} (missing property: {missing})")
        k3 = 0
        if "sh" in by_name:
            _, nsh, sprops = by_name["sh"]
            if any(t not in ("uchar", "uint8") for t, _ in sprops):
                raise ValueError(f"{what}: the sh element must hold uchar properties only")
            k3 = _rest_count([p for _, p in sprops], what)
            if len(sprops) != k3 or (k3 and nsh != n):
                raise ValueError(f"{what}: the sh element must hold f_rest_* only, one row per vertex ({nsh} rows, {n} vertices)")
        if nch != (n + 255) // 256:
            raise ValueError(f"{what}: {nch} chunks for {n} vertices; the chunk count must be ceil(n / 256) = {(n + 255) // 256}")
        _payload_size(len(data) - off, 72 * nch + 16 * n + k3 * n, what)
        return "ply_compressed", n, k3 // 3, {}, off
    what = "float PLY"
    if len(elements) != 1:
        raise ValueError(f"{what}: elements {[e[0] for e in elements]}; one vertex element is required")
    for t, p in by_name["vertex"][2]:
        if t not in FLOAT_TYPES:
            raise ValueError(f"{what}: non-float vertex property `{t} {p}`; every vertex property must be a float")
    if len(set(names)) != len(names):
        raise ValueError(f"{what}: a vertex property is declared twice")
    k3 = _rest_count(names, what)
    table = {"P": len(names)}
    for p in ops.PLY_COLUMNS:
        if p == "f_rest_0" and k3 == 0:
            table[p] = 0
            continue
        if p not in names:
            raise ValueError(f"{what}: missing property `{p}`")
        table[p] = names.index(p)
    if table["P"] > MAX_ROW_FLOATS:
        raise ValueError(f"{what}: {table['P']} properties per vertex; at most {MAX_ROW_FLOATS} are read")
    _payload_size(len(data) - off, 4 * n * table["P"], what)
    return "ply", n, k3 // 3, table, off


def _read(path_or_bytes: Union[str, os.PathLike, bytes, bytearray, memoryview]) -> bytes:
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    return Path(path_or_bytes).read_bytes()


def load_scene(path_or_bytes, *, opacity: str = "logit", quats_xyzw: bool = True, strict: bool = True) -> dict:
    """A scene file (a path or its bytes) as the trainer's storage: dict(means [n,3], scales (logs) [n,3], quats [n,4] (x y z w, or
    w x y z with quats_xyzw=False), opacities (logits) [n], sh [n,3,K+1]), float32 on the device - what export_scene takes.
    opacity: how a float PLY stores it - "logit" (a standard 3DGS PLY, export_splats) or "linear" (gaussians.ply).  The rows keep the
    file's order.  One value is read back: the number of rows that decoded to a NaN or Inf; strict=True raises ValueError with it,
    strict=False returns the scene as decoded."""
    data = _read(path_or_bytes)
    fmt, n, K, table, off = parse_header(data)
    if not torch.cuda.is_available():
        raise RuntimeError("load_scene decodes on the device (the HIP path has no CPU fallback); none is visible")
    raw = np.frombuffer(data, np.uint8)[off:]
    payload = torch.from_numpy(raw.copy()).cuda() if raw.size else torch.empty(0, dtype=torch.uint8, device="cuda")
    if fmt == "ply":
        scene, bad = ops.splat_import_ply(payload, n, K, table, opacity=opacity, quats_xyzw=quats_xyzw)
    elif fmt == "ply_compressed":
        scene, bad = ops.splat_import_compressed(payload, n, K, quats_xyzw=quats_xyzw)
    else:
        scene, bad = ops.splat_import_splat(payload, n, quats_xyzw=quats_xyzw)
    count = int(bad.item()) if n else 0      # the one synchronisation
    if strict and count:
        raise ValueError(f"load_scene: {count} of the {n} splats of this `{fmt}` file decode to a NaN or Inf (strict=False returns them)")
    return scene


def load_gaussians(path_or_bytes, **kw):
    """A scene file as a `Gaussians` batch of 1 (linear scales and opacities, unit x y z w rotations, covariances rebuilt): what
    DecoderSplattingCUDA, evaluate_views and create_splats take.  Keywords as load_scene (opacity, strict)."""
    from ..post_opt.trainer import splats_to_gaussians
    return splats_to_gaussians(dict(params=load_scene(path_or_bytes, quats_xyzw=True, **kw)))


def load_gaussians_ply(path):
    """This package's own gaussians.ply (utils/ply_export.py: linear opacities, nx ny nz columns) as `Gaussians`."""
    return load_gaussians(path, opacity="linear")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Convert a scene file between ply, splat and ply_compressed (decoded and packed on the GPU).")
    ap.add_argument("input")
    ap.add_argument("--out", required=True)
    ap.add_argument("--to", required=True, choices=FORMATS)
    ap.add_argument("--opacity", default="logit", choices=("linear", "logit"), help="how a float PLY input stores its opacity (gaussians.ply: linear)")
    ap.add_argument("--dc_only", action="store_true", help="write the DC colour only")
    ap.add_argument("--transform", default=None, metavar="FILE.json",
                    help="move the scene by a 4x4 similarity before writing it: a JSON matrix, or a world_transform.json (its `transform`)")
    ap.add_argument("--align_principal_axes", action="store_true",
                    help="then centre the scene on the median of its means and turn its principal axes onto x, y, z (descending variance)")
    args = ap.parse_args(argv)
    scene = load_scene(args.input, opacity=args.opacity, quats_xyzw=True)
    if args.dc_only:
        scene["sh"] = scene["sh"][..., :1].contiguous()
    if args.transform or args.align_principal_axes:      # on the device, harmonics rotated (csrc/splat_transform.hip)
        from .splat_transform import align_principal_axes, read_transform, transform_scene
        if args.transform:
            scene = transform_scene(scene, read_transform(args.transform), scene)
        if args.align_principal_axes:
            scene = transform_scene(scene, align_principal_axes(scene["means"]), scene)
    data = export_scene(scene, args.to, args.out, quats_xyzw=True)
    print(f"{args.out}: {len(data)} bytes, {args.to}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
