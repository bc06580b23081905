"""A scene's five tensors as the splat kernels take them: export, import and similarity transforms."""
import ctypes as C
import math
from typing import Optional

import torch

from .. import lib as L
from .common import _f32_dev, _ptr, _stream, _workspace, f32


SPLAT_TENSORS = ("means", "scales", "quats", "opacities", "sh")   # a scene's five tensors, in the order of lib.SPLAT_FIELDS


def _splat_inner(K: int) -> dict:   # the shape of one row of each tensor; K = the last dimension of sh (the DC term included where stored)
    return dict(means=(3,), scales=(3,), quats=(4,), opacities=(), sh=(3, K))


def _splat_dicts(what: str, params: dict, m: dict, v: dict, rows: int) -> int:
    """`params`, `m` and `v` each hold the five SPLAT_TENSORS as contiguous f32 device tensors of `rows` rows -> K of sh [rows,3,K]"""
    sh = params["sh"]
    if sh.dim() != 3 or sh.shape[1] != 3 or sh.shape[2] < 1:
        raise ValueError(f"{what}: sh must be [rows,3,K], got {tuple(sh.shape)}")
    K = sh.shape[2]
    for group, d in (("params", params), ("m", m), ("v", v)):
        for name, inner in _splat_inner(K).items():
            _f32_dev(d[name], f"{group}[{name!r}]", (rows,) + inner)
    return K


def _scene_view(args, tensors: dict, rows: int, K_plus: int, what: str, label: str, pre: str = "") -> None:
    """Sets the five pointers and row strides (`pre` + `field`, `pre` + `ld_field`) of a SplatExportArgs / SplatImportArgs /
    SplatTransformArgs from `tensors`: float32 device tensors [rows, ...], sh [rows,3,K_plus], whose rows may be strided (a row's own
    elements contiguous).  `label` formats a name."""
    for field, (name, inner) in zip(L.SPLAT_FIELDS, _splat_inner(K_plus).items()):
        t, shape, width = tensors[name], (rows,) + inner, math.prod(inner)
        if not t.is_cuda or t.dtype != f32 or tuple(t.shape) != shape:
            raise ValueError(f"{what}: {label.format(name)} must be a float32 device tensor (the HIP path has no CPU fallback) of shape {shape}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if rows > 0 and width > 1 and not t[0].is_contiguous():
            raise ValueError(f"{what}: the elements of a row of {label.format(name)} must be contiguous, got strides {t.stride()}")
        ld = t.stride(0) if rows > 1 else width
        if ld < width:
            raise ValueError(f"{what}: rows of {label.format(name)} overlap (row stride {ld} < {width})")
        setattr(args, pre + field, t.data_ptr())
        setattr(args, pre + "ld_" + field, ld)


# ------------------------------------------------------------------------------------------------ scene export (csrc/splat_export.hip)
def _export_scene(scene: dict, quats_xyzw: bool, what: str) -> L.SplatExportArgs:
    """The scene part of v3a_splat_export_args from dict(means [U,3], scales (logs) [U,3], quats [U,4], opacities (logits) [U],
    sh [U,3,K+1]): float32 device tensors whose rows may be strided (a row's own elements contiguous)."""
    means, sh = scene["means"], scene["sh"]
    if means.dim() != 2 or means.shape[1] != 3 or sh.dim() != 3 or sh.shape[1] != 3 or sh.shape[2] < 1:
        raise ValueError(f"{what}: means [U,3] and sh [U,3,K+1] required, got {tuple(means.shape)} and {tuple(sh.shape)}")
    U, K = means.shape[0], sh.shape[2] - 1
    a = L.SplatExportArgs()
    _scene_view(a, scene, U, K + 1, what, "{}")
    a.U, a.K, a.quats_xyzw = U, K, int(bool(quats_xyzw))
    return a


def _export_list(t: torch.Tensor, name: str, n: int, U: int) -> None:
    if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.shape[0] < n or not 0 <= n <= U:
        raise ValueError(f"{name} must be a contiguous int32 device vector of at least n = {n} <= {U} entries, got {t.dtype} {tuple(t.shape)} on {t.device}")


def splat_export_filter(scene: dict, *, quats_xyzw: bool, opacity_threshold: Optional[float] = None):
    """The rows that go into an export (v3a_splat_export_filter): every value finite and, with `opacity_threshold`,
    1 / (1 + exp(-logit)) above it.  -> (rows int32 [U], of which the first `count` are set, in ascending order; count int64 [1] on
    the device - reading it is the caller's one synchronisation)."""
    a = _export_scene(scene, quats_xyzw, "splat_export_filter")
    dev = scene["means"].device
    rows, count = torch.empty(a.U, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int64)
    if a.U == 0:
        return rows, count
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_splat_export_filter_workspace_bytes(a.U, a.K), f"v3a_splat_export_filter_workspace_bytes (U = {a.U})", dev)
    a.filter_opacity, a.opacity_threshold = int(opacity_threshold is not None), float(opacity_threshold or 0.0)
    a.rows, a.count, a.workspace, a.workspace_bytes = rows.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.v3a_splat_export_filter(C.byref(a), _stream()), "v3a_splat_export_filter")
    return rows, count


def splat_export_sort(scene: dict, rows: torch.Tensor, n: int, *, quats_xyzw: bool) -> torch.Tensor:
    """rows[:n] in the Morton order of their means, equal keys in ascending row order (v3a_splat_export_sort) -> int32 [n]."""
    a = _export_scene(scene, quats_xyzw, "splat_export_sort")
    _export_list(rows, "rows", n, a.U)
    order = torch.empty(n, device=rows.device, dtype=torch.int32)
    if n == 0:
        return order
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_splat_export_sort_workspace_bytes(a.U, a.K), f"v3a_splat_export_sort_workspace_bytes (U = {a.U})", rows.device)
    a.rows, a.n, a.order, a.workspace, a.workspace_bytes = rows.data_ptr(), n, order.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.v3a_splat_export_sort(C.byref(a), _stream()), "v3a_splat_export_sort")
    return order


def splat_export_pack_compressed(scene: dict, order: torch.Tensor, n: int, *, quats_xyzw: bool):
    """The compressed PLY's three elements of the splats order[:n] (v3a_splat_export_pack_compressed) -> (chunks f32 [ceil(n/256),18],
    vertices int32 [n,4] (the packed words' bits), sh uint8 [n,3K])."""
    a = _export_scene(scene, quats_xyzw, "splat_export_pack_compressed")
    _export_list(order, "order", n, a.U)
    dev = order.device
    chunks = torch.empty((n + 255) // 256, 18, device=dev, dtype=f32)
    vertices = torch.empty(n, 4, device=dev, dtype=torch.int32)
    sh = torch.empty(n, 3 * a.K, device=dev, dtype=torch.uint8)
    if n:
        a.order, a.n, a.out_chunks, a.out_vertices, a.out_sh = order.data_ptr(), n, chunks.data_ptr(), vertices.data_ptr(), sh.data_ptr()
        L.check(L.load().v3a_splat_export_pack_compressed(C.byref(a), _stream()), "v3a_splat_export_pack_compressed")
    return chunks, vertices, sh


def splat_export_pack_splat(scene: dict, order: torch.Tensor, n: int, *, quats_xyzw: bool) -> torch.Tensor:
    """The .splat records of the splats order[:n] (v3a_splat_export_pack_splat) -> uint8 [n,32]."""
    a = _export_scene(scene, quats_xyzw, "splat_export_pack_splat")
    _export_list(order, "order", n, a.U)
    out = torch.empty(n, 32, device=order.device, dtype=torch.uint8)
    if n:
        a.order, a.n, a.out_splat = order.data_ptr(), n, out.data_ptr()
        L.check(L.load().v3a_splat_export_pack_splat(C.byref(a), _stream()), "v3a_splat_export_pack_splat")
    return out


def splat_export_pack_ply(scene: dict, rows: torch.Tensor, n: int, *, quats_xyzw: bool) -> torch.Tensor:
    """The float PLY's vertex rows of rows[:n] (v3a_splat_export_pack_ply) -> f32 [n, 14 + 3K]."""
    a = _export_scene(scene, quats_xyzw, "splat_export_pack_ply")
    _export_list(rows, "rows", n, a.U)
    out = torch.empty(n, 14 + 3 * a.K, device=rows.device, dtype=f32)
    if n:
        a.rows, a.n, a.out_ply = rows.data_ptr(), n, out.data_ptr()
        L.check(L.load().v3a_splat_export_pack_ply(C.byref(a), _stream()), "v3a_splat_export_pack_ply")
    return out


# ------------------------------------------------------------------------------------------------ scene import (csrc/splat_import.hip)
PLY_COLUMNS = (("x", "y", "z") + tuple(f"f_dc_{j}" for j in range(3)) + ("f_rest_0", "opacity") + tuple(f"scale_{j}" for j in range(3))
               + tuple(f"rot_{j}" for j in range(4)))     # the order of v3a_splat_import_args.offsets


def _import_outputs(n: int, K: int, dev, out: Optional[dict], what: str):
    """The five output tensors of a load - fresh, or the caller's (strided rows allowed, as for the exporter) - and the args struct
    with them, `bad` and the workspace set.  -> (args, scene dict, bad int32 [1], workspace)"""
    if out is None:
        out = {name: torch.empty((n,) + inner, device=dev, dtype=f32) for name, inner in _splat_inner(K + 1).items()}
    a = L.SplatImportArgs()
    _scene_view(a, out, n, K + 1, what, "out[{!r}]")
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = None
    if n > 0:
        ws, a.workspace_bytes = _workspace(L.load().v3a_splat_import_workspace_bytes(n), f"v3a_splat_import_workspace_bytes (n = {n})", dev)
        a.workspace = ws.data_ptr()
    a.n, a.n_rest, a.bad = n, 3 * K, bad.data_ptr()
    return a, {name: out[name] for name in SPLAT_TENSORS}, bad, ws


def _import_payload(payload: torch.Tensor, what: str) -> None:
    if not payload.is_cuda or payload.dtype != torch.uint8 or payload.dim() != 1 or not payload.is_contiguous():
        raise ValueError(f"{what}: the payload must be a contiguous uint8 device vector (the HIP path has no CPU fallback), got {payload.dtype} "
                         f"{tuple(payload.shape)} on {payload.device}")


def splat_import_ply(payload: torch.Tensor, n: int, K: int, table: dict, *, opacity: str = "logit", quats_xyzw: bool = True, out: Optional[dict] = None):
    """The vertex rows of a float PLY (v3a_splat_import_ply): payload uint8 [4 n P] on the device; table = {"P": floats per row,
    name: column of each of PLY_COLUMNS}.  opacity: "logit" (copied) or "linear" (logit of the value clamped to [1e-6, 1 - 1e-6]).
    -> (dict(means, scales (logs), quats, opacities (logits), sh [n,3,K+1]), bad int32 [1] on the device: rows with a NaN or Inf)."""
    if opacity not in ("logit", "linear"):
        raise ValueError(f"splat_import_ply: opacity must be 'logit' or 'linear', got {opacity!r}")
    _import_payload(payload, "splat_import_ply")
    a, scene, bad, ws = _import_outputs(n, K, payload.device, out, "splat_import_ply")
    if n:
        a.payload, a.payload_bytes, a.quats_xyzw = payload.data_ptr(), payload.numel(), int(bool(quats_xyzw))
        a.P, a.opacity_linear = int(table["P"]), int(opacity == "linear")
        for j, name in enumerate(PLY_COLUMNS):
            a.offsets[j] = int(table[name]) if K or name != "f_rest_0" else 0      # K = 0: an empty range, it overlaps nothing
        L.check(L.load().v3a_splat_import_ply(C.byref(a), _stream()), "v3a_splat_import_ply")
    return scene, bad


def splat_import_compressed(payload: torch.Tensor, n: int, K: int, *, quats_xyzw: bool = True, out: Optional[dict] = None):
    """A compressed PLY's three elements, back to back (v3a_splat_import_compressed): payload uint8 [72 ceil(n/256) + 16 n + 3 K n].
    -> (scene dict, bad) as splat_import_ply."""
    _import_payload(payload, "splat_import_compressed")
    a, scene, bad, ws = _import_outputs(n, K, payload.device, out, "splat_import_compressed")
    if n:
        a.payload, a.payload_bytes, a.quats_xyzw, a.nch = payload.data_ptr(), payload.numel(), int(bool(quats_xyzw)), (n + 255) // 256
        L.check(L.load().v3a_splat_import_compressed(C.byref(a), _stream()), "v3a_splat_import_compressed")
    return scene, bad


def splat_import_splat(payload: torch.Tensor, n: int, *, quats_xyzw: bool = True, out: Optional[dict] = None):
    """The 32-byte records of a .splat (v3a_splat_import_splat): payload uint8 [32 n].  -> (scene dict with K = 0, bad)."""
    _import_payload(payload, "splat_import_splat")
    a, scene, bad, ws = _import_outputs(n, 0, payload.device, out, "splat_import_splat")
    if n:
        a.payload, a.payload_bytes, a.quats_xyzw = payload.data_ptr(), payload.numel(), int(bool(quats_xyzw))
        L.check(L.load().v3a_splat_import_splat(C.byref(a), _stream()), "v3a_splat_import_splat")
    return scene, bad


# ------------------------------------------------------------------------------------------------ scene transforms (csrc/splat_transform.hip)
SH_BAND_COUNTS = (1, 4, 9, 16, 25)     # K + 1 of a scene that v3a_splat_transform takes: whole bands up to degree 4


def similarity_parts(T, what: str = "similarity_parts"):
    """A 4x4 similarity [[s R, t], [0, 1]] split on the host in fp64 -> (s, R float64 [3,3], t float64 [3]).  ValueError for what
    is none: a bottom row other than 0 0 0 1, a non-finite entry, det <= 0 (a reflection, s <= 0) or |R R^T - I|_max > 1e-6 (shear,
    unequal scales)."""
    T = torch.as_tensor(T, dtype=torch.float64, device="cpu") if not isinstance(T, torch.Tensor) else T.detach().to("cpu", torch.float64)
    if tuple(T.shape) != (4, 4) or not bool(torch.isfinite(T).all()):
        raise ValueError(f"{what}: T must be a finite 4x4 matrix, got shape {tuple(T.shape)}")
    if not torch.equal(T[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)):
        raise ValueError(f"{what}: the bottom row of T must be 0 0 0 1, got {T[3].tolist()}")
    M = T[:3, :3]
    det = float(torch.linalg.det(M))
    if not det > 0.0:
        raise ValueError(f"{what}: det of the linear part is {det:g}; a similarity needs s > 0 and a proper rotation (no reflection)")
    s = det ** (1.0 / 3.0)
    R = M / s
    off = float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max())
    if not off <= 1e-6:
        raise ValueError(f"{what}: the linear part is not a scaled rotation (|R R^T - I|_max = {off:.3g} > 1e-6): shear or unequal scales")
    return s, R.contiguous(), T[:3, 3].contiguous()


def sh_rotation_matrices(R, deg: int) -> list:
    """D_1(R) .. D_deg(R) of the rasteriser's SH basis, Y_l(R d) = D_l(R) Y_l(d), in fp64 on the host (v3a_sh_rotation_matrices;
    no device needed) -> [float64 [2l+1, 2l+1]]"""
    R = torch.as_tensor(R, dtype=torch.float64, device="cpu").contiguous() if not isinstance(R, torch.Tensor) else R.detach().to("cpu", torch.float64).contiguous()
    if tuple(R.shape) != (3, 3):
        raise ValueError(f"sh_rotation_matrices: R must be 3x3, got {tuple(R.shape)}")
    out = torch.zeros(max(sum((2 * l + 1) ** 2 for l in range(1, max(int(deg), 0) + 1)), 1), dtype=torch.float64)
    dp = C.POINTER(C.c_double)
    rc = L.load().v3a_sh_rotation_matrices(C.cast(R.data_ptr(), dp), int(deg), C.cast(out.data_ptr(), dp))
    if rc == L.V3A_OK:
        mats, o = [], 0
        for l in range(1, deg + 1):
            n = 2 * l + 1
            mats.append(out[o:o + n * n].reshape(n, n).clone())
            o += n * n
        return mats
    if rc == -1:
        raise ValueError("sh_rotation_matrices: R is not a proper rotation (|R R^T - I|_max > 1e-6 or det < 0)")
    L.check(rc, "v3a_sh_rotation_matrices")


def splat_transform(scene: dict, T, out: Optional[dict] = None, *, quats_xyzw: bool = True) -> dict:
    """x' = s R x + t applied to a scene (v3a_splat_transform): `scene` as load_scene / create_splats hold it - means [U,3], scales
    (logs) [U,3], quats [U,4], opacities (logits) [U], sh [U,3,K+1] with K + 1 in SH_BAND_COUNTS; float32 device tensors whose rows
    may be strided.  T: a 4x4 similarity (similarity_parts; ValueError otherwise).  Means move, log-scales gain log s, quaternions
    are multiplied by R's from the left, the harmonics' bands 1.. are rotated in the rasteriser's basis; logits and DC are copied.
    out: None (fresh tensors), another scene dict of the same shapes, or `scene` itself (in place).  -> the five output tensors."""
    s, R, t = similarity_parts(T, "splat_transform")
    means, sh = scene["means"], scene["sh"]
    if means.dim() != 2 or means.shape[1] != 3 or sh.dim() != 3 or sh.shape[1] != 3:
        raise ValueError(f"splat_transform: means [U,3] and sh [U,3,K+1] required, got {tuple(means.shape)} and {tuple(sh.shape)}")
    U, Kp = means.shape[0], sh.shape[2]
    if Kp not in SH_BAND_COUNTS:
        raise ValueError(f"splat_transform: sh holds {Kp} coefficients per channel; whole bands are required, one of {SH_BAND_COUNTS}")
    if out is None:
        out = {name: torch.empty((U,) + inner, device=means.device, dtype=f32) for name, inner in _splat_inner(Kp).items()}
    a = L.SplatTransformArgs()
    _scene_view(a, scene, U, Kp, "splat_transform", "scene[{!r}]")
    _scene_view(a, out, U, Kp, "splat_transform", "out[{!r}]", pre="out_")
    a.rows, a.K, a.quats_xyzw, a.scale = U, Kp - 1, int(bool(quats_xyzw)), s
    for i, x in enumerate(R.reshape(-1).tolist()):
        a.R[i] = x
    for i, x in enumerate(t.tolist()):
        a.t[i] = x
    if U:
        L.check(L.load().v3a_splat_transform(C.byref(a), _stream()), "v3a_splat_transform")
    return {name: out[name] for name in SPLAT_TENSORS}


def splat_moments(means: torch.Tensor, centre) -> torch.Tensor:
    """Count, first and second moments of the rows of `means` (float32 device [n,3], rows may be strided) about `centre` (three host
    floats), in fp64 and in a fixed order (v3a_splat_moments) -> float64 [10] on the device: n, sum (x - c) [3], and
    sum (x - c)(x - c)^T as xx xy xz yy yz zz."""
    if not means.is_cuda or means.dtype != f32 or means.dim() != 2 or means.shape[1] != 3 or (means.shape[0] > 0 and means.stride(1) != 1):
        raise ValueError(f"splat_moments: means must be a float32 device tensor [n,3] with contiguous rows (the HIP path has no CPU fallback), got "
                         f"{means.dtype} {tuple(means.shape)} on {means.device}")
    n = means.shape[0]
    ld = means.stride(0) if n > 1 else 3
    if ld < 3:
        raise ValueError(f"splat_moments: rows of means overlap (row stride {ld} < 3)")
    c = (C.c_double * 3)(*[float(x) for x in (centre.tolist() if isinstance(centre, torch.Tensor) else centre)])
    out = torch.empty(10, device=means.device, dtype=torch.float64)
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_splat_moments_workspace_bytes(n), f"v3a_splat_moments_workspace_bytes (n = {n})", means.device)
    L.check(lib.v3a_splat_moments(_ptr(means) if n else None, ld, n, c, _ptr(out), _ptr(ws), ws_bytes, _stream()), "v3a_splat_moments")
    return out
