"""Similarity transforms of a scene, x' = s R x + t, and the world normalisation of the reference's post_opt/datasets/normalize.py
(similarity_from_cameras, align_principal_axes, transform_cameras, normalize).  The scene itself - means, scales, rotations and the
harmonics' bands 1..4 in the rasteriser's basis - is moved on the device (csrc/splat_transform.hip); the
camera arithmetic (V <= 21 matrices) and the 3x3 eigenproblem are numpy fp64 on the host.

One deviation from the reference, stated in DESIGN.md 7i: the signs of the principal axes.  numpy's eigh leaves them to LAPACK; here
each eigenvector's largest-magnitude component is made positive (the first such component on a tie), then - the reference's rule -
column 0 is flipped if the determinant is negative."""
from __future__ import annotations

import dataclasses
import json
from pathlib import Path

import numpy as np
import torch

from .. import ops


def _matrix(T) -> np.ndarray:
    T = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else np.asarray(T)
    T = T.astype(np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"a 4x4 matrix is required, got shape {T.shape}")
    return T


# ------------------------------------------------------------------------------------------------------------------- cameras
def transform_cameras(T, camtoworlds) -> np.ndarray:
    """T applied to camera-to-world matrices [V,4,4] (normalize.py:115-130): T @ c2w, the rotation part divided by the scale that
    row 0 picked up -> float64 [V,4,4]"""
    T = _matrix(T)
    c = camtoworlds.detach().cpu().numpy() if isinstance(camtoworlds, torch.Tensor) else np.asarray(camtoworlds)
    c = c.astype(np.float64)
    if c.ndim != 3 or c.shape[1:] != (4, 4):
        raise ValueError(f"camtoworlds must be [V,4,4], got {c.shape}")
    c = np.einsum("nij, ki -> nkj", c, T)
    scaling = np.linalg.norm(c[:, 0, :3], axis=1)
    c[:, :3, :3] = c[:, :3, :3] / scaling[:, None, None]
    return c


def similarity_from_cameras(c2w: np.ndarray) -> np.ndarray:
    """normalize.py:4-63 with its defaults (center_method="focus", median scaling): z+ becomes the mean camera up axis, the median of
    the points of the optical axes nearest to the origin becomes the origin, the median camera distance becomes 1."""
    c2w = np.asarray(c2w, dtype=np.float64)
    t, R = c2w[:, :3, 3], c2w[:, :3, :3]
    ups = np.sum(R * np.array([0, -1.0, 0]), axis=-1)
    world_up = np.mean(ups, axis=0)
    world_up /= np.linalg.norm(world_up)
    up_camspace = np.array([0.0, -1.0, 0.0])
    c = (up_camspace * world_up).sum()
    cross = np.cross(world_up, up_camspace)
    skew = np.array([[0.0, -cross[2], cross[1]], [cross[2], 0.0, -cross[0]], [-cross[1], cross[0], 0.0]])
    if c > -1:
        R_align = np.eye(3) + skew + (skew @ skew) * 1 / (1 + c)
    else:      # the data has y+ up: half a turn about x
        R_align = np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    R = R_align @ R
    fwds = np.sum(R * np.array([0, 0.0, 1.0]), axis=-1)
    t = (R_align @ t[..., None])[..., 0]
    nearest = t + (fwds * -t).sum(-1)[:, None] * fwds
    translate = -np.median(nearest, axis=0)
    T = np.eye(4)
    T[:3, 3] = translate
    T[:3, :3] = R_align
    T[:3, :] *= 1.0 / np.median(np.linalg.norm(t + translate, axis=-1))
    return T


def principal_axes(cov: np.ndarray):
    """-> (eigenvalues descending, rotation whose ROWS are the principal axes) of a symmetric 3x3 matrix, with this package's sign
    convention: each axis has its largest-magnitude component positive, then axis 0 is flipped if that leaves a reflection."""
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = w.argsort()[::-1]
    w, v = w[order], v[:, order].copy()
    for j in range(3):
        if v[np.argmax(np.abs(v[:, j])), j] < 0:
            v[:, j] *= -1
    if np.linalg.det(v) < 0:
        v[:, 0] *= -1
    return w, v.T


def covariance_of(means: torch.Tensor, centre) -> np.ndarray:
    """np.cov (normalised by n - 1) of the device rows `means` from one pass of ops.splat_moments about `centre`"""
    m = ops.splat_moments(means, centre).cpu().numpy()
    n, s1 = m[0], m[1:4]
    S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    if n < 2:
        raise ValueError("align_principal_axes needs at least two points")
    return (S - np.outer(s1, s1) / n) / (n - 1)


def align_principal_axes(means: torch.Tensor, pre=None) -> np.ndarray:
    """normalize.py:66-97 on the device rows `means` [n,3] as they stand after the similarity `pre` (None: as they are): the median
    becomes the origin, the principal axes x, y, z in descending variance.  The median is one torch.median, the covariance one
    ops.splat_moments pass over the UNMOVED means (cov' = s^2 R cov R^T about the moved centre), the eigenproblem is the host's."""
    pre = np.eye(4) if pre is None else _matrix(pre)
    s, R, t = ops.similarity_parts(pre, "align_principal_axes")
    R = R.numpy()
    A = s * R
    # the median of the moved cloud, per axis, as the reference takes it: the moved coordinates themselves are needed
    moved = means.detach().double() @ torch.from_numpy(A.T).to(means.device) + torch.from_numpy(t.numpy()).to(means.device)
    centroid = _median(moved)
    # the moments about the point that the centroid came from: c0 = A^-1 (centroid - t)
    c0 = R.T @ (centroid - t.numpy()) / s
    cov = (s * s) * R @ covariance_of(means, c0) @ R.T
    _, rot = principal_axes(cov)
    T = np.eye(4)
    T[:3, :3] = rot
    T[:3, 3] = -rot @ centroid
    return T


def _median(x: torch.Tensor) -> np.ndarray:
    """np.median over axis 0 (the mean of the two middle values for an even count) of a device tensor [n,3]"""
    n = x.shape[0]
    if n == 0:
        raise ValueError("align_principal_axes needs at least two points")
    srt = torch.sort(x, dim=0).values
    return (0.5 * (srt[(n - 1) // 2] + srt[n // 2])).cpu().numpy()


def world_normalisation(camtoworlds, means: torch.Tensor = None) -> np.ndarray:
    """The reference's normalize(): T1 = similarity_from_cameras(camtoworlds) and, with `means` (device float32 [n,3]),
    T2 = align_principal_axes of the means moved by T1 -> T2 @ T1 (float64 [4,4]); without, T1."""
    c = camtoworlds.detach().cpu().numpy() if isinstance(camtoworlds, torch.Tensor) else np.asarray(camtoworlds)
    if c.ndim != 3 or c.shape[1:] != (4, 4) or c.shape[0] < 1:
        raise ValueError(f"camtoworlds must be [V,4,4] with V >= 1, got {c.shape}")
    T1 = similarity_from_cameras(c.astype(np.float64))
    if means is None:
        return T1
    return align_principal_axes(means, T1) @ T1


# --------------------------------------------------------------------------------------------------------------------- scenes
def transform_scene(scene: dict, T, out: dict = None, *, quats_xyzw: bool = True) -> dict:
    """ops.splat_transform on the trainer's storage (load_scene / create_splats' "params"): log-scales, logits, sh [U,3,K+1]."""
    return ops.splat_transform(scene, T, out, quats_xyzw=quats_xyzw)


def transform_gaussians(gaussians, T):
    """A `Gaussians` batch of 1 moved by the similarity T -> a new `Gaussians`.  Means, rotations (x y z w) and harmonics go through
    the kernel; the scales are linear here, so they are multiplied by s; covariances become s^2 R C R^T; opacities are kept."""
    if gaussians.means.dim() != 3 or gaussians.means.shape[0] != 1:
        raise ValueError(f"transform_gaussians takes one scene (batch dimension 1), got means of shape {tuple(gaussians.means.shape)}")
    s, R, _ = ops.similarity_parts(T, "transform_gaussians")
    with torch.no_grad():
        f = lambda t: t[0].float().contiguous()
        scales = f(gaussians.scales)
        scene = dict(means=f(gaussians.means), scales=scales, quats=f(gaussians.rotations), opacities=f(gaussians.opacities).reshape(-1),
                     sh=f(gaussians.harmonics))
        moved = ops.splat_transform(scene, T, quats_xyzw=True)      # its scales slot (+ log s) is not used: these are linear
        Rf = (R * s).to(scales.device, torch.float32)
        cov = Rf @ f(gaussians.covariances) @ Rf.T
        return dataclasses.replace(gaussians, means=moved["means"][None], covariances=cov[None], harmonics=moved["sh"][None],
                                   opacities=gaussians.opacities, scales=(scales * float(s))[None], rotations=moved["quats"][None])


# ---------------------------------------------------------------------------------------------------------------------- files
def write_world_transform(path, T, extrinsics) -> None:
    """world_transform.json: {"transform": 4x4, "extrinsics": the cameras moved by it}"""
    Path(path).write_text(json.dumps({"transform": _matrix(T).tolist(), "extrinsics": transform_cameras(T, extrinsics).tolist()}, indent=1))


def read_transform(path) -> np.ndarray:
    """A 4x4 matrix from a JSON file: the bare matrix, or world_transform.json's {"transform": ...}"""
    data = json.loads(Path(path).read_text())
    if isinstance(data, dict):
        if "transform" not in data:
            raise ValueError(f"{path}: no `transform` key")
        data = data["transform"]
    return _matrix(np.asarray(data, dtype=np.float64))
