"""Golden vectors for the world normalisation (vist3a_amd/utils/splat_transform.py), produced by the reference's own module
(third_party_model/anysplat/src/post_opt/datasets/normalize.py), loaded by file path.

    python tests/golden/make_golden_world_normalize.py   ->  tests/golden/world_normalize_ref.safetensors

Three seeded camera sets, V = 2, 13 and 21 (OpenCV camera-to-world matrices on a tilted, noisy orbit), each with a cloud of 500 points
whose coordinates are float32 values (the device tests feed the same numbers).  Per set v<V>.:
  cams [V,4,4], points [500,3]                       the inputs, float64
  T1                                                 similarity_from_cameras(cams)
  cams1, points1                                     transform_cameras(T1, cams), transform_points(T1, points)
  cov, eigenvalues                                   np.cov and the eigenvalues (ascending, as eigh returns them) inside
                                                     align_principal_axes(points1), captured by wrapping numpy's two functions
  T2, cams2, points2, T                              align_principal_axes' matrix and normalize()'s three outputs.  The signs of T2's
                                                     rows are LAPACK's choice: tests compare through cov / eigenvalues, not through these
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import numpy as np
import torch
from safetensors.torch import save_file

SETS = (2, 13, 21)
N_POINTS = 500


def make_inputs(V: int):
    rng = np.random.default_rng(1000 + V)
    up = np.array([0.3, -0.9, 0.2])
    up /= np.linalg.norm(up)
    a = np.cross(up, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(up, a)
    cams = np.tile(np.eye(4), (V, 1, 1))
    for i in range(V):
        phi = 2 * np.pi * i / V + 0.1 * rng.standard_normal()
        pos = (2.0 + 0.2 * rng.standard_normal()) * (np.cos(phi) * a + np.sin(phi) * b) + (0.5 + 0.1 * rng.standard_normal()) * up
        pos = pos + np.array([0.4, -0.2, 0.7])
        fwd = np.array([0.4, -0.2, 0.7]) + 0.1 * rng.standard_normal(3) - pos
        fwd /= np.linalg.norm(fwd)
        x = np.cross(-up, fwd)
        x /= np.linalg.norm(x)
        y = np.cross(fwd, x)
        cams[i, :3, 0], cams[i, :3, 1], cams[i, :3, 2], cams[i, :3, 3] = x, y, fwd, pos
    pts = rng.standard_normal((N_POINTS, 3)) * np.array([1.5, 0.3, 0.8]) @ np.linalg.qr(rng.standard_normal((3, 3)))[0].T
    pts = (pts + np.array([0.4, -0.2, 0.7])).astype(np.float32).astype(np.float64)
    return cams, pts


def _ref_module():
    sys.path.insert(0, str(HERE))
    import _ref_import
    _ref_import.install()
    spec = importlib.util.spec_from_file_location("ref_normalize", _ref_import.REF + "/third_party_model/anysplat/src/post_opt/datasets/normalize.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    m = _ref_module()
    out = {}
    for V in SETS:
        cams, pts = make_inputs(V)
        T1 = m.similarity_from_cameras(cams.copy())
        cams1, pts1 = m.transform_cameras(T1, cams.copy()), m.transform_points(T1, pts)
        seen = {}
        plain_cov, plain_eigh = np.cov, np.linalg.eigh

        def cov(*a, **k):
            seen["cov"] = plain_cov(*a, **k)
            return seen["cov"]

        def eigh(*a, **k):
            r = plain_eigh(*a, **k)
            seen["eigenvalues"] = np.array(r[0])
            return r

        np.cov, np.linalg.eigh = cov, eigh
        try:
            T2 = m.align_principal_axes(pts1)
        finally:
            np.cov, np.linalg.eigh = plain_cov, plain_eigh
        cams2, pts2, T = m.normalize(cams.copy(), pts)
        rec = dict(cams=cams, points=pts, T1=T1, cams1=cams1, points1=pts1, cov=seen["cov"], eigenvalues=seen["eigenvalues"], T2=T2,
                   cams2=cams2, points2=pts2, T=T)
        for k, v in rec.items():
            out[f"v{V}.{k}"] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
        print(f"V = {V}: scale {np.linalg.det(T1[:3, :3]) ** (1 / 3):.4f}, eigenvalues {seen['eigenvalues']}")
    dst = HERE / "world_normalize_ref.safetensors"
    save_file(out, str(dst))
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
