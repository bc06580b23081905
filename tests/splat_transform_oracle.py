"""The fp64 statement of csrc/splat_transform.hip in numpy: the rasteriser's SH basis (sh_eval of csrc/gs_raster.h) in fp64, the band
matrices D_l(R) with Y_l(R d) = D_l(R) Y_l(d) by a least-squares fit over 64 fixed directions, whole scenes moved by
x' = s R x + t, and the derived per-element error bounds that tests/test_splat_transform_gpu.py holds the kernel to.

Bounds (u = 2^-24, the unit roundoff of fp32; every coefficient A_ij is an fp64 value that the library rounds to fp32 once):
a dot product of n terms evaluated as one product and n - 1 fmaf carries n roundings, each at most u times a partial sum that
sum_j |A_ij| |x_j| bounds, and the rounding of A adds u sum_j |A_ij| |x_j|: (n + 1) u sum |A| |x| to first order; (n + 2) covers
the second-order terms with room.  The means add t inside the chain: the same factor times |t|.  The log-scale is one addition of
an fp32-rounded constant: 2 u (|v| + |log s|)."""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
BAND_COUNTS = (1, 4, 9, 16, 25)


def sh_basis(d: np.ndarray) -> np.ndarray:
    """sh_eval<4> in fp64: d [..., 3] unit vectors -> [..., 25]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = np.empty(d.shape[:-1] + (25,), dtype=np.float64)
    b[..., 0] = 0.2820947917738781
    b[..., 1] = -0.48860251190292 * y; b[..., 2] = 0.48860251190292 * z; b[..., 3] = -0.48860251190292 * x
    z2, t0b, c1, s1 = z * z, -1.092548430592079 * z, x * x - y * y, 2.0 * x * y
    p6 = 0.9461746957575601 * z2 - 0.3153915652525201
    b[..., 4] = 0.5462742152960395 * s1; b[..., 5] = t0b * y; b[..., 6] = p6; b[..., 7] = t0b * x; b[..., 8] = 0.5462742152960395 * c1
    t0c, t1b = -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
    c2, s2 = x * c1 - y * s1, x * s1 + y * c1
    p12 = z * (1.865881662950577 * z2 - 1.119528997770346)
    b[..., 9] = -0.5900435899266435 * s2; b[..., 10] = t1b * s1; b[..., 11] = t0c * y; b[..., 12] = p12; b[..., 13] = t0c * x
    b[..., 14] = t1b * c1; b[..., 15] = -0.5900435899266435 * c2
    t0d, t1c = z * (-4.683325804901025 * z2 + 2.007139630671868), 3.31161143515146 * z2 - 0.47308734787878
    t2b, c3, s3 = -1.770130769779931 * z, x * c2 - y * s2, x * s2 + y * c2
    b[..., 16] = 0.6258357354491763 * s3; b[..., 17] = t2b * s2; b[..., 18] = t1c * s1; b[..., 19] = t0d * y
    b[..., 20] = 1.984313483298443 * z * p12 - 1.006230589874905 * p6
    b[..., 21] = t0d * x; b[..., 22] = t1c * c1; b[..., 23] = t2b * c2; b[..., 24] = 0.6258357354491763 * c3
    return b


def fit_directions() -> np.ndarray:
    d = np.random.default_rng(20240611).standard_normal((64, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def band_matrices(R: np.ndarray, deg: int = 4) -> list:
    """[D_1 .. D_deg] of a rotation R: the least-squares solution of D_l Y_l(d_k) = Y_l(R d_k) over the 64 fixed directions"""
    d = fit_directions()
    A, B = sh_basis(d), sh_basis(d @ np.asarray(R, dtype=np.float64).T)
    out = []
    for l in range(1, deg + 1):
        sl = slice(l * l, (l + 1) * (l + 1))
        X, *_ = np.linalg.lstsq(A[:, sl], B[:, sl], rcond=None)      # A X = B, X = D^T
        out.append(X.T.copy())
    return out


def random_rotation(rng) -> np.ndarray:
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def quat_of_rotation(R: np.ndarray) -> np.ndarray:
    """(w, x, y, z), unit, w >= 0: the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix of R (Bar-Itzhack)"""
    R = np.asarray(R, dtype=np.float64)
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    x, y, z, qw = v[:, -1]
    q = np.array([qw, x, y, z])
    return -q if q[0] < 0 else q


def hamilton_matrix(r: np.ndarray) -> np.ndarray:
    """the 4x4 matrix of q -> r (x) q on (w, x, y, z)"""
    w, x, y, z = r
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def transform_scene(scene: dict, s: float, R: np.ndarray, t: np.ndarray, quats_xyzw: bool):
    """fp64 transform of a scene of fp32 arrays (means [n,3], scales (logs) [n,3], quats [n,4], opacities [n], sh [n,3,K+1]) ->
    (values, bounds): two dicts of float64 arrays of the inputs' shapes; |kernel - value| <= bound must hold elementwise."""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    x = {k: np.asarray(v, dtype=np.float64) for k, v in scene.items()}
    val, bnd = {}, {}
    A = s * R
    val["means"] = x["means"] @ A.T + t
    bnd["means"] = 5 * U32 * (np.abs(x["means"]) @ np.abs(A).T + np.abs(t))
    val["scales"] = x["scales"] + np.log(s)
    bnd["scales"] = 2 * U32 * (np.abs(x["scales"]) + abs(np.log(s)))
    q = x["quats"][:, [3, 0, 1, 2]] if quats_xyzw else x["quats"]
    H = hamilton_matrix(quat_of_rotation(R))
    qv, qb = q @ H.T, 6 * U32 * (np.abs(q) @ np.abs(H).T)
    back = [1, 2, 3, 0] if quats_xyzw else [0, 1, 2, 3]
    val["quats"], bnd["quats"] = qv[:, back], qb[:, back]
    val["opacities"], bnd["opacities"] = x["opacities"].copy(), np.zeros_like(x["opacities"])
    sh = x["sh"]
    deg = BAND_COUNTS.index(sh.shape[2])
    val["sh"], bnd["sh"] = sh.copy(), np.zeros_like(sh)
    for l, D in enumerate(band_matrices(R, deg), start=1):
        sl = slice(l * l, (l + 1) * (l + 1))
        val["sh"][:, :, sl] = sh[:, :, sl] @ D.T
        bnd["sh"][:, :, sl] = (2 * l + 1 + 2) * U32 * (np.abs(sh[:, :, sl]) @ np.abs(D).T)
    return val, bnd


def make_scene(n: int, Kp: int, seed: int) -> dict:
    """a random fp32 scene of n rows with Kp coefficients per channel"""
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(means=f(n, 3) * 2, scales=f(n, 3) - 3, quats=f(n, 4), opacities=f(n), sh=f(n, 3, Kp))
