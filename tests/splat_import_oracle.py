"""Host twin of the scene import (csrc/splat_import.hip, vist3a_amd/utils/splat_import.py): numpy **fp32** decoders of the float PLY,
the compressed PLY and the .splat in the kernels' operation order, the fp64 value of every decoded field
(built on the fp64 decoders of tests/splat_export_oracle.py, which stay the contract of what a code means), the bounds the two are
held to, and small header builders for the parser's tests.

A decoded scene here is dict(means [n,3], scales (logs) [n,3], quats (w x y z) [n,4], opacities (logits) [n], sh [n,3,K+1])."""
from __future__ import annotations

import math

import numpy as np

import splat_export_oracle as SO

F = np.float32
C0 = F(SO.C0)
SQRT2 = F(math.sqrt(2))
TOP = np.array([2047, 1023, 2047], dtype=F)
PLY_NAMES = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")
EPS = 2.0 ** -24          # half an ulp of 1 in fp32


# ------------------------------------------------------------------------------------------------------------------ float PLY
def ply_header(n: int, names, types=None, fmt: str = "binary_little_endian") -> bytes:
    types = types or ["float"] * len(names)
    return ("ply\n" + f"format {fmt} 1.0\n" + f"element vertex {n}\n" + "".join(f"property {t} {p}\n" for t, p in zip(types, names))
            + "end_header\n").encode()


def ply_names(data: bytes):
    head, _ = SO.split_header(data)
    return [l.split()[2] for l in head.decode().split("\n") if l.startswith("property ")]


def ply_columns(data: bytes):
    """-> (float32 [n,P] rows, names)"""
    head, body = SO.split_header(data)
    names = ply_names(data)
    n = int(next(l for l in head.decode().split("\n") if l.startswith("element vertex")).split()[-1])
    return np.frombuffer(body, "<f4", n * len(names)).reshape(n, len(names)).copy(), names


def permute_ply(data: bytes, order, extra=()) -> bytes:
    """the same float PLY with its properties in `order` (indices into the file's own) and zero-filled `extra` properties in front"""
    rows, names = ply_columns(data)
    out = np.concatenate([np.zeros((rows.shape[0], len(extra)), F), rows[:, list(order)]], axis=1)
    return ply_header(rows.shape[0], list(extra) + [names[i] for i in order]) + out.astype("<f4").tobytes()


def logit_linear32(o: np.ndarray) -> np.ndarray:
    o = o.astype(F)
    lo, hi = F(1e-6), F(1 - 1e-6)
    with np.errstate(all="ignore"):
        c = np.where(o < lo, lo, np.where(o > hi, hi, o)).astype(F)      # a NaN stays a NaN
        return np.log(c / (F(1) - c)).astype(F)


def logit_linear64(o: np.ndarray) -> np.ndarray:
    c = np.clip(o.astype(F), F(1e-6), F(1 - 1e-6)).astype(np.float64)
    return np.log(c / (1 - c))


def twin_ply(data: bytes, opacity: str = "logit") -> dict:
    rows, names = ply_columns(data)
    col = lambda p: rows[:, names.index(p)]
    k3 = sum(p.startswith("f_rest_") for p in names)
    K, n = k3 // 3, rows.shape[0]
    sh = np.zeros((n, 3, K + 1), F)
    for c in range(3):
        sh[:, c, 0] = col(f"f_dc_{c}")
        for k in range(K):
            sh[:, c, 1 + k] = col(f"f_rest_{c * K + k}")
    op = col("opacity")
    return dict(means=np.stack([col(p) for p in "xyz"], 1), scales=np.stack([col(f"scale_{j}") for j in range(3)], 1),
                quats=np.stack([col(f"rot_{j}") for j in range(4)], 1), opacities=op.copy() if opacity == "logit" else logit_linear32(op), sh=sh)


# ------------------------------------------------------------------------------------------------------------ compressed PLY
def _place_rot(three: np.ndarray, dropped: np.ndarray, big: np.ndarray) -> np.ndarray:
    """the dropped component at index `big` (w x y z numbering), the stored three in the other places in ascending order"""
    q = np.zeros((three.shape[0], 4), three.dtype)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[big]
    np.put_along_axis(q, others, three, axis=1)
    np.put_along_axis(q, big[:, None], dropped[:, None], axis=1)
    return q


def _sh_of(sh0: np.ndarray, rest: np.ndarray, K: int) -> np.ndarray:
    return np.concatenate([sh0[:, :, None], rest.reshape(rest.shape[0], 3, K)], axis=2)


def twin_compressed(data: bytes) -> dict:
    p = SO.parse_compressed(data)
    f = SO.fields_compressed(p["vertices"])
    n, K = p["n"], p["K"]
    b = np.repeat(p["chunks"].astype(F), SO.CHUNK, axis=0)[:n]
    with np.errstate(all="ignore"):
        lerp = lambda lo, hi, code, top: (lo + (hi - lo) * (code.astype(F) / top)).astype(F)
        means, scales = lerp(b[:, 0:3], b[:, 3:6], f["pos"], TOP), lerp(b[:, 6:9], b[:, 9:12], f["scale"], TOP)
        sh0 = ((lerp(b[:, 12:15], b[:, 15:18], f["rgb"], F(255)) - F(0.5)) / C0).astype(F)
    rest = (((p["sh"].astype(F) + F(0.5)) / F(256) - F(0.5)) * F(8)).astype(F)
    c = np.clip(f["opacity"].astype(F), F(0.5), F(254.5))
    v = ((f["rot"].astype(F) / F(1023) - F(0.5)) * SQRT2).astype(F)
    dropped = np.sqrt(np.maximum(F(0), F(1) - ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))).astype(F)
    return dict(means=means, scales=scales, quats=_place_rot(v, dropped, f["rot_index"]), opacities=np.log(c / (F(255) - c)).astype(F),
                sh=_sh_of(sh0, rest, K), rot_index=f["rot_index"])


def ref_compressed(data: bytes) -> dict:
    """fp64, from SO.decode_compressed"""
    d = SO.decode_compressed(data)
    f = SO.fields_compressed(SO.parse_compressed(data)["vertices"])
    c = np.clip(f["opacity"].astype(np.float64), 0.5, 254.5)
    dropped = np.sqrt(np.maximum(0.0, 1 - (d["rot"] ** 2).sum(axis=1)))
    return dict(means=d["means"], scales=d["scales"], quats=_place_rot(d["rot"], dropped, d["rot_index"]), opacities=np.log(c / (255 - c)),
                sh=_sh_of((d["rgb"] - 0.5) / SO.C0, d["shN"], d["K"]), rot_index=d["rot_index"], chunks=d["chunks"])


# ------------------------------------------------------------------------------------------------------------------- .splat
def twin_splat(data: bytes) -> dict:
    p = SO.parse_splat(data)
    rgb = ((p["rgba"][:, :3].astype(F) + F(0.5)) / F(255)).astype(F)
    c = np.clip(p["rgba"][:, 3].astype(F) + F(0.5), F(0.5), F(254.5))
    with np.errstate(all="ignore"):
        scales = np.log(p["scales"].astype(F)).astype(F)
    return dict(means=p["means"].astype(F), scales=scales, quats=((p["rot"].astype(F) + F(0.5) - F(128)) / F(128)).astype(F),
                opacities=np.log(c / (F(255) - c)).astype(F), sh=(((rgb - F(0.5)) / C0).astype(F))[:, :, None])


def ref_splat(data: bytes) -> dict:
    """fp64, from SO.decode_splat"""
    d = SO.decode_splat(data)
    c = np.clip(SO.parse_splat(data)["rgba"][:, 3] + 0.5, 0.5, 254.5)
    with np.errstate(all="ignore"):
        scales = np.log(d["scales"])
    return dict(means=d["means"], scales=scales, quats=d["quats"], opacities=np.log(c / (255 - c)), sh=((d["rgba"][:, :3] - 0.5) / SO.C0)[:, :, None])


# ------------------------------------------------------------------------------------------------------------------ bounds
def ulp32(x: np.ndarray) -> np.ndarray:
    """the spacing of fp32 at |x| (x fp64)"""
    a = np.abs(x.astype(F))
    return (np.nextafter(a, F(np.inf)) - a).astype(np.float64)


def log_bound(ref64: np.ndarray) -> np.ndarray:
    """fields through logf: 2 ulp of the fp32 result (a logf within 1 ulp, and the rounding of the comparison's own reference) plus
    1.2e-7 absolute (the argument carries 0.5 ulp = 6e-8 relative, which the log turns into an absolute error; x 2)"""
    return 2 * ulp32(ref64) + 1.2e-7


DROPPED_BOUND = 1e-6      # the reconstructed component: radicand >= ~0.25 (it is the largest), component errors a few 2^-24 each


def lerp_bound(lo, hi) -> np.ndarray:
    """lo + (hi - lo) * (code / top) in fp32 against fp64: four roundings (hi - lo, the quotient, the product: each 2^-24 of at most
    |hi - lo|; the sum: 2^-24 of at most |lo| + |hi - lo|), over-estimated as 2^-23 (|lo| + 2.5 |hi - lo|)"""
    lo, hi = np.abs(lo.astype(np.float64)), np.abs((hi.astype(np.float64) - lo.astype(np.float64)))
    return 2 * EPS * (lo + 2.5 * hi)


def sh0_bound(colour_err, rgb64) -> np.ndarray:
    """(rgb - 0.5) / C0: the colour's own error, the subtraction's and the division's rounding and C0's own (2^-24 each, of at most
    |rgb| + 0.5), all divided by C0"""
    return (colour_err + 4 * EPS * (np.abs(rgb64) + 0.5)) / SO.C0


ROT_BOUND = 6 * EPS       # (code / 1023 - 0.5) * sqrt(2): quotient, difference, sqrt(2) itself and the product, each 2^-24 of at most 1
