"""Host restatement of the scene exporters (csrc/splat_export.hip, vist3a_amd/utils/splat_export.py): compressed PLY, .splat, float PLY.

Written from the formats, vectorised over ALL chunks at once (the reference, post_opt/exporter.py, loops over chunks and splats);
tests/test_splat_export_host.py holds it byte for byte to tests/golden/splat_export_ref.safetensors, which the reference's own
functions produced.  fp32 on torch's CPU kernels: exp, sigmoid and the quaternion norm are torch's, as the fixture's are.

Inputs follow the reference's export_splats: means [N,3], scales (logs) [N,3], quats (w x y z) [N,4], opacities (logits) [N],
sh0 [N,1,3], shN [N,K,3]; CPU float32 tensors.

Two definitions where the reference leaves the result to the platform:
  * equal Morton keys keep ascending row index (a stable sort);
  * a channel whose max == min inside a chunk packs to 0 (the reference converts a NaN to an integer).
One deviation: a NaN / Inf opacity drops ITS row here; the reference's mask reduces the opacities over dim 0 and drops every row.

Also: the fp64 evaluation of the fields that pass through sqrt / exp (`judged_fields`, `judge`), and decoders of the two compact formats."""
from __future__ import annotations

import math

import numpy as np
import torch

C0 = 0.28209479177387814
CHUNK = 256
CHUNK_PROPS = [f"{m}_{a}" for g in (("x", "y", "z"), ("scale_x", "scale_y", "scale_z"), ("r", "g", "b")) for m in ("min", "max") for a in g]
VERTEX_PROPS = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]
FORMATS = ("ply", "splat", "ply_compressed")
BOUNDARY = 1e-3        # a judged code may be either neighbour when its fp64 pre-rounding value lies this close to a code boundary
MAX_ALLOWANCE = 0.02   # ... for at most this share of a case's splats


# ------------------------------------------------------------------------------------------------------------------ headers
def header_ply(n: int, K: int) -> bytes:
    names = ["x", "y", "z"] + [f"f_dc_{j}" for j in range(3)] + [f"f_rest_{j}" for j in range(3 * K)] + ["opacity"]
    names += [f"scale_{j}" for j in range(3)] + [f"rot_{j}" for j in range(4)]
    return ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property float {p}\n" for p in names)
            + "end_header\n").encode()


def header_compressed(n: int, K: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\n" + f"element chunk {(n + CHUNK - 1) // CHUNK}\n"
            + "".join(f"property float {p}\n" for p in CHUNK_PROPS) + f"element vertex {n}\n"
            + "".join(f"property uint {p}\n" for p in VERTEX_PROPS) + f"element sh {n}\n"
            + "".join(f"property uchar f_rest_{j}\n" for j in range(3 * K)) + "end_header\n").encode()


def split_header(data: bytes):
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end], data[end:]


# ------------------------------------------------------------------------------------------------------------------- stages
def valid_rows(means, scales, quats, opacities, sh0, shN) -> torch.Tensor:
    N = means.shape[0]
    every = torch.cat([means, scales, quats, opacities[:, None], sh0.reshape(N, -1), shN.reshape(N, -1)], dim=1)
    return torch.isfinite(every).all(dim=1)


def morton_order(means: torch.Tensor) -> torch.Tensor:
    """int64 [n]: the rows by their 30-bit Morton key, equal keys in ascending row order."""
    if means.shape[0] == 0:
        return torch.zeros(0, dtype=torch.long)
    lo, hi = means.min(dim=0).values, means.max(dim=0).values
    ln = hi - lo
    ln = torch.where(ln == 0, torch.ones_like(ln), ln)
    q = ((means - lo) / ln * 1024).floor().to(torch.int32).numpy().astype(np.int64) & 0x3FF
    key = np.zeros(means.shape[0], dtype=np.int64)
    for bit in range(10):
        for axis in range(3):
            key |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return torch.from_numpy(np.argsort(key, kind="stable"))


def _unorm(v: torch.Tensor, bits: int) -> torch.Tensor:
    t = (1 << bits) - 1
    f = (v * t + 0.5).floor()
    return torch.where(torch.isnan(f), torch.zeros_like(f), f.clamp(0, t)).to(torch.int64)


def _survivors(fmt, means, scales, quats, opacities, sh0, shN):
    keep = valid_rows(means, scales, quats, opacities, sh0, shN)
    if fmt == "ply_compressed":
        keep = keep & (torch.sigmoid(opacities) > 1 / 255)
    rows = keep.nonzero()[:, 0]
    return rows if fmt == "ply" else rows[morton_order(means[rows])]


def sorted_rows(fmt, means, scales, quats, opacities, sh0, shN) -> torch.Tensor:
    """the input rows in file order"""
    return _survivors(fmt, means, scales, quats, opacities, sh0, shN)


def pack_compressed(means, scales, quats, opacities, sh0, shN):
    """-> (chunks f32 [C,18], vertices int64 [n,4] (values < 2^32), sh uint8 [n,3K], rows)"""
    rows = _survivors("ply_compressed", means, scales, quats, opacities, sh0, shN)
    n, K = rows.shape[0], shN.shape[1]
    nch = (n + CHUNK - 1) // CHUNK
    if n == 0:
        return torch.zeros(0, 18), torch.zeros(0, 4, dtype=torch.int64), torch.zeros(0, 3 * K, dtype=torch.uint8), rows
    slot = torch.arange(nch * CHUNK)
    pad = rows[torch.where(slot < n, slot, slot // CHUNK * CHUNK)]      # a short chunk repeats its first splat: the bounds do not move
    x = torch.cat([means[pad], scales[pad], sh0[pad, 0] * C0 + 0.5], dim=1).reshape(nch, CHUNK, 9)
    lo, hi = x.amin(dim=1), x.amax(dim=1)
    lo[:, 3:6], hi[:, 3:6] = lo[:, 3:6].clamp(-20, 20), hi[:, 3:6].clamp(-20, 20)
    chunks = torch.cat([lo[:, 0:3], hi[:, 0:3], lo[:, 3:6], hi[:, 3:6], lo[:, 6:9], hi[:, 6:9]], dim=1)
    nrm = ((x - lo[:, None]) / (hi - lo)[:, None]).reshape(nch * CHUNK, 9)[:n]
    pos = _unorm(nrm[:, 0], 11) << 21 | _unorm(nrm[:, 1], 10) << 11 | _unorm(nrm[:, 2], 11)
    scl = _unorm(nrm[:, 3], 11) << 21 | _unorm(nrm[:, 4], 10) << 11 | _unorm(nrm[:, 5], 11)
    op = 1 / (1 + torch.exp(-opacities[rows]))
    col = _unorm(nrm[:, 6], 8) << 24 | _unorm(nrm[:, 7], 8) << 16 | _unorm(nrm[:, 8], 8) << 8 | _unorm(op, 8)
    q = quats[rows]
    q = q / torch.linalg.norm(q, dim=-1, keepdim=True)
    big = q.abs().argmax(dim=-1)
    q = q * torch.where(q.gather(1, big[:, None]) < 0, -1.0, 1.0)
    others = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[big]
    code = _unorm(q.gather(1, others) * (math.sqrt(2) * 0.5) + 0.5, 10)
    rot = big << 30 | code[:, 0] << 20 | code[:, 1] << 10 | code[:, 2]
    rest = shN[rows].permute(0, 2, 1).reshape(n, 3 * K)
    sh = torch.trunc((rest / 8 + 0.5) * 256).clamp(0, 255).to(torch.uint8)
    return chunks, torch.stack([pos, rot, scl, col], dim=1), sh, rows


def export(fmt, means, scales, quats, opacities, sh0, shN) -> bytes:
    K = shN.shape[1]
    if fmt == "ply_compressed":
        chunks, vertices, sh, rows = pack_compressed(means, scales, quats, opacities, sh0, shN)
        return (header_compressed(rows.shape[0], K) + chunks.numpy().astype("<f4").tobytes() + vertices.numpy().astype("<u4").tobytes()
                + sh.numpy().tobytes())
    rows = _survivors(fmt, means, scales, quats, opacities, sh0, shN)
    n = rows.shape[0]
    if fmt == "ply":
        data = torch.cat([means[rows], sh0[rows, 0], shN[rows].permute(0, 2, 1).reshape(n, 3 * K), opacities[rows, None], scales[rows],
                          quats[rows]], dim=1)
        return header_ply(n, K) + data.numpy().astype("<f4").tobytes()
    if fmt != "splat":
        raise ValueError(f"Unsupported format: {fmt}")
    rec = np.zeros((n, 32), dtype=np.uint8)
    rec[:, 0:12] = means[rows].numpy().astype("<f4").view(np.uint8).reshape(n, 12)
    rec[:, 12:24] = torch.exp(scales[rows]).numpy().astype("<f4").view(np.uint8).reshape(n, 12)
    colour = torch.cat([sh0[rows, 0] * C0 + 0.5, torch.sigmoid(opacities[rows])[:, None]], dim=1)
    rec[:, 24:28] = (colour * 255).clamp(0, 255).to(torch.uint8).numpy()
    q = quats[rows]
    rec[:, 28:32] = ((q / torch.linalg.norm(q, dim=1, keepdim=True)) * 128 + 128).clamp(0, 255).to(torch.uint8).numpy()
    return rec.tobytes()


# -------------------------------------------------------------------------------------------------------- parsing, decoding
def parse_compressed(data: bytes):
    """-> dict(header, n, K, chunks f32 [C,18], vertices u32 [n,4], sh u8 [n,3K])"""
    head, body = split_header(data)
    lines = head.decode().split("\n")
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    nch = int(next(l for l in lines if l.startswith("element chunk")).split()[-1])
    k3 = sum(l.startswith("property uchar f_rest_") for l in lines)
    assert len(body) == nch * 72 + n * 16 + n * k3, (len(body), nch, n, k3)
    chunks = np.frombuffer(body, "<f4", nch * 18).reshape(nch, 18)
    vertices = np.frombuffer(body, "<u4", n * 4, nch * 72).reshape(n, 4)
    sh = np.frombuffer(body, np.uint8, n * k3, nch * 72 + n * 16).reshape(n, k3)
    return dict(header=head, n=n, K=k3 // 3, chunks=chunks, vertices=vertices, sh=sh)


def fields_compressed(vertices: np.ndarray):
    """the bit fields of packed vertices [n,4] as int64 arrays"""
    v = vertices.astype(np.int64)
    return dict(pos=np.stack([v[:, 0] >> 21, (v[:, 0] >> 11) & 1023, v[:, 0] & 2047], 1),
                scale=np.stack([v[:, 2] >> 21, (v[:, 2] >> 11) & 1023, v[:, 2] & 2047], 1),
                rgb=np.stack([v[:, 3] >> 24, (v[:, 3] >> 16) & 255, (v[:, 3] >> 8) & 255], 1), opacity=v[:, 3] & 255,
                rot_index=v[:, 1] >> 30, rot=np.stack([(v[:, 1] >> 20) & 1023, (v[:, 1] >> 10) & 1023, v[:, 1] & 1023], 1))


def decode_compressed(data: bytes):
    """-> dict(means, scales (logs), rgb (sh0 * C0 + 0.5), opacity (linear), rot (the three stored components, the largest positive),
    rot_index, shN [n,3K]; float64), every code decoded at the value it stands for (harmonics: the middle of their truncation bin)"""
    p = parse_compressed(data)
    f = fields_compressed(p["vertices"])
    b = np.repeat(p["chunks"].astype(np.float64), CHUNK, axis=0)[:p["n"]]
    lerp = lambda lo, hi, code, t: lo + (hi - lo) * code / t
    t3 = np.array([2047.0, 1023.0, 2047.0])
    return dict(means=lerp(b[:, 0:3], b[:, 3:6], f["pos"], t3), scales=lerp(b[:, 6:9], b[:, 9:12], f["scale"], t3),
                rgb=lerp(b[:, 12:15], b[:, 15:18], f["rgb"], 255.0), opacity=f["opacity"] / 255.0,
                rot=(f["rot"] / 1023.0 - 0.5) * math.sqrt(2), rot_index=f["rot_index"], shN=((p["sh"] + 0.5) / 256 - 0.5) * 8,
                chunks=p["chunks"], n=p["n"], K=p["K"])


def parse_splat(data: bytes):
    assert len(data) % 32 == 0
    rec = np.frombuffer(data, np.uint8).reshape(-1, 32)
    return dict(n=rec.shape[0], means=rec[:, 0:12].copy().view("<f4"), scales=rec[:, 12:24].copy().view("<f4"), rgba=rec[:, 24:28], rot=rec[:, 28:32])


def decode_splat(data: bytes):
    """-> dict(means, scales (linear), rgba, quats (w x y z, unit); float64), the truncated bytes at the middle of their bins"""
    p = parse_splat(data)
    return dict(n=p["n"], means=p["means"].astype(np.float64), scales=p["scales"].astype(np.float64), rgba=(p["rgba"] + 0.5) / 255,
                quats=(p["rot"] + 0.5 - 128) / 128)


# --------------------------------------------------------------------------------------------- fp64 judge of the sqrt / exp fields
def judged_fields(fmt, rows, quats, opacities, scales):
    """fp64 PRE-ROUNDING values (in units of a code; the code is floor of it, clamped) of the fields that pass through sqrt or exp,
    for the splats `rows` in file order.  ply_compressed: rot [n,3], rot_index [n], rot_gap [n] (|largest| - |second|), opacity [n].
    splat: rot [n,4], opacity [n], scale64 [n,3] (exp in fp64)."""
    q = quats[rows].double().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    sig = 1 / (1 + np.exp(-opacities[rows].double().numpy()))
    if fmt == "splat":
        return dict(rot=q * 128 + 128, opacity=sig * 255, scale64=np.exp(scales[rows].double().numpy()))
    a = np.abs(q)
    big = a.argmax(axis=1)
    srt = np.sort(a, axis=1)
    q = q * np.where(np.take_along_axis(q, big[:, None], 1) < 0, -1.0, 1.0)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[big]
    return dict(rot=(np.take_along_axis(q, others, 1) * (math.sqrt(2) * 0.5) + 0.5) * 1023 + 0.5, rot_index=big, rot_gap=srt[:, 3] - srt[:, 2],
                opacity=sig * 255 + 0.5)


def judge(got: np.ndarray, pre: np.ndarray, top: int):
    """got: integer codes; pre: their fp64 pre-rounding values.  -> (wrong, allowed): boolean arrays.  A code is right when it is
    clamp(floor(pre), 0, top); when pre lies within BOUNDARY of an integer the code on the other side of it is `allowed`."""
    got = got.astype(np.int64)
    fl = np.floor(pre)
    want = np.clip(fl, 0, top).astype(np.int64)
    frac = pre - fl
    below = (frac < BOUNDARY) & (got == np.clip(fl - 1, 0, top))
    above = (1 - frac < BOUNDARY) & (got == np.clip(fl + 1, 0, top))
    allowed = (got != want) & (below | above)
    return (got != want) & ~allowed, allowed


# ------------------------------------------------------------------------------------------------------------------ fixtures
CASES = dict(A=(700, 24), B=(257, 3), C=(256, 0), D=(300, 8), E=(1, 2))
LOGIT_EDGE = math.log((1 / 255) / (1 - 1 / 255))


def make_inputs(case: str, seed: int = 0):
    """the inputs of a fixture case, reference signature (CPU float32)"""
    N, K = CASES[case]
    g = torch.Generator().manual_seed(1000 * seed + ord(case))
    rn = lambda *s: torch.randn(*s, generator=g)
    means = rn(N, 3) * torch.tensor([2.0, 1.0, 3.0])
    scales = (rn(N, 3) * 0.8 - 3.0).clamp(-19, 19)
    quats = rn(N, 4)
    quats[::7] *= -1
    opacities = rn(N) * 2.0 + 1.0
    sh0 = (rn(N, 1, 3) * 0.6).clamp(-1.7, 1.7)
    shN = (rn(N, K, 3) * 1.5).clamp(-3.9, 3.9)
    if case == "D":
        means[:40] = means[40:50].repeat(4, 1)                      # 40 rows on 10 distinct means: Morton ties
        opacities[60:90] = -7.0 - torch.rand(30, generator=g)       # clearly below the threshold
        opacities[90:96] = -4.0 + torch.rand(6, generator=g)        # clearly above it
        means[100, 1] = float("nan")
        scales[101, 0] = float("inf")
        quats[102, 3] = float("-inf")
        sh0[103, 0, 2] = float("nan")
        shN[104, 5, 1] = float("inf")
    near = (opacities - LOGIT_EDGE).abs() < 1e-2
    opacities[near] = LOGIT_EDGE + 0.5
    return dict(means=means, scales=scales, quats=quats, opacities=opacities, sh0=sh0, shN=shN)


# ------------------------------------------------------------------------------------------------------- comparing two files
def exact_parts(fmt: str, data: bytes) -> dict:
    """the parts of a file that are made of IEEE add / sub / mul / div, floor, min / max and clamp only: they must match bit for bit"""
    if fmt == "ply":
        return dict(file=data)
    if fmt == "splat":
        p = parse_splat(data)
        return dict(n=p["n"], means=p["means"].tobytes(), rgb=p["rgba"][:, :3].tobytes())
    p = parse_compressed(data)
    f = fields_compressed(p["vertices"])
    return dict(header=p["header"], chunks=p["chunks"].tobytes(), pos=f["pos"].tobytes(), scale=f["scale"].tobytes(), rgb=f["rgb"].tobytes(),
                sh=p["sh"].tobytes())


INDEX_GAP = 1e-6   # the largest-component index may differ from fp64's when the two largest |components| are this close: a normalised
                   # fp32 component carries ~2e-7 of error, x5 as for BOUNDARY


def judge_file(fmt: str, data: bytes, x: dict) -> dict:
    """The sqrt / exp fields of a `splat` or `ply_compressed` file against their fp64 evaluation -> dict(n, wrong, allowed (splats
    that are right only by the boundary allowance), scale_ulp (splat: the largest distance of a scale float from fp64's exp rounded
    to fp32, in ulps))."""
    rows = sorted_rows(fmt, **x)
    f = judged_fields(fmt, rows, x["quats"], x["opacities"], x["scales"])
    n = rows.shape[0]
    if fmt == "ply_compressed":
        p = fields_compressed(parse_compressed(data)["vertices"])
        assert p["rot"].shape[0] == n
        other = p["rot_index"] != f["rot_index"]
        w_rot, a_rot = judge(p["rot"], f["rot"], 1023)
        w_op, a_op = judge(p["opacity"], f["opacity"], 255)
        wrong = (other & (f["rot_gap"] >= INDEX_GAP)) | (~other & w_rot.any(axis=1)) | w_op
        allowed = ~wrong & ((other & (f["rot_gap"] < INDEX_GAP)) | (~other & a_rot.any(axis=1)) | a_op)
        return dict(n=n, wrong=int(wrong.sum()), allowed=int(allowed.sum()), scale_ulp=0)
    p = parse_splat(data)
    assert p["n"] == n
    w_rot, a_rot = judge(p["rot"], f["rot"], 255)
    w_op, a_op = judge(p["rgba"][:, 3], f["opacity"], 255)
    wrong = w_rot.any(axis=1) | w_op
    allowed = ~wrong & (a_rot.any(axis=1) | a_op)
    want = f["scale64"].astype(np.float32)
    ulp = np.abs(p["scales"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))      # positive floats: ordered as integers
    return dict(n=n, wrong=int(wrong.sum()), allowed=int(allowed.sum()), scale_ulp=int(ulp.max()) if n else 0)


def load_fixture():
    from pathlib import Path
    from safetensors.torch import load_file
    return load_file(str(Path(__file__).resolve().parent / "golden" / "splat_export_ref.safetensors"))


def fixture_inputs(fx: dict, case: str) -> dict:
    return {k: fx[f"{case}.{k}"] for k in ("means", "scales", "quats", "opacities", "sh0", "shN")}
