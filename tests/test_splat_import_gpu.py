"""GPU: the scene import (csrc/splat_import.hip through vist3a_amd/utils/splat_import.py) on the files the reference's own exporter
wrote (tests/golden/splat_export_ref.safetensors; cases A-E of tests/splat_export_oracle.py: 700/K24, 257/K3, 256/K0, 300/K8, 1/K2 -
odd and even chunk counts, an odd 3K, a last chunk of one splat, a single-splat file).

Exact (bit-equal to the fp32 twin of tests/splat_import_oracle.py): means, the compressed log-scales, every harmonics entry, the
float PLY's copies, the three stored quaternion components, the .splat quaternions - IEEE add / sub / mul / div only.
Through logf (logits, the .splat log-scales), against the fp64 decode: 2 ulp of the fp32 result + 1.2e-7 (a logf within 1 ulp on an
argument carrying 0.5 ulp).  The reconstructed quaternion component, against fp64: 1e-6 (radicand >= ~0.25, component errors a few
2^-24).  The logits of a `linear` float PLY (gaussians.ply) pass through logf too and are held to the same logf bound."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import splat_export_oracle as SO  # noqa: E402
import splat_import_oracle as IO  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = tuple(SO.CASES)
FIELDS = ("means", "scales", "quats", "opacities", "sh")


@pytest.fixture(scope="module")
def fx():
    return SO.load_fixture()


def _bytes(fx, case, fmt):
    return fx[f"{case}.{fmt}"].numpy().tobytes()


def _load(data, **kw):
    from vist3a_amd.utils.splat_import import load_scene
    kw.setdefault("quats_xyzw", False)
    return {k: v.cpu().numpy() for k, v in load_scene(data, **kw).items()}


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _judge(fmt, got, data, tag):
    """the contract of the module docstring; prints the measured maxima"""
    if fmt == "ply":
        t = IO.twin_ply(data)
        for k in FIELDS:
            assert _same(got[k], t[k]), f"{tag}: {k} is not the file's floats"
        return
    t, r = (IO.twin_compressed(data), IO.ref_compressed(data)) if fmt == "ply_compressed" else (IO.twin_splat(data), IO.ref_splat(data))
    err = lambda k: np.abs(got[k].astype(np.float64) - r[k])
    assert _same(got["means"], t["means"]) and _same(got["sh"], t["sh"]), tag
    logit = err("opacities") / IO.log_bound(r["opacities"])
    if fmt == "splat":
        assert _same(got["quats"], t["quats"]), tag
        scale = err("scales") / IO.log_bound(r["scales"])
        print(f"[splat import] {tag}: logit err {err('opacities').max():.3g} ({logit.max():.2f} of its bound), log-scale err "
              f"{err('scales').max():.3g} ({scale.max():.2f} of its bound), logits equal to the twin's: {_same(got['opacities'], t['opacities'])}")
        assert (scale <= 1).all(), (tag, scale.max())
    else:
        assert _same(got["scales"], t["scales"]), tag
        stored = np.arange(4)[None, :] != r["rot_index"][:, None]
        assert np.array_equal(got["quats"][stored].view(np.int32), t["quats"][stored].view(np.int32)), tag
        dropped = err("quats")[~stored]
        print(f"[splat import] {tag}: logit err {err('opacities').max():.3g} ({logit.max():.2f} of its bound), dropped component err "
              f"{dropped.max():.3g} (bound {IO.DROPPED_BOUND}), min dropped {got['quats'][~stored].min():.3f}")
        assert (dropped <= IO.DROPPED_BOUND).all(), (tag, dropped.max())
    assert (logit <= 1).all(), (tag, logit.max())


@pytest.mark.parametrize("fmt", SO.FORMATS)
@pytest.mark.parametrize("case", CASES)
def test_fixture(hip_lib, fx, case, fmt):
    data = _bytes(fx, case, fmt)
    got = _load(data)
    n, K = got["means"].shape[0], 0 if fmt == "splat" else SO.CASES[case][1]
    assert got["sh"].shape == (n, 3, K + 1) and got["quats"].shape == (n, 4) and got["opacities"].shape == (n,)
    _judge(fmt, got, data, f"{case} {fmt}")


@pytest.mark.parametrize("fmt", SO.FORMATS)
def test_quats_order_and_determinism(hip_lib, fx, fmt):
    data = _bytes(fx, "A", fmt)
    wxyz, xyzw, again = _load(data), _load(data, quats_xyzw=True), _load(data)
    assert _same(xyzw["quats"], np.ascontiguousarray(wxyz["quats"][:, [1, 2, 3, 0]]))
    for k in FIELDS:
        assert _same(wxyz[k], again[k]), k
        if k != "quats":
            assert _same(wxyz[k], xyzw[k]), k


@pytest.mark.parametrize("case", CASES)
def test_float_ply_round_trip_is_byte_exact(hip_lib, fx, case):
    from vist3a_amd.utils.splat_export import export_splats
    from vist3a_amd.utils.splat_import import load_scene
    data = _bytes(fx, case, "ply")
    s = load_scene(data, quats_xyzw=False)
    sh0, shN = s["sh"][:, :, :1].permute(0, 2, 1).contiguous(), s["sh"][:, :, 1:].permute(0, 2, 1).contiguous()
    assert export_splats(s["means"], s["scales"], s["quats"], s["opacities"], sh0, shN, "ply") == data


def test_own_gaussians_ply(hip_lib, tmp_path):
    """utils/ply_export.py's file: nx ny nz columns, linear opacities"""
    from vist3a_amd.utils.ply_export import export_ply
    from vist3a_amd.utils.splat_import import load_gaussians_ply, parse_header
    g = torch.Generator().manual_seed(5)
    U, K = 300, 3
    op = torch.rand(U, generator=g)
    op[:4] = torch.tensor([0.0, 1.0, 1e-7, 1 - 1e-8])
    path = tmp_path / "gaussians.ply"
    export_ply(torch.randn(U, 3, generator=g), torch.rand(U, 3, generator=g) * 0.1 + 0.01, torch.randn(U, 4, generator=g),
               torch.randn(U, 3, K + 1, generator=g), op, path, save_sh_dc_only=False)
    data = path.read_bytes()
    fmt, n, k, table, _ = parse_header(data)
    assert (fmt, n, k, table["P"]) == ("ply", U, K, 17 + 3 * K) and table["f_dc_0"] == 6
    got, t = _load(data, opacity="linear"), IO.twin_ply(data, opacity="linear")
    for k in ("means", "scales", "quats", "sh"):
        assert _same(got[k], t[k]), k
    rows, names = IO.ply_columns(data)
    ref = IO.logit_linear64(rows[:, names.index("opacity")])
    err = np.abs(got["opacities"].astype(np.float64) - ref) / IO.log_bound(ref)
    print(f"[splat import] gaussians.ply: logit err {err.max():.2f} of its bound, equal to the twin's: {_same(got['opacities'], t['opacities'])}")
    assert (err <= 1).all() and np.isfinite(got["opacities"]).all()
    gs = load_gaussians_ply(path)
    assert tuple(gs.means.shape) == (1, U, 3) and tuple(gs.harmonics.shape) == (1, U, 3, K + 1) and tuple(gs.covariances.shape) == (1, U, 3, 3)
    assert torch.equal(gs.means[0].cpu(), torch.from_numpy(t["means"]))
    assert torch.allclose(gs.opacities[0].cpu(), op.clamp(1e-6, 1 - 1e-6), atol=1e-6, rtol=0)
    assert torch.allclose(gs.scales[0].cpu(), torch.from_numpy(np.exp(t["scales"])), rtol=1e-6)
    assert torch.allclose(gs.rotations[0].norm(dim=-1).cpu(), torch.ones(U), atol=1e-6)


def test_compressed_round_trip_of_a_large_scene(hip_lib):
    """70 001 splats, fewer after the opacity filter: every decoded value within half a quantisation step of the
    exporter's input, the step from the chunk bounds in the file as tests/test_splat_export_host.py derives it"""
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_export import OPACITY_THRESHOLD, export_scene
    g = torch.Generator().manual_seed(11)
    U, K = 70001, 3
    rn = lambda *s: torch.randn(*s, generator=g)
    scene = dict(means=rn(U, 3) * torch.tensor([2.0, 1.0, 3.0]), scales=(rn(U, 3) * 0.8 - 3).clamp(-19, 19), quats=rn(U, 4),
                 opacities=rn(U) * 2 + 1, sh=torch.cat([(rn(U, 3, 1) * 0.6).clamp(-1.7, 1.7), (rn(U, 3, K) * 1.5).clamp(-3.9, 3.9)], dim=2))
    dev = {k: v.cuda() for k, v in scene.items()}
    data = export_scene(dev, "ply_compressed", quats_xyzw=True)
    rows, count = ops.splat_export_filter(dev, quats_xyzw=True, opacity_threshold=OPACITY_THRESHOLD)
    n = int(count.item())
    order = ops.splat_export_sort(dev, rows, n, quats_xyzw=True).cpu().long()
    got = _load(data, quats_xyzw=True)
    assert got["means"].shape[0] == n and 0 < n < U
    src = {k: v[order].double().numpy() for k, v in scene.items()}
    b = np.repeat(SO.parse_compressed(data)["chunks"].astype(np.float64), 256, axis=0)[:n]
    slack = lambda bound: bound * (1 + 1e-5) + 1e-6
    t3 = np.array([2047.0, 1023.0, 2047.0])
    lo, hi = b[:, 0:3], b[:, 3:6]
    edge = IO.lerp_bound(lo, hi)                                   # the fp32 lerp may round a top code past its bound by this much
    m = got["means"].astype(np.float64)
    outside = int(((m < lo) | (m > hi)).sum())
    print(f"[splat import] round trip: {n} of {U} splats, {outside} means outside their chunk's bounds by rounding")
    assert (m >= lo - edge).all() and (m <= hi + edge).all()
    assert (np.abs(m - src["means"]) <= slack((hi - lo) / (2 * t3))).all()
    assert (np.abs(got["scales"] - src["scales"]) <= slack((b[:, 9:12] - b[:, 6:9]) / (2 * t3))).all()
    rgb = got["sh"][:, :, 0].astype(np.float64) * SO.C0 + 0.5
    assert (np.abs(rgb - (src["sh"][:, :, 0] * SO.C0 + 0.5)) <= slack((b[:, 15:18] - b[:, 12:15]) / 510)).all()
    assert (np.abs(got["sh"][:, :, 1:] - src["sh"][:, :, 1:]) <= slack(8 / 512)).all()
    sig = lambda x: 1 / (1 + np.exp(-x))
    assert (np.abs(sig(got["opacities"].astype(np.float64)) - sig(src["opacities"])) <= slack(1 / 510)).all()
    q = src["quats"] / np.linalg.norm(src["quats"], axis=1, keepdims=True)
    wxyz = q[:, [3, 0, 1, 2]]
    big = np.abs(wxyz).argmax(axis=1)
    q = q * np.where(np.take_along_axis(wxyz, big[:, None], 1) < 0, -1.0, 1.0)
    qerr = np.abs(got["quats"] - q)
    stored = np.arange(4)[None, :] != ((big + 3) % 4)[:, None]      # w x y z index -> its x y z w place
    assert (qerr[stored] <= slack(np.sqrt(2) / 2046)).all()
    # d sqrt(1 - sum v^2) = sum |v_i| dv_i / dropped <= 3 dv (the dropped one is the largest), second order below 3e-6
    assert (qerr[~stored] <= 3 * slack(np.sqrt(2) / 2046) + 3e-6).all()


def test_bad_rows_are_counted(hip_lib, fx):
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_import import load_scene, parse_header
    data = bytearray(_bytes(fx, "B", "ply"))
    fmt, n, K, table, off = parse_header(bytes(data))
    row, colm = 130, table["f_rest_0"] + 4
    at = off + 4 * (row * table["P"] + colm)
    data[at:at + 4] = np.array([np.inf], "<f4").tobytes()
    with pytest.raises(ValueError, match="1 of the 257 splats"):
        load_scene(bytes(data))
    s = load_scene(bytes(data), strict=False)
    assert s["means"].shape[0] == n and int((~torch.isfinite(s["sh"])).sum()) == 1 and bool(torch.isinf(s["sh"][row, 1, 2]))
    payload = torch.from_numpy(np.frombuffer(bytes(data), np.uint8)[off:].copy()).cuda()
    assert int(ops.splat_import_ply(payload, n, K, table)[1].item()) == 1
    data = bytearray(_bytes(fx, "A", "splat"))
    n = len(data) // 32
    data[32 * 300 + 16:32 * 300 + 20] = np.array([0.0], "<f4").tobytes()       # scale_1 of splat 300
    with pytest.raises(ValueError, match=f"1 of the {n} splats"):
        load_scene(bytes(data))
    s = load_scene(bytes(data), strict=False)
    assert s["scales"].shape[0] == n and bool(torch.isinf(s["scales"][300, 1])) and int((~torch.isfinite(s["scales"])).sum()) == 1
    assert int(ops.splat_import_splat(torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda(), n)[1].item()) == 1
    data[32 * 600 + 12:32 * 600 + 16] = np.array([-1.0], "<f4").tobytes()      # and a negative one, elsewhere: two rows
    with pytest.raises(ValueError, match=f"2 of the {n} splats"):
        load_scene(bytes(data))


def test_empty_files(hip_lib):
    from vist3a_amd.utils.splat_import import load_scene
    for data, K in ((SO.header_ply(0, 2), 2), (SO.header_compressed(0, 1), 1), (b"", 0)):
        s = load_scene(data)
        assert tuple(s["means"].shape) == (0, 3) and tuple(s["sh"].shape) == (0, 3, K + 1) and tuple(s["opacities"].shape) == (0,)
        assert all(v.is_cuda and v.dtype == torch.float32 for v in s.values())


@pytest.mark.parametrize("fmt", SO.FORMATS)
def test_strides_and_guard_bands(hip_lib, fx, fmt):
    """The payload 4 bytes off alignment inside a poisoned arena, the outputs strided views of poisoned arenas: the result equals the
    tight run bit for bit (a poison byte read as data, or an element left unwritten, would show), nothing outside the views is
    written, the payload keeps its bits, and a payload one byte short is refused."""
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_import import parse_header
    data = _bytes(fx, "B", fmt)                                    # 257 rows (ply, splat) / an odd 3K and a last chunk of one (compressed)
    _, n, K, table, off = parse_header(data)
    tight_payload = torch.from_numpy(np.frombuffer(data, np.uint8)[off:].copy()).cuda()
    call = {"ply": lambda p, **kw: ops.splat_import_ply(p, n, K, table, quats_xyzw=False, **kw),
            "ply_compressed": lambda p, **kw: ops.splat_import_compressed(p, n, K, quats_xyzw=False, **kw),
            "splat": lambda p, **kw: ops.splat_import_splat(p, n, quats_xyzw=False, **kw)}[fmt]
    want, bad_w = call(tight_payload)
    payload = G.carve_like(tight_payload, offset_bytes=4)
    assert payload.data_ptr() % 256 == 4
    W = 3 * (K + 1)
    carved = dict(means=G.carve((n, 3), torch.float32, ld=5, device="cuda"), scales=G.carve((n, 3), torch.float32, ld=4, device="cuda"),
                  quats=G.carve((n, 4), torch.float32, ld=7, device="cuda"), opacities=G.carve((n, 1), torch.float32, ld=2, device="cuda"),
                  sh=G.carve((n, 3, K + 1), torch.float32, strides=(W + 3, K + 1, 1), device="cuda"))
    out = dict(carved, opacities=carved["opacities"][:, 0])
    got, bad = call(payload, out=out)
    torch.cuda.synchronize()
    assert int(bad.item()) == int(bad_w.item()) == 0
    for k in FIELDS:
        assert got[k].data_ptr() == out[k].data_ptr() and not (n > 1 and got[k].is_contiguous())
        assert torch.equal(G.bits(got[k]), G.bits(want[k])), k
        cnt, where = G.violations(carved[k])
        assert cnt == 0, (k, cnt, where)
    assert G.unchanged(payload, tight_payload)
    with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
        call(payload[:-1])


def _wide(t, pad):
    """t's values in a view whose rows lie `pad` floats further apart than they need to, NaNs between them"""
    flat = t.reshape(t.shape[0], -1)
    buf = torch.full((flat.shape[0], flat.shape[1] + pad), float("nan"), device=t.device)
    buf[:, :flat.shape[1]] = flat
    return buf[:, 0] if t.dim() == 1 else buf[:, :flat.shape[1]].view(t.shape)


def _export_then_import(scene, xyzw, pads):
    """every format packed from `scene` and decoded again, the decoders' outputs `pads` floats wider than their rows (None: fresh
    contiguous tensors) -> {format: scene dict}"""
    from vist3a_amd import ops
    U, K = scene["means"].shape[0], scene["sh"].shape[2] - 1
    out = lambda k: None if pads is None else {name: _wide(torch.zeros((U,) + inner, device="cuda"), pad)
                                               for (name, inner), pad in zip(ops._splat_inner(k + 1).items(), pads)}
    rows, count = ops.splat_export_filter(scene, quats_xyzw=xyzw)
    assert int(count.item()) == U
    order = ops.splat_export_sort(scene, rows, U, quats_xyzw=xyzw)
    flat = lambda *ts: torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for t in ts])
    cols = (0, 1, 2, 3, 4, 5, 6) + tuple(6 + 3 * K + j for j in range(8))
    table = dict(zip(ops.PLY_COLUMNS, cols), P=14 + 3 * K)
    got = {"ply": ops.splat_import_ply(flat(ops.splat_export_pack_ply(scene, rows, U, quats_xyzw=xyzw)), U, K, table, quats_xyzw=xyzw, out=out(K)),
           "ply_compressed": ops.splat_import_compressed(flat(*ops.splat_export_pack_compressed(scene, order, U, quats_xyzw=xyzw)), U, K,
                                                         quats_xyzw=xyzw, out=out(K)),
           "splat": ops.splat_import_splat(flat(ops.splat_export_pack_splat(scene, order, U, quats_xyzw=xyzw)), U, quats_xyzw=xyzw, out=out(0))}
    assert all(int(bad.item()) == 0 for _, bad in got.values())
    return {fmt: s for fmt, (s, _) in got.items()}


@pytest.mark.parametrize("xyzw", [False, True])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("U", [1, 257])
def test_strided_round_trip_equals_the_contiguous_one(hip_lib, U, K, xyzw):
    """Export then import with every tensor of both a strided view (a different stride above the width for each), against the same
    round trip through contiguous tensors: bit for bit, in all three formats.  A stride or a field taken from the wrong slot of the
    kernels' shared view shows here; the float PLY, a copy, must also return the scene itself."""
    from vist3a_amd import ops
    assert FIELDS == ops.SPLAT_TENSORS
    g = torch.Generator().manual_seed(100 * U + 10 * K + xyzw)
    rn = lambda *s: torch.randn(*s, generator=g)
    tight = {k: v.cuda() for k, v in dict(means=rn(U, 3), scales=rn(U, 3) * 0.5 - 2, quats=rn(U, 4), opacities=rn(U), sh=rn(U, 3, K + 1)).items()}
    wide = {k: _wide(v, pad) for (k, v), pad in zip(tight.items(), (2, 1, 3, 1, 5))}
    assert all(U == 1 or not v.is_contiguous() for v in wide.values())
    want, got = _export_then_import(tight, xyzw, None), _export_then_import(wide, xyzw, (4, 2, 1, 3, 2))
    for fmt in SO.FORMATS:
        for k in FIELDS:
            assert U == 1 or not got[fmt][k].is_contiguous()
            assert torch.equal(G.bits(got[fmt][k]), G.bits(want[fmt][k])), (fmt, k)
    for k in FIELDS:
        assert torch.equal(G.bits(got["ply"][k]), G.bits(tight[k])), k
