"""GPU: the scene exporters (csrc/splat_export.hip through vist3a_amd/utils/splat_export.py) against the fixture the reference's own
exporter produced (tests/golden/splat_export_ref.safetensors; cases in tests/splat_export_oracle.py).

Exact: header, splat order, chunk bounds, the packed position / scale / colour fields, the harmonics bytes, the .splat means and
colours, the whole `ply` file - they are made of IEEE add / sub / mul / div, floor, min / max and clamp.  The fields that pass
through sqrt or exp (rotation codes and index, opacity codes, the .splat rotation and opacity bytes) are judged against their fp64
evaluation: equal, or the neighbouring code when the fp64 value lies within 1e-3 of a code boundary (fp32 error of a normalised
component or a sigmoid ~2e-7, x 1023 ~2e-4 of a code: a x5 margin), for at most 2 % of a case's splats.  .splat scales: within
2 ulp of fp64's exp rounded to fp32 (the device's expf and the reference's are each within 1 ulp of the true value)."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import splat_export_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = tuple(SO.CASES)


@pytest.fixture(scope="module")
def fx():
    return SO.load_fixture()


def _want(fx, case, fmt):
    return fx[f"{case}.{fmt}"].numpy().tobytes()


def _run(x, fmt):
    from vist3a_amd.utils.splat_export import export_splats
    return export_splats(**{k: v.cuda() for k, v in x.items()}, format=fmt)


def _check(fmt, got, want, x, tag):
    a, b = SO.exact_parts(fmt, got), SO.exact_parts(fmt, want)
    for k in b:
        assert a[k] == b[k], f"{tag}: {k} differs from the reference's bytes"
    assert len(got) == len(want)
    if fmt == "ply":
        return
    r = SO.judge_file(fmt, got, x)
    print(f"[splat export judge] {tag}: {r}")
    assert r["wrong"] == 0, r
    assert r["allowed"] <= SO.MAX_ALLOWANCE * r["n"], r
    assert r["scale_ulp"] <= 2, r


@pytest.mark.parametrize("fmt", SO.FORMATS)
@pytest.mark.parametrize("case", CASES)
def test_fixture(hip_lib, fx, case, fmt, tmp_path):
    x = SO.fixture_inputs(fx, case)
    got = _run(x, fmt)
    _check(fmt, got, _want(fx, case, fmt), x, f"{case} {fmt}")
    assert _run(x, fmt) == got                                                     # two runs, identical bytes


@pytest.mark.parametrize("fmt", SO.FORMATS)
def test_strided_inputs_equal_their_contiguous_copies(hip_lib, fx, fmt):
    """rows strided in every tensor (padding of NaNs between them), the trainer's layout and x y z w quaternions"""
    from vist3a_amd.utils.splat_export import export_scene
    x = SO.fixture_inputs(fx, "D")
    N, K = x["shN"].shape[:2]
    sh = torch.cat([x["sh0"], x["shN"]], dim=1).permute(0, 2, 1).contiguous()
    tight = dict(means=x["means"], scales=x["scales"], quats=x["quats"][:, [1, 2, 3, 0]].contiguous(), opacities=x["opacities"], sh=sh)
    tight = {k: v.cuda() for k, v in tight.items()}
    wide = {}
    for k, v in tight.items():
        flat = v.reshape(N, -1)
        buf = torch.full((N, flat.shape[1] + 3), float("nan"), device="cuda")
        buf[:, :flat.shape[1]] = flat
        wide[k] = buf[:, :flat.shape[1]].view(N, *v.shape[1:]) if v.dim() == 3 else (buf[:, 0] if v.dim() == 1 else buf[:, :flat.shape[1]])
        assert not wide[k].is_contiguous() and torch.equal(wide[k].nan_to_num(7.0), v.nan_to_num(7.0))
    a = export_scene(tight, fmt, quats_xyzw=True)
    assert export_scene(wide, fmt, quats_xyzw=True) == a
    _check(fmt, a, _want(fx, "D", fmt), x, f"D {fmt} xyzw")


def test_reference_signature_and_gaussians_agree(hip_lib, fx, tmp_path):
    from vist3a_amd.models.types import Gaussians
    from vist3a_amd.post_opt import export_splats_from
    from vist3a_amd.utils.splat_export import export_gaussians
    x = {k: v.cuda() for k, v in SO.fixture_inputs(fx, "A").items()}
    sh = torch.cat([x["sh0"], x["shN"]], dim=1).permute(0, 2, 1).contiguous()
    xyzw = x["quats"][:, [1, 2, 3, 0]].contiguous()
    g = Gaussians(means=x["means"][None], covariances=torch.zeros(1, 700, 3, 3, device="cuda"), harmonics=sh[None],
                  opacities=torch.sigmoid(x["opacities"])[None], scales=torch.exp(x["scales"])[None], rotations=xyzw[None])
    # the Gaussians object holds exp / sigmoid of the fixture's values: its logs and logits are the fixture's to rounding, so the
    # reference-signature call is made on exactly those
    back = dict(x, scales=torch.log(g.scales[0]), opacities=torch.logit(g.opacities[0].clamp(1e-6, 1 - 1e-6)))
    for fmt in ("ply_compressed", "splat", "ply"):
        path = tmp_path / f"a.{fmt}"
        a = export_gaussians(g, path, fmt, sh_rest=True)
        assert path.read_bytes() == a
        assert a == _run({k: v.cpu() for k, v in back.items()}, fmt), fmt
        splats = dict(params=dict(means=x["means"], scales=back["scales"], quats=xyzw, opacities=back["opacities"], sh=sh))
        assert export_splats_from(splats, fmt) == a, fmt
    dc = SO.parse_compressed(export_gaussians(g, tmp_path / "dc.ply", "ply_compressed"))
    full = SO.parse_compressed(export_gaussians(g, tmp_path / "full.ply", "ply_compressed", sh_rest=True))
    assert dc["K"] == 0 and dc["sh"].size == 0 and dc["vertices"].tobytes() == full["vertices"].tobytes()


def test_everything_filtered_gives_an_empty_file(hip_lib, fx):
    x = SO.fixture_inputs(fx, "B")
    x = dict(x, opacities=torch.full_like(x["opacities"], -9.0))
    got = _run(x, "ply_compressed")
    assert got == SO.header_compressed(0, 3)
    x = dict(x, means=torch.full_like(x["means"], float("inf")))
    assert _run(x, "splat") == b"" and _run(x, "ply") == SO.header_ply(0, 3)


@pytest.mark.parametrize("U", [257, 1])
def test_guard_bands(hip_lib, fx, U):
    """Through the C ABI with every tensor carved out of a poisoned arena and the workspaces at exactly their stated size: no byte
    outside the views changes, the inputs keep their bits, the results equal the plain calls', a short workspace is refused."""
    from vist3a_amd import lib, ops
    K = 3
    x = SO.fixture_inputs(fx, "B")
    sh = torch.cat([x["sh0"], x["shN"]], dim=1).permute(0, 2, 1).contiguous()
    tight = {k: v[:U].contiguous().cuda() for k, v in dict(means=x["means"], scales=x["scales"], quats=x["quats"], opacities=x["opacities"], sh=sh).items()}
    rows_w, count_w = ops.splat_export_filter(tight, quats_xyzw=False, opacity_threshold=1 / 255)
    n = int(count_w.item())
    assert 0 < n <= U
    order_w = ops.splat_export_sort(tight, rows_w, n, quats_xyzw=False)
    want = dict(zip(("chunks", "vertices", "sh"), ops.splat_export_pack_compressed(tight, order_w, n, quats_xyzw=False)),
                splat=ops.splat_export_pack_splat(tight, order_w, n, quats_xyzw=False), ply=ops.splat_export_pack_ply(tight, rows_w, n, quats_xyzw=False))
    p = lambda t: t.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = hip_lib
    g_in = {k: G.carve_like(v) for k, v in tight.items()}
    a = lib.SplatExportArgs()
    for field, name in zip(lib.SPLAT_FIELDS, ops.SPLAT_TENSORS):
        setattr(a, field, p(g_in[name]))
    a.ld_means, a.ld_log_scales, a.ld_quats, a.ld_logits, a.ld_sh = 3, 3, 4, 1, 3 * (K + 1)
    a.U, a.K, a.quats_xyzw, a.filter_opacity, a.opacity_threshold = U, K, 0, 1, 1 / 255
    need_f, need_s = int(L.v3a_splat_export_filter_workspace_bytes(U, K)), int(L.v3a_splat_export_sort_workspace_bytes(U, K))
    ws_f, ws_s = G.carve((need_f,), torch.uint8, device="cuda"), G.carve((need_s,), torch.uint8, device="cuda")
    rows = G.carve_like(torch.full((U,), -7, dtype=torch.int32, device="cuda"))
    count = G.carve_like(torch.full((1,), -7, dtype=torch.int64, device="cuda"))
    a.rows, a.count, a.workspace, a.workspace_bytes = p(rows), p(count), p(ws_f), need_f - 1
    assert L.v3a_splat_export_filter(C.byref(a), stream) == -4
    a.workspace_bytes = need_f
    assert L.v3a_splat_export_filter(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == n and torch.equal(rows[:n], rows_w[:n]) and bool((rows[n:] == -7).all())
    order = G.carve_like(torch.full((n,), -7, dtype=torch.int32, device="cuda"))
    a.n, a.order, a.workspace, a.workspace_bytes = n, p(order), p(ws_s), need_s - 1
    assert L.v3a_splat_export_sort(C.byref(a), stream) == -4
    a.workspace_bytes = need_s
    assert L.v3a_splat_export_sort(C.byref(a), stream) == 0
    out = {k: G.carve_like(torch.full_like(v, 3)) for k, v in want.items()}                       # every element must be WRITTEN
    a.out_chunks, a.out_vertices, a.out_sh, a.out_splat, a.out_ply = (p(out[k]) for k in ("chunks", "vertices", "sh", "splat", "ply"))
    assert L.v3a_splat_export_pack_compressed(C.byref(a), stream) == 0
    assert L.v3a_splat_export_pack_splat(C.byref(a), stream) == 0
    assert L.v3a_splat_export_pack_ply(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    views = dict(out, rows=rows, count=count, order=order, ws_filter=ws_f, ws_sort=ws_s)
    bad = {k: G.violations(v) for k, v in views.items()}
    print(f"[splat export guard] U={U} n={n} violations { {k: v[0] for k, v in bad.items()} }")
    for k, (cnt, where) in bad.items():
        assert cnt == 0, (k, cnt, where)
    for k, v in g_in.items():
        assert G.unchanged(v, tight[k]), k
    assert torch.equal(order, order_w)
    for k, v in want.items():
        assert torch.equal(G.bits(out[k]), G.bits(v)), k
