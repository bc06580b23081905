"""Host checks of the scene exporters: tests/splat_export_oracle.py is held byte for byte to the fixture the reference's own
exporter produced (tests/golden/splat_export_ref.safetensors), its decoders bring the compact formats back to the inputs within
half a quantisation step, the reference's own bytes pass the fp64 judge the GPU test applies to the kernels, and the host side of
vist3a_amd/utils/splat_export.py (headers, --export_format, refusals) behaves."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import splat_export_oracle as SO  # noqa: E402

CASES = tuple(SO.CASES)


@pytest.fixture(scope="module")
def fx():
    return SO.load_fixture()


def _bytes(fx, case, fmt):
    return fx[f"{case}.{fmt}"].numpy().tobytes()


@pytest.mark.parametrize("fmt", SO.FORMATS)
@pytest.mark.parametrize("case", CASES)
def test_oracle_equals_the_reference_bytes(fx, case, fmt):
    x = SO.fixture_inputs(fx, case)
    for k, v in SO.make_inputs(case).items():                # the committed inputs are the generator's
        assert torch.equal(v.view(torch.int32), x[k].view(torch.int32)), k
    assert SO.export(fmt, **x) == _bytes(fx, case, fmt)


def test_fixture_cases_are_what_they_claim(fx):
    n = {c: SO.parse_compressed(_bytes(fx, c, "ply_compressed"))["n"] for c in CASES}
    assert n["A"] == 700 - int((torch.sigmoid(fx["A.opacities"]) <= 1 / 255).sum()) and n["A"] > 512 and n["A"] % 256 != 0
    assert n["C"] == 256 and n["E"] == 1 and n["B"] % 256 == 1                     # B: the last chunk holds one splat
    assert len(_bytes(fx, "D", "splat")) == 32 * 295 and n["D"] == 295 - 30        # five NaN / Inf rows; 30 logits below the threshold
    lg = torch.cat([fx[f"{c}.opacities"] for c in CASES])
    assert float((lg[torch.isfinite(lg)] - SO.LOGIT_EDGE).abs().min()) >= 1e-2
    rows = SO.sorted_rows("splat", **SO.fixture_inputs(fx, "D"))
    tied = [int(r) for r in rows if int(r) < 50]
    groups = [tied[i:i + 5] for i in range(0, 50, 5)]
    assert all(g == sorted(g) and len({r % 10 for r in g}) == 1 for g in groups), groups   # equal means: adjacent, in row order


@pytest.mark.parametrize("case", CASES)
def test_decoders_return_the_inputs_within_half_a_step(fx, case):
    """Bounds from the formats: a b-bit unorm over [min, max] is off by at most (max - min) / (2 (2^b - 1)); a rotation component by
    sqrt(2) / (2 * 1023); a truncated harmonics byte, decoded at the middle of its bin, by 8 / 512; a .splat colour byte by 1 / 510
    and a rotation byte by 1 / 256.  Slack 1e-5 relative + 1e-6 for the fp32 arithmetic of the encoder."""
    x = SO.fixture_inputs(fx, case)
    d = SO.decode_compressed(_bytes(fx, case, "ply_compressed"))
    rows = SO.sorted_rows("ply_compressed", **x).numpy()
    assert d["n"] == rows.shape[0] and d["K"] == x["shN"].shape[1]
    b = np.repeat(d["chunks"].astype(np.float64), 256, axis=0)[:d["n"]]
    slack = lambda bound: bound * (1 + 1e-5) + 1e-6
    t3 = np.array([2047.0, 1023.0, 2047.0])
    for name, src, lo, hi, t in (("means", x["means"], b[:, 0:3], b[:, 3:6], t3), ("scales", x["scales"], b[:, 6:9], b[:, 9:12], t3),
                                 ("rgb", x["sh0"][:, 0] * SO.C0 + 0.5, b[:, 12:15], b[:, 15:18], 255.0)):
        err = np.abs(d[name] - src[rows].double().numpy())
        assert (err <= slack((hi - lo) / (2 * t))).all(), (name, err.max())
    q = x["quats"][rows].double().numpy()
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    big = np.abs(q).argmax(axis=1)
    q *= np.where(np.take_along_axis(q, big[:, None], 1) < 0, -1.0, 1.0)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[big]
    assert (d["rot_index"] == big).all()
    assert (np.abs(d["rot"] - np.take_along_axis(q, others, 1)) <= slack(np.sqrt(2) / 2046)).all()
    sig = 1 / (1 + np.exp(-x["opacities"][rows].double().numpy()))
    assert (np.abs(d["opacity"] - sig) <= slack(1 / 510)).all()
    rest = x["shN"][rows].permute(0, 2, 1).reshape(d["n"], -1).double().numpy()
    assert (np.abs(d["shN"] - rest) <= slack(8 / 512)).all()
    s = SO.decode_splat(_bytes(fx, case, "splat"))
    rows = SO.sorted_rows("splat", **x).numpy()
    assert s["n"] == rows.shape[0]
    assert np.array_equal(s["means"], x["means"][rows].double().numpy())
    assert np.allclose(s["scales"], np.exp(x["scales"][rows].double().numpy()), rtol=1e-6, atol=0)
    rgba = np.concatenate([(x["sh0"][rows, 0] * SO.C0 + 0.5).double().numpy(), 1 / (1 + np.exp(-x["opacities"][rows].double().numpy()))[:, None]], 1)
    assert (np.abs(s["rgba"] - rgba) <= slack(1 / 510)).all()
    q = x["quats"][rows].double().numpy()
    assert (np.abs(s["quats"] - q / np.linalg.norm(q, axis=1, keepdims=True)) <= slack(1 / 256)).all()


@pytest.mark.parametrize("fmt", ("splat", "ply_compressed"))
@pytest.mark.parametrize("case", CASES)
def test_reference_bytes_pass_the_fp64_judge(fx, case, fmt):
    r = SO.judge_file(fmt, _bytes(fx, case, fmt), SO.fixture_inputs(fx, case))
    print(f"[splat export judge, reference] {case} {fmt}: {r}")
    assert r["wrong"] == 0 and r["allowed"] <= SO.MAX_ALLOWANCE * r["n"] and r["scale_ulp"] <= 2


def test_judge_allows_only_the_neighbour_at_a_boundary():
    pre = np.array([5.4, 5.0004, 5.9996, 5.0004, -3.0, 300.2])
    wrong, allowed = SO.judge(np.array([5, 4, 6, 6, 0, 255]), pre, 255)
    assert wrong.tolist() == [False, False, False, True, False, False] and allowed.tolist() == [False, True, True, False, False, False]
    assert SO.judge(np.array([4]), np.array([5.4]), 255)[0].all()


@pytest.mark.parametrize("fmt", SO.FORMATS)
def test_header_text(fx, fmt):
    from vist3a_amd.utils import splat_export as E
    for case in CASES:
        data = _bytes(fx, case, fmt)
        K = fx[f"{case}.shN"].shape[1]
        if fmt == "splat":
            assert E.header(fmt, len(data) // 32, K) == b""
            continue
        head, _ = SO.split_header(data)
        n = int(next(l for l in head.decode().split("\n") if l.startswith("element vertex")).split()[-1])
        assert E.header(fmt, n, K) == head
    with pytest.raises(ValueError, match="Unsupported format"):
        E.header("png", 1, 0)


def test_export_format_argument():
    from vist3a_amd.utils import splat_export as E
    from vist3a_amd.utils.argument import inference_vist3a_argument
    base = ["--checkpoint_path", "x", "--input_texts_path", "y", "--transformer_lora_path", "z"]
    p = inference_vist3a_argument()
    known = lambda extra: p.parse_known_args(base + extra)[0]
    a = known([])
    assert a.export_format == "" and a.export_sh_rest is False and E.parse_formats(a.export_format) == ()
    a = known(["--export_format", "ply_compressed,splat", "--export_sh_rest"])
    assert E.parse_formats(a.export_format) == ("ply_compressed", "splat") and a.export_sh_rest is True
    assert E.parse_formats("splat, splat") == ("splat",)
    assert E.FILE_NAMES == {"ply_compressed": "gaussians.compressed.ply", "splat": "gaussians.splat"}
    for bad in ("ply", "png", "splat;ply_compressed"):
        with pytest.raises(ValueError, match="export_format"):
            E.parse_formats(bad)


def test_refusals_before_any_launch(fx):
    from vist3a_amd import ops
    from vist3a_amd.utils import splat_export as E
    x = SO.fixture_inputs(fx, "E")
    with pytest.raises(ValueError, match="device tensor"):
        E.export_splats(**x, format="ply")
    with pytest.raises(ValueError, match="required"):
        E.export_splats(**{**x, "quats": x["quats"][:, :3]}, format="ply")
    with pytest.raises(ValueError, match="required"):
        E.export_splats(**{**x, "sh0": x["sh0"][:, 0]}, format="ply")
    scene = dict(means=x["means"], scales=x["scales"], quats=x["quats"], opacities=x["opacities"], sh=torch.zeros(1, 3, 1))
    with pytest.raises(ValueError, match="device tensor"):
        ops.splat_export_filter(scene, quats_xyzw=False)
    with pytest.raises(ValueError, match="sh \\[U,3,K\\+1\\]"):
        ops.splat_export_filter({**scene, "sh": torch.zeros(1, 3)}, quats_xyzw=False)
    with pytest.raises(ValueError, match="Unsupported format"):
        E.export_scene(scene, "png", quats_xyzw=False)


def test_c_abi_refuses_bad_arguments():
    """the entry points return their error codes before any launch (safe without a GPU)"""
    import ctypes as C
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_splat_export_filter(None, None) == -1
    assert L.v3a_splat_export_filter_workspace_bytes(-1, 0) == -2 and L.v3a_splat_export_sort_workspace_bytes(5, -1) == -2
    assert L.v3a_splat_export_filter_workspace_bytes(257, 3) == 256 * 2 + 256
    a = lib.SplatExportArgs()
    a.U, a.K = 4, 1
    for f in (L.v3a_splat_export_filter, L.v3a_splat_export_sort, L.v3a_splat_export_pack_compressed, L.v3a_splat_export_pack_splat,
              L.v3a_splat_export_pack_ply):
        assert f(C.byref(a), None) == -1                                   # null tensors
    a.means = a.log_scales = a.quats = a.logits = a.sh = 256
    a.ld_means = a.ld_log_scales = 3
    a.ld_quats, a.ld_logits, a.ld_sh = 4, 1, 5                              # sh rows overlap: 3 (K + 1) = 6
    assert L.v3a_splat_export_filter(C.byref(a), None) == -2
    a.ld_sh, a.count, a.rows = 6, 256, 256
    assert L.v3a_splat_export_filter(C.byref(a), None) == -4                # no workspace
    a.n = 5
    assert L.v3a_splat_export_pack_splat(C.byref(a), None) == -2            # more survivors than rows
    a.n, a.order, a.out_splat = 4, 256, 8
    assert L.v3a_splat_export_pack_splat(C.byref(a), None) == -2            # output not 16-byte aligned
