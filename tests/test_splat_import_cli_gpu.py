"""GPU: the converter `python -m vist3a_amd.utils.splat_import` turns a fixture float PLY into a compressed PLY and a .splat that are
byte for byte what export_splats writes from the fixture's inputs (the float PLY holds those inputs' finite rows bit for bit), a
loaded scene goes through evaluate_views exactly as the same tensors handed over directly, and load_splats_into gives a trainer
state that exports to the file it came from."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import splat_export_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return SO.load_fixture()


def test_converter_equals_the_exporter(hip_lib, fx, tmp_path, capsys):
    from vist3a_amd.utils.splat_export import export_splats
    from vist3a_amd.utils.splat_import import main
    x = {k: v.cuda() for k, v in SO.fixture_inputs(fx, "D").items()}           # NaN / Inf rows, opacities under the threshold, Morton ties
    src = tmp_path / "in.ply"
    src.write_bytes(fx["D.ply"].numpy().tobytes())
    for fmt, name in (("ply_compressed", "out.compressed.ply"), ("splat", "out.splat"), ("ply", "out.ply")):
        assert main([str(src), "--out", str(tmp_path / name), "--to", fmt]) == 0
        assert (tmp_path / name).read_bytes() == export_splats(**x, format=fmt), fmt
    assert "out.ply" in capsys.readouterr().out
    assert main([str(src), "--out", str(tmp_path / "dc.splat"), "--to", "splat", "--dc_only"]) == 0
    assert (tmp_path / "dc.splat").read_bytes() == (tmp_path / "out.splat").read_bytes()      # a .splat holds the DC colour only
    assert main([str(tmp_path / "out.splat"), "--out", str(tmp_path / "back.ply"), "--to", "ply"]) == 0
    assert (tmp_path / "back.ply").read_bytes().startswith(SO.header_ply(295, 0))


def test_loaded_gaussians_evaluate_like_the_same_tensors(hip_lib, fx):
    from vist3a_amd.post_opt import evaluate_views
    from vist3a_amd.post_opt.trainer import splats_to_gaussians
    from vist3a_amd.utils.splat_import import load_gaussians
    x = SO.fixture_inputs(fx, "B")                                              # 257 splats, K = 3: degree 1
    sh = torch.cat([x["sh0"], x["shN"]], dim=1).permute(0, 2, 1).contiguous()
    direct = splats_to_gaussians(dict(params={k: v.cuda() for k, v in dict(means=x["means"], scales=x["scales"], quats=x["quats"][:, [1, 2, 3, 0]].contiguous(),
                                                                           opacities=x["opacities"], sh=sh).items()}))
    loaded = load_gaussians(fx["B.ply"].numpy().tobytes())
    for f in ("means", "covariances", "harmonics", "opacities", "scales", "rotations"):
        assert torch.equal(getattr(loaded, f).view(torch.int32), getattr(direct, f).view(torch.int32)), f
    ext = torch.eye(4)[None].clone()
    ext[0, 2, 3] = -12.0                                                        # the camera on the -z axis, looking at the origin
    Kn = torch.tensor([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]])
    images = torch.rand(1, 32, 32, 3, generator=torch.Generator().manual_seed(3)).cuda()
    a = evaluate_views(loaded, images, ext.cuda(), Kn.cuda())
    b = evaluate_views(direct, images, ext.cuda(), Kn.cuda())
    assert a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"] and a["num_GS"] == 257
    assert 0 < a["psnr"] < 60                                                   # something was rendered and compared


def test_load_splats_into_inverts_export_splats_from(hip_lib, fx):
    from vist3a_amd.post_opt import PARAM_NAMES, PostOptConfig, export_splats_from, load_splats_into
    data = fx["A.ply"].numpy().tobytes()
    splats = load_splats_into(data, PostOptConfig())
    assert splats["step"] == 0 and bool(splats["keep"].all()) and set(splats["params"]) == set(PARAM_NAMES)
    assert all(not bool(splats[m][k].any()) and splats[m][k].shape == splats["params"][k].shape for m in ("m", "v") for k in PARAM_NAMES)
    assert export_splats_from(splats, "ply") == data
