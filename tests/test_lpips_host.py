"""LPIPS(VGG) host side, no GPU: the weight loader (torchvision / lpips key layouts, .pth and .safetensors), its errors, the
calculate_metric.py flags, and properties of the CPU oracle."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lpips_oracle as LO  # noqa: E402


def _save(tmp_path, vgg, lin, fmt="pth"):
    from safetensors.torch import save_file
    vp, lp = tmp_path / f"vgg16.{fmt}", tmp_path / "vgg.pth"
    if fmt == "safetensors":
        save_file({k: v.contiguous() for k, v in vgg.items()}, str(vp))
    else:
        torch.save(vgg, vp)
    torch.save(lin, lp)
    return vp, lp


@pytest.mark.parametrize("fmt", ["pth", "safetensors"])
def test_loader_reads_reference_layouts(tmp_path, fmt):
    from vist3a_amd.evaluation.lpips import LPIPSWeights
    vgg, lin = LO.make_weights(seed=1)
    assert any(k.startswith("classifier.") for k in vgg)
    vp, lp = _save(tmp_path, vgg, lin, fmt)
    for cin_pad in (8, 16):
        w = LPIPSWeights.load(vp, lp, device="cpu", cin_pad=cin_pad)
        assert len(w.convs) == 13 and w.cin_pad == cin_pad
        assert w.convs[0].CinP == cin_pad and w.convs[0].Cout == 64
        assert [c.Cout for c in w.convs] == [co for _, co in LO.CHANNELS.values()]
        # the packed (hi, lo) weight is the fp32 weight, channel-padded with zeros
        c1 = w.convs[1]
        K = 9 * c1.CinP
        wp = c1.w[:, :K].float() + c1.w[:, K:2 * K].float()
        want = vgg["features.2.weight"].permute(0, 2, 3, 1).reshape(64, K)
        assert (wp - want).abs().max().item() <= 2 ** -16 * want.abs().max().item()
        assert torch.equal(c1.bias, vgg["features.2.bias"])
        assert (w.convs[0].w_halo is not None) == (cin_pad == 16)
        for k, c in enumerate(LO.LIN):
            assert w.lins[k].dtype == torch.float32 and torch.equal(w.lins[k], lin[f"lin{k}.model.1.weight"].reshape(c))


def test_loader_names_missing_and_misshaped_keys(tmp_path):
    from vist3a_amd.evaluation.lpips import LPIPSWeights
    vgg, lin = LO.make_weights(seed=2, classifier=False)
    bad = dict(vgg)
    del bad["features.12.bias"]
    vp, lp = _save(tmp_path, bad, lin)
    with pytest.raises(ValueError, match="features.12.bias"):
        LPIPSWeights.load(vp, lp, device="cpu")
    bad = dict(vgg)
    bad["features.19.weight"] = bad["features.19.weight"][:, :256]
    vp, lp = _save(tmp_path, bad, lin)
    with pytest.raises(ValueError, match="features.19.weight"):
        LPIPSWeights.load(vp, lp, device="cpu")
    bl = dict(lin)
    del bl["lin3.model.1.weight"]
    vp, lp = _save(tmp_path, vgg, bl)
    with pytest.raises(ValueError, match="lin3.model.1.weight"):
        LPIPSWeights.load(vp, lp, device="cpu")
    bl = dict(lin)
    bl["lin0.model.1.weight"] = torch.rand(1, 32, 1, 1)
    vp, lp = _save(tmp_path, vgg, bl)
    with pytest.raises(ValueError, match="lin0.model.1.weight"):
        LPIPSWeights.load(vp, lp, device="cpu")
    with pytest.raises(FileNotFoundError):
        LPIPSWeights.load(tmp_path / "nope.pth", lp, device="cpu")


def test_calculate_metric_flags():
    from vist3a_amd.evaluation.argument import calculate_metric_argument
    base = ["--dataset", f"re10k:{ROOT}", "--seq_id_map", "ids.json"]
    a = calculate_metric_argument().parse_args(base + ["--lpips_vgg_weights", "v.pth", "--lpips_lin_weights", "l.pth", "--save_suffix", "x"])
    assert (a.lpips_vgg_weights, a.lpips_lin_weights, a.save_suffix) == ("v.pth", "l.pth", "x")
    a = calculate_metric_argument().parse_args(base)
    assert a.lpips_vgg_weights is None and a.lpips_lin_weights is None
    for one in (["--lpips_vgg_weights", "v.pth"], ["--lpips_lin_weights", "l.pth"]):
        with pytest.raises(SystemExit):
            calculate_metric_argument().parse_args(base + one)


def test_metrics_main_rejects_one_weight_file(tmp_path):
    from vist3a_amd.evaluation.metrics import main
    with pytest.raises(ValueError, match="both"):
        main(str(tmp_path), lpips_vgg_weights="v.pth")


def test_oracle_zero_for_identical_and_symmetric():
    vgg, lin = LO.make_weights(seed=3)
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (2, 16, 24, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (2, 16, 24, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(LO.lpips(vgg, lin, a, a), torch.zeros(2, dtype=torch.float64))
    ab, ba = LO.lpips(vgg, lin, a, b), LO.lpips(vgg, lin, b, a)
    assert torch.allclose(ab, ba, rtol=1e-13, atol=0) and (ab > 0).all()
    # u8 NHWC and f32 NCHW give the same network input
    assert torch.equal(LO.to_input(a), LO.to_input(a.permute(0, 3, 1, 2).float() / 255))


def test_lpips_rejects_bad_images_before_any_launch():
    from vist3a_amd.evaluation.lpips import LPIPS, LPIPSWeights
    vgg, lin = LO.make_weights(seed=4)
    m = LPIPS(LPIPSWeights.from_state_dicts(vgg, lin, device="cpu"))
    for bad in (torch.zeros(1, 32, 32, 4, dtype=torch.uint8), torch.zeros(1, 32, 32, 1, dtype=torch.uint8),
                torch.zeros(1, 4, 32, 32), torch.zeros(1, 15, 32, 3, dtype=torch.uint8), torch.zeros(1, 3, 32, 8)):
        with pytest.raises(ValueError):
            m(bad, bad)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), torch.zeros(1, 3, 32, 32))
