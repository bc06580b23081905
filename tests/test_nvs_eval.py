"""RE10K novel-view-synthesis evaluation, host side (no GPU): the dataset reader and its resize/crop against the reference's own
outputs, the context/target split and pose-scale alignment against the reference's `inference_nvs`, the CLI against the
reference's parser, the CSV layout, the metric ABI's argument checks, and the CPU SSIM / PSNR oracle against closed forms."""
import ctypes
import csv
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image
from safetensors.torch import load_file

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(GOLD))

import ssim_oracle as SO  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    return load_file(str(GOLD / "nvs_eval_ref.safetensors"))


@pytest.mark.parametrize("case", ["landscape", "portrait", "square", "odd"])
def test_rescale_image_w_crop_matches_reference(ref, case):
    from make_golden_nvs import CASES
    from vist3a_amd.evaluation.re10k import rescale_image_w_crop
    _, _, _, o1, o2 = next(c for c in CASES if c[0] == case)
    img = Image.fromarray(ref[f"rescale.{case}.input"].numpy())
    ff, K, vae = rescale_image_w_crop(img, ref[f"rescale.{case}.intrinsic_in"].numpy(), o1, o2)
    assert np.array_equal(np.asarray(ff), ref[f"rescale.{case}.ff"].numpy())
    assert np.array_equal(np.asarray(vae), ref[f"rescale.{case}.vae"].numpy())
    assert K.dtype == np.float32
    np.testing.assert_allclose(K, ref[f"rescale.{case}.intrinsic"].numpy(), rtol=0, atol=1e-6)


def test_split_and_scale_alignment_match_reference(ref):
    from make_golden_nvs import StubModel, nvs_inputs
    from vist3a_amd.evaluation.nvs import inference_nvs, split_views
    images, vae_images = nvs_inputs()
    target, source = split_views(len(images))
    assert target == [11, 10, 9, 8] and source == list(range(8))
    model, rec = StubModel(), {}
    inference_nvs(images, vae_images, model, target, device="cpu", record=rec)
    assert len(model.calls) == 2
    for i, c in enumerate(model.calls):            # views received by the context pass (9) and the pose pass (13)
        assert torch.equal(c["images"], ref[f"nvs.call{i}.images"])
        assert torch.equal(c["feedforward_image"], ref[f"nvs.call{i}.feedforward_image"])
    assert model.calls[0]["images"].shape[2] == 9 and model.calls[1]["images"].shape[2] == 13
    assert torch.equal(rec["scale_factor"].reshape(1), ref["nvs.scale_factor"])
    for k in ("extrinsic", "intrinsic", "near", "far"):
        assert torch.equal(model.render[k], ref[f"nvs.render.{k}"]), k
    assert model.render["shape"] == list(images.shape[-2:])   # the feed-forward size (the reference hard-codes 448 x 448)


@pytest.mark.parametrize("n", [4, 7, 10, 11, 13])
def test_split_rejects_view_counts_the_encoder_cannot_take(n):
    from vist3a_amd.evaluation.nvs import split_views
    with pytest.raises(ValueError, match="1 \\+ 4k"):
        split_views(n)


def test_cli_flags_match_reference():
    from vist3a_amd.evaluation.argument import stitching_nvs_evaluation_argument
    want = json.loads((GOLD / "nvs_cli_ref.json").read_text())["flags"]
    p = stitching_nvs_evaluation_argument()
    got = {a.option_strings[0]: a for a in p._actions if a.option_strings and a.dest != "help"}
    for flag, w in want.items():
        a = got[flag]
        d = a.default if isinstance(a.default, (str, int, float, bool, type(None))) else repr(a.default)
        assert (a.dest, d, bool(a.required), getattr(a.type, "__name__", None), type(a).__name__) == \
            (w["dest"], w["default"], w["required"], w["type"], w["action"]), flag
        assert (list(a.choices) if a.choices else None) == w["choices"], flag
    extras = set(got) - set(want)
    assert extras == {"--anysplat_weights", "--model_id", "--seq_file", "--seed", "--max_sequences", "--save_suffix"}
    assert all(not got[e].required for e in extras)


def _write_re10k(root: Path, seqs, n=5, size=(40, 24)):
    rng = np.random.default_rng(3)
    for s in seqs:
        (root / s).mkdir(parents=True)
        annos = []
        for i in range(n):
            fp = f"{s}/{i:03d}.png"
            Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(root / fp)
            annos.append(dict(idx=i, filepath=fp, intrinsics=[[30.0 + i, 0, 20], [0, 31.0, 12], [0, 0, 1]],
                              extrinsics=np.eye(4).tolist()))
        (root / s / "annotations.json").write_text(json.dumps(annos))


def test_reader_order_and_skips(tmp_path, capsys):
    from vist3a_amd.evaluation.re10k import Re10KNVSDataset, rescale_image_w_crop, to_tensor
    _write_re10k(tmp_path, ["b_seq", "a_seq", "c_seq"])
    (tmp_path / "bad_seq").mkdir()
    (tmp_path / "bad_seq" / "annotations.json").write_text("{not json")
    idmap = {"b_seq": [4, 0, 2], "bad_seq": [0], "a_seq": [1, 3, 0]}           # c_seq listed but absent from the map
    seq_file = tmp_path / "test.txt"
    seq_file.write_text("c_seq\nb_seq\nbad_seq\na_seq\nmissing\n")
    ds = Re10KNVSDataset(tmp_path, idmap, 32, 16, seq_file=str(seq_file))
    assert ds.sequence_list == ["b_seq", "a_seq"]
    assert sorted(ds.skipped_missing) == ["c_seq", "missing"] and ds.skipped_unreadable == ["bad_seq"]
    assert "skipped 3 of 5 sequences" in capsys.readouterr().out
    assert Re10KNVSDataset(tmp_path, idmap, 32, 16, verbose=False).sequence_list == ["b_seq", "a_seq"]   # map order by default
    b = ds.get_data("b_seq", idmap["b_seq"])
    assert b["ind"].tolist() == [4, 0, 2]                       # positions, in the map's order, not sorted
    assert b["images"].shape == (3, 3, 16, 16) and b["vae_images"].shape == (3, 3, 32, 32)
    for k, pos in enumerate([4, 0, 2]):
        img = Image.open(tmp_path / f"b_seq/{pos:03d}.png")
        intr = torch.tensor([[30.0 + pos, 0, 20], [0, 31.0, 12], [0, 0, 1]]).numpy()
        ff, K, vae = rescale_image_w_crop(img, intr, 32, 16)
        assert torch.equal(b["images"][k], to_tensor(ff)) and torch.equal(b["vae_images"][k], to_tensor(vae))
        assert torch.equal(b["intrs"][k], torch.from_numpy(K))
    assert float(b["images"].min()) >= 0 and float(b["images"].max()) <= 1


def test_csv_layout(tmp_path):
    from vist3a_amd.evaluation.metrics import psnr_from_mse, write_csv
    rows = [dict(seq="a", PSNR=20.5, SSIM=0.7), dict(seq="b", PSNR=21.0, SSIM=0.75)]
    write_csv(tmp_path / "_all_samples.csv", rows)
    write_csv(tmp_path / "_all_samples.csv", rows)            # rewritten, not appended
    with open(tmp_path / "_all_samples.csv") as f:
        got = list(csv.reader(f))
    assert got == [["seq", "PSNR", "SSIM"], ["a", "20.5", "0.7"], ["b", "21.0", "0.75"]]
    write_csv(tmp_path / "overall-metric.csv", [dict(PSNR=20.75, SSIM=0.725)])
    assert (tmp_path / "overall-metric.csv").read_text().splitlines() == ["PSNR,SSIM", "20.75,0.725"]
    assert psnr_from_mse(0.0) == float("inf") and psnr_from_mse(0.01) == pytest.approx(20.0)


def test_image_metrics_argument_checks_without_gpu():
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_image_metrics(None, None) == -1
    a = lib.ImageMetricsArgs()
    a.N, a.H, a.W, a.C = 2, 16, 16, 3
    assert L.v3a_image_metrics(ctypes.byref(a), None) == -1              # null image pointers
    a.a = a.b = a.ssim = a.mse = 1
    for h, w, c in ((10, 16, 3), (16, 10, 3), (16, 16, 0), (16, 16, 5)):
        a.H, a.W, a.C = h, w, c
        assert L.v3a_image_metrics(ctypes.byref(a), None) == -2, (h, w, c)
        assert L.v3a_image_metrics_workspace_bytes(2, h, w, c) == -2
    a.H, a.W, a.C = 16, 16, 3
    need = L.v3a_image_metrics_workspace_bytes(2, 16, 16, 3)
    assert need == 2 * 2 * 3 * 1 * 8                                     # one 32 x 32 tile: two fp64 partials per (pair, channel)
    assert L.v3a_image_metrics_workspace_bytes(1, 448, 448, 3) == 2 * 3 * 14 * 14 * 8
    a.workspace, a.workspace_bytes = 1, need - 1
    assert L.v3a_image_metrics(ctypes.byref(a), None) == -4
    a.workspace, a.workspace_bytes = None, need
    assert L.v3a_image_metrics(ctypes.byref(a), None) == -4


def test_oracle_closed_forms():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert SO.ssim(x, x) == 1.0 and SO.psnr(x, x) == float("inf")
    # constant images: ux, uy are the constants, variances 0 -> S = (2ab + C1) / (a^2 + b^2 + C1) everywhere
    a, b = np.full((20, 24, 3), 100, np.uint8), np.full((20, 24, 3), 180, np.uint8)
    fa, fb = np.float32(100) / np.float32(255), np.float32(180) / np.float32(255)
    want = (2 * fa * fb + 1e-4) / (fa * fa + fb * fb + 1e-4)
    assert SO.ssim(a, b) == pytest.approx(float(want), rel=1e-6)
    # a uniform offset of k levels: mse = (k / 255)^2 -> PSNR = 20 log10(255 / k)
    y = rng.integers(0, 200, (16, 16, 3), dtype=np.uint8)
    assert SO.psnr(y, y + np.uint8(7)) == pytest.approx(20 * np.log10(255 / 7), abs=1e-4)
    with pytest.raises(ValueError):
        SO.ssim(np.zeros((10, 20, 3), np.uint8), np.zeros((10, 20, 3), np.uint8))
