"""GPU: the RE10K novel-view-synthesis evaluation end to end.
  * `StitchVAE3D.predict_poses` (backbone + camera head only) is bit-identical to the poses of the full `forward`;
  * `evaluation.nvs.inference_nvs` renders what oracle/gsplat_raster renders from the HIP Gaussians at the aligned poses;
  * the two scripts (evaluation/novel_view_synthesis_bench/{nvs_eval,calculate_metric}.py) as subprocesses on reduced checkpoints in
    the reference's layouts and a synthetic RE10K-layout dataset: PNG layout, byte-identical reruns, CSVs = the oracle's scores;
  * one `--checkpoint_path synthetic` run at full size."""
import csv
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import gsplat_raster as G
from oracle import recon as R
from oracle import wan_vae as OV

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
RECON_TINY = dict(C=64, heads=1, n_dino=22, depth=24, cam_heads=2, cam_trunk=2, features=32, oc=(16, 32, 64, 64))
SPEC = "conv3d_k5x3x3_o64_s1x2x2_p2x1x1"
LORA_CFG = "r4,a8,d0.0,f0"


def _tiny_model():
    from vist3a_amd.models.anysplat_stitched import AnySplatWeights
    from vist3a_amd.models.stitched_model import StitchVAE3D
    from vist3a_amd.models.stitching_layer_builder import parse_conv_spec
    from vist3a_amd.recon.engine import ReconCfg
    from vist3a_amd.wan.vae import WanVAEConfig, WanVAEDecoder
    vcfg = OV.WanVAEConfig(base_dim=16)
    vsd = dict(OV.make_weights(vcfg, seed=5))
    vsd.update(OV.make_encoder_weights(vcfg, seed=6))
    vae = WanVAEDecoder(WanVAEConfig(base_dim=16), vsd)
    sd = R.make_recon_weights(R.ReconCfg(**RECON_TINY), seed=7)
    model = StitchVAE3D(vae, AnySplatWeights(dict(sd), ReconCfg(**RECON_TINY)), "cuda", "enc_blocks_2", parse_conv_spec(SPEC), resolution=32)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        model.stitching_layer.weight.copy_(torch.randn(64, 16, 5, 3, 3, generator=g) * 0.08)
    return model


@pytest.mark.parametrize("S", [9, 13])
def test_predict_poses_bit_identical_to_forward_reduced(hip_lib, S):
    model = _tiny_model()
    g = torch.Generator().manual_seed(S)
    images = (torch.rand(1, 3, S, 32, 32, generator=g) * 2 - 1).cuda()
    ff = (torch.rand(1, 3, S, 28, 28, generator=g) * 2 - 1).cuda()
    full = model.forward(images, ff, train=False, generator=torch.Generator().manual_seed(1)).pred_context_pose
    poses = model.predict_poses(images, ff, generator=torch.Generator().manual_seed(1))
    assert poses["extrinsic"].shape == (1, S, 4, 4) and poses["intrinsic"].shape == (1, S, 3, 3)
    assert torch.equal(poses["extrinsic"], full["extrinsic"]) and torch.equal(poses["intrinsic"], full["intrinsic"])
    # a second call (the workspace now holds a finished forward) gives the same poses
    again = model.predict_poses(images, ff, generator=torch.Generator().manual_seed(1))
    assert torch.equal(again["extrinsic"], full["extrinsic"])


def _synthetic_args(**kw):
    from vist3a_amd.evaluation.argument import stitching_nvs_evaluation_argument
    a = stitching_nvs_evaluation_argument().parse_args(["--dataset", f"re10k:{ROOT}", "--seq_id_map", "unused.json",
                                                         "--checkpoint_path", "synthetic", "--model_id", "none"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_predict_poses_bit_identical_full_width(hip_lib):
    from vist3a_amd.evaluation.nvs import load_nvs_model
    model = load_nvs_model(_synthetic_args())
    g = torch.Generator().manual_seed(4)
    images = (torch.rand(1, 3, 9, 512, 512, generator=g) * 2 - 1).cuda()
    ff = (torch.rand(1, 3, 9, 448, 448, generator=g) * 2 - 1).cuda()
    full = model.forward(images, ff, train=False, generator=torch.Generator(device="cuda").manual_seed(2)).pred_context_pose
    poses = model.predict_poses(images, ff, generator=torch.Generator(device="cuda").manual_seed(2))
    assert torch.equal(poses["extrinsic"], full["extrinsic"]) and torch.equal(poses["intrinsic"], full["intrinsic"])


def test_inference_nvs_renders_what_the_oracle_rasteriser_renders(hip_lib, parity):
    from vist3a_amd.evaluation.nvs import inference_nvs, split_views
    model = _tiny_model()
    g = torch.Generator().manual_seed(21)
    images, vae_images = torch.rand(12, 3, 28, 28, generator=g), torch.rand(12, 3, 32, 32, generator=g)
    target, _ = split_views(12)
    rec = {}
    pred = inference_nvs(images, vae_images, model, target, generator=torch.Generator().manual_seed(0), record=rec)
    assert pred.shape == (4, 3, 28, 28)
    gs = rec["gaussians"]
    means, cov = gs.means[0].float().cpu(), gs.covariances[0].float().cpu()
    sh, op = gs.harmonics[0].float().cpu(), gs.opacities[0].reshape(-1).float().cpu()
    H = W = 28
    worst = 0.0
    for j in range(4):
        c2w = rec["target_extrinsic"][0, j].float().cpu()
        w2c = torch.linalg.inv(c2w)
        K = rec["target_intrinsic"][0, j].float().cpu().clone()
        K[0] *= W
        K[1] *= H
        img, _, _ = G.rasterization(means, cov, op, sh.permute(0, 2, 1), w2c, K, W, H, sh_degree=int(math.isqrt(sh.shape[-1])) - 1,
                                    background=torch.ones(3))
        ref = img[..., :3].clamp(0, 1).permute(2, 0, 1)
        err = (pred[j].cpu() - ref).abs()
        worst = max(worst, err.mean().item())
        assert err.mean().item() < 2e-5 and (err.amax(0) < 1e-3).float().mean().item() > 0.999
    parity("nvs inference_nvs render vs oracle rasteriser", max_mean_abs=worst, tol_mean_abs=2e-5)


# ---------------------------------------------------------------- the two scripts
def _write_dataset(root: Path, seqs=("seq_a", "seq_b"), n=12):
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:360, 0:640]
    for s_i, s in enumerate(seqs):
        (root / s).mkdir(parents=True)
        annos = []
        for i in range(n):
            base = 127 + 90 * np.sin((xx + 9 * i) / (23.0 + s_i) + np.arange(3)[:, None, None]) * np.cos(yy / 31.0)
            img = np.clip(base.transpose(1, 2, 0) + rng.normal(0, 8, (360, 640, 3)), 0, 255).astype(np.uint8)
            fp = f"{s}/{i:05d}.png"
            Image.fromarray(img).save(root / fp)
            annos.append(dict(idx=i, filepath=fp, intrinsics=[[300.0, 0, 320], [0, 300.0, 180], [0, 0, 1]],
                              extrinsics=np.eye(4).tolist()))
        (root / s / "annotations.json").write_text(json.dumps(annos))
    idmap = {s: [int(v) for v in rng.permutation(n)] for s in seqs}
    (root / "indexmap.json").write_text(json.dumps(idmap, indent=1))
    return root / "indexmap.json"


def _assets(tmp: Path):
    from safetensors.torch import load_file, save_file
    from test_cli_gpu import _write_assets
    a = _write_assets(tmp)
    vae = a.model / "vae" / "diffusion_pytorch_model.safetensors"
    sd = load_file(str(vae))
    sd.update({k: v.contiguous() for k, v in OV.make_encoder_weights(OV.WanVAEConfig(base_dim=16), seed=6).items()})
    save_file(sd, str(vae))
    return a


def _run(script: str, args, timeout=900):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    return subprocess.run([sys.executable, str(ROOT / "evaluation" / "novel_view_synthesis_bench" / script), *map(str, args)],
                          capture_output=True, text=True, env=env, timeout=timeout, cwd=str(ROOT))


def test_nvs_scripts_on_reference_layout_checkpoints(hip_lib, tmp_path, parity):
    a = _assets(tmp_path)
    data = tmp_path / "re10k"
    idmap = _write_dataset(data)
    common = ["--dataset", f"re10k:{data}", "--seq_id_map", idmap]
    model = ["--model_id", a.model, "--anysplat_weights", a.snap, "--checkpoint_path", a.ckpt, "--stitching_layer_config", SPEC,
             "--lora_config", LORA_CFG, "--resolution", 32, "--feedforward_resolution", 28, "--seed", 5]
    outs = [tmp_path / "out1", tmp_path / "out2"]
    for out in outs:
        r = _run("nvs_eval.py", common + model + ["--output_dir", out])
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.count("pose pass") == 2, r.stdout
    for seq in ("seq_a", "seq_b"):
        for kind in ("gt", "pred"):
            names = sorted(os.listdir(outs[0] / "images" / seq / kind))
            assert names == [f"{i:06d}.png" for i in range(4)]
            for nme in names:
                p0, p1 = outs[0] / "images" / seq / kind / nme, outs[1] / "images" / seq / kind / nme
                assert Image.open(p0).size == (28, 28) and Image.open(p0).mode == "RGB"
                assert p0.read_bytes() == p1.read_bytes(), (seq, kind, nme)
    r = _run("calculate_metric.py", common + ["--output_dir", outs[0]])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "LPIPS not computed" in r.stdout and "PSNR" in r.stdout
    import ssim_oracle as SO
    with open(outs[0] / "_all_samples.csv") as f:
        rows = list(csv.DictReader(f))
    assert [r_["seq"] for r_ in rows] == ["seq_a", "seq_b"] and list(rows[0]) == ["seq", "PSNR", "SSIM"]
    per_seq = []
    worst_s = worst_p = 0.0
    for row in rows:
        d = outs[0] / "images" / row["seq"]
        ps, ss = [], []
        for i in range(4):
            gt = np.asarray(Image.open(d / "gt" / f"{i:06d}.png"))
            pr = np.asarray(Image.open(d / "pred" / f"{i:06d}.png"))
            ps.append(SO.psnr(pr, gt))
            ss.append(SO.ssim(pr, gt))
        per_seq.append((np.mean(ps), np.mean(ss)))
        worst_p, worst_s = max(worst_p, abs(float(row["PSNR"]) - per_seq[-1][0])), max(worst_s, abs(float(row["SSIM"]) - per_seq[-1][1]))
        assert abs(float(row["PSNR"]) - per_seq[-1][0]) <= 1e-4 and abs(float(row["SSIM"]) - per_seq[-1][1]) <= 1e-5
    with open(outs[0] / "overall-metric.csv") as f:
        (overall,) = list(csv.DictReader(f))
    assert abs(float(overall["PSNR"]) - np.mean([p for p, _ in per_seq])) <= 1e-4
    assert abs(float(overall["SSIM"]) - np.mean([s for _, s in per_seq])) <= 1e-5
    parity("nvs calculate_metric.py vs oracle", max_abs_dssim=worst_s, max_abs_dpsnr_db=worst_p)


def test_nvs_eval_synthetic_full_size(hip_lib, tmp_path):
    data = tmp_path / "re10k"
    idmap = _write_dataset(data, seqs=("seq_a",))
    out = tmp_path / "out"
    r = _run("nvs_eval.py", ["--dataset", f"re10k:{data}", "--seq_id_map", idmap, "--checkpoint_path", "synthetic", "--model_id", "none",
                             "--output_dir", out, "--max_sequences", 1])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "encode+forward" in r.stdout and "render" in r.stdout
    for kind in ("gt", "pred"):
        names = sorted(os.listdir(out / "images" / "seq_a" / kind))
        assert names == [f"{i:06d}.png" for i in range(4)]
        assert Image.open(out / "images" / "seq_a" / kind / names[0]).size == (448, 448)
    print(r.stdout)
