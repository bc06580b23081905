"""GPU: LPIPS(VGG) (vist3a_amd.evaluation.lpips; csrc/lpips.hip + the split convolutions) against the float64 CPU restatement
tests/lpips_oracle.py, on seeded He-scaled VGG-16 weights and non-negative lin weights in the reference's key layouts.

Gate: |gpu - oracle| <= GATE per pair.  Measured on MI355X: max 6.4e-9 (448x448, halo form), 5.0e-9 (50x70, implicit GEMM and floor
pooling), 1.0e-8 (16x16 minimum), 1.1e-8 (the CLI's per-sequence means) on values of 0.005-0.01, i.e. about 2e-6 relative; the gate
is set at about twice the largest.
Exact properties: identical pairs give 0.0, LPIPS(a, b) == LPIPS(b, a) bitwise, reruns are bit-identical, a pair scores the same alone
and inside a batch of five, and uint8 NHWC / f32 NCHW inputs of the same pixels agree bitwise.  The CLI test runs calculate_metric.py
with the two weight files and checks the reference's three-column CSVs."""
import csv
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lpips_oracle as LO  # noqa: E402

GATE = 2.5e-8


@pytest.fixture(scope="module")
def weights():
    return LO.make_weights(seed=11)


@pytest.fixture(scope="module")
def model(hip_lib, weights):
    from vist3a_amd.evaluation.lpips import LPIPS, LPIPSWeights
    return LPIPS(LPIPSWeights.from_state_dicts(*weights, device="cuda"))


def smooth(H, W, seed=0):
    """uint8 [H,W,3]: a few low-frequency sinusoids per channel"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    chans = []
    for _ in range(3):
        f = torch.rand(4, generator=g) * 0.15 + 0.01
        p = torch.rand(4, generator=g) * 6.28
        v = 0.5 + 0.12 * (torch.sin(f[0] * x + p[0]) + torch.sin(f[1] * y + p[1]) + torch.sin(f[2] * (x + y) + p[2])
                          + torch.sin(f[3] * (x - y) + p[3]))
        chans.append(v)
    return (torch.stack(chans, -1).clamp(0, 1) * 255).round().to(torch.uint8)


def variants(img, seed=1):
    """noisy, shifted and blurred copies of an image"""
    g = torch.Generator().manual_seed(seed)
    f = img.float()
    noisy = (f + torch.randn(f.shape, generator=g) * 12).clamp(0, 255).round().to(torch.uint8)
    shifted = torch.roll(img, shifts=(2, 3), dims=(0, 1))
    k = torch.ones(1, 1, 5, 5) / 25
    blurred = torch.nn.functional.conv2d(f.permute(2, 0, 1)[:, None], k, padding=2)[:, 0].permute(1, 2, 0).round().to(torch.uint8)
    return [noisy, shifted, blurred]


def pairs(H, W, n):
    base = smooth(H, W)
    v = variants(base)
    pred = torch.stack([v[i % 3] for i in range(n)])
    gt = base[None].expand(n, H, W, 3).contiguous()
    return pred, gt


@pytest.mark.parametrize("H,W,n", [(448, 448, 2), (50, 70, 3), (16, 16, 2)])
def test_lpips_matches_fp64_oracle(model, weights, parity, H, W, n):
    pred, gt = pairs(H, W, n)
    got = model(pred.cuda(), gt.cuda()).cpu()
    want = LO.lpips(*weights, pred, gt)
    assert got.dtype == torch.float64 and got.shape == (n,)
    err = (got - want).abs().max().item()
    parity(f"lpips vs fp64 oracle {H}x{W}", max_abs_err=err, value_min=want.min().item(), value_max=want.max().item())
    assert (want > 1e-3).all()
    assert err <= GATE, (got, want)


def test_lpips_exact_properties(model):
    H, W = 224, 224   # halo form at 224^2, implicit GEMM from 112^2 on
    pred, gt = pairs(H, W, 5)
    p, q = pred.cuda(), gt.cuda()
    ab = model(p, q)
    assert torch.equal(model(q, q), torch.zeros(5, dtype=torch.float64, device="cuda"))
    assert torch.equal(model(q, p), ab)
    assert torch.equal(model(p, q), ab)
    for i in (0, 3):
        assert torch.equal(model(p[i: i + 1], q[i: i + 1]), ab[i: i + 1])
    pf = (pred.permute(0, 3, 1, 2).float() / 255).cuda()
    qf = (gt.permute(0, 3, 1, 2).float() / 255).cuda()
    assert torch.equal(model(pf, qf), ab)
    # chunked scoring (one pair per chunk) gives the same values
    from vist3a_amd.evaluation.lpips import LPIPS
    small = LPIPS(model.w, max_bytes=1)
    assert torch.equal(small(p, q), ab)


def test_lpips_rejects_bad_inputs(model):
    ok = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros(1, 32, 32, 4, dtype=torch.uint8, device="cuda"), torch.zeros(1, 32, 32, 1, dtype=torch.uint8, device="cuda"),
                torch.zeros(1, 15, 40, 3, dtype=torch.uint8, device="cuda"), torch.zeros(1, 3, 40, 12, device="cuda")):
        with pytest.raises(ValueError):
            model(bad, bad)
    with pytest.raises(ValueError):
        model(ok, torch.zeros(1, 32, 32, 4, dtype=torch.uint8, device="cuda"))
    from vist3a_amd import lib, ops
    x = torch.zeros(2, 2, 8, 8, 24, dtype=torch.bfloat16, device="cuda")   # 24 channels: not 8 * 2^k
    with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
        ops.lpips_head(x, torch.zeros(24, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
    assert lib.load().v3a_lpips_head_workspace_bytes(1, 4, 4, 24) == -2


def _write_images(root: Path):
    seqs = {"seq_a": (28, 28, 4), "seq_b": (28, 28, 3), "seq_c": (64, 64, 2)}
    for k, (seq, (H, W, n)) in enumerate(seqs.items()):
        base = smooth(H, W, seed=k)
        v = variants(base, seed=k + 5)
        for kind in ("gt", "pred"):
            (root / "images" / seq / kind).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(base.numpy()).save(root / "images" / seq / "gt" / f"{i:06d}.png")
            Image.fromarray(v[i % 3].numpy()).save(root / "images" / seq / "pred" / f"{i:06d}.png")
    return seqs


def _read(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_calculate_metric_with_lpips(hip_lib, weights, tmp_path, parity):
    from safetensors.torch import save_file
    vgg, lin = weights
    vp, lp = tmp_path / "vgg16.safetensors", tmp_path / "vgg.pth"
    save_file({k: v.contiguous() for k, v in vgg.items()}, str(vp))
    torch.save(lin, lp)
    outs = {}
    for mode in ("plain", "lpips"):
        out = tmp_path / mode
        seqs = _write_images(out)
        extra = ["--lpips_vgg_weights", vp, "--lpips_lin_weights", lp] if mode == "lpips" else []
        env = dict(os.environ, PYTHONPATH=str(ROOT))
        r = subprocess.run([sys.executable, str(ROOT / "evaluation" / "novel_view_synthesis_bench" / "calculate_metric.py"),
                            "--dataset", f"re10k:{tmp_path}", "--seq_id_map", "ids.json", "--output_dir", str(out), *map(str, extra)],
                           capture_output=True, text=True, env=env, timeout=600, cwd=str(ROOT))
        assert r.returncode == 0, r.stderr[-3000:]
        outs[mode] = (r.stdout, _read(out / "_all_samples.csv"), _read(out / "overall-metric.csv"))
    stdout, rows, (overall,) = outs["lpips"]
    assert "LPIPS not computed" not in stdout and "LPIPS" in stdout
    assert list(rows[0]) == ["seq", "PSNR", "SSIM", "LPIPS"] and list(overall) == ["PSNR", "SSIM", "LPIPS"]
    _, prow, (pover,) = outs["plain"]
    assert list(prow[0]) == ["seq", "PSNR", "SSIM"] and "LPIPS not computed" in outs["plain"][0]
    for a, b in zip(rows, prow):
        assert (a["seq"], a["PSNR"], a["SSIM"]) == (b["seq"], b["PSNR"], b["SSIM"])
    assert (overall["PSNR"], overall["SSIM"]) == (pover["PSNR"], pover["SSIM"])
    worst, means = 0.0, []
    for row in rows:
        d = tmp_path / "lpips" / "images" / row["seq"]
        n = seqs[row["seq"]][2]
        gt = torch.from_numpy(np.stack([np.asarray(Image.open(d / "gt" / f"{i:06d}.png")) for i in range(n)]))
        pr = torch.from_numpy(np.stack([np.asarray(Image.open(d / "pred" / f"{i:06d}.png")) for i in range(n)]))
        means.append(LO.lpips(vgg, lin, pr, gt).mean().item())
        worst = max(worst, abs(float(row["LPIPS"]) - means[-1]))
    assert worst <= GATE
    assert abs(float(overall["LPIPS"]) - np.mean(means)) <= GATE
    parity("calculate_metric.py LPIPS vs fp64 oracle", max_abs_err=worst)
