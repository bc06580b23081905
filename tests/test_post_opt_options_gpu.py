"""GPU tests of the post-optimisation loop's antialiased / random_bkgd / opacity_reg / scale_reg options (vist3a_amd/post_opt/trainer.py)
on the 300-Gaussian scene and views of tests/post_opt_oracle.py, at most 20 steps.

The antialiased loop is compared with the same loop on the CPU - oracle/gsplat_raster.py with the compensation of
tests/raster_aa_oracle.py, tests/ssim_loss_oracle.py and torch.optim.Adam in fp64 (and fp32, the comparison figure) - as
tests/test_post_opt_gpu.py::test_loop_follows_oracle compares the classic one.  Gate: the project's rule min(2 x the largest value
measured on an MI355X, 1e-3); MEASURED["loop_aa"] is the run recorded in DESIGN.md section 7f (None would select the ceiling)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import gsplat_raster as G

sys.path.insert(0, str(Path(__file__).resolve().parent))
import post_opt_oracle as PO  # noqa: E402
import raster_aa_oracle as AO  # noqa: E402
import ssim_loss_oracle as SO  # noqa: E402
import test_cli_gpu as CLI  # noqa: E402
from test_post_opt_gpu import _scene_gaussians, _targets  # noqa: E402

pytestmark = pytest.mark.gpu

CEILING = 1e-3
MEASURED = dict(loop_aa=2.355e-7)   # largest per-step relative loss difference, hip vs the fp64 loop (MI355X); the fp32 oracle loop: 9.1e-6
FIELDS = ("means", "covariances", "harmonics", "opacities", "scales", "rotations")


def gate(name):
    return CEILING if MEASURED[name] is None else min(2 * MEASURED[name], CEILING)


@pytest.fixture(scope="module")
def scene():
    sc = PO.loop_scene()
    target, _, _, _ = _targets(sc, _scene_gaussians(sc))
    return sc, target, _scene_gaussians(sc, perturb_seed=43), sc["c2w"].cuda(), sc["Kn"].cuda()


def _same(a, b):
    return torch.equal(a[1], b[1]) and all(torch.equal(getattr(a[0], f), getattr(b[0], f)) for f in FIELDS)


def test_options_off_change_nothing(hip_lib, scene):
    from vist3a_amd.post_opt import PostOptConfig, post_optimize
    sc, target, start, ext, Kn = scene
    plain = post_optimize(start, target, ext, Kn, PostOptConfig(seed=1), steps=12)
    off = post_optimize(start, target, ext, Kn, PostOptConfig(seed=1, antialiased=False, random_bkgd=False, opacity_reg=0.0, scale_reg=0.0), steps=12)
    assert plain[1].shape == (12, 3) and _same(plain, off)


def test_antialiased_loop_follows_oracle(hip_lib, parity, monkeypatch):
    """20 steps on opacity logits and harmonics (geometry fixed: radii, order and compensations stay put) in the antialiased mode."""
    from vist3a_amd import ops
    from vist3a_amd.models.types import Gaussians
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, view_order
    from vist3a_amd.post_opt.trainer import _cameras
    sc = PO.loop_scene()
    W, H, steps = sc["W"], sc["H"], 20
    target, _, _, _ = _targets(sc, _scene_gaussians(sc))
    start = _scene_gaussians(sc, perturb_seed=42, geometry=False)
    cfg = PostOptConfig(params=("opacities", "sh"), seed=5, antialiased=True)
    out, log = post_optimize(start, target, sc["c2w"].cuda(), sc["Kn"].cuda(), cfg, steps=steps)
    _, log_classic = post_optimize(start, target, sc["c2w"].cuda(), sc["Kn"].cuda(), PostOptConfig(params=("opacities", "sh"), seed=5), steps=steps)
    assert not torch.equal(log, log_classic)                      # the mode is on
    c_hip = log[:, 0].cpu()
    sp = create_splats(start, cfg)
    keep = sp["keep"]
    kept = _scene_gaussians(sc)
    kept = Gaussians(*(getattr(kept, f)[:, keep].contiguous() for f in FIELDS))
    view, campos, K = _cameras(sc["c2w"], sc["Kn"], W, H, "cuda")
    with torch.no_grad():
        pr = ops.gs_project(kept.means[0], kept.covariances[0], kept.harmonics[0], view, campos, K, W, H, sh_degree=1, sh_layout=1,
                            rasterize_mode="antialiased")
        r = ops.gs_rasterize(pr, kept.opacities[0], W, H, background=torch.zeros(3, device="cuda"), clamp_rgb=True, return_order=True)
    U = int(keep.sum())
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    offs_all, ids_all = r["tile_offsets"].cpu().long(), r["flatten_ids"].cpu().long()
    order = view_order(3, steps, cfg.seed)
    means, cov = kept.means[0].cpu(), kept.covariances[0].cpu()
    logit0, sh_start = sp["params"]["opacities"].cpu(), sp["params"]["sh"].cpu()

    def fit(dt):
        lg = logit0.clone().to(dt).requires_grad_(True)
        s0, sN = sh_start[..., :1].clone().to(dt).requires_grad_(True), sh_start[..., 1:].clone().to(dt).requires_grad_(True)
        opts = [torch.optim.Adam([t], lr=lr, eps=cfg.eps, betas=cfg.betas) for t, lr in ((lg, cfg.lr_opacities), (s0, cfg.lr_sh), (sN, cfg.lr_sh / 20))]
        curve = []
        for j in order:
            lo, hi = int(offs_all[j * ntiles]), int(offs_all[(j + 1) * ntiles])
            offs, ids = offs_all[j * ntiles:(j + 1) * ntiles + 1] - lo, ids_all[lo:hi] - j * U
            mask = (pr["radii"][j] > 0).cpu()
            col, _, _, _, _ = AO.render(dt, means.to(dt), cov.to(dt), torch.cat([s0, sN], -1).permute(0, 2, 1), torch.sigmoid(lg), view[j].cpu(),
                                        campos[j].cpu(), K[j].cpu(), W, H, 1, mask, offs, ids, monkeypatch, background=(0.0, 0.0, 0.0))
            loss = SO.photometric_loss(col[None], target[j:j + 1].cpu().to(dt), cfg.ssim_lambda)[0]
            for o in opts:
                o.zero_grad()
            loss.backward()
            for o in opts:
                o.step()
            curve.append(float(loss))
        return torch.tensor(curve, dtype=torch.float64)

    c64, c32 = fit(torch.float64), fit(torch.float32)
    e, e32 = float(((c_hip - c64).abs() / c64).max()), float(((c32 - c64).abs() / c64).max())
    print(f"[aa loop] loss {c64[0]:.5e} -> {c64[-1]:.5e} (oracle fp64), {c_hip[0]:.5e} -> {c_hip[-1]:.5e} (hip); classic first step {float(log_classic[0, 0]):.5e}")
    print(f"[aa loop] per-step relative loss difference, max over {steps} steps: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {gate('loop_aa'):.1e}")
    parity("post_opt_options::loop_aa", rel_max=e, oracle_fp32_rel_max=e32, gate=gate("loop_aa"), first=float(c64[0]), last=float(c64[-1]))
    assert torch.equal(out.means, kept.means)
    assert e <= gate("loop_aa"), e


def test_random_background(hip_lib, scene):
    from vist3a_amd import ops
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, random_backgrounds, train_view_order
    from vist3a_amd.post_opt.trainer import _cameras
    sc, target, start, ext, Kn = scene
    cfg = PostOptConfig(seed=3, random_bkgd=True)
    a, b = post_optimize(start, target, ext, Kn, cfg, steps=8), post_optimize(start, target, ext, Kn, cfg, steps=8)
    assert _same(a, b) and bool(torch.isfinite(a[1]).all())                                  # two runs: bit-identical
    black = post_optimize(start, target, ext, Kn, PostOptConfig(seed=3), steps=8)
    assert not torch.equal(a[1], black[1])
    assert train_view_order(3, 8, 3) == train_view_order(3, 8, 3)
    # step 0 by hand: the first view of the (unchanged) order over the first background of the seed
    sp = create_splats(start, cfg)
    p = sp["params"]
    j = train_view_order(3, 8, cfg.seed)[0]
    view, campos, K = _cameras(ext, Kn, sc["W"], sc["H"], "cuda")
    with torch.no_grad():
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        for bg, want in ((random_backgrounds(8, cfg.seed)[0].cuda(), a[1]), (torch.zeros(3, device="cuda"), black[1])):
            col, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view[j:j + 1], campos[j:j + 1], K[j:j + 1], sc["W"], sc["H"], sh_degree=1,
                                      sh_layout=1, background=bg, clamp_rgb=True)
            loss, l1, ssim = ops.photometric_loss(col, target[j:j + 1], cfg.ssim_lambda)
            assert torch.equal(torch.stack([loss, l1, ssim]), want[0])


def test_regularisers(hip_lib, scene):
    from vist3a_amd import ops
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize
    sc, target, start, ext, Kn = scene
    cfg = PostOptConfig(seed=2, opacity_reg=0.01, scale_reg=0.01)
    sp = create_splats(start, cfg)
    rows = []
    for _ in range(4):   # one step at a time on the same splats: the parameters at each step are in hand
        want = torch.stack(ops.splat_regularisers(sp["params"]["scales"], sp["params"]["opacities"]))
        _, log = post_optimize(start, target, ext, Kn, cfg, steps=1, splats=sp)
        assert log.shape == (1, 5) and torch.equal(log[0, 3:], want)
        total = log[0, 0]
        photo = (1 - cfg.ssim_lambda) * log[0, 1] + cfg.ssim_lambda * (1 - log[0, 2])
        assert abs(float(total - (photo + 0.01 * want[0] + 0.01 * want[1]))) <= 1e-12 * float(total)
        rows.append(log[0])
    only_op = post_optimize(start, target, ext, Kn, PostOptConfig(seed=2, opacity_reg=0.01), steps=2)
    only_sc = post_optimize(start, target, ext, Kn, PostOptConfig(seed=2, scale_reg=0.01), steps=2)
    assert only_op[1].shape == (2, 4) and only_sc[1].shape == (2, 4)
    assert torch.equal(only_op[1][0, 3], rows[0][3]) and torch.equal(only_sc[1][0, 3], rows[0][4])
    reg = post_optimize(start, target, ext, Kn, cfg, steps=4)
    plain = post_optimize(start, target, ext, Kn, PostOptConfig(seed=2), steps=4)
    assert plain[1].shape == (4, 3)
    assert not torch.equal(reg[0].scales, plain[0].scales) and not torch.equal(reg[0].opacities, plain[0].opacities)


def test_cli_antialiased(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text("a red chair in a white room\n")
    r = CLI._cli(a, tmp_path / "aa", extra=("--no_video", "--post_opt_antialiased", "--post_opt_random_bkgd", "--post_opt_opacity_reg", "0.01",
                                            "--post_opt_scale_reg", "0.01", "--post_opt_steps", "4"))
    assert r.returncode == 0, r.stderr[-3000:]
    _, _, data = CLI._read_ply(tmp_path / "aa" / "a red chair in a white room" / "gaussians.ply")
    assert data.shape[0] > 0 and np.isfinite(data).all()
