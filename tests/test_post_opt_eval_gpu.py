"""GPU tests of vist3a_amd.post_opt.evaluate_views and of the hold-out split of the loop (PostOptConfig.test_every), on the tiny
scene of tests/test_post_opt_gpu.py (300 Gaussians, 3 cameras of 48 x 64)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import color_correct_oracle as CO  # noqa: E402
import post_opt_oracle as PO  # noqa: E402
import test_post_opt_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

# a fixed cast per view that clips nothing: gain x + bias stays inside [0.02, 0.98] (to float32 rounding) for x in [0, 1]
GAIN = torch.tensor([[0.80, 0.90, 0.70], [0.90, 0.75, 0.85], [0.70, 0.85, 0.90]])
BIAS = torch.tensor([[0.04, 0.02, 0.06], [0.02, 0.05, 0.03], [0.06, 0.03, 0.02]])


@pytest.fixture(scope="module")
def scene():
    sc = PO.loop_scene()
    truth = T._scene_gaussians(sc)
    target, _, _, _ = T._targets(sc, truth)
    return dict(sc=sc, truth=truth, target=target, ext=sc["c2w"].cuda(), Kn=sc["Kn"].cuda(), start=T._scene_gaussians(sc, perturb_seed=43))


def _render(gs, scene):
    return T._targets(scene["sc"], gs)[0]


def test_cc_psnr_removes_a_colour_cast(hip_lib, parity, scene):
    """Targets = the scene's own renders through a per-view gain and bias.  The cast is affine and clips nothing, so its inverse lies
    inside color_correct's model: what is left after the fit is float32 rounding (of the cast target, 6e-8 of a value, and of the
    stored result) - beyond 100 dB - while plain PSNR sees the cast itself.  The fp64 oracle on the same render says the same."""
    from vist3a_amd.post_opt import evaluate_views
    cast = (scene["target"] * GAIN.cuda()[:, None, None] + BIAS.cuda()[:, None, None]).contiguous()
    assert float(cast.min()) > 0.019 and float(cast.max()) < 0.981      # far inside [eps, 1 - eps]: nothing is clipped or masked in the target
    r = evaluate_views(scene["truth"], cast, scene["ext"], scene["Kn"], color_correct=True)
    render = _render(scene["truth"], scene).cpu()
    o64 = CO.color_correct(render, cast.cpu())
    cc64 = CO.psnr(CO.mse(o64.float(), cast.cpu())).tolist()
    for j, v in enumerate(r["per_view"]):
        print(f"[eval cast view {j}] psnr {v['psnr']:.3f} dB   cc_psnr {v['cc_psnr']:.3f} dB   fp64 oracle rounded to f32 {cc64[j]:.3f} dB   status {v['cc_status']}")
        parity(f"post_opt_eval::cast[view={j}]", psnr=v["psnr"], cc_psnr=v["cc_psnr"], oracle_cc_psnr=cc64[j])
        assert v["cc_status"] == [0, 0, 0]
        assert v["psnr"] < 40 and v["cc_psnr"] > 100 and cc64[j] > 100
    assert set(r) == {"psnr", "ssim", "cc_psnr", "num_GS", "ellipse_time", "per_view"}
    assert r["cc_psnr"] > r["psnr"] + 60 and r["num_GS"] == scene["truth"].means.shape[1] and r["ellipse_time"] > 0
    assert "cc_psnr" not in evaluate_views(scene["truth"], cast, scene["ext"], scene["Kn"])


def test_cc_psnr_of_an_uncast_render(hip_lib, parity, scene):
    """No cast, a perturbed scene: there is little for the fit to remove.  cc_psnr equals the fp64 oracle's on the same render within
    the parity bound of tests/test_color_correct_gpu.py (2e-7 of the MSE = 1e-6 dB), and is not below psnr by more than that."""
    from vist3a_amd.post_opt import evaluate_views
    r = evaluate_views(scene["start"], scene["target"], scene["ext"], scene["Kn"], color_correct=True)
    render = _render(scene["start"], scene).cpu()
    cc64 = CO.psnr(CO.mse(CO.color_correct(render, scene["target"].cpu()), scene["target"].cpu())).tolist()
    for j, v in enumerate(r["per_view"]):
        print(f"[eval uncast view {j}] psnr {v['psnr']:.6f} dB   cc_psnr {v['cc_psnr']:.6f} dB   fp64 oracle {cc64[j]:.6f} dB")
        parity(f"post_opt_eval::uncast[view={j}]", psnr=v["psnr"], cc_psnr=v["cc_psnr"], oracle_cc_psnr=cc64[j])
    for j, v in enumerate(r["per_view"]):
        assert abs(v["cc_psnr"] - cc64[j]) <= 1e-6, (j, v["cc_psnr"], cc64[j])
        assert v["cc_psnr"] >= v["psnr"] - 1e-6, (j, v)


def test_psnr_and_ssim_match_torch_fp64(hip_lib, parity, scene):
    from vist3a_amd import ops
    from vist3a_amd.post_opt import evaluate_views
    r = evaluate_views(scene["start"], scene["target"], scene["ext"], scene["Kn"])
    render = _render(scene["start"], scene)
    mse64 = CO.mse(render.cpu(), scene["target"].cpu())
    hip = ops.image_mse(render, scene["target"]).cpu()
    e = float(((hip - mse64).abs() / mse64).max())
    ep = max(abs(v["psnr"] - p) for v, p in zip(r["per_view"], CO.psnr(mse64).tolist()))
    print(f"[eval psnr] image_mse vs torch fp64 {e:.3e} relative;  per-view psnr vs -10 log10 of it {ep:.3e} dB")
    parity("post_opt_eval::psnr", mse_rel=e, psnr_abs_db=ep)
    assert e <= 1e-13 and ep <= 1e-11
    assert abs(r["psnr"] - float(CO.psnr(mse64).mean())) <= 1e-11
    ssim = [float(ops.photometric_loss(render[j:j + 1], scene["target"][j:j + 1], 0.2)[2]) for j in range(3)]
    assert [v["ssim"] for v in r["per_view"]] == ssim and set(r) == {"psnr", "ssim", "num_GS", "ellipse_time", "per_view"}


def _parent_loop(start, images, ext, Kn, cfg, steps):
    """the loop as it stood before test_every existed (no depth term, no grids), written out on the ops"""
    from math import isqrt
    from vist3a_amd import ops
    from vist3a_amd.post_opt import create_splats, view_order
    from vist3a_amd.post_opt.trainer import _cameras
    V, H, W, _ = images.shape
    sp = create_splats(start, cfg)
    p, m, v = sp["params"], sp["m"], sp["v"]
    Ksh = p["sh"].shape[-1]
    view, campos, Kpix = _cameras(ext, Kn, W, H, "cuda")
    bg = torch.zeros(3, device="cuda")
    log = torch.zeros(steps, 3, device="cuda", dtype=torch.float64)
    lrs = dict(means=cfg.lr_means, scales=cfg.lr_scales, quats=cfg.lr_quats, opacities=cfg.lr_opacities, sh=cfg.lr_sh)
    decay = 0.01 ** (1.0 / cfg.max_steps)
    ws = ops.GsWorkspace()
    trained = cfg.trained()
    leaves = [p[n].requires_grad_(True) for n in trained]
    for i, j in enumerate(view_order(V, steps, cfg.seed)):
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        color, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view[j:j + 1], campos[j:j + 1], Kpix[j:j + 1], W, H,
                                    sh_degree=isqrt(Ksh) - 1, sh_layout=1, background=bg, clamp_rgb=True, workspace=ws)
        loss, l1, ssim = ops.photometric_loss(color, images[j:j + 1], cfg.ssim_lambda)
        grads = torch.autograd.grad(loss, leaves)
        log[i].copy_(torch.stack([loss.detach(), l1.detach(), ssim.detach()]))
        with torch.no_grad():
            for n, g in zip(trained, grads):
                lr = lrs[n] * (decay ** i if n == "means" else 1.0)
                sh = n == "sh"
                ops.adam_step(p[n], g.contiguous(), m[n], v[n], lr=lr, step=i + 1, betas=cfg.betas, eps=cfg.eps,
                              lr2=lr / 20 if sh else None, period=Ksh if sh and Ksh > 1 else 0)
    return {n: t.detach() for n, t in p.items()}, log


def test_test_every_zero_is_the_loop_as_it_was(hip_lib, scene):
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, train_view_order, view_order
    cfg = PostOptConfig(seed=1)
    assert cfg.test_every == 0 and train_view_order(3, 12, 1, 0) == view_order(3, 12, 1)
    sp = create_splats(scene["start"], cfg, 3)
    _, log = post_optimize(scene["start"], scene["target"], scene["ext"], scene["Kn"], cfg, steps=12, splats=sp)
    params, log_parent = _parent_loop(scene["start"], scene["target"], scene["ext"], scene["Kn"], cfg, 12)
    assert torch.equal(log, log_parent) and log.shape == (12, 3)
    assert all(torch.equal(sp["params"][n], params[n]) for n in params)


def test_held_out_views_never_enter_the_loop(hip_lib, scene):
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, train_view_order, train_views
    order = train_view_order(3, 40, 1, 2)
    assert set(order) == {1} and train_views(3, 2) == [1]
    assert set(train_view_order(7, 60, 0, 3)) == {1, 2, 4, 5}
    with pytest.raises(ValueError, match="no view is left"):
        train_views(3, 1)
    cfg = PostOptConfig(seed=1, test_every=2, use_bilateral_grid=True, bilateral_grid_shape=(4, 4, 2))
    poisoned = scene["target"].clone()
    poisoned[0], poisoned[2] = float("nan"), float("nan")      # a step on a held-out view would put NaN into the log and the scene
    runs = []
    for images in (scene["target"], poisoned):
        sp = create_splats(scene["start"], cfg, 1)
        g, log = post_optimize(scene["start"], images, scene["ext"], scene["Kn"], cfg, steps=6, splats=sp)
        assert sp["bil_grids"].shape[0] == 1                    # one grid per TRAINING view
        runs.append((g.means, g.harmonics, log))
    assert bool(torch.isfinite(runs[1][2]).all()) and all(torch.equal(a, b) for a, b in zip(*runs))
    with pytest.raises(ValueError, match="no view is left"):
        post_optimize(scene["start"], scene["target"], scene["ext"], scene["Kn"], PostOptConfig(test_every=1), steps=1)
