"""GPU tests of the post-optimisation loop's MCMC strategy (vist3a_amd/post_opt/trainer.py, cfg.strategy = "mcmc") on the scene and the
three 48 x 64 views of tests/post_opt_oracle.py, with all 300 Gaussians alive at creation (the scene's first ten are lifted above
min_opacity, so that the row counts are those of a 300-Gaussian scene: 300 -> 315 -> 330 -> 340 under a cap of 340).

Off, the loop is bit for bit what it was; on, it is the same loop written out on ops.mcmc_sample / mcmc_relocate / mcmc_noise, bit
for bit; two runs agree, `splats` carried through two calls gives what one call gives, and nothing but the seed is random."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import post_opt_oracle as PO  # noqa: E402
from test_post_opt_eval_gpu import _parent_loop  # noqa: E402
from test_post_opt_gpu import _scene_gaussians, _targets  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("means", "covariances", "harmonics", "opacities", "scales", "rotations")
NAMES = ("means", "scales", "quats", "opacities", "sh")
REFINE = dict(mcmc_refine_start_iter=1, mcmc_refine_stop_iter=100, mcmc_refine_every=4, mcmc_cap_max=340)


def _cfg(**kw):
    from vist3a_amd.post_opt import PostOptConfig
    return PostOptConfig(**{**dict(seed=1, strategy="mcmc"), **REFINE, **kw})


@pytest.fixture(scope="module")
def scene():
    sc = PO.loop_scene()
    sc["op"][:10] = 0.4
    target, _, _, _ = _targets(sc, _scene_gaussians(sc))
    return dict(sc=sc, target=target, start=_scene_gaussians(sc, perturb_seed=43), ext=sc["c2w"].cuda(), Kn=sc["Kn"].cuda())


def _run(scene, cfg, steps, splats=None, prepare=None):
    from vist3a_amd.post_opt import create_splats, post_optimize
    sp = create_splats(scene["start"], cfg, 3) if splats is None else splats
    if prepare is not None:
        prepare(sp)
    out, log = post_optimize(scene["start"], scene["target"], scene["ext"], scene["Kn"], cfg, steps=steps, splats=sp)
    return out, log, sp


def _same_splats(a, b):
    return (all(torch.equal(a[g][n], b[g][n]) for g in ("params", "m", "v") for n in NAMES) and a["step"] == b["step"]
            and torch.equal(a["mcmc_counts"], b["mcmc_counts"]))


def _written_out(scene, cfg, steps, prepare=None):
    """post_optimize with cfg.strategy = "mcmc" (no depth term, no grids, no regularisers), written out on the ops"""
    from math import isqrt
    from vist3a_amd import ops
    from vist3a_amd.post_opt import create_splats, view_order
    from vist3a_amd.post_opt.trainer import _cameras
    images = scene["target"]
    V, H, W, _ = images.shape
    sp = create_splats(scene["start"], cfg)
    if prepare is not None:
        prepare(sp)
    p, m, v = sp["params"], sp["m"], sp["v"]
    Ksh = p["sh"].shape[-1]
    view, campos, Kpix = _cameras(scene["ext"], scene["Kn"], W, H, "cuda")
    bg = torch.zeros(3, device="cuda")
    log = torch.zeros(steps, 3, device="cuda", dtype=torch.float64)
    lrs = dict(means=cfg.lr_means, scales=cfg.lr_scales, quats=cfg.lr_quats, opacities=cfg.lr_opacities, sh=cfg.lr_sh)
    decay = 0.01 ** (1.0 / cfg.max_steps)
    ws = ops.GsWorkspace()
    counts_log = []
    for i, j in enumerate(view_order(V, steps, cfg.seed)):
        leaves = [p[n].requires_grad_(True) for n in NAMES]
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        color, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view[j:j + 1], campos[j:j + 1], Kpix[j:j + 1], W, H,
                                    sh_degree=isqrt(Ksh) - 1, sh_layout=1, background=bg, clamp_rgb=True, workspace=ws)
        loss, l1, ssim = ops.photometric_loss(color, images[j:j + 1], cfg.ssim_lambda)
        grads = torch.autograd.grad(loss, leaves)
        log[i].copy_(torch.stack([loss.detach(), l1.detach(), ssim.detach()]))
        t = i + 1
        with torch.no_grad():
            for n, g in zip(NAMES, grads):
                lr = lrs[n] * (decay ** i if n == "means" else 1.0)
                ops.adam_step(p[n], g.contiguous(), m[n], v[n], lr=lr, step=t, betas=cfg.betas, eps=cfg.eps,
                              lr2=lr / 20 if n == "sh" else None, period=Ksh if n == "sh" and Ksh > 1 else 0)
            for d in (p, m, v):
                for n in NAMES:
                    d[n] = d[n].detach()
            if cfg.mcmc_refine_start_iter < i < cfg.mcmc_refine_stop_iter and i % cfg.mcmc_refine_every == 0:
                U = p["means"].shape[0]
                _, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
                src, counts = ops.mcmc_sample(op, min_weight=cfg.mcmc_min_opacity, alive_only=True, n_slots=U, seed=cfg.seed, stream=0, step=t)
                ops.mcmc_relocate(src, counts, p, m, v, dst_offset=0, min_opacity=cfg.mcmc_min_opacity)
                n_new = max(0, min(cfg.mcmc_cap_max, int(1.05 * U)) - U)
                counts_log.append([int((src >= 0).sum()), n_new])
                if n_new > 0:
                    _, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
                    src, counts = ops.mcmc_sample(op, min_weight=cfg.mcmc_min_opacity, alive_only=False, n_slots=n_new, seed=cfg.seed, stream=1, step=t)
                    for d in (p, m, v):
                        for n in NAMES:
                            d[n] = torch.cat([d[n], torch.zeros((n_new,) + tuple(d[n].shape[1:]), device="cuda")])
                    ops.mcmc_relocate(src, counts, p, m, v, dst_offset=U, min_opacity=cfg.mcmc_min_opacity)
            ops.mcmc_noise(p["means"], p["scales"], p["quats"], p["opacities"], scaler=cfg.mcmc_noise_lr * (cfg.lr_means * decay ** t),
                           seed=cfg.seed, step=t)
    sp["step"] = steps
    sp["mcmc_counts"] = torch.tensor(counts_log, dtype=torch.int64, device="cuda").reshape(-1, 2)
    return log, sp


def test_strategy_off_changes_nothing(hip_lib, scene):
    from vist3a_amd.post_opt import PostOptConfig
    plain = _run(scene, PostOptConfig(seed=1), 12)
    off = _run(scene, PostOptConfig(seed=1, strategy="none", mcmc_noise_lr=1e9, mcmc_min_opacity=0.5, **REFINE), 12)
    assert plain[1].shape == (12, 3) and torch.equal(plain[1], off[1])
    assert all(torch.equal(getattr(plain[0], f), getattr(off[0], f)) for f in FIELDS)
    assert all(torch.equal(plain[2][g][n], off[2][g][n]) for g in ("params", "m", "v") for n in NAMES)
    assert "mcmc_counts" not in off[2] and off[2]["params"]["means"].shape[0] == 300
    params, log_parent = _parent_loop(scene["start"], scene["target"], scene["ext"], scene["Kn"], PostOptConfig(seed=1), 12)
    assert torch.equal(off[1], log_parent) and all(torch.equal(off[2]["params"][n], params[n]) for n in NAMES)     # the loop as it was
    with pytest.raises(ValueError, match="strategy"):
        _run(scene, PostOptConfig(seed=1, strategy="default"), 1)


def test_strategy_on_is_the_ops_written_out(hip_lib, scene):
    cfg = _cfg()
    out, log, sp = _run(scene, cfg, 12)
    log2, sp2 = _written_out(scene, cfg, 12)
    assert torch.equal(log, log2) and bool(torch.isfinite(log).all())
    assert _same_splats(sp, sp2)
    assert sp["mcmc_counts"].dtype == torch.int64 and sp["mcmc_counts"].is_cuda and sp["mcmc_counts"].tolist() == [[0, 15], [0, 15]]
    assert sp["params"]["means"].shape[0] == 330 and out.means.shape == (1, 330, 3) and out.harmonics.shape[1] == 330
    assert sp["keep"].shape == (300,) and bool(sp["keep"].all())                 # "keep" describes creation only
    plain = _run(scene, type(cfg)(seed=1), 12)
    assert not torch.equal(plain[1], log) and torch.equal(plain[1][0], log[0])   # the first step sees the scene as created; the noise follows it


def test_row_count_follows_the_cap(hip_lib, scene):
    from vist3a_amd.post_opt import mcmc_growth
    cfg = _cfg()
    sp, rows = None, []
    for steps in (4, 1, 4, 4, 4, 4):      # refines after the steps with 4, 8, 12, 16, 20 steps before them
        out, _, sp = _run(scene, cfg, steps, splats=sp)
        rows.append(sp["params"]["means"].shape[0])
        assert out.means.shape[1] == rows[-1] and all(sp[g][n].shape[0] == rows[-1] for g in ("params", "m", "v") for n in NAMES)
    assert rows == [300, 315, 330, 340, 340, 340]
    want, U = [], 300
    for _ in range(5):
        want.append(mcmc_growth(cfg, U))
        U += want[-1]
    assert want == [15, 15, 10, 0, 0] and sp["mcmc_counts"][:, 1].tolist() == want and sp["step"] == 21


def test_dead_gaussians_are_relocated(hip_lib, scene):
    def kill(sp):
        sp["params"]["opacities"][:60] = torch.logit(torch.tensor(0.001)).item()
    cfg = _cfg(params=("sh",), mcmc_noise_lr=0.0, mcmc_cap_max=300)        # nothing but the harmonics moves before the refine
    _, _, sp = _run(scene, cfg, 5, prepare=kill)
    assert sp["mcmc_counts"].tolist() == [[60, 0]] and sp["params"]["means"].shape[0] == 300
    p = sp["params"]
    match = (p["means"][:60, None, :] == p["means"][None, 60:, :]).all(-1)
    assert bool((match.sum(1) >= 1).all())                                     # every relocated row sits on a live one
    j = 60 + match.float().argmax(1)
    assert torch.equal(p["sh"][:60], p["sh"][j]) and torch.equal(p["quats"][:60], p["quats"][j])
    assert torch.equal(p["opacities"][:60], p["opacities"][j]) and torch.equal(p["scales"][:60], p["scales"][j])
    assert bool((torch.sigmoid(p["opacities"]) >= 0.005 - 1e-9).all())
    # and with the whole strategy on: the count is the same, the scene grows
    _, _, sp = _run(scene, _cfg(), 5, prepare=kill)
    assert sp["mcmc_counts"].tolist() == [[60, 15]] and sp["params"]["means"].shape[0] == 315


def test_reproducible_and_seeded(hip_lib, scene):
    a, b = _run(scene, _cfg(), 12), _run(scene, _cfg(), 12)
    assert torch.equal(a[1], b[1]) and _same_splats(a[2], b[2]) and all(torch.equal(getattr(a[0], f), getattr(b[0], f)) for f in FIELDS)
    c = _run(scene, _cfg(seed=2), 12)
    assert not torch.equal(a[2]["params"]["means"], c[2]["params"]["means"])


def test_continuation(hip_lib, scene):
    """`splats` through two calls of 6 steps is one call of 12.  The view order has always restarted with every call, so the seed is
    one whose steps 6-11 see the views of steps 0-5 again: what is left to go wrong is the strategy's own state - the steps done,
    which key the random numbers and time the refines (here after steps 4 and 8, one in each half), and the grown tensors."""
    from vist3a_amd.post_opt import view_order
    cfg = _cfg(seed=5)
    assert view_order(3, 12, cfg.seed)[6:] == view_order(3, 6, cfg.seed)
    whole = _run(scene, cfg, 12)
    _, log_a, sp = _run(scene, cfg, 6)
    assert sp["step"] == 6 and sp["mcmc_counts"].shape == (1, 2) and sp["params"]["means"].shape[0] == 315
    out, log_b, sp = _run(scene, cfg, 6, splats=sp)
    assert torch.equal(torch.cat([log_a, log_b]), whole[1]) and _same_splats(sp, whole[2])
    assert all(torch.equal(getattr(out, f), getattr(whole[0], f)) for f in FIELDS) and sp["params"]["means"].shape[0] == 330
