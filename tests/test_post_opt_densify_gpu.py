"""GPU tests of the post-optimisation loop's densification strategy (vist3a_amd/post_opt/trainer.py, cfg.strategy = "densify") on the
300-Gaussian scene and the three 48 x 64 views of tests/post_opt_oracle.py (K = 4), 12 steps with (start, stop, every, reset) =
(1, 100, 3, 6): refines after the steps i = 3, 6, 9, resets after i = 6; the scale criterion of pruning acts at i = 9 only.

The thresholds are chosen from the state a probe run has accumulated when the first refine comes (between neighbouring values, so
that no decision sits on its threshold) so that clone, split and prune all occur.  Off, the loop is bit for bit what it was; on, it
is the same loop written out on ops.densify_accumulate / densify_classify / densify_apply / densify_reset_opacity, bit for bit, and
the row counts after every refine are those of the numpy oracle (tests/densify_oracle.py) fed with the device's state."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import densify_oracle as DO  # noqa: E402
from test_post_opt_mcmc_gpu import FIELDS, NAMES, _run, scene  # noqa: E402,F401  (scene: the module-scoped fixture)

pytestmark = pytest.mark.gpu

REFINE = dict(densify_refine_start_iter=1, densify_refine_stop_iter=100, densify_refine_every=3, densify_reset_every=6)


def _between(x, q):
    """a value between two neighbouring entries of x near its quantile q, away from both"""
    s = np.unique(np.asarray(x, dtype=np.float64))
    i = min(max(int(q * len(s)), 1), len(s) - 1)
    gaps = [(s[j] - s[j - 1], j) for j in range(max(i - 3, 1), min(i + 4, len(s)))]
    j = max(gaps)[1]
    return float(0.5 * (s[j] + s[j - 1]))


@pytest.fixture(scope="module")
def thresholds(scene):
    """from the state at the first refine (after the Adam updates of step 3) of a run that never refines"""
    from vist3a_amd.post_opt import PostOptConfig
    probe = PostOptConfig(seed=1, strategy="densify", **{**REFINE, "densify_refine_start_iter": 50})
    _, _, sp = _run(scene, probe, 4)
    st = sp["densify"]
    grad, count = st["grad2d"].cpu().numpy(), st["count"].cpu().numpy()
    assert grad.shape == (300,) and count.max() >= 2 and (count > 0).sum() > 100 and sp["step"] == 4 and "densify_counts" not in sp
    avg = grad.astype(np.float64) / np.maximum(count, 1)
    smax = np.exp(sp["params"]["scales"].cpu().numpy().astype(np.float64)).max(1)
    op = 1 / (1 + np.exp(-sp["params"]["opacities"].cpu().numpy().astype(np.float64)))
    th = dict(densify_grow_grad2d=_between(avg[count > 0], 0.5), densify_grow_scale3d=_between(smax, 0.5),
              densify_prune_opa=_between(op, 0.1), densify_prune_scale3d=_between(smax, 0.9))
    assert th["densify_prune_opa"] < 0.5
    return th


def _cfg(th, **kw):
    from vist3a_amd.post_opt import PostOptConfig
    return PostOptConfig(**{**dict(seed=1, strategy="densify"), **REFINE, **th, **kw})


def _same_splats(a, b):
    return (all(torch.equal(a[g][n], b[g][n]) for g in ("params", "m", "v") for n in NAMES) and a["step"] == b["step"]
            and torch.equal(a["densify_counts"], b["densify_counts"]) and all(torch.equal(a["densify"][k], b["densify"][k]) for k in ("grad2d", "count")))


def _written_out(scene, cfg, steps):
    """post_optimize with cfg.strategy = "densify", written out on the ops; also the oracle's row count at every refine"""
    from math import isqrt
    from vist3a_amd import ops
    from vist3a_amd.post_opt import create_splats, view_order
    from vist3a_amd.post_opt.trainer import _cameras
    images = scene["target"]
    V, H, W, _ = images.shape
    sp = create_splats(scene["start"], cfg)
    p, m, v = sp["params"], sp["m"], sp["v"]
    Ksh = p["sh"].shape[-1]
    view, campos, Kpix = _cameras(scene["ext"], scene["Kn"], W, H, "cuda")
    bg = torch.zeros(3, device="cuda")
    log = torch.zeros(steps, 3, device="cuda", dtype=torch.float64)
    lrs = dict(means=cfg.lr_means, scales=cfg.lr_scales, quats=cfg.lr_quats, opacities=cfg.lr_opacities, sh=cfg.lr_sh)
    decay = 0.01 ** (1.0 / cfg.max_steps)
    ws = ops.GsWorkspace()
    U = p["means"].shape[0]
    grad2d, count = torch.zeros(U, device="cuda"), torch.zeros(U, device="cuda", dtype=torch.int32)
    counts_log, oracle_rows, resets = [], [], []
    for i, j in enumerate(view_order(V, steps, cfg.seed)):
        leaves = [p[n].requires_grad_(True) for n in NAMES]
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        info = {}
        color, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view[j:j + 1], campos[j:j + 1], Kpix[j:j + 1], W, H, sh_degree=isqrt(Ksh) - 1,
                                    sh_layout=1, background=bg, clamp_rgb=True, workspace=ws, info_out=info, absgrad=cfg.densify_absgrad)
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
            if i >= cfg.densify_refine_stop_iter:
                continue
            ops.densify_accumulate(grad2d, count, info["d_means2d_abs" if cfg.densify_absgrad else "d_means2d"], info["radii"], W, H)
            if i > cfg.densify_refine_start_iter and i % cfg.densify_refine_every == 0 and i % cfg.densify_reset_every >= cfg.densify_pause_refine_after_reset:
                kw = dict(grow_grad2d=cfg.densify_grow_grad2d, grow_scale3d=cfg.densify_grow_scale3d * cfg.scene_scale, prune_opa=cfg.densify_prune_opa,
                          prune_scale3d=cfg.densify_prune_scale3d * cfg.scene_scale, prune_big=i > cfg.densify_reset_every)
                cls = ops.densify_classify(grad2d, count, p["scales"], p["opacities"], grow=True, **kw)
                grow = True
                if cfg.densify_cap_max > 0 and int(cls["totals"][0] + cls["totals"][1] + 2 * cls["totals"][2]) > cfg.densify_cap_max:
                    cls, grow = ops.densify_classify(grad2d, count, p["scales"], p["opacities"], grow=False, **kw), False
                want = DO.classify(grad2d.cpu().numpy(), count.cpu().numpy(), p["scales"].cpu().numpy(), p["opacities"].cpu().numpy(), grow=grow, **kw)
                oracle_rows.append((int(want["totals"][0] + want["totals"][1] + 2 * want["totals"][2]),
                                    DO.margin(grad2d.cpu().numpy(), count.cpu().numpy(), p["scales"].cpu().numpy(), p["opacities"].cpu().numpy(), **kw)))
                nA, nB, nC = cls["totals"].tolist()
                new = ops.densify_apply(cls, p, m, v, seed=cfg.seed, step=t)
                for d, nd in zip((p, m, v), new):
                    d.update(nd)
                U_out = p["means"].shape[0]
                counts_log.append([nB, nC, U + nB + nC - U_out, U_out])
                U = U_out
                grad2d, count = torch.zeros(U, device="cuda"), torch.zeros(U, device="cuda", dtype=torch.int32)
            if i % cfg.densify_reset_every == 0 and i > 0:
                before = p["opacities"].clone()
                ops.densify_reset_opacity(p["opacities"], m["opacities"], v["opacities"], 2.0 * cfg.densify_prune_opa)
                resets.append((i, before, p["opacities"].clone()))
    sp["step"] = steps
    sp["densify"] = dict(grad2d=grad2d, count=count)
    sp["densify_counts"] = torch.tensor(counts_log, dtype=torch.int64, device="cuda").reshape(-1, 4)
    return log, sp, oracle_rows, resets


def test_strategy_off_changes_nothing(hip_lib, scene, thresholds):
    from vist3a_amd.post_opt import PostOptConfig
    plain = _run(scene, PostOptConfig(seed=1), 12)
    off = _run(scene, PostOptConfig(seed=1, strategy="none", densify_absgrad=True, densify_revised_opacity=True, densify_cap_max=10,
                                    densify_pause_refine_after_reset=1, **REFINE, **thresholds), 12)
    assert plain[1].shape == (12, 3) and torch.equal(plain[1], off[1])
    assert all(torch.equal(getattr(plain[0], f), getattr(off[0], f)) for f in FIELDS)
    assert all(torch.equal(plain[2][g][n], off[2][g][n]) for g in ("params", "m", "v") for n in NAMES)
    assert "densify" not in off[2] and "densify_counts" not in off[2] and off[2]["params"]["means"].shape[0] == 300


def test_strategy_on_is_the_ops_written_out(hip_lib, scene, thresholds):
    cfg = _cfg(thresholds)
    out, log, sp = _run(scene, cfg, 12)
    log2, sp2, oracle_rows, resets = _written_out(scene, cfg, 12)
    assert torch.equal(log, log2) and bool(torch.isfinite(log).all())
    assert _same_splats(sp, sp2)
    counts = sp["densify_counts"]
    print(f"[densify loop] thresholds {thresholds}; (cloned, split, pruned, U_after) per refine {counts.tolist()}; oracle rows and margins {oracle_rows}")
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.shape == (3, 4)
    assert min(counts[0, :3].tolist()) > 0                                              # clone, split and prune all occur at the first refine
    assert all(mg >= 1e-6 for _, mg in oracle_rows)
    assert [r for r, _ in oracle_rows] == counts[:, 3].tolist()                          # the numpy oracle on the device's state
    U = int(counts[-1, 3])
    assert sp["params"]["means"].shape[0] == U and out.means.shape == (1, U, 3) and out.harmonics.shape[1] == U
    assert all(sp[g][n].shape[0] == U for g in ("params", "m", "v") for n in NAMES) and sp["densify"]["grad2d"].shape == (U,)
    assert sp["keep"].shape == (300,)                                                   # "keep" describes creation only
    # the opacity reset after step 6
    assert [i for i, _, _ in resets] == [6]
    _, before, after = resets[0]
    cap = math.log(2 * cfg.densify_prune_opa / (1 - 2 * cfg.densify_prune_opa))
    assert bool((before > cap).any()) and float(after.max()) == np.float32(cap) and torch.equal(after[before <= cap], before[before <= cap])
    plain = _run(scene, type(cfg)(seed=1), 12)
    assert torch.equal(plain[1][:4], log[:4]) and not torch.equal(plain[1], log)          # nothing changes before the first refine


def test_opacity_reset_is_visible(hip_lib, scene, thresholds):
    cfg = _cfg(thresholds)
    cap = np.float32(math.log(2 * cfg.densify_prune_opa / (1 - 2 * cfg.densify_prune_opa)))
    _, _, six = _run(scene, cfg, 6)
    _, _, seven = _run(scene, cfg, 7)
    assert float(six["params"]["opacities"].max()) > cap and bool(six["m"]["opacities"].any())
    assert float(seven["params"]["opacities"].max()) == cap
    assert not bool(seven["m"]["opacities"].any()) and not bool(seven["v"]["opacities"].any())
    assert bool(seven["m"]["means"][:10].any())                                         # the other moments are left alone


def test_reproducible_and_continued(hip_lib, scene, thresholds):
    """two runs agree bit for bit; `splats` through two calls of 6 steps is one call of 12 (seed 5: the view order of steps 6-11
    repeats that of steps 0-5, as in test_post_opt_mcmc_gpu.test_continuation)"""
    from vist3a_amd.post_opt import view_order
    a, b = _run(scene, _cfg(thresholds), 12), _run(scene, _cfg(thresholds), 12)
    assert torch.equal(a[1], b[1]) and _same_splats(a[2], b[2]) and all(torch.equal(getattr(a[0], f), getattr(b[0], f)) for f in FIELDS)
    cfg = _cfg(thresholds, seed=5)
    assert view_order(3, 12, cfg.seed)[6:] == view_order(3, 6, cfg.seed)
    whole = _run(scene, cfg, 12)
    _, log_a, sp = _run(scene, cfg, 6)
    assert sp["step"] == 6 and sp["densify_counts"].shape == (1, 4)
    out, log_b, sp = _run(scene, cfg, 6, splats=sp)
    assert torch.equal(torch.cat([log_a, log_b]), whole[1]) and _same_splats(sp, whole[2]) and sp["densify_counts"].shape == (3, 4)
    assert all(torch.equal(getattr(out, f), getattr(whole[0], f)) for f in FIELDS)


def test_absgrad_changes_the_fates_only(hip_lib, scene, thresholds):
    plain, absg = _run(scene, _cfg(thresholds), 5), _run(scene, _cfg(thresholds, densify_absgrad=True), 5)
    assert torch.equal(plain[1][:4], absg[1][:4])                                        # the renders and updates before the first refine
    assert plain[2]["densify_counts"].shape == absg[2]["densify_counts"].shape == (1, 4)
    a, b = plain[2]["densify_counts"][0].tolist(), absg[2]["densify_counts"][0].tolist()
    print(f"[densify loop] first refine (cloned, split, pruned, U_after): plain {a}, absgrad {b}")
    assert a != b and b[0] + b[1] > a[0] + a[1]                                          # sums of absolute values are larger: more grow


def test_cap_turns_a_growing_refine_into_prune_only(hip_lib, scene, thresholds):
    free = _run(scene, _cfg(thresholds), 4)[2]["densify_counts"][0].tolist()
    assert free[3] > 300 and free[0] > 0 and free[1] > 0
    capped = _run(scene, _cfg(thresholds, densify_cap_max=300), 4)[2]
    row = capped["densify_counts"][0].tolist()
    assert row[0] == row[1] == 0 and row[2] > 0 and row[3] == 300 - row[2] and capped["params"]["means"].shape[0] == row[3]
    roomy = _run(scene, _cfg(thresholds, densify_cap_max=free[3]), 4)[2]["densify_counts"][0].tolist()
    assert roomy == free                                                                # at the cap is not above it


def test_an_empty_scene_raises(hip_lib, scene, thresholds):
    with pytest.raises(RuntimeError, match="pruned all"):
        _run(scene, _cfg({**thresholds, "densify_prune_opa": 0.49, "densify_grow_grad2d": 1e9}, lr_opacities=0.0), 4,
             prepare=lambda sp: sp["params"]["opacities"].fill_(-3.0))
