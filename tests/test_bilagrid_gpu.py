"""GPU tests of the bilateral-grid colour compensation: csrc/bilagrid.hip (ops.bilagrid_slice, ops.bilagrid_tv) and its use in
vist3a_amd.post_opt (PostOptConfig.use_bilateral_grid).

Reference: tests/bilagrid_oracle.py in fp64 (pinned to the reference's own module by tests/test_bilagrid_host.py; its fp32 run is
the comparison figure), and for the loop oracle/gsplat_raster.py + tests/ssim_loss_oracle.py + the bilateral-grid oracle +
torch.optim.Adam in fp64 with the closed-form rate, built as tests/test_post_opt_gpu.py builds it.

Bounds.  Output, d_rgb, d_grids and the TV gradient: ||a - a64|| / ||a64|| <= 1.2e-7, one fp32 rounding of the stored value (6e-8)
with a factor 2 (the kernels work in fp64 and round once).  TV value: 1e-12 relative (fp64 on both sides, only the summation
order differs).  Identity grids: 6e-8 relative (one rounding).  Loop: the project's rule min(2 x the largest value measured on
an MI355X, 1e-3), MEASURED["loop_bilagrid"] (the run recorded in DESIGN.md section 7f; None selects the ceiling).
Every test prints its figures before it asserts and logs them through the `parity` fixture."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

from oracle import gsplat_raster as G

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bilagrid_oracle as BO  # noqa: E402
import post_opt_oracle as PO  # noqa: E402
import ssim_loss_oracle as SO  # noqa: E402
import test_post_opt_gpu as TP  # noqa: E402

pytestmark = pytest.mark.gpu

CEILING = 1e-3
TOL, TV_TOL, IDENTITY_TOL = 1.2e-7, 1e-12, 6e-8
MEASURED = dict(loop_bilagrid=1.970e-5)
# rgb (N, H, W), grid (GX, GY, L): the smallest; ragged; two images with different grids; most vertex columns without a pixel in
# their support (they must come out exactly 0); several workgroups at the default shape
CASES = [((1, 1, 1), (2, 2, 2)), ((1, 5, 7), (4, 3, 5)), ((2, 13, 37), (5, 3, 4)), ((1, 3, 2), (16, 16, 8)), ((1, 45, 70), (16, 16, 8))]
_id = lambda c: "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1]))


def gate(name):
    return CEILING if MEASURED[name] is None else min(2 * MEASURED[name], CEILING)


def _rel(a, b):
    return float((a.detach().cpu().double() - b.detach().double()).norm() / b.detach().double().norm().clamp_min(1e-300))


_REF = {}


def reference(case):
    """inputs and the fp64 / fp32 oracle results of one case (reference layout), computed once and shared"""
    if case not in _REF:
        (N, H, W), (GX, GY, L) = case
        inp = BO.make_inputs(N, H, W, GX, GY, L)
        _REF[case] = (inp, BO.run(*inp, torch.float64), BO.run(*inp, torch.float32))
    return _REF[case]


def hip(rgb, grids_ref, d_out, scale=1.0):
    """-> dict(out, d_rgb, d_grids, tv, d_tv) on the device, grids and their gradients in the package's layout"""
    from vist3a_amd import ops
    r, g = rgb.cuda().requires_grad_(True), ops.bilagrid_from_reference(grids_ref).cuda().requires_grad_(True)
    out = ops.bilagrid_slice(r, g)
    d_rgb, d_grids = torch.autograd.grad(out, (r, g), scale * d_out.cuda())
    tv = ops.bilagrid_tv(g)
    d_tv, = torch.autograd.grad(tv, g, torch.tensor(scale, dtype=torch.float64, device="cuda"))
    return dict(out=out.detach(), d_rgb=d_rgb, d_grids=d_grids, tv=tv.detach().reshape(1), d_tv=d_tv)


def _ours(t):   # a gradient in the reference layout -> the package's
    return t.permute(0, 2, 3, 4, 1)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_matches_oracle(hip_lib, parity, case):
    (rgb, grids, d_out), r64, r32 = reference(case)
    (N, H, W), (GX, GY, L) = case
    h = hip(rgb, grids, d_out)
    want = {k: (_ours(v) if k in ("d_grids", "d_tv") else v) for k, v in r64.items()}
    want32 = {k: (_ours(v) if k in ("d_grids", "d_tv") else v) for k, v in r32.items()}
    e = {k: _rel(h[k], want[k]) for k in want}
    e32 = {k: _rel(want32[k], want[k]) for k in want}
    print(f"[bilagrid {_id(case)}] hip vs fp64 (oracle fp32 vs fp64): " + "  ".join(f"{k} {e[k]:.3e} ({e32[k]:.3e})" for k in e)
          + f"   bounds {TOL:.1e}, tv {TV_TOL:.1e}")
    parity(f"bilagrid::parity[{_id(case)}]", **{k + "_rel_l2": v for k, v in e.items()}, **{"oracle_fp32_" + k + "_rel_l2": v for k, v in e32.items()},
           bound=TOL, bound_tv=TV_TOL)
    assert h["out"].dtype == torch.float32 and h["out"].shape == rgb.shape and h["d_rgb"].shape == rgb.shape
    assert h["d_grids"].shape == (N, L, GY, GX, 12) and h["d_tv"].shape == (N, L, GY, GX, 12) and h["d_grids"].dtype == torch.float32
    assert h["tv"].dtype == torch.float64
    for k in ("out", "d_rgb", "d_grids", "d_tv"):
        assert e[k] <= TOL, (k, e[k])
    assert e["tv"] <= TV_TOL, e["tv"]
    # a vertex that no pixel reaches has a gradient of exactly 0, as in the oracle
    zero = want["d_grids"] == 0
    assert bool((h["d_grids"].cpu()[zero] == 0).all())
    if case[0] == (1, 3, 2):
        assert float(zero.float().mean()) > 0.5


# ------------------------------------------------------------------------------------------------ 2. exact properties
def test_guidance_gradient_is_zero_at_the_clamps(hip_lib, parity):
    """Black, white and out-of-range pixels sit on a clamp of the guidance axis: d_rgb there is the matrix term alone.  Against the
    oracle with the guidance detached (1.2e-7; a guidance term left in would be of order 1), and exactly: at the lower clamp the
    upper plane must not matter (its vertices are rewritten and the gradient keeps its bits), and with identity grids, where the
    matrix term is d_out itself and the planes differ only past the upper end, d_rgb == d_out bit for bit."""
    from vist3a_amd import ops
    case = ((1, 45, 70), (16, 16, 8))
    (rgb, grids, d_out), _, _ = reference(case)
    L = 8
    gz = BO.guidance(rgb.double()) * (L - 1)
    low, high = gz <= 0, gz >= L - 1
    black, white = (rgb == 0).all(-1), (rgb == 1).all(-1)
    assert int(black.sum()) > 100 and int(white.sum()) == 2 and bool(low[black].all()) and bool(high[white].all())
    assert int((low & ~black).sum()) >= 1 and int((high & ~white).sum()) >= 1      # the -0.2 and the 1.3 pixel
    r = rgb.double().requires_grad_(True)
    matrix_only, = torch.autograd.grad(BO.slice_grid(r, grids.double(), guide=r.detach()), r, d_out.double())
    h = hip(rgb, grids, d_out)
    clamped = low | high
    e, e_in = _rel(h["d_rgb"].cpu()[clamped], matrix_only[clamped]), _rel(h["d_rgb"].cpu()[~clamped], matrix_only[~clamped])
    print(f"[bilagrid clamps] d_rgb against the matrix term alone: clamped pixels {e:.3e} (bound {TOL:.1e}), the others {e_in:.3e}")
    parity("bilagrid::clamps", clamped_rel_l2=e, inside_rel_l2=e_in, bound=TOL)
    assert e <= TOL and e_in > 1e-3
    # lower clamp: plane 1 rewritten
    other = grids.clone()
    other[:, :, 1] += 3.0
    h2 = hip(rgb, other, d_out)
    assert torch.equal(h2["d_rgb"].cpu()[low], h["d_rgb"].cpu()[low]) and not torch.equal(h2["d_rgb"].cpu()[~clamped], h["d_rgb"].cpu()[~clamped])
    # identity grids: the input comes back, and the gradient is d_out
    ident = BO.identity(1, 16, 16, 8)
    hi = hip(rgb, ident, d_out)
    ei = _rel(hi["out"], rgb)
    print(f"[bilagrid identity] output against the input {ei:.3e} (bound {IDENTITY_TOL:.1e}); tv {float(hi['tv']):.3e}")
    parity("bilagrid::identity", out_rel_l2=ei, bound=IDENTITY_TOL)
    assert ei <= IDENTITY_TOL and float(hi["tv"]) == 0.0 and bool((hi["d_tv"] == 0).all())
    assert torch.equal(hi["d_rgb"].cpu()[clamped], d_out[clamped])
    assert torch.equal(ops.bilagrid_identity(1, 16, 16, 8, "cuda").cpu(), ops.bilagrid_from_reference(ident))


def test_linear_and_deterministic(hip_lib):
    (rgb, grids, d_out), _, _ = reference(((2, 13, 37), (5, 3, 4)))
    a, b, c = hip(rgb, grids, d_out), hip(rgb, grids, d_out), hip(rgb, grids, d_out, scale=2.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in ("d_rgb", "d_grids", "d_tv"):
        assert torch.equal(c[k], 2 * a[k]) and float(a[k].abs().max()) > 0, k
    (rgb, grids, d_out), _, _ = reference(((1, 45, 70), (16, 16, 8)))
    a, b, c = hip(rgb, grids, d_out), hip(rgb, grids, d_out), hip(rgb, grids, d_out, scale=2.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in ("d_rgb", "d_grids", "d_tv"):
        assert torch.equal(c[k], 2 * a[k]), k


def test_every_gradient_element_is_written_and_shape_errors(hip_lib):
    from vist3a_amd import lib as L
    from vist3a_amd import ops
    lib = L.load()
    case = ((1, 3, 2), (16, 16, 8))
    (rgb, grids, d_out), _, _ = reference(case)
    want = hip(rgb, grids, d_out)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r, g, go = rgb.cuda(), ops.bilagrid_from_reference(grids).cuda(), d_out.cuda().contiguous()
    d_rgb, d_grids, d_tv = torch.full_like(r, float("nan")), torch.full_like(g, float("nan")), torch.full_like(g, float("nan"))
    a = L.BilagridSliceArgs(p(r), p(g), 1, 3, 2, 16, 16, 8)
    assert lib.v3a_bilagrid_slice_backward(C.byref(a), p(go), p(d_rgb), p(d_grids), st) == 0
    tv = L.BilagridTvArgs(p(g), 1, 16, 16, 8, None, None, 0)
    one = torch.ones(1, device="cuda", dtype=torch.float64)
    assert lib.v3a_bilagrid_tv_backward(C.byref(tv), p(one), p(d_tv), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_rgb, want["d_rgb"]) and torch.equal(d_grids, want["d_grids"]) and torch.equal(d_tv, want["d_tv"])
    # a grid that is not 16-byte aligned takes the scalar loads: the same bits
    buf = torch.zeros(g.numel() + 4, device="cuda")
    gu = buf[1:1 + g.numel()].view(g.shape)
    gu.copy_(g)
    assert gu.data_ptr() % 16 != 0
    ru = r.clone().requires_grad_(True)
    out_u = ops.bilagrid_slice(ru, gu)
    gr_u, = torch.autograd.grad(out_u, ru, go)
    assert torch.equal(out_u.detach(), want["out"]) and torch.equal(gr_u, want["d_rgb"])
    # shapes the kernels refuse
    z = torch.zeros(1, 4, 5, 3, device="cuda")
    for shape in ((1, 8, 16, 1, 12), (1, 8, 1, 16, 12), (1, 1, 16, 16, 12)):       # GX = 1, GY = 1, L = 1
        with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
            ops.bilagrid_slice(z, torch.zeros(shape, device="cuda"))
        with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
            ops.bilagrid_tv(torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError, match="one grid per image"):
        ops.bilagrid_slice(z, torch.zeros(2, 2, 2, 2, 12, device="cuda"))
    with pytest.raises(ValueError):
        ops.bilagrid_slice(z, torch.zeros(1, 12, 2, 2, 2, device="cuda"))
    with pytest.raises(ValueError):
        ops.bilagrid_slice(z.double(), torch.zeros(1, 2, 2, 2, 12, device="cuda"))
    with pytest.raises(ValueError):
        ops.bilagrid_slice(z.permute(0, 2, 1, 3), torch.zeros(1, 2, 2, 2, 12, device="cuda"))


# ------------------------------------------------------------------------------------------------ 3. the loop
def oracle_loop(dt, sc, cams, raster, order, start, targets, cfg, train, grid_on):
    """The post-optimisation loop on the CPU in `dt`: oracle rasteriser, SSIM oracle, bilateral-grid oracle, torch.optim.Adam, the
    grid's closed-form rate.  cams = (view, campos, K) per view; raster[j] = (tile offsets, flatten ids, radii > 0) of view j;
    start = dict(means, cov, logits, sh); train: names out of ("opacities", "sh").  -> (loss curve, tv curve, sh [U,3,K], grids)"""
    W, H, V = sc["W"], sc["H"], targets.shape[0]
    view, campos, K = cams
    lg = start["logits"].clone().to(dt).requires_grad_("opacities" in train)
    s0 = start["sh"][..., :1].clone().to(dt).requires_grad_("sh" in train)
    sN = start["sh"][..., 1:].clone().to(dt).requires_grad_("sh" in train)
    opts = []
    if "opacities" in train:
        opts.append(torch.optim.Adam([lg], lr=cfg.lr_opacities, eps=cfg.eps, betas=cfg.betas))
    if "sh" in train:
        opts += [torch.optim.Adam([s0], lr=cfg.lr_sh, eps=cfg.eps, betas=cfg.betas), torch.optim.Adam([sN], lr=cfg.lr_sh / 20, eps=cfg.eps, betas=cfg.betas)]
    grids = gopt = None
    if grid_on:
        GX, GY, L = cfg.bilateral_grid_shape
        grids = BO.identity(V, GX, GY, L, dt).requires_grad_(True)
        gopt = torch.optim.Adam([grids], lr=cfg.bilagrid_lr, eps=1e-15, betas=cfg.betas)
        opts.append(gopt)
    means, cov = start["means"].to(dt), start["cov"].to(dt)
    curve, tvs = [], []
    for s, j in enumerate(order):
        offs, ids, mask = raster[j]
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(G, "f32", dt)
            p = G.project(means, cov, view[j].cpu().to(dt), K[j].cpu().to(dt), W, H)
            col = G.sh_colors(means, campos[j].cpu().to(dt), torch.cat([s0, sN], -1).permute(0, 2, 1), 1) * mask[:, None]
            col4 = torch.cat([col, p["depths"][:, None]], -1)
            img, _ = G.rasterize(p["means2d"], p["conics"], col4, torch.sigmoid(lg), W, H, offs, ids, torch.zeros(4, dtype=dt))
        color = img[None, ..., :3].clamp(0, 1)
        tv = torch.zeros((), dtype=dt)
        if grid_on:
            color = BO.slice_grid(color, grids[j:j + 1])
            tv = BO.total_variation(grids)
            gopt.param_groups[0]["lr"] = BO.learning_rate(s, cfg.bilagrid_lr, cfg.bilagrid_warmup_steps, cfg.max_steps)
        loss = SO.photometric_loss(color, targets[j:j + 1].cpu().to(dt), cfg.ssim_lambda)[0] + (cfg.bilagrid_tv_lambda * tv if grid_on else 0)
        for o in opts:
            o.zero_grad()
        loss.backward()
        for o in opts:
            o.step()
        curve.append(float(loss.detach()))
        tvs.append(float(tv.detach()))
    return (torch.tensor(curve, dtype=torch.float64), torch.tensor(tvs, dtype=torch.float64), torch.cat([s0, sN], -1).detach(),
            None if grids is None else grids.detach())


def _hip_raster(sc, kept, W, H):
    """what the HIP forward fixes for the oracle: cameras, and per view its composite order and radii mask"""
    _, pr, r, cams = TP._targets(sc, kept)
    U = kept.means.shape[1]
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    offs_all, ids_all, radii = r["tile_offsets"].cpu().long(), r["flatten_ids"].cpu().long(), pr["radii"].cpu()
    raster = []
    for j in range(3):
        lo, hi = int(offs_all[j * ntiles]), int(offs_all[(j + 1) * ntiles])
        raster.append((offs_all[j * ntiles:(j + 1) * ntiles + 1] - lo, ids_all[lo:hi] - j * U, radii[j] > 0))
    return cams, raster


def test_loop_with_grids_follows_oracle(hip_lib, parity):
    """20 steps on opacity logits, harmonics and the grids (shape (4,4,3), bilagrid_warmup_steps = 5) against the same loop on the
    CPU in fp64 (and fp32): the start, the targets and the view order of tests/test_post_opt_gpu.py's loop test.
    Measured on an MI355X (MEASURED): total loss within 1.970e-5 per step (fp32 oracle 2.390e-5), the TV column
    within 7.0e-4 (it starts at 4.8e-10: the grids leave the identity by steps of 2e-5), the final grids within 6.0e-5;
    loss 3.77220e-02 -> 1.35323e-02."""
    from vist3a_amd.models.types import Gaussians
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, view_order
    sc = PO.loop_scene()
    W, H, steps = sc["W"], sc["H"], 20
    target, _, _, _ = TP._targets(sc, TP._scene_gaussians(sc))
    start = TP._scene_gaussians(sc, perturb_seed=42, geometry=False)
    cfg = PostOptConfig(params=("opacities", "sh"), seed=5, use_bilateral_grid=True, bilateral_grid_shape=(4, 4, 3), bilagrid_warmup_steps=5)
    sp = create_splats(start, cfg, 3)
    assert sp["bil_grids"].shape == (3, 3, 4, 4, 12) and torch.equal(sp["bil_grids"].cpu(), BO.identity(3, 4, 4, 3).permute(0, 2, 3, 4, 1))
    out, log = post_optimize(start, target, sc["c2w"].cuda(), sc["Kn"].cuda(), cfg, steps=steps, splats=sp)
    c_hip, tv_hip = log[:, 0].cpu(), log[:, 3].cpu()
    keep = sp["keep"]
    kept = TP._scene_gaussians(sc)
    kept = Gaussians(*(getattr(kept, f)[:, keep].contiguous() for f in ("means", "covariances", "harmonics", "opacities", "scales", "rotations")))
    cams, raster = _hip_raster(sc, kept, W, H)
    sp0 = create_splats(start, cfg)
    st = dict(means=kept.means[0].cpu(), cov=kept.covariances[0].cpu(), logits=sp0["params"]["opacities"].cpu(), sh=sp0["params"]["sh"].cpu())
    order = view_order(3, steps, cfg.seed)
    c64, tv64, _, g64 = oracle_loop(torch.float64, sc, cams, raster, order, st, target, cfg, ("opacities", "sh"), True)
    c32, _, _, _ = oracle_loop(torch.float32, sc, cams, raster, order, st, target, cfg, ("opacities", "sh"), True)
    e, e32 = float(((c_hip - c64).abs() / c64).max()), float(((c32 - c64).abs() / c64).max())
    etv = float(((tv_hip - tv64).abs() / tv64.clamp_min(1e-300))[1:].max())
    eg = _rel(sp["bil_grids"], g64.permute(0, 2, 3, 4, 1))
    print(f"[loop+grids] loss {c64[0]:.5e} -> {c64[-1]:.5e} (oracle fp64), {c_hip[0]:.5e} -> {c_hip[-1]:.5e} (hip); tv {tv64[1]:.3e} -> {tv64[-1]:.3e}")
    print(f"[loop+grids] per-step relative loss difference, max over {steps} steps: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   "
          f"gate {gate('loop_bilagrid'):.1e};  tv alone {etv:.3e};  final grids rel l2 {eg:.3e}")
    parity("bilagrid::loop", rel_max=e, oracle_fp32_rel_max=e32, tv_rel_max=etv, grids_rel_l2=eg, gate=gate("loop_bilagrid"), first=float(c64[0]),
           last=float(c64[-1]))
    assert log.shape == (steps, 4) and float(tv_hip[0]) == 0.0 and float(tv64[0]) == 0.0 and float(tv_hip[-1]) > 0
    assert torch.equal(out.means, kept.means) and not sp["bil_grids"].requires_grad and sp["step"] == steps
    assert not torch.equal(sp["bil_grids"].cpu(), BO.identity(3, 4, 4, 3).permute(0, 2, 3, 4, 1))
    assert e <= gate("loop_bilagrid"), e


def test_loop_off_is_unchanged(hip_lib):
    from vist3a_amd.post_opt import PostOptConfig, post_optimize
    sc = PO.loop_scene()
    target, _, _, _ = TP._targets(sc, TP._scene_gaussians(sc))
    start = TP._scene_gaussians(sc, perturb_seed=43)
    ext, Kn = sc["c2w"].cuda(), sc["Kn"].cuda()
    off = PostOptConfig(seed=1, use_bilateral_grid=False, bilateral_grid_shape=(4, 4, 3), bilagrid_lr=1.0, bilagrid_warmup_steps=2, bilagrid_tv_lambda=3.0)
    (g1, log1), (g2, log2) = post_optimize(start, target, ext, Kn, PostOptConfig(seed=1), steps=6), post_optimize(start, target, ext, Kn, off, steps=6)
    fields = ("means", "covariances", "harmonics", "opacities", "scales", "rotations")
    assert log1.shape == (6, 3) and torch.equal(log1, log2) and all(torch.equal(getattr(g1, f), getattr(g2, f)) for f in fields)
    on = PostOptConfig(seed=1, use_bilateral_grid=True, bilateral_grid_shape=(4, 4, 3))
    g3, log3 = post_optimize(start, target, ext, Kn, on, steps=6)
    assert log3.shape == (6, 4) and bool(torch.isfinite(log3).all()) and torch.equal(log3[0, :3], log1[0, :3])      # identity grids at step 0
    assert not torch.equal(g3.harmonics, g1.harmonics) and g3.means.shape == g1.means.shape


CASTS = dict(gain=torch.tensor([[1.25, 1.10, 0.90], [0.80, 0.90, 1.10], [1.00, 0.85, 1.20]]), bias=torch.tensor([0.03, -0.02, 0.01]))
BEHAVIOUR = dict(steps=45, cfg=dict(params=("sh",), seed=0, use_bilateral_grid=True, bilateral_grid_shape=(4, 4, 3), bilagrid_lr=1e-2, bilagrid_warmup_steps=1))


def cast_targets(renders):
    """each view's render through its fixed colour cast (gain per channel, one bias), clamped to [0,1]"""
    return (renders * CASTS["gain"].to(renders.device)[:, None, None, :] + CASTS["bias"].to(renders.device)[:, None, None, None]).clamp(0, 1).contiguous()


def test_grids_absorb_a_per_view_colour_cast(hip_lib, parity):
    """Set-up: the targets are the scene's own renders (tests/post_opt_oracle.py::loop_scene, 3 views), each through a fixed colour
    cast (CASTS: per-channel gains between 0.8 and 1.25 and a bias, different for every view).  Only the harmonics train, from the
    TRUE scene, 45 steps, seed 0, once without grids and once with grids of shape (4,4,3) at bilagrid_lr = 1e-2 with a warm-up of
    one step (the reference's 2e-3 over 1000 steps would leave the grids at a hundredth of their rate for the whole test).  Without
    grids the casts can only go into the harmonics; with them most of it goes into the grids, so the harmonics end closer to their
    true values.  The fp64 oracle loop on the CPU shows the same direction: |sh - sh_true| = 1.317 without, 0.369 with (its own
    composite order; loss 4.67e-2 -> 5.24e-2 without, -> 5.31e-3 with); on an MI355X 1.316 and 0.366."""
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize
    sc = PO.loop_scene()
    true = TP._scene_gaussians(sc)
    renders, _, _, _ = TP._targets(sc, true)
    target = cast_targets(renders)
    ext, Kn = sc["c2w"].cuda(), sc["Kn"].cuda()
    on = PostOptConfig(**BEHAVIOUR["cfg"])
    off = PostOptConfig(**{**BEHAVIOUR["cfg"], "use_bilateral_grid": False})
    keep = create_splats(true, off)["keep"]
    sh_true = true.harmonics[0][keep]
    dist = {}
    for name, cfg in (("off", off), ("on", on)):
        g, log = post_optimize(true, target, ext, Kn, cfg, steps=BEHAVIOUR["steps"])
        dist[name] = float((g.harmonics[0] - sh_true).norm())
        print(f"[bilagrid behaviour] grids {name}: loss {float(log[0, 0]):.4e} -> {float(log[-3:, 0].mean()):.4e}, |sh - sh_true| = {dist[name]:.4e}")
    parity("bilagrid::behaviour", sh_distance_off=dist["off"], sh_distance_on=dist["on"])
    assert dist["on"] < dist["off"], dist
