"""GPU parity of the rasteriser's backward pass (csrc/raster_bwd.hip, ops.gs_render, DecoderSplattingCUDA with grad) against
torch.autograd through oracle/gsplat_raster.py in fp64.

Metric of tests 1-3: per gradient tensor ||g_hip - g_ref64|| / ||g_ref64|| over ALL Gaussians, nothing left out.  The fp64
reference is always driven with the HIP forward's radii mask and composite order, so both sides differentiate the same function.
Every test prints its measured errors, and beside them the fp32 oracle's error against the same fp64 gradients (the reference's
own rounding spread), before it asserts.

Gates: GATE below.  The project's per-kernel ceiling is 1e-3; a gate is 2x the error measured on an MI355X and never above the
ceiling.  MEASURED holds the figures of the run recorded in DESIGN.md section 7a; the 12-camera / 3 x 4-camera comparison of
test 4 measured 7e-8 .. 1e-7 and is asserted within the same gates."""
import math

import pytest
import torch

from oracle import gsplat_raster as G

pytestmark = pytest.mark.gpu

CEILING = 1e-3
# largest error measured per tensor over every case that reports it (MI355X), hip vs the fp64 oracle; beside it the fp32 oracle's
# own error against fp64 in the same cases was 6e-8 .. 1.2e-5.  "fit" is test 6's largest per-step relative loss difference.
MEASURED = dict(means2d=9.240e-6, conics=1.455e-6, colors=9.419e-7, opacity=1.020e-6,      # test 1 (entry gradients)
                means=2.889e-6, covars=2.539e-5, sh=1.624e-6, opacities=1.949e-6,           # tests 2 and 3
                scales=6.123e-7, quats=1.142e-6,                                            # test 3, covariance built in torch
                fit=3.993e-7)
GATE = {k: min(2 * v, CEILING) for k, v in MEASURED.items()}


def _scene(U, seed, spread=1.5, scale=0.15, z0=4.0, K=25):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(U, 3, generator=g) * torch.tensor([spread, spread, 1.0]) + torch.tensor([0.0, 0.0, z0])
    A = torch.randn(U, 3, 3, generator=g) * scale
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)
    sh = (torch.randn(U, 3, 25, generator=g) * 0.3)[:, :, :K].contiguous()  # Gaussians.harmonics layout [U,3,K]
    op = torch.rand(U, generator=g)
    return means, cov, sh, op


def _camera(W, H, f, yaw=0.2, t=(0.1, -0.2, 0.3)):
    c, s = math.cos(yaw), math.sin(yaw)
    view = torch.eye(4)
    view[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    view[:3, 3] = torch.tensor(t)
    K = torch.tensor([[f, 0, W / 2], [0, f * 1.1, H / 2], [0, 0, 1.0]])
    return view, K


def _cams(W, H, n=3, f=60.0):
    cs = [_camera(W, H, f + 5 * i, yaw=0.1 * i - 0.1, t=(0.05 * i, 0.0, 0.1 * i)) for i in range(n)]
    view = torch.stack([c[0] for c in cs])
    K = torch.stack([c[1] for c in cs])
    campos = torch.stack([torch.linalg.inv(c[0].double())[:3, 3].float() for c in cs]).contiguous()
    return view, campos, K


def _rel(a, b):
    return float((a.detach().cpu().double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _report(parity, test, name, hip, ref64, ref32):
    e, e32 = _rel(hip, ref64), _rel(ref32, ref64)
    print(f"[{test}] d_{name}: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {GATE[name]:.1e}")
    parity(f"raster_bwd::{test}", tensor=name, rel_l2=e, oracle_fp32_rel_l2=e32, gate=GATE[name])
    return e


def _order_of(out, j, U, ntiles):
    """camera j's tile offsets / local ids (int64, as the oracle takes them) out of a batched return_order result"""
    offs = out["tile_offsets"].cpu().long()
    lo, hi = int(offs[j * ntiles]), int(offs[(j + 1) * ntiles])
    return offs[j * ntiles:(j + 1) * ntiles + 1] - lo, out["flatten_ids"].cpu().long()[lo:hi] - j * U


def _oracle_render(dtype, means, cov, sh_uk3, op, view, campos, K, W, H, deg, mask, offs, ids, monkeypatch):
    """One camera, clamped RGB over white + depth + alpha, in `dtype`, with the given radii mask and composite order."""
    with monkeypatch.context() as m:
        m.setattr(G, "f32", dtype)
        pr = G.project(means, cov, view.to(dtype), K.to(dtype), W, H)
        col = G.sh_colors(means, campos.to(dtype), sh_uk3, deg) * mask[:, None]
        col4 = torch.cat([col, pr["depths"][:, None]], -1)
        img, alpha = G.rasterize(pr["means2d"], pr["conics"], col4, op, W, H, offs, ids, torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=dtype))
    return img[..., :3].clamp(0, 1), img[..., 3], alpha


# ------------------------------------------------------------------------------------------------ 1. blend backward alone
@pytest.mark.parametrize("U,W,H,seed", [(3000, 100, 70, 3), (400, 64, 48, 4)])
def test_blend_backward_matches_oracle(hip_lib, parity, monkeypatch, U, W, H, seed):
    from vist3a_amd import ops
    means, cov, sh, op = _scene(U, seed, scale=0.25)
    view, campos, K = _cams(W, H, 1)
    pr = ops.gs_project(means.cuda(), cov.cuda(), sh.cuda(), view.cuda(), campos.cuda(), K.cuda(), W, H)
    bg = torch.ones(3, device="cuda")
    out = ops.gs_rasterize(pr, op.cuda(), W, H, background=bg, clamp_rgb=True, return_order=True)
    g = torch.Generator().manual_seed(seed + 100)
    dc, dd, da = torch.randn(1, H, W, 3, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    eg = ops.gs_rasterize_backward(pr, op.cuda(), W, H, out["tile_offsets"], out["flatten_ids"].contiguous(), dc.cuda(), dd.cuda(), da.cuda(),
                                   background=bg, clamp_rgb=True)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    offs, ids = _order_of(out, 0, U, ntiles)
    ref = {}
    for dt in (torch.float64, torch.float32):
        lv = [pr[k][0].cpu().to(dt).requires_grad_(True) for k in ("means2d", "conics", "colors")] + [op.clone().to(dt).requires_grad_(True)]
        with monkeypatch.context() as m:
            m.setattr(G, "f32", dt)
            img, alpha = G.rasterize(lv[0], lv[1], lv[2], lv[3], W, H, offs, ids, torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=dt))
        loss = (img[..., :3].clamp(0, 1) * dc[0].to(dt)).sum() + (img[..., 3] * dd[0].to(dt)).sum() + (alpha * da[0].to(dt)).sum()
        loss.backward()
        ref[dt] = [t.grad for t in lv]
    errs = {}
    for i, (name, key) in enumerate((("means2d", "d_means2d"), ("conics", "d_conics"), ("colors", "d_colors"), ("opacity", "d_opacity"))):
        errs[name] = _report(parity, f"blend[{U}]", name, eg[key][0], ref[torch.float64][i], ref[torch.float32][i])
    for name, e in errs.items():
        assert e < GATE[name], (name, e)


# ------------------------------------------------------------------------------------------------ 2. projection backward alone
@pytest.mark.parametrize("deg,layout", [(4, 1), (3, 0), (1, 1)])
def test_projection_backward_matches_oracle(hip_lib, parity, monkeypatch, deg, layout):
    from vist3a_amd import ops
    U, W, H = 2000, 96, 80
    means, cov, sh, op = _scene(U, 11, scale=0.2)
    view, campos, K = _cams(W, H, 2)
    shl = (sh if layout == 1 else sh.permute(0, 2, 1)).contiguous()
    pr = ops.gs_project(means.cuda(), cov.cuda(), shl.cuda(), view.cuda(), campos.cuda(), K.cuda(), W, H, sh_degree=deg, sh_layout=layout)
    radii = pr["radii"]
    g = torch.Generator().manual_seed(12)
    vm2, vcon, vcol, vop = (torch.randn(2, U, n, generator=g) for n in (2, 3, 4, 1))
    eg = dict(d_means2d=vm2.cuda(), d_conics=vcon.cuda(), d_colors=vcol.cuda(), d_opacity=vop[..., 0].contiguous().cuda())
    dm, dcov, dsh, dop = ops.gs_project_backward(means.cuda(), cov.cuda(), shl.cuda(), view.cuda(), campos.cuda(), K.cuda(), W, H, radii, eg,
                                                 sh_degree=deg, sh_layout=layout)
    ref = {}
    for dt in (torch.float64, torch.float32):
        lv = [t.clone().to(dt).requires_grad_(True) for t in (means, cov, sh)]
        loss = 0
        for j in range(2):
            mask = (radii[j] > 0).cpu()
            with monkeypatch.context() as m:
                m.setattr(G, "f32", dt)
                p = G.project(lv[0], lv[1], view[j].to(dt), K[j].to(dt), W, H)
                col = G.sh_colors(lv[0], campos[j].to(dt), lv[2].permute(0, 2, 1), deg)
            col4 = torch.cat([col, p["depths"][:, None]], -1)
            mk = mask[:, None].to(dt)
            loss = loss + (p["means2d"] * mk * vm2[j].to(dt)).sum() + (p["conics"] * mk * vcon[j].to(dt)).sum() + (col4 * mk * vcol[j].to(dt)).sum()
        loss.backward()
        ref[dt] = [t.grad for t in lv]
    ref_sh = {dt: (ref[dt][2] if layout == 1 else ref[dt][2].permute(0, 2, 1)) for dt in ref}
    errs = dict(means=_report(parity, f"project[deg{deg},layout{layout}]", "means", dm, ref[torch.float64][0], ref[torch.float32][0]),
                covars=_report(parity, f"project[deg{deg},layout{layout}]", "covars", dcov, ref[torch.float64][1], ref[torch.float32][1]),
                sh=_report(parity, f"project[deg{deg},layout{layout}]", "sh", dsh, ref_sh[torch.float64], ref_sh[torch.float32]))
    # the opacity gradient is the sum of the per-camera shares over visible entries, cameras in index order
    want = (vop[..., 0] * (radii > 0).cpu()).sum(0)
    assert torch.allclose(dop.cpu(), want, rtol=1e-6, atol=1e-6)
    nb = (deg + 1) ** 2
    hi = dsh[:, :, nb:] if layout == 1 else dsh[:, nb:, :]
    assert float(hi.abs().max()) == 0 if hi.numel() else True                      # bands above the degree are written as zero
    gone = (radii == 0).all(0)
    assert int(gone.sum()) > 0 and float(dm[gone].abs().max()) == 0 and float(dcov[gone].abs().max()) == 0 and float(dsh[gone].abs().max()) == 0
    assert float(dcov[:, [1, 2, 2], [0, 0, 1]].abs().max()) == 0                   # lower triangle
    for name, e in errs.items():
        assert e < GATE[name], (name, e)


# ------------------------------------------------------------------------------------------------ 3. end to end through the decoder
def _decoder_inputs(view, K, W, H):
    c2w = torch.stack([torch.linalg.inv(v) for v in view])[None]
    Kn = K.clone()
    Kn[:, 0] /= W
    Kn[:, 1] /= H
    return c2w, Kn[None]


def _quat_to_R(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(*q.shape[:-1], 3, 3)


def _cov_from(scales, quats):
    R = _quat_to_R(quats)
    return R @ torch.diag_embed(scales * scales) @ R.transpose(-1, -2)


@pytest.mark.parametrize("case,K,W,H", [("deg4", 25, 64, 48), ("deg2", 9, 64, 48), ("deg0", 1, 64, 48), ("odd_size", 25, 70, 50),
                                         ("scales_quats", 25, 64, 48), ("layout0_gs_render", 25, 64, 48)])
def test_end_to_end_gradients_match_oracle(hip_lib, parity, monkeypatch, case, K, W, H):
    from vist3a_amd import ops
    from vist3a_amd.models.decoder_splatting import DecoderSplattingCUDA
    from vist3a_amd.models.types import Gaussians
    U, deg = 500, math.isqrt(K) - 1
    means, cov, sh, op = _scene(U, 21, scale=0.25, K=K)
    view, campos, Kpix = _cams(W, H, 3)
    g = torch.Generator().manual_seed(22)
    scales = 0.1 + 0.3 * torch.rand(U, 3, generator=g)
    quats = torch.randn(U, 4, generator=g)
    wc, wd, wa = torch.randn(3, 3, H, W, generator=g), torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g)
    sq = case == "scales_quats"
    # ---- HIP
    lv = [t.clone().cuda().requires_grad_(True) for t in ((means, scales, quats, sh, op) if sq else (means, cov, sh, op))]
    cov_d = _cov_from(lv[1], lv[2]) if sq else lv[1]
    sh_d, op_d = lv[-2], lv[-1]
    if case == "layout0_gs_render":
        sh0 = sh.permute(0, 2, 1).contiguous().cuda().requires_grad_(True)
        lv[2] = sh0
        col, dep, alp = ops.gs_render(lv[0], lv[1], sh0, lv[3], view.cuda(), campos.cuda(), Kpix.cuda(), W, H, sh_degree=deg, sh_layout=0,
                                      background=torch.ones(3, device="cuda"), clamp_rgb=True)
        col = col.permute(0, 3, 1, 2)
    else:
        gs = Gaussians(means=lv[0][None], covariances=cov_d[None], harmonics=sh_d[None], opacities=op_d[None],
                       scales=torch.ones(1, U, 3).cuda(), rotations=torch.zeros(1, U, 4).cuda())
        c2w, Kn = _decoder_inputs(view, Kpix, W, H)
        dec = DecoderSplattingCUDA(background_color=(1.0, 1.0, 1.0), camera_batch=2)   # 3 views -> batches of 2 + 1
        out = dec.forward(gs, c2w.cuda(), Kn.cuda(), torch.full((1, 3), 0.1).cuda(), torch.full((1, 3), 100.0).cuda(), (H, W))
        assert out.color.grad_fn is not None and out.depth.grad_fn is not None and out.alpha.grad_fn is not None
        col, dep, alp = out.color[0], out.depth[0], out.alpha[0]
    loss = (col * wc.cuda()).sum() + (dep * wd.cuda()).sum() + (alp * wa.cuda()).sum()
    loss.backward()
    hip = [t.grad for t in lv]
    # ---- the function the HIP forward computed: its radii mask and composite order, per camera (cameras exactly as the decoder derives them)
    with torch.no_grad():
        cov_f = cov_d.detach().contiguous()
        sh_f = (lv[2] if case == "layout0_gs_render" else sh_d).detach().contiguous()
        if case == "layout0_gs_render":
            v_d, cp_d, K_d = view.cuda(), campos.cuda(), Kpix.cuda()
        else:
            w2c = torch.linalg.inv(c2w[0].float())
            v_d, cp_d = w2c.contiguous().cuda(), torch.linalg.inv(w2c)[:, :3, 3].contiguous().cuda()
            Kd = Kn[0].clone()
            Kd[:, 0] *= W
            Kd[:, 1] *= H
            K_d = Kd.contiguous().cuda()
        pr = ops.gs_project(lv[0].detach(), cov_f, sh_f, v_d, cp_d, K_d, W, H, sh_degree=deg, sh_layout=0 if case == "layout0_gs_render" else 1)
        fo = ops.gs_rasterize(pr, op_d.detach(), W, H, background=torch.ones(3, device="cuda"), return_order=True)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    ref = {}
    for dt in (torch.float64, torch.float32):
        rl = [t.clone().to(dt).requires_grad_(True) for t in ((means, scales, quats, sh, op) if sq else (means, cov, sh, op))]
        cov_r = _cov_from(rl[1], rl[2]) if sq else rl[1]
        tot = 0
        for j in range(3):
            offs, ids = _order_of(fo, j, U, ntiles)
            c, d, a = _oracle_render(dt, rl[0], cov_r, rl[-2].permute(0, 2, 1), rl[-1], v_d[j].cpu(), cp_d[j].cpu(), K_d[j].cpu(), W, H, deg,
                                     (pr["radii"][j] > 0).cpu(), offs, ids, monkeypatch)
            tot = tot + (c.permute(2, 0, 1) * wc[j].to(dt)).sum() + (d * wd[j].to(dt)).sum() + (a * wa[j].to(dt)).sum()
        tot.backward()
        ref[dt] = [t.grad for t in rl]
    if case == "layout0_gs_render":
        hip[2] = hip[2].permute(0, 2, 1)
    names = ("means", "scales", "quats", "sh", "opacities") if sq else ("means", "covars", "sh", "opacities")
    errs = {n: _report(parity, f"end_to_end[{case}]", n, h, r64, r32) for n, h, r64, r32 in zip(names, hip, ref[torch.float64], ref[torch.float32])}
    for n, e in errs.items():
        assert e < GATE[n], (n, e)


# ------------------------------------------------------------------------------------------------ 4. exact properties, production shape
def test_full_size_backward_properties(hip_lib, parity):
    from vist3a_amd import ops
    U, W, H, Cn = 1_000_000, 448, 448, 12
    means, cov, sh, op = _scene(U, 9, spread=2.0, scale=0.02, z0=5.0)
    op[::7] = 0
    cams = [_camera(W, H, 400.0, yaw=0.03 * i - 0.15, t=(0.02 * i, 0.0, 0.05 * i)) for i in range(Cn)]
    view = torch.stack([c[0] for c in cams]).cuda()
    K = torch.stack([c[1] for c in cams]).cuda()
    campos = torch.stack([torch.linalg.inv(c[0])[:3, 3] for c in cams]).contiguous().cuda()
    lv = [t.cuda().requires_grad_(True) for t in (means, cov, sh, op)]
    bg = torch.ones(3, device="cuda")
    g = torch.Generator().manual_seed(10)
    wc, wd, wa = (torch.randn(Cn, H, W, 3, generator=g).cuda(), torch.randn(Cn, H, W, generator=g).cuda(), torch.randn(Cn, H, W, generator=g).cuda())
    ws = ops.GsWorkspace()

    def run(scale, sl=slice(0, Cn)):
        col, dep, alp = ops.gs_render(*lv, view[sl].contiguous(), campos[sl].contiguous(), K[sl].contiguous(), W, H, background=bg,
                                      clamp_rgb=True, workspace=ws)
        loss = (col * (scale * wc[sl])).sum() + (dep * (scale * wd[sl])).sum() + (alp * (scale * wa[sl])).sum()
        return torch.autograd.grad(loss, lv)

    g1, g1b, g2, g0 = run(1.0), run(1.0), run(2.0), run(0.0)
    for a, b, c, z in zip(g1, g1b, g2, g0):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)                       # bit-identical run to run
        assert torch.equal(c, 2 * a)                   # linear in the incoming gradient, bit for bit
        assert bool((z == 0).all())
    assert float(g1[0].abs().max()) > 0 and float(g1[2].abs().max()) > 0
    with torch.no_grad():
        radii = ops.gs_project(lv[0], lv[1], lv[2], view, campos, K, W, H)["radii"]
    for rows, what in (((radii == 0).all(0), "culled in every camera"), (lv[3] == 0, "opacity 0")):
        assert int(rows.sum()) > 1000, what
        for t in g1:
            assert float(t[rows].abs().max()) == 0, what
    # 12 cameras in one call against the decoder's batching (3 x 4): autograd adds the per-batch sums in another association
    parts = [run(1.0, slice(j, j + 4)) for j in range(0, Cn, 4)]
    for name, a, *ps in zip(("means", "covars", "sh", "opacities"), g1, *parts):
        s = ps[0] + ps[1] + ps[2]
        e = float((s.double() - a.double()).norm() / a.double().norm())
        print(f"[full_size] d_{name}: 3 x 4 cameras vs 12 in one call {e:.3e}   gate {GATE[name]:.1e}")
        parity("raster_bwd::full_size_batching", tensor=name, rel_l2=e, gate=GATE[name])
        assert e < GATE[name], (name, e)


# ------------------------------------------------------------------------------------------------ 5. no behaviour change
def test_forward_unchanged_without_grad(hip_lib):
    from vist3a_amd.models.decoder_splatting import DecoderSplattingCUDA
    from vist3a_amd.models.types import Gaussians
    U, W, H = 2500, 112, 96
    means, cov, sh, op = _scene(U, 8, scale=0.2)
    view, campos, Kpix = _cams(W, H, 3, f=80.0)
    c2w, Kn = _decoder_inputs(view, Kpix, W, H)
    dec = DecoderSplattingCUDA(background_color=(1.0, 1.0, 1.0), camera_batch=2)

    def render(grad):
        t = [x.clone().cuda().requires_grad_(grad) for x in (means, cov, sh, op)]
        gs = Gaussians(means=t[0][None], covariances=t[1][None], harmonics=t[2][None], opacities=t[3][None],
                       scales=torch.ones(1, U, 3).cuda(), rotations=torch.zeros(1, U, 4).cuda())
        return dec.forward(gs, c2w.cuda(), Kn.cuda(), torch.full((1, 3), 0.1).cuda(), torch.full((1, 3), 100.0).cuda(), (H, W))

    with_grad = render(True)
    plain = render(False)
    with torch.no_grad():
        muted = render(True)
    assert with_grad.color.grad_fn is not None
    for o in (plain, muted):
        for k in ("color", "depth", "alpha"):
            t = getattr(o, k)
            assert t.grad_fn is None and not t.requires_grad
            assert torch.equal(t, getattr(with_grad, k).detach())
    ex = c2w.cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        t = [x.clone().cuda().requires_grad_(True) for x in (means, cov, sh, op)]
        gs = Gaussians(means=t[0][None], covariances=t[1][None], harmonics=t[2][None], opacities=t[3][None],
                       scales=torch.ones(1, U, 3).cuda(), rotations=torch.zeros(1, U, 4).cuda())
        dec.forward(gs, ex, Kn.cuda(), torch.full((1, 3), 0.1).cuda(), torch.full((1, 3), 100.0).cuda(), (H, W))


# ------------------------------------------------------------------------------------------------ 6. a short fit
def test_short_fit_follows_oracle(hip_lib, parity, monkeypatch):
    """20 Adam steps on opacity logits and SH coefficients (means / covariances fixed: the order and the radii stay put) against
    a target rendered from the unperturbed scene; the same loop on the CPU through the oracle's autograd in fp64 (and fp32)."""
    from vist3a_amd import ops
    U, W, H, steps = 200, 48, 48, 20
    means, cov, sh, op = _scene(U, 31, spread=0.8, scale=0.2)
    op = 0.05 + 0.9 * op
    view, campos, K = _cams(W, H, 3, f=50.0)
    g = torch.Generator().manual_seed(32)
    logit0 = torch.logit(op) + 0.8 * torch.randn(U, generator=g)
    sh0 = sh + 0.2 * torch.randn(U, 3, 25, generator=g)
    bg = torch.ones(3, device="cuda")
    md, cd, vd, pd, kd = means.cuda(), cov.cuda(), view.cuda(), campos.cuda(), K.cuda()
    with torch.no_grad():
        pr = ops.gs_project(md, cd, sh.cuda(), vd, pd, kd, W, H)
        tgt = ops.gs_rasterize(pr, op.cuda(), W, H, background=bg, return_order=True)
    target = tgt["color"].cpu()
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    orders = [_order_of(tgt, j, U, ntiles) for j in range(3)]
    masks = [(pr["radii"][j] > 0).cpu() for j in range(3)]

    def fit(loss_fn, dev, dt):
        lg, s = logit0.clone().to(dev, dt).requires_grad_(True), sh0.clone().to(dev, dt).requires_grad_(True)
        opt = torch.optim.Adam([lg, s], lr=0.05)
        curve = []
        for _ in range(steps):
            opt.zero_grad()
            loss = loss_fn(torch.sigmoid(lg), s)
            loss.backward()
            opt.step()
            curve.append(float(loss))
        return torch.tensor(curve, dtype=torch.float64)

    def hip_loss(o, s):
        col, _, _ = ops.gs_render(md, cd, s, o, vd, pd, kd, W, H, background=bg, clamp_rgb=True)
        return ((col - target.cuda()) ** 2).mean()

    def oracle_loss(dt):
        def f(o, s):
            cols = [_oracle_render(dt, means.to(dt), cov.to(dt), s.permute(0, 2, 1), o, view[j], campos[j], K[j], W, H, 4, masks[j],
                                   *orders[j], monkeypatch)[0] for j in range(3)]
            return ((torch.stack(cols) - target.to(dt)) ** 2).mean()
        return f

    c_hip = fit(hip_loss, "cuda", torch.float32)
    c64 = fit(oracle_loss(torch.float64), "cpu", torch.float64)
    c32 = fit(oracle_loss(torch.float32), "cpu", torch.float32)
    e = float(((c_hip - c64).abs() / c64).max())
    e32 = float(((c32 - c64).abs() / c64).max())
    print(f"[fit] loss {c64[0]:.5e} -> {c64[-1]:.5e} (oracle fp64), {c_hip[0]:.5e} -> {c_hip[-1]:.5e} (hip)")
    print(f"[fit] per-step relative loss difference, max over {steps} steps: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {GATE['fit']:.1e}")
    parity("raster_bwd::fit", rel_max=e, oracle_fp32_rel_max=e32, gate=GATE["fit"], first=float(c64[0]), last=float(c64[-1]))
    assert c_hip[-1] < c_hip[0] and c64[-1] < c64[0]
    assert e < GATE["fit"], e
