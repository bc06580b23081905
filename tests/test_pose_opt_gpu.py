"""GPU tests of pose optimisation: csrc/post_opt.hip (ops.camera_adjust), the CAM instantiations of csrc/raster_bwd.hip
(ops.gs_project_backward / ops.gs_render with camera_grad=True) and the loop's cfg.pose_opt.

References: tests/pose_opt_oracle.py (pinned to the reference's CameraOptModule by tests/test_pose_opt_host.py) and torch.autograd
through oracle/gsplat_raster.py in fp64 (G.f32 patched), driven with the HIP forward's radii mask and composite order; the oracle's
own fp32 run is printed beside every figure (its rounding spread) and logged through the `parity` fixture.

Metric: ||hip - ref64|| / ||ref64|| - for a camera gradient over the 15-vector (d_viewmat[:3,:], d_campos) of all cameras of the
call.  Gates: 2x the largest error measured on an MI355X (MEASURED), never above the per-kernel ceiling 1e-3."""
import sys
from pathlib import Path

import pytest
import torch

from oracle import gsplat_raster as G

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_opt_oracle as PO  # noqa: E402
import post_opt_oracle as SC  # noqa: E402
import raster_aa_oracle as AA  # noqa: E402
import ssim_loss_oracle as SO  # noqa: E402
import depth_loss_oracle as DO  # noqa: E402

pytestmark = pytest.mark.gpu

CEILING = 1e-3
# largest error per quantity over every case that reports it (MI355X), hip vs the fp64 reference; beside them the fp32 oracle's own
# error against fp64 in the same cases was 0 .. 1.2e-7 (adjust forward), 1.8e-8 .. 2.1e-7 (adjust backward), 7.6e-8 .. 1.1e-6
# (projection: the HIP error never exceeded it) and 4.1e-7 .. 9.95e-6 (end to end: the classic cases sit on a 0.999 alpha cap that
# both fp32 runs round across)
MEASURED = dict(adjust_fwd=2.337e-8, adjust_bwd=3.183e-8, cam_project=2.743e-7, cam_end_to_end=9.938e-6,
                loop=4.099e-7, loop_deltas=1.799e-7)   # 4(c); the fp32 oracle loop beside them: 4.8e-6 and 1.2e-6
GATE = {k: CEILING if v is None else min(2 * v, CEILING) for k, v in MEASURED.items()}


def _rel(a, b):
    return float((a.detach().cpu().double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _vec15(d_view, d_campos):
    return torch.cat([d_view.detach().cpu().double()[..., :3, :].reshape(-1, 12), d_campos.detach().cpu().double().reshape(-1, 3)], -1)


# ------------------------------------------------------------------------------------------------ 1. camera_adjust
@pytest.mark.parametrize("V", [1, 3, 13])
@pytest.mark.parametrize("size", [0.0, 1e-2, 0.5])
def test_camera_adjust_matches_oracle(hip_lib, parity, V, size):
    from vist3a_amd import ops
    c2w = PO.cameras(V, 20 + V, torch.float32)
    w2c = torch.linalg.inv(c2w).contiguous()                      # f32: the two bases are not exact inverses, as in the loop
    d = PO.deltas(V, 30 + V, size, torch.float32)
    g = torch.Generator().manual_seed(40 + V)
    gv, gc = torch.randn(V, 4, 4, generator=g), torch.randn(V, 3, generator=g)
    dd = d.cuda().requires_grad_(True)
    view, campos = ops.camera_adjust(w2c.cuda(), c2w.cuda(), dd)
    gd, = torch.autograd.grad((view * gv.cuda()).sum() + (campos * gc.cuda()).sum(), dd)
    if size == 0.0:                                               # every product is by exactly 1 or 0
        assert torch.equal(view.cpu(), w2c) and torch.equal(campos.cpu(), c2w[:, :3, 3])
    ref = {}
    for dt in (torch.float64, torch.float32):
        dr = d.to(dt).requires_grad_(True)
        v, p = PO.closed_form(w2c.to(dt), c2w.to(dt), dr)
        gr, = torch.autograd.grad((v * gv.to(dt)).sum() + (p * gc.to(dt)).sum(), dr)
        ref[dt] = (torch.cat([v.detach().reshape(V, 16), p.detach()], -1), gr)
    out = torch.cat([view.detach().reshape(V, 16), campos.detach()], -1)
    ef, ef32 = _rel(out, ref[torch.float64][0]), _rel(ref[torch.float32][0], ref[torch.float64][0])
    eb, eb32 = _rel(gd, ref[torch.float64][1]), _rel(ref[torch.float32][1], ref[torch.float64][1])
    print(f"[camera_adjust V={V} |delta|={size}] forward: hip vs fp64 {ef:.3e} (oracle fp32 {ef32:.3e}, gate {GATE['adjust_fwd']:.1e});  "
          f"backward: hip {eb:.3e} (oracle fp32 {eb32:.3e}, gate {GATE['adjust_bwd']:.1e})")
    parity(f"pose_opt::camera_adjust[V={V},size={size}]", fwd_rel_l2=ef, oracle_fp32_fwd=ef32, bwd_rel_l2=eb, oracle_fp32_bwd=eb32,
           gate_fwd=GATE["adjust_fwd"], gate_bwd=GATE["adjust_bwd"])
    # exact properties: linear in the incoming gradients, bit-identical run to run, the bottom row of d_viewmat is not read
    dd2 = d.cuda().requires_grad_(True)
    v2, p2 = ops.camera_adjust(w2c.cuda(), c2w.cuda(), dd2)
    g2, = torch.autograd.grad((v2 * (2 * gv).cuda()).sum() + (p2 * (2 * gc).cuda()).sum(), dd2)
    assert torch.equal(v2, view) and torch.equal(p2, campos) and torch.equal(g2, 2 * gd)
    dd3 = d.cuda().requires_grad_(True)
    v3, p3 = ops.camera_adjust(w2c.cuda(), c2w.cuda(), dd3)
    gv3 = gv.clone()
    gv3[:, 3] = 7.0
    g3, = torch.autograd.grad((v3 * gv3.cuda()).sum() + (p3 * gc.cuda()).sum(), dd3)
    assert torch.equal(g3, gd)
    assert torch.equal(view[:, 3].cpu(), w2c[:, 3])
    assert ef <= GATE["adjust_fwd"] and eb <= GATE["adjust_bwd"], (ef, eb)


def test_camera_adjust_refusals(hip_lib):
    from vist3a_amd import ops
    w, c, d = torch.eye(4).repeat(2, 1, 1).cuda(), torch.eye(4).repeat(2, 1, 1).cuda(), torch.zeros(2, 9).cuda()
    with pytest.raises(NotImplementedError, match="w2c_base"):
        ops.camera_adjust(w.clone().requires_grad_(True), c, d)
    with pytest.raises(NotImplementedError, match="c2w_base"):
        ops.camera_adjust(w, c.clone().requires_grad_(True), d)
    with pytest.raises(ValueError):
        ops.camera_adjust(w, c, torch.zeros(3, 9).cuda())
    with pytest.raises(ValueError):
        ops.camera_adjust(w, c, torch.zeros(2, 6).cuda())
    with pytest.raises(ValueError):
        ops.camera_adjust(w.cpu(), c, d)


# ------------------------------------------------------------------------------------------------ 2. projection backward, CAM
def _scene(U, seed, K=25):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(U, 3, generator=g) * torch.tensor([1.5, 1.5, 1.0]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(U, 3, 3, generator=g) * 0.2
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)
    sh = (torch.randn(U, 3, 25, generator=g) * 0.3)[:, :, :K].contiguous()
    return means, cov, sh, torch.rand(U, generator=g)


def _cams(W, H, n, f=60.0):
    import math
    views, Ks = [], []
    for i in range(n):
        yaw = 0.1 * i - 0.1
        c, s = math.cos(yaw), math.sin(yaw)
        v = torch.eye(4)
        v[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        v[:3, 3] = torch.tensor([0.05 * i, 0.0, 0.1 * i])
        views.append(v)
        Ks.append(torch.tensor([[f + 5 * i, 0, W / 2], [0, (f + 5 * i) * 1.1, H / 2], [0, 0, 1.0]]))
    view = torch.stack(views)
    campos = torch.stack([torch.linalg.inv(v.double())[:3, 3].float() for v in views]).contiguous()
    return view, campos, torch.stack(Ks)


def _project_case(ops, U, Cn, deg, layout, aa, seed=11):
    W, H = 96, 80
    means, cov, sh, op = _scene(U, seed)
    view, campos, K = _cams(W, H, Cn)
    shl = (sh if layout == 1 else sh.permute(0, 2, 1)).contiguous()
    mode = "antialiased" if aa else "classic"
    dev = [t.cuda() for t in (means, cov, shl, view, campos, K)]
    pr = ops.gs_project(*dev, W, H, sh_degree=deg, sh_layout=layout, rasterize_mode=mode)
    g = torch.Generator().manual_seed(seed + 1)
    vm2, vcon, vcol, vop = (torch.randn(Cn, U, n, generator=g) for n in (2, 3, 4, 1))
    return dict(W=W, H=H, means=means, cov=cov, sh=sh, op=op, view=view, campos=campos, K=K, dev=dev, radii=pr["radii"], mode=mode,
                cot=(vm2, vcon, vcol, vop[..., 0].contiguous()))


def _project_bwd(ops, cs, deg, layout, aa, scale=1.0, camera_grad=True, radii=None):
    vm2, vcon, vcol, vop = cs["cot"]
    eg = dict(d_means2d=(scale * vm2).cuda(), d_conics=(scale * vcon).cuda(), d_colors=(scale * vcol).cuda(), d_opacity=(scale * vop).cuda())
    return ops.gs_project_backward(*cs["dev"], cs["W"], cs["H"], cs["radii"] if radii is None else radii, eg, sh_degree=deg,
                                   sh_layout=layout, rasterize_mode=cs["mode"], opacities=cs["op"].cuda() if aa else None,
                                   camera_grad=camera_grad)


def _project_oracle(cs, deg, aa, dt, monkeypatch):
    """d(sum of the entries' outputs times their cotangents) / d(viewmat, campos) per camera, by torch.autograd in `dt`"""
    vm2, vcon, vcol, vop = cs["cot"]
    Cn = cs["view"].shape[0]
    view, campos = cs["view"].to(dt).requires_grad_(True), cs["campos"].to(dt).requires_grad_(True)
    means, cov, sh = cs["means"].to(dt), cs["cov"].to(dt), cs["sh"].to(dt)
    loss = 0
    for j in range(Cn):
        mk = (cs["radii"][j] > 0).cpu().to(dt)
        with monkeypatch.context() as m:
            m.setattr(G, "f32", dt)
            p = G.project(means, cov, view[j], cs["K"][j].to(dt), cs["W"], cs["H"])
            col = G.sh_colors(means, campos[j], sh.permute(0, 2, 1), deg)
            col4 = torch.cat([col, p["depths"][:, None]], -1)
            loss = loss + (p["means2d"] * mk[:, None] * vm2[j].to(dt)).sum() + (p["conics"] * mk[:, None] * vcon[j].to(dt)).sum() \
                + (col4 * mk[:, None] * vcol[j].to(dt)).sum()
            if aa:
                comp = AA.compensation(AA.cov2d(means, cov, view[j], cs["K"][j].to(dt), cs["W"], cs["H"]))
                loss = loss + (cs["op"].to(dt) * comp * mk * vop[j].to(dt)).sum()
    if not isinstance(loss, torch.Tensor) or not loss.requires_grad:
        return torch.zeros(Cn, 15, dtype=torch.float64)
    gv, gc = torch.autograd.grad(loss, (view, campos), allow_unused=True)
    gv = torch.zeros_like(view) if gv is None else gv
    gc = torch.zeros_like(campos) if gc is None else gc
    return _vec15(gv, gc)


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("deg,layout", [(4, 1), (3, 0), (0, 1)])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("U", [1, 64, 65, 1027, 20001])
def test_projection_backward_camera_gradients(hip_lib, parity, monkeypatch, U, Cn, deg, layout, aa):
    from vist3a_amd import ops
    cs = _project_case(ops, U, Cn, deg, layout, aa)
    out = _project_bwd(ops, cs, deg, layout, aa)
    plain = _project_bwd(ops, cs, deg, layout, aa, camera_grad=False)
    assert len(out) == 6 and len(plain) == 4
    d_view, d_campos = out[4], out[5]
    assert d_view.shape == (Cn, 4, 4) and d_campos.shape == (Cn, 3) and d_view.dtype == torch.float32
    for a, b, name in zip(out[:4], plain, ("means", "covars", "sh", "opacities")):
        assert torch.equal(a, b), f"d_{name} differs from camera_grad=False"
    assert float(d_view[:, 3].abs().max()) == 0                                   # the bottom row is written as zeros
    again, twice = _project_bwd(ops, cs, deg, layout, aa), _project_bwd(ops, cs, deg, layout, aa, scale=2.0)
    for a, b, c in zip(out, again, twice):
        assert torch.equal(a, b) and torch.equal(c, 2 * a)                        # run to run; linear in the cotangents
    visible = int((cs["radii"] > 0).sum())
    got = _vec15(d_view, d_campos)
    r64, r32 = _project_oracle(cs, deg, aa, torch.float64, monkeypatch), _project_oracle(cs, deg, aa, torch.float32, monkeypatch)
    if visible == 0:
        assert float(got.abs().max()) == 0
        return
    e, e32 = _rel(got, r64), _rel(r32, r64)
    name = f"U={U},C={Cn},deg={deg},layout={layout},{'aa' if aa else 'classic'}"
    print(f"[cam project {name}] {visible} visible entries: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {GATE['cam_project']:.1e}")
    parity(f"pose_opt::cam_project[{name}]", rel_l2=e, oracle_fp32_rel_l2=e32, gate=GATE["cam_project"], visible=visible)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert e <= GATE["cam_project"], e


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
def test_camera_that_sees_nothing_gets_exact_zeros(hip_lib, aa):
    from vist3a_amd import ops
    cs = _project_case(ops, 1027, 3, 4, 1, aa)
    radii = cs["radii"].clone()
    radii[1] = 0                                                                    # camera 1 sees nothing
    out = _project_bwd(ops, cs, 4, 1, aa, radii=radii)
    ref = _project_bwd(ops, cs, 4, 1, aa)
    assert float(out[4][1].abs().max()) == 0 and float(out[5][1].abs().max()) == 0
    for j in (0, 2):                                                                # the other cameras' sums are their own
        assert torch.equal(out[4][j], ref[4][j]) and torch.equal(out[5][j], ref[5][j]) and float(out[4][j].abs().max()) > 0


def test_gs_render_camera_grad_switch(hip_lib):
    from vist3a_amd import ops
    W, H = 64, 48
    means, cov, sh, op = _scene(300, 3)
    view, campos, K = _cams(W, H, 2)
    a = [t.cuda() for t in (means, cov, sh, op)]
    v, p, k = view.cuda(), campos.cuda(), K.cuda()
    for t in ("viewmat", "campos"):
        with pytest.raises(NotImplementedError):                                   # the default keeps its refusal
            ops.gs_render(*a, v.clone().requires_grad_(t == "viewmat"), p.clone().requires_grad_(t == "campos"), k, W, H)
    with pytest.raises(NotImplementedError, match="K"):
        ops.gs_render(*a, v, p, k.clone().requires_grad_(True), W, H, camera_grad=True)
    with torch.no_grad():
        want = ops.gs_rasterize(ops.gs_project(a[0], a[1], a[2], v, p, k, W, H), a[3], W, H)
    lv = [t.clone().requires_grad_(True) for t in a]
    vg, pg = v.clone().requires_grad_(True), p.clone().requires_grad_(True)
    col, dep, alp = ops.gs_render(*lv, vg, pg, k, W, H, camera_grad=True)
    assert torch.equal(col, want["color"]) and torch.equal(dep, want["depth"]) and torch.equal(alp, want["alpha"])
    g = torch.Generator().manual_seed(1)
    wc = torch.randn(2, H, W, 3, generator=g).cuda()
    grads = torch.autograd.grad((col * wc).sum() + dep.sum(), lv + [vg, pg])
    lv2 = [t.clone().requires_grad_(True) for t in a]
    col2, dep2, _ = ops.gs_render(*lv2, v, p, k, W, H)
    plain = torch.autograd.grad((col2 * wc).sum() + dep2.sum(), lv2)
    assert all(torch.equal(x, y) for x, y in zip(grads[:4], plain))
    assert grads[4].shape == (2, 4, 4) and grads[5].shape == (2, 3) and float(grads[4].abs().max()) > 0 and float(grads[5].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. end to end
def _gaussians(sc):
    from vist3a_amd.models.types import Gaussians
    cov, _ = SC.splat_activate(torch.log(sc["scales"]), sc["quats"], torch.zeros(len(sc["op"])))
    d = lambda t: t.contiguous().cuda()[None]
    return Gaussians(means=d(sc["means"]), covariances=d(cov), harmonics=d(sc["sh"]), opacities=d(sc["op"]), scales=d(sc["scales"]),
                     rotations=d(sc["quats"]))


def _render_targets(sc, gs, ext=None):
    from vist3a_amd import ops
    from vist3a_amd.post_opt.trainer import _cameras
    view, campos, K = _cameras(sc["c2w"] if ext is None else ext, sc["Kn"], sc["W"], sc["H"], "cuda")
    with torch.no_grad():
        pr = ops.gs_project(gs.means[0], gs.covariances[0], gs.harmonics[0], view, campos, K, sc["W"], sc["H"], sh_degree=1, sh_layout=1)
        r = ops.gs_rasterize(pr, gs.opacities[0], sc["W"], sc["H"], background=torch.zeros(3, device="cuda"), clamp_rgb=True)
    return r["color"].contiguous(), r["depth"].contiguous()


@pytest.mark.parametrize("case", ["classic", "antialiased", "classic+depth"])
def test_end_to_end_delta_gradient(hip_lib, parity, monkeypatch, case):
    """d loss / d deltas at non-zero deltas through ops.camera_adjust -> ops.gs_render(camera_grad=True) -> ops.photometric_loss
    (+ 0.01 ops.depth_loss) against fp64 autograd through the oracles, composite order and radii mask from the HIP forward."""
    from vist3a_amd import ops
    from vist3a_amd.post_opt.trainer import _camera_bases, _cameras
    sc = SC.loop_scene()
    W, H = sc["W"], sc["H"]
    gs = _gaussians(sc)
    aa, with_depth = case == "antialiased", case.endswith("depth")
    mode = "antialiased" if aa else "classic"
    target, tdepth = _render_targets(sc, gs)
    _, _, K = _cameras(sc["c2w"], sc["Kn"], W, H, "cuda")
    w2c, c2w = _camera_bases(sc["c2w"], "cuda")
    d0 = PO.deltas(3, 77, 2e-2, torch.float32)
    means, cov, sh, op = gs.means[0], gs.covariances[0], gs.harmonics[0], gs.opacities[0]
    bg = torch.zeros(3, device="cuda")
    dd = d0.cuda().requires_grad_(True)
    view, campos = ops.camera_adjust(w2c, c2w, dd)
    col, dep, alp = ops.gs_render(means, cov, sh, op, view, campos, K, W, H, sh_degree=1, sh_layout=1, background=bg, clamp_rgb=True,
                                  rasterize_mode=mode, camera_grad=True)
    loss = ops.photometric_loss(col, target, 0.2)[0]
    if with_depth:
        loss = loss + 0.01 * ops.depth_loss(dep, alp, tdepth, None, 1.0)[0]
    g_hip, = torch.autograd.grad(loss, dd)
    with torch.no_grad():
        pr = ops.gs_project(means, cov, sh, view.detach(), campos.detach(), K, W, H, sh_degree=1, sh_layout=1, rasterize_mode=mode)
        fo = ops.gs_rasterize(pr, op, W, H, background=bg, return_order=True)
    U = means.shape[0]
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    offs_all, ids_all = fo["tile_offsets"].cpu().long(), fo["flatten_ids"].cpu().long()
    ref = {}
    for dt in (torch.float64, torch.float32):
        dr = d0.to(dt).requires_grad_(True)
        v, p = PO.closed_form(w2c.cpu().to(dt), c2w.cpu().to(dt), dr)
        cols, deps, alps = [], [], []
        for j in range(3):
            lo, hi = int(offs_all[j * ntiles]), int(offs_all[(j + 1) * ntiles])
            offs, ids = offs_all[j * ntiles:(j + 1) * ntiles + 1] - lo, ids_all[lo:hi] - j * U
            c, d_, a_, _, _ = AA.render(dt, means.cpu().to(dt), cov.cpu().to(dt), sh.cpu().to(dt).permute(0, 2, 1), op.cpu().to(dt), v[j], p[j],
                                        K[j].cpu(), W, H, 1, (pr["radii"][j] > 0).cpu(), offs, ids, monkeypatch, background=(0.0, 0.0, 0.0),
                                        antialiased=aa)
            cols.append(c), deps.append(d_), alps.append(a_)
        lr = SO.photometric_loss(torch.stack(cols), target.cpu().to(dt), 0.2)[0]
        if with_depth:
            lr = lr + 0.01 * DO.depth_loss(torch.stack(deps), torch.stack(alps), tdepth.cpu().to(dt), None, 1.0)[0]
        ref[dt], = torch.autograd.grad(lr, dr)
    e, e32 = _rel(g_hip, ref[torch.float64]), _rel(ref[torch.float32], ref[torch.float64])
    print(f"[end to end {case}] d_deltas: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {GATE['cam_end_to_end']:.1e}   "
          f"|g| {float(ref[torch.float64].norm()):.3e}")
    parity(f"pose_opt::end_to_end[{case}]", rel_l2=e, oracle_fp32_rel_l2=e32, gate=GATE["cam_end_to_end"])
    assert float(g_hip.abs().min(dim=1).values.max()) > 0
    assert e <= GATE["cam_end_to_end"], e


# ------------------------------------------------------------------------------------------------ 4. the loop
def _start(sc, seed=42):
    g = torch.Generator().manual_seed(seed)
    sc2 = dict(sc)
    sc2["sh"] = sc["sh"] + torch.randn(sc["sh"].shape, generator=g) * 0.15
    return _gaussians(sc2)


def _loop_on_ops(start, target, ext, Kn, cfg, steps):
    """post_optimize's step as it stood before cfg.pose_opt, written out on the ops (opacity logits and harmonics only)"""
    from vist3a_amd import ops
    from vist3a_amd.post_opt import create_splats, view_order
    from vist3a_amd.post_opt.trainer import _cameras
    V, H, W, _ = target.shape
    sp = create_splats(start, cfg, V)
    p, m, v = sp["params"], sp["m"], sp["v"]
    view, campos, K = _cameras(ext, Kn, W, H, "cuda")
    bg, ws = torch.zeros(3, device="cuda"), ops.GsWorkspace()
    log = torch.zeros(steps, 3, device="cuda", dtype=torch.float64)
    Ksh = p["sh"].shape[-1]
    leaves = [p["opacities"].requires_grad_(True), p["sh"].requires_grad_(True)]
    for i, j in enumerate(view_order(V, steps, cfg.seed)):
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        color, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view[j:j + 1], campos[j:j + 1], K[j:j + 1], W, H, sh_degree=1, sh_layout=1,
                                    background=bg, clamp_rgb=True, workspace=ws)
        loss, l1, ssim = ops.photometric_loss(color, target[j:j + 1], cfg.ssim_lambda)
        g_op, g_sh = torch.autograd.grad(loss, leaves)
        log[i].copy_(torch.stack([loss.detach(), l1.detach(), ssim.detach()]))
        with torch.no_grad():
            ops.adam_step(p["opacities"], g_op.contiguous(), m["opacities"], v["opacities"], lr=cfg.lr_opacities, step=i + 1, betas=cfg.betas,
                          eps=cfg.eps, lr2=None, period=0)
            ops.adam_step(p["sh"], g_sh.contiguous(), m["sh"], v["sh"], lr=cfg.lr_sh, step=i + 1, betas=cfg.betas, eps=cfg.eps,
                          lr2=cfg.lr_sh / 20, period=Ksh)
    for t in leaves:
        t.requires_grad_(False)
    return sp, log


def test_loop_off_is_the_loop_as_it_stood_and_first_row(hip_lib):
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize
    sc = SC.loop_scene()
    target, _ = _render_targets(sc, _gaussians(sc))
    start = _start(sc)
    ext, Kn = sc["c2w"].cuda(), sc["Kn"].cuda()
    cfg = PostOptConfig(params=("opacities", "sh"), seed=5)
    sp_ref, log_ref = _loop_on_ops(start, target, ext, Kn, cfg, 8)
    sp = create_splats(start, cfg, 3)
    _, log = post_optimize(start, target, ext, Kn, cfg, steps=8, splats=sp)
    assert torch.equal(log, log_ref)                                                # (a) pose_opt off: the same bits
    assert "pose_deltas" not in sp
    for n in ("means", "scales", "quats", "opacities", "sh"):
        assert torch.equal(sp["params"][n], sp_ref["params"][n]) and torch.equal(sp["m"][n], sp_ref["m"][n]) and torch.equal(sp["v"][n], sp_ref["v"][n]), n
    cfg_on = PostOptConfig(params=("opacities", "sh"), seed=5, pose_opt=True)
    sp_on = create_splats(start, cfg_on, 3)
    _, log_on = post_optimize(start, target, ext, Kn, cfg_on, steps=8, splats=sp_on)
    assert torch.equal(log_on[0], log[0])                                           # (b) zero deltas: the first step sees the given cameras
    assert tuple(sp_on["pose_deltas"].shape) == (3, 9) and float(sp_on["pose_deltas"].abs().max()) > 0
    assert bool((sp_on["pose_deltas"].abs().amax(dim=1) > 0).all())                 # momentum and decay move every row
    assert not sp_on["pose_deltas"].requires_grad
    with pytest.raises(NotImplementedError):
        post_optimize(start, target, ext.clone().requires_grad_(True), Kn, cfg_on, steps=1)
    with pytest.raises(ValueError, match="pose_deltas"):
        post_optimize(start, target, ext, Kn, cfg_on, steps=1, splats=dict(sp_on, pose_deltas=torch.zeros(2, 9, device="cuda")))


def test_loop_reproducible_and_state_carries_over(hip_lib):
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize
    sc = SC.loop_scene()
    target, _ = _render_targets(sc, _gaussians(sc))
    start = _start(sc)
    ext, Kn = sc["c2w"].cuda(), sc["Kn"].cuda()
    cfg = PostOptConfig(params=("opacities", "sh"), seed=5, pose_opt=True, pose_opt_lr=1e-3, max_steps=12)
    runs = []
    for _ in range(2):
        sp = create_splats(start, cfg, 3)
        g, log = post_optimize(start, target, ext, Kn, cfg, steps=6, splats=sp)
        runs.append((sp, log, g))
    (s1, l1, g1), (s2, l2, g2) = runs
    assert torch.equal(l1, l2) and bool(torch.isfinite(l1).all())
    for k in ("pose_deltas", "pose_m", "pose_v"):
        assert torch.equal(s1[k], s2[k])
    assert torch.equal(g1.harmonics, g2.harmonics) and torch.equal(g1.opacities, g2.opacities)
    d6 = s1["pose_deltas"].clone()
    post_optimize(start, target, ext, Kn, cfg, steps=3, splats=s1)                  # carried over: step, moments and deltas continue
    assert s1["step"] == 9 and not torch.equal(s1["pose_deltas"], d6)
    # a pose-only fit: no scene parameter is trained, the scene comes back as it went in
    cfg_p = PostOptConfig(params=(), seed=5, pose_opt=True, pose_opt_lr=1e-3, max_steps=12)
    sp = create_splats(start, cfg_p, 3)
    g, log = post_optimize(start, target, ext, Kn, cfg_p, steps=4, splats=sp)
    keep = sp["keep"]
    assert torch.equal(g.harmonics[0], start.harmonics[0][keep]) and float(sp["pose_deltas"].abs().max()) > 0
    with pytest.raises(Exception):
        post_optimize(start, target, ext, Kn, PostOptConfig(params=(), seed=5), steps=1)   # nothing to train without pose_opt


def test_loop_follows_oracle_loop(hip_lib, parity):
    """4(c): 10 steps on opacity logits + harmonics + pose deltas (means / scales / quaternions fixed) from extrinsics off by deltas
    of size 0.01, pose_opt_lr = 1e-3 and pose_opt_reg = 1e-2 (so that the decay term shows), max_steps = 10 (so that the rate falls
    to 1 % within the run), against PO.oracle_pose_loop on the CPU in fp64 and fp32: oracle/gsplat_raster.py culling, binning and
    sorting for itself every step, torch.optim.Adam(weight_decay) + ExponentialLR for the deltas.  Reported: the per-step relative
    loss difference (max over the steps) beside the fp32 oracle's, and the trained deltas' norm-relative difference."""
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, view_order
    sc = SC.loop_scene()
    W, H, steps = sc["W"], sc["H"], 10
    target, _ = _render_targets(sc, _gaussians(sc))
    start = _start(sc)
    ext = PO.adjust(sc["c2w"].double(), PO.deltas(3, 19, 0.01).double()).float()
    cfg = PostOptConfig(params=("opacities", "sh"), seed=5, pose_opt=True, pose_opt_lr=1e-3, pose_opt_reg=1e-2, max_steps=steps)
    sp = create_splats(start, cfg, 3)
    keep = sp["keep"].cpu()
    logit0, sh0 = sp["params"]["opacities"].cpu().clone(), sp["params"]["sh"].cpu().clone()
    means, cov = start.means[0].cpu()[keep], start.covariances[0].cpu()[keep]
    _, log = post_optimize(start, target, ext.cuda(), sc["Kn"].cuda(), cfg, steps=steps, splats=sp)
    c_hip, d_hip = log[:, 0].cpu(), sp["pose_deltas"].cpu()
    Kpix = sc["Kn"].clone()
    Kpix[:, 0] *= W
    Kpix[:, 1] *= H
    order = view_order(3, steps, cfg.seed)
    run = lambda dt: PO.oracle_pose_loop(dt, means, cov, sh0, logit0, ext, Kpix, target.cpu(), order, W, H, sh_degree=1, max_steps=steps,
                                         pose_lr=cfg.pose_opt_lr, pose_reg=cfg.pose_opt_reg, train_scene=True,
                                         lr_opacities=cfg.lr_opacities, lr_sh=cfg.lr_sh, ssim_lambda=cfg.ssim_lambda)
    (c64, d64), (c32, d32) = run(torch.float64), run(torch.float32)
    e, e32 = float(((c_hip - c64).abs() / c64).max()), float(((c32 - c64).abs() / c64).max())
    ed, ed32 = _rel(d_hip, d64), _rel(d32, d64)
    print(f"[pose loop] loss {c64[0]:.5e} -> {c64[-1]:.5e} (oracle fp64), {c_hip[0]:.5e} -> {c_hip[-1]:.5e} (hip)")
    print(f"[pose loop] per-step relative loss difference, max over {steps} steps: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   "
          f"gate {GATE['loop']:.1e};  deltas after {steps} steps: hip {ed:.3e}   oracle fp32 {ed32:.3e}   gate {GATE['loop_deltas']:.1e}")
    parity("pose_opt::loop", rel_max=e, oracle_fp32_rel_max=e32, deltas_rel_l2=ed, oracle_fp32_deltas_rel_l2=ed32, gate=GATE["loop"],
           gate_deltas=GATE["loop_deltas"], first=float(c64[0]), last=float(c64[-1]))
    assert bool((d64.abs().amax(dim=1) > 0).all())
    assert e <= GATE["loop"] and ed <= GATE["loop_deltas"], (e, ed)


@pytest.mark.parametrize("combo", ["bilateral_grid", "test_every", "mcmc", "depth+antialiased"])
def test_loop_composes(hip_lib, combo):
    from vist3a_amd.post_opt import PostOptConfig, adjusted_extrinsics, create_splats, post_optimize
    sc = SC.loop_scene()
    target, tdepth = _render_targets(sc, _gaussians(sc))
    start = _start(sc)
    ext, Kn = sc["c2w"].cuda(), sc["Kn"].cuda()
    kw = dict(seed=3, pose_opt=True, pose_opt_lr=1e-3, max_steps=20)
    extra, Vt = {}, 3
    if combo == "bilateral_grid":
        kw.update(use_bilateral_grid=True, bilateral_grid_shape=(4, 4, 2))
    elif combo == "test_every":
        kw.update(test_every=2)
        Vt = 1
        target = target.clone()
        target[0::2] = float("nan")                                                 # held-out images are never read
    elif combo == "mcmc":
        kw.update(strategy="mcmc", mcmc_refine_start_iter=1, mcmc_refine_every=2, mcmc_cap_max=400)
    else:
        kw.update(depth_loss=True, antialiased=True)
        extra = dict(depths=tdepth)
    cfg = PostOptConfig(**kw)
    outs = []
    for _ in range(2):
        sp = create_splats(start, cfg, Vt)
        g, log = post_optimize(start, target, ext, Kn, cfg, steps=6, splats=sp, **extra)
        outs.append((sp, log, g))
    (s1, l1, g1), (s2, l2, g2) = outs
    assert bool(torch.isfinite(l1).all()) and torch.equal(l1, l2)
    assert tuple(s1["pose_deltas"].shape) == (Vt, 9) and torch.equal(s1["pose_deltas"], s2["pose_deltas"])
    assert bool(torch.isfinite(s1["pose_deltas"]).all()) and float(s1["pose_deltas"].abs().max()) > 0
    assert torch.equal(g1.means, g2.means) and torch.equal(g1.harmonics, g2.harmonics) and bool(torch.isfinite(g1.means).all())
    adj = adjusted_extrinsics(ext, s1, cfg)
    assert adj.shape == (3, 4, 4) and bool(torch.isfinite(adj).all())
    if combo == "test_every":
        assert torch.equal(adj[0], ext[0]) and torch.equal(adj[2], ext[2]) and not torch.equal(adj[1], ext[1])


# ------------------------------------------------------------------------------------------------ 5. poses are recovered
def test_poses_are_recovered(hip_lib, parity):
    """Targets: the scene's own renders at the true poses.  The loop starts from extrinsics off by a known rigid transform per view
    (deltas of size 0.02: ~3 cm and ~2.5 degrees on a scene 4 units away), the scene frozen (params=()), pose_opt_lr = 1e-3,
    300 steps of a 3000-step schedule.  These settings were checked on the CPU with the fp64 oracle loop (PO.oracle_pose_loop,
    train_scene=False, targets from PO.oracle_render at the true poses, the same view order): translation error 3.2606e-02 ->
    2.0297e-03, rotation error 4.4257e-02 -> 1.0433e-03 rad, loss 6.6237e-02 -> 3.9853e-04 - the halving condition with a factor
    of 8 to spare on the translation and 21 on the rotation.  (Why a budget this long: at 4 units a rotation error of 0.044 rad shifts
    the image as a translation of ~0.17 would, so translation and rotation trade against each other on the way and a delta travels
    several times its own offset, while Adam moves a coordinate by at most ~lr per step.)
    Condition: the mean translation and the mean rotation error of adjusted_extrinsics against the true poses both
    end below HALF their start; the same run without pose_opt leaves them where they were."""
    from vist3a_amd.post_opt import PostOptConfig, adjusted_extrinsics, create_splats, post_optimize
    sc = SC.loop_scene()
    gs = _gaussians(sc)
    target, _ = _render_targets(sc, gs)
    true = sc["c2w"]
    off = PO.deltas(3, 9, 0.02, torch.float32)
    start_ext = PO.adjust(true.double(), off.double()).float()
    t0, r0 = PO.pose_error(start_ext, true)
    steps = 300
    cfg = PostOptConfig(params=(), seed=2, pose_opt=True, pose_opt_lr=1e-3, max_steps=3000)
    sp = create_splats(gs, cfg, 3)
    _, log = post_optimize(gs, target, start_ext.cuda(), sc["Kn"].cuda(), cfg, steps=steps, splats=sp)
    t1, r1 = PO.pose_error(adjusted_extrinsics(start_ext.cuda(), sp, cfg), true)
    first, last = float(log[:3, 0].mean()), float(log[-3:, 0].mean())
    print(f"[pose recovery] translation error {t0:.4e} -> {t1:.4e}, rotation error {r0:.4e} -> {r1:.4e} rad, loss {first:.4e} -> {last:.4e}")
    parity("pose_opt::recovery", trans_start=t0, trans_end=t1, rot_start=r0, rot_end=r1, loss_first=first, loss_last=last)
    assert t1 < 0.5 * t0 and r1 < 0.5 * r0, (t0, t1, r0, r1)
    # without pose_opt nothing can move a camera: the loss of a frozen scene stays at the level of the perturbed poses, every epoch
    cfg_off = PostOptConfig(params=("sh",), seed=2, lr_sh=1e-12)
    sp_off = create_splats(gs, cfg_off, 3)
    _, log_off = post_optimize(gs, target, start_ext.cuda(), sc["Kn"].cuda(), cfg_off, steps=30, splats=sp_off)
    assert "pose_deltas" not in sp_off
    e_first, e_last = float(log_off[:3, 0].mean()), float(log_off[-3:, 0].mean())
    print(f"[pose recovery, pose_opt off] loss of the first epoch {e_first:.4e}, of the tenth {e_last:.4e}")
    assert abs(e_last - e_first) <= 1e-6 * e_first and e_last > 10 * last
    assert torch.equal(adjusted_extrinsics(start_ext.cuda(), sp_off, cfg_off).cpu(), start_ext)
