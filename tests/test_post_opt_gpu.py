"""GPU tests of the post-optimisation feature: csrc/ssim_loss.hip (ops.photometric_loss), csrc/post_opt.hip (ops.splat_activate,
ops.adam_step) and vist3a_amd.post_opt.

References: tests/golden/ssim_loss_ref.safetensors (the reference's loss_ssim.py in fp64, and its own fp32 run as the comparison
figure), fp64 torch autograd through tests/post_opt_oracle.py, torch.optim.Adam in fp64 on the CPU (fp32 torch Adam as the
comparison figure), and for the loop oracle/gsplat_raster.py + tests/ssim_loss_oracle.py + torch.optim.Adam in fp64.

Gates: 2x the largest error measured on an MI355X (MEASURED, the run recorded in DESIGN.md section 7f), never above the project's
per-kernel ceiling of 1e-3, and in addition the bound each test states against the fp32 reference's own error.  Every test prints
its figures before it asserts and logs them through the `parity` fixture."""
import sys
from pathlib import Path

import pytest
import torch
from safetensors.torch import load_file

from oracle import gsplat_raster as G

sys.path.insert(0, str(Path(__file__).resolve().parent))
import post_opt_oracle as PO  # noqa: E402
import ssim_loss_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu

CEILING = 1e-3
MEASURED = dict(loss_value=9.992e-15, loss_grad=2.843e-8,
                act_cov=5.478e-7, act_opacity=3.027e-8, act_d_log_scales=1.488e-7, act_d_quats=3.029e-7, act_d_logits=8.491e-8,
                adam=2.413e-3, loop=3.114e-7)
# Adam's metric is the largest elementwise RELATIVE error: where the first moment nearly cancels it is set by the fp32 state's own
# rounding, not by the kernel (torch's fp32 Adam measures 1.9e-3 on the largest case), so the norm ceiling does not apply to it.
NO_CEILING = ("adam",)
GOLD = Path(__file__).resolve().parent / "golden" / "ssim_loss_ref.safetensors"
CASES = [f"{s}.{k}" for s in ("11x11", "13x37", "45x70") for k in ("smooth", "noise")]


def gate(name):
    if MEASURED[name] is None:
        return CEILING
    return 2 * MEASURED[name] if name in NO_CEILING else min(2 * MEASURED[name], CEILING)


def _rel(a, b):
    return float((a.detach().cpu().double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def gold():
    return load_file(str(GOLD))


def _case(gold, case):
    x, y = gold[case + ".x"].float() / 255, gold[case + ".y"].float() / 255
    numel = x.numel()
    g_l1 = torch.sign(x.double() - y.double()) / numel
    return x, y, g_l1


# ------------------------------------------------------------------------------------------------ 1. loss parity
@pytest.mark.parametrize("case", CASES)
def test_loss_matches_reference(hip_lib, parity, gold, case):
    from vist3a_amd import ops
    x, y, g_l1 = _case(gold, case)
    s64, l64, s32, l32 = (float(gold[case + k]) for k in (".ssim64", ".l164", ".ssim32", ".l132"))
    gs64, gs32 = gold[case + ".g_ssim64"], gold[case + ".g_ssim32"].double()
    worst = []
    for lam in (0.0, 0.2, 1.0):
        xd = x.cuda().requires_grad_(True)
        loss, l1, ssim = ops.photometric_loss(xd, y.cuda(), lam)
        g, = torch.autograd.grad(loss, xd)
        ref = (1 - lam) * l64 + lam * (1 - s64)
        ref32 = float(torch.tensor((1 - lam), dtype=torch.float32) * torch.tensor(l32, dtype=torch.float32)
                      + torch.tensor(lam, dtype=torch.float32) * (1 - torch.tensor(s32, dtype=torch.float32)))
        g_ref, g_ref32 = (1 - lam) * g_l1 - lam * gs64, (1 - lam) * g_l1.float().double() - lam * gs32
        ev, ev32 = abs(float(loss.detach()) - ref), abs(ref32 - ref)
        eg, eg32 = _rel(g, g_ref), _rel(g_ref32, g_ref)
        print(f"[loss {case} lambda {lam}] value {float(loss):.9f}: hip vs fp64 {ev:.3e} (reference fp32 vs fp64 {ev32:.3e}, gate {gate('loss_value'):.1e});"
              f"  grad rel: hip {eg:.3e} (reference fp32 {eg32:.3e}, gate {gate('loss_grad'):.1e})")
        parity(f"post_opt::loss[{case},lambda={lam}]", value_abs=ev, ref_fp32_value_abs=ev32, grad_rel_l2=eg, ref_fp32_grad_rel_l2=eg32,
               gate_value=gate("loss_value"), gate_grad=gate("loss_grad"))
        assert loss.dtype == torch.float64 and g.dtype == torch.float32 and g.shape == x.shape
        assert abs(float(l1) - l64) <= gate("loss_value") and abs(float(ssim) - s64) <= gate("loss_value")
        worst.append((lam, ev, ev32, eg, eg32))
    for lam, ev, ev32, eg, eg32 in worst:
        assert ev <= gate("loss_value"), (lam, ev)
        assert eg <= gate("loss_grad"), (lam, eg)
        # a different summation order is the only legitimate difference: within 8x the fp32 reference's own error for this case
        assert ev <= 8 * ev32, (lam, ev, ev32)
        assert eg <= 8 * eg32, (lam, eg, eg32)


def test_loss_exact_properties(hip_lib, parity, gold):
    from vist3a_amd import ops
    x, y, _ = _case(gold, "45x70.smooth")
    xd, yd = x.cuda(), y.cuda()
    # identical images: exactly (0, 0, 1); the SSIM part of the gradient vanishes
    a = xd.clone().requires_grad_(True)
    loss, l1, ssim = ops.photometric_loss(a, xd.clone(), 1.0)
    g, = torch.autograd.grad(loss, a)
    assert (float(loss), float(l1), float(ssim)) == (0.0, 0.0, 1.0)
    for lam in (0.0, 0.2):
        l_, l1_, s_ = ops.photometric_loss(xd, xd.clone(), lam)
        assert (float(l_), float(l1_), float(s_)) == (0.0, 0.0, 1.0)
    e = float(g.double().norm() / gold["45x70.smooth.g_ssim64"].norm())
    print(f"[loss identical] SSIM gradient norm relative to the smooth case's {e:.3e}   gate {gate('loss_grad'):.1e}")
    parity("post_opt::loss_identical", grad_rel_l2=e, gate=gate("loss_grad"))
    assert e <= gate("loss_grad")
    # sizes under the window are an argument error, in either direction
    for shape in ((1, 10, 40, 3), (1, 40, 10, 3), (1, 16, 16, 5)):
        with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
            ops.photometric_loss(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    with pytest.raises(NotImplementedError):
        ops.photometric_loss(xd, yd.clone().requires_grad_(True))
    # bit-identical run to run; exactly linear in the incoming gradient

    def run(scale):
        a = xd.clone().requires_grad_(True)
        out = ops.photometric_loss(a, yd, 0.2)
        return out, torch.autograd.grad(scale * out[0], a)[0]

    (o1, g1), (o2, g2), (_, g3) = run(1.0), run(1.0), run(2.0)
    assert all(torch.equal(p, q) for p, q in zip(o1, o2)) and torch.equal(g1, g2)
    assert torch.equal(g3, 2 * g1) and float(g1.abs().max()) > 0
    # gradients of the l1 and ssim outputs alone add up to the loss's
    a = xd.clone().requires_grad_(True)
    l_, l1_, s_ = ops.photometric_loss(a, yd, 0.2)
    gl, = torch.autograd.grad(l1_, a, retain_graph=True)
    gsm, = torch.autograd.grad(s_, a)
    assert _rel(0.8 * gl.double() - 0.2 * gsm.double(), g1.cpu()) < 1e-6
    # without a gradient the values are the same
    with torch.no_grad():
        assert all(torch.equal(p, q) for p, q in zip(ops.photometric_loss(xd, yd, 0.2), o1))


# ------------------------------------------------------------------------------------------------ 2. activation
def test_activation_round_trip(hip_lib, parity):
    from vist3a_amd import ops
    U = 1000
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(U, 8 + 3 * 25, generator=g)
    feats[:, 1:4] = feats[:, 1:4] * 2 + 4          # softplus scales spread below the 0.3 clamp
    pts = torch.randn(U, 3, generator=g)
    ad = ops.gaussian_adapter(pts.cuda(), feats.cuda(), torch.ones(25, device="cuda"))
    op = ad["opacities"].clamp(0.02, 0.98)
    cov, o = ops.splat_activate(torch.log(ad["scales"]).contiguous(), ad["rotations"].contiguous(), torch.logit(op).contiguous())
    ec, eo = _rel(cov, ad["covariances"].cpu()), _rel(o, op.cpu())
    print(f"[activation round trip] covariances {ec:.3e} (gate {gate('act_cov'):.1e})   opacities {eo:.3e} (gate {gate('act_opacity'):.1e})")
    parity("post_opt::activation_round_trip", cov_rel_l2=ec, opacity_rel_l2=eo, gate_cov=gate("act_cov"), gate_opacity=gate("act_opacity"))
    assert ec <= gate("act_cov") and eo <= gate("act_opacity")


@pytest.mark.parametrize("upper", [False, True])
def test_activation_backward_matches_autograd(hip_lib, parity, upper):
    from vist3a_amd import ops
    ls, q, lg, Gf, Gu, d_op = PO.activation_case(1000, 7)
    Gin = Gu if upper else Gf
    lv = [t.float().cuda().requires_grad_(True) for t in (ls, q, lg)]
    cov, op = ops.splat_activate(*lv)
    hip = torch.autograd.grad((cov * Gin.float().cuda()).sum() + (op * d_op.float().cuda()).sum(), lv)
    ref = {}
    for dt in (torch.float64, torch.float32):
        rl = [t.float().to(dt).requires_grad_(True) for t in (ls, q, lg)]
        c, o = PO.splat_activate(*rl)
        ref[dt] = torch.autograd.grad((c * Gin.float().to(dt)).sum() + (o * d_op.float().to(dt)).sum(), rl)
    errs = {}
    for name, h, r64, r32 in zip(("act_d_log_scales", "act_d_quats", "act_d_logits"), hip, ref[torch.float64], ref[torch.float32]):
        errs[name] = _rel(h, r64)
        print(f"[activation backward upper={upper}] {name}: hip vs fp64 {errs[name]:.3e}   torch fp32 vs fp64 {_rel(r32, r64):.3e}   gate {gate(name):.1e}")
        parity(f"post_opt::activation_backward[upper={upper}]", tensor=name, rel_l2=errs[name], torch_fp32_rel_l2=_rel(r32, r64), gate=gate(name))
    # the rows with norm 0.5 / 2 quaternions get gradients 2x / 0.5x those of the unit ones: R does not depend on the length
    for name, e in errs.items():
        assert e <= gate(name), (name, e)


# ------------------------------------------------------------------------------------------------ 3. Adam
def _adam_torch(p0, grads, dt, lr, eps=1e-15):
    p = p0.clone().to(dt).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, eps=eps)
    for g in grads:
        p.grad = g.to(dt)
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("shape", [(1,), (7,), (1027,), (1000, 3, 75)])
def test_adam_matches_torch(hip_lib, parity, shape):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    p0 = torch.randn(*shape, generator=g)
    grads = [torch.randn(*shape, generator=g) * 0.1 for _ in range(5)]
    lr = 2.5e-3
    p, m, v = p0.clone().cuda(), torch.zeros(*shape, device="cuda"), torch.zeros(*shape, device="cuda")
    for t, gr in enumerate(grads, 1):
        ops.adam_step(p, gr.cuda(), m, v, lr=lr, step=t, eps=1e-15)
    r64, r32 = _adam_torch(p0, grads, torch.float64, lr), _adam_torch(p0, grads, torch.float32, lr)
    mx = lambda a, b: float(((a.cpu().double() - b) / b).abs().max())
    e = max(mx(a, b) for a, b in zip((p, m, v), r64))
    e32 = max(mx(a, b) for a, b in zip(r32, r64))
    print(f"[adam {shape}] max relative error of p, m, v after 5 steps: hip {e:.3e}   torch fp32 {e32:.3e}   gate {gate('adam'):.1e}")
    parity(f"post_opt::adam[{'x'.join(map(str, shape))}]", rel_max=e, torch_fp32_rel_max=e32, gate=gate("adam"))
    assert e <= gate("adam") and e <= 4 * e32, (e, e32)


def test_adam_exact_properties(hip_lib):
    from vist3a_amd import ops
    U, K = 1001, 9
    g = torch.Generator().manual_seed(2)
    sh0 = torch.randn(U, 3, K, generator=g)
    grads = [torch.randn(U, 3, K, generator=g) for _ in range(3)]
    z = lambda t: torch.zeros_like(t)
    # two rates in one tensor == the reference's two optimisers on the two slices, bit for bit
    p = sh0.clone().cuda()
    m, v = z(p), z(p)
    a, b = sh0[..., :1].contiguous().cuda(), sh0[..., 1:].contiguous().cuda()
    ma, va, mb, vb = z(a), z(a), z(b), z(b)
    for t, gr in enumerate(grads, 1):
        gr = gr.cuda()
        ops.adam_step(p, gr, m, v, lr=2.5e-3, lr2=2.5e-3 / 20, period=K, step=t, eps=1e-15)
        ops.adam_step(a, gr[..., :1].contiguous(), ma, va, lr=2.5e-3, step=t, eps=1e-15)
        ops.adam_step(b, gr[..., 1:].contiguous(), mb, vb, lr=2.5e-3 / 20, step=t, eps=1e-15)
    assert torch.equal(p, torch.cat([a, b], -1)) and torch.equal(m, torch.cat([ma, mb], -1)) and torch.equal(v, torch.cat([va, vb], -1))
    assert not torch.equal(p.cpu(), sh0)
    # a zero gradient with zero moments leaves p unchanged
    q = sh0.clone().cuda()
    mq, vq = z(q), z(q)
    ops.adam_step(q, z(q), mq, vq, lr=1.0, step=1, eps=1e-15)
    assert torch.equal(q.cpu(), sh0) and float(mq.abs().max()) == 0 and float(vq.abs().max()) == 0
    # a view that is not 16-byte aligned takes the scalar path and gives the same bits
    buf = torch.zeros(4 * 1027 + 4, device="cuda")
    pu, gu, mu, vu = (buf[i * 1027 + 1:(i + 1) * 1027 + 1] for i in range(4))
    pa, ga = torch.randn(1027, generator=g).cuda(), torch.randn(1027, generator=g).cuda()
    pu.copy_(pa)
    gu.copy_(ga)
    ma2, va2 = z(pa), z(pa)
    ops.adam_step(pu, gu, mu, vu, lr=1e-2, step=1)
    ops.adam_step(pa, ga, ma2, va2, lr=1e-2, step=1)
    assert torch.equal(pu, pa) and torch.equal(mu, ma2) and torch.equal(vu, va2)
    with pytest.raises(ValueError):
        ops.adam_step(pa, ga[:5], ma2, va2, lr=1e-2, step=1)


# ------------------------------------------------------------------------------------------------ 4. / 5. the loop
def _scene_gaussians(sc, perturb_seed=None, geometry=True):
    from vist3a_amd.models.types import Gaussians
    means, scales, quats, sh, op = sc["means"], sc["scales"], sc["quats"], sc["sh"], sc["op"]
    if perturb_seed is not None:
        g = torch.Generator().manual_seed(perturb_seed)
        r = lambda t, s: torch.randn(t.shape, generator=g) * s
        if geometry:
            means, scales = means + r(means, 0.02), scales * torch.exp(r(scales, 0.15))
            quats = torch.nn.functional.normalize(quats + r(quats, 0.08), dim=-1)
        sh = sh + r(sh, 0.15)
        op = torch.where(op > 0.01, torch.sigmoid(torch.logit(op) + r(op, 0.6)).clamp(0.03, 0.97), op)
    cov, _ = PO.splat_activate(torch.log(scales), quats, torch.zeros(len(op)))
    d = lambda t: t.contiguous().cuda()[None]
    return Gaussians(means=d(means), covariances=d(cov), harmonics=d(sh), opacities=d(op), scales=d(scales), rotations=d(quats))


def _targets(sc, gs):
    from vist3a_amd import ops
    from vist3a_amd.post_opt.trainer import _cameras
    view, campos, K = _cameras(sc["c2w"], sc["Kn"], sc["W"], sc["H"], "cuda")
    with torch.no_grad():
        pr = ops.gs_project(gs.means[0], gs.covariances[0], gs.harmonics[0], view, campos, K, sc["W"], sc["H"], sh_degree=1, sh_layout=1)
        r = ops.gs_rasterize(pr, gs.opacities[0], sc["W"], sc["H"], background=torch.zeros(3, device="cuda"), clamp_rgb=True, return_order=True)
    return r["color"].contiguous(), pr, r, (view, campos, K)


def test_loop_follows_oracle(hip_lib, parity, monkeypatch):
    """20 steps on opacity logits and harmonics (means / scales / quaternions fixed: radii and composite order stay put) against the
    same loop on the CPU: oracle/gsplat_raster.py autograd + tests/ssim_loss_oracle.py + torch.optim.Adam, in fp64 (and fp32)."""
    from vist3a_amd.post_opt import PostOptConfig, create_splats, post_optimize, view_order
    sc = PO.loop_scene()
    W, H, steps = sc["W"], sc["H"], 20
    target, _, _, _ = _targets(sc, _scene_gaussians(sc))
    start = _scene_gaussians(sc, perturb_seed=42, geometry=False)
    cfg = PostOptConfig(params=("opacities", "sh"), seed=5)
    out, log = post_optimize(start, target, sc["c2w"].cuda(), sc["Kn"].cuda(), cfg, steps=steps)
    c_hip = log[:, 0].cpu()
    # the function the HIP forward computes: its radii mask and composite order per camera, on the kept Gaussians
    sp = create_splats(start, cfg)
    kept = _scene_gaussians(sc)
    keep = sp["keep"]
    from vist3a_amd.models.types import Gaussians
    kept = Gaussians(*(getattr(kept, f)[:, keep].contiguous() for f in ("means", "covariances", "harmonics", "opacities", "scales", "rotations")))
    _, pr, r, (view, campos, K) = _targets(sc, kept)
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
            with monkeypatch.context() as mp:
                mp.setattr(G, "f32", dt)
                p = G.project(means.to(dt), cov.to(dt), view[j].cpu().to(dt), K[j].cpu().to(dt), W, H)
                col = G.sh_colors(means.to(dt), campos[j].cpu().to(dt), torch.cat([s0, sN], -1).permute(0, 2, 1), 1) * mask[:, None]
                col4 = torch.cat([col, p["depths"][:, None]], -1)
                img, _ = G.rasterize(p["means2d"], p["conics"], col4, torch.sigmoid(lg), W, H, offs, ids, torch.zeros(4, dtype=dt))
            loss = SO.photometric_loss(img[None, ..., :3].clamp(0, 1), target[j:j + 1].cpu().to(dt), cfg.ssim_lambda)[0]
            for o in opts:
                o.zero_grad()
            loss.backward()
            for o in opts:
                o.step()
            curve.append(float(loss))
        return torch.tensor(curve, dtype=torch.float64)

    c64, c32 = fit(torch.float64), fit(torch.float32)
    e, e32 = float(((c_hip - c64).abs() / c64).max()), float(((c32 - c64).abs() / c64).max())
    print(f"[loop] loss {c64[0]:.5e} -> {c64[-1]:.5e} (oracle fp64), {c_hip[0]:.5e} -> {c_hip[-1]:.5e} (hip)")
    print(f"[loop] per-step relative loss difference, max over {steps} steps: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {gate('loop'):.1e}")
    parity("post_opt::loop", rel_max=e, oracle_fp32_rel_max=e32, gate=gate("loop"), first=float(c64[0]), last=float(c64[-1]))
    assert torch.equal(out.means, kept.means) and torch.equal(out.rotations, torch.nn.functional.normalize(kept.rotations, dim=-1))
    assert c64[-1] < c64[0]
    assert e <= gate("loop"), e


def test_full_loop_all_tensors(hip_lib, parity):
    from vist3a_amd import ops
    from vist3a_amd.post_opt import PostOptConfig, post_optimize
    sc = PO.loop_scene()
    target, _, _, _ = _targets(sc, _scene_gaussians(sc))
    start = _scene_gaussians(sc, perturb_seed=43)
    cfg = PostOptConfig(seed=1)
    ext, Kn = sc["c2w"].cuda(), sc["Kn"].cuda()
    before = [t.clone() for t in (start.means, start.scales, start.rotations, start.opacities, start.harmonics)]
    (g1, log1), (g2, log2) = post_optimize(start, target, ext, Kn, cfg, steps=60), post_optimize(start, target, ext, Kn, cfg, steps=60)
    first, last = float(log1[:3, 0].mean()), float(log1[-3:, 0].mean())
    print(f"[full loop] mean loss of the first epoch {first:.5e}, of the last {last:.5e}: ratio {last / first:.3f}")
    parity("post_opt::full_loop", first_epoch=first, last_epoch=last, ratio=last / first)
    assert last < first
    assert bool(torch.isfinite(log1).all()) and log1.shape == (60, 3) and log1.dtype == torch.float64
    fields = ("means", "covariances", "harmonics", "opacities", "scales", "rotations")
    assert torch.equal(log1, log2) and all(torch.equal(getattr(g1, f), getattr(g2, f)) for f in fields)
    # the caller's object is untouched, and every tensor moved
    for t, b in zip((start.means, start.scales, start.rotations, start.opacities, start.harmonics), before):
        assert torch.equal(t, b)
    keep = start.opacities[0] > cfg.min_opacity
    U = int(keep.sum())
    assert U == start.means.shape[1] - 10 and g1.means.shape == (1, U, 3) and g1.harmonics.shape == (1, U, 3, 4)   # under min_opacity: absent
    assert float(g1.opacities.min()) > 0
    for f, b in zip(("means", "scales", "rotations", "opacities", "harmonics"), before):
        assert not torch.equal(getattr(g1, f)[0], b[0][keep]), f
    # consistent: unit rotations, and covariances = splat_activate of its own scales and rotations.  Worst case in units of
    # eps = 6e-8: the returned scale is exp(x) rounded (1), its log is rounded at |x| < 4 (2), the kernel's expf is good to 2 on either
    # side (4) - 7 eps per scale, 14 per s^2, and a few more from the renormalised quaternion's R: below 2e-6 of the Gaussian's
    # largest covariance entry
    assert torch.allclose(g1.rotations.norm(dim=-1), torch.ones(1, U, device="cuda"), atol=1e-6)
    cov, op = ops.splat_activate(torch.log(g1.scales[0]).contiguous(), g1.rotations[0].contiguous(), torch.logit(g1.opacities[0]).contiguous())
    tol = 2e-6 * g1.covariances[0].abs().amax(dim=(1, 2), keepdim=True)
    assert bool(((cov - g1.covariances[0]).abs() <= tol).all())
    assert torch.allclose(op, g1.opacities[0], rtol=0, atol=1e-6)
