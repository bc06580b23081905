"""GPU parity of the rasteriser's antialiased mode (rasterize_mode="antialiased": csrc/raster.hip, csrc/raster_bwd.hip,
ops.gs_project / gs_rasterize / gs_render) against tests/raster_aa_oracle.py in fp64.

Scenes: the generator and cameras of tests/test_raster_bwd_gpu.py, 3 cameras in ONE call (the compensation is indexed by
camera-Gaussian entry, the opacity by Gaussian: a mix-up only shows with more than one camera), SH degree 2, both SH layouts:
  wide   _scene(400, 4, scale=0.25), 64 x 48     compensation 0.26 .. 0.9999, median 0.99
  thin   _scene(400, 4, scale=0.02), 64 x 48     compensation 0.05 .. 0.86, median 0.4: most opacities change by more than 2x
  small  _scene(64, 1, scale=0.05),  17 x 33     partial tiles
  tail   _scene(70, 1, scale=0.05),  17 x 33     70 = one wave + 6 lanes of the second

Metric: ||x_hip - x_ref64|| / ||x_ref64|| per tensor over ALL entries / Gaussians / pixels, nothing left out.  The fp64 reference is
driven with the HIP forward's radii mask and composite order, as in test_raster_bwd_gpu.py.  Every figure is printed, with the fp32
oracle's own error beside it, before it is asserted.

Gates: 2 x the largest error measured on an MI355X, never above the project's ceiling 1e-3.  MEASURED holds those figures (the run
recorded in DESIGN.md section 7a; None would select the ceiling)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import raster_aa_oracle as AO  # noqa: E402
from test_raster_bwd_gpu import _cams, _order_of, _rel, _scene  # noqa: E402

pytestmark = pytest.mark.gpu

CEILING = 1e-3
# hip vs the fp64 oracle, largest over the four scenes and both layouts (MI355X); the fp32 oracle's own error is printed beside each
# comp_entry: the largest RELATIVE error of a single visible entry's compensation (the others are norms)
# fp32 oracle in the same cases: comp 3.1e-7, colour 2.2e-7, depth 1.3e-6, alpha 1.2e-6; entry gradients 3.6e-5 .. 2.5e-3; end to end
# means 2.2e-6, covars 2.9e-6, sh 1.4e-6, opacities 1.6e-6.  The thin scene (scale=0.02) sits where the others do: comp 8.6e-8,
# comp_entry 8.7e-7, end to end 1.2e-6 .. 2.2e-6; the largest single-entry compensation error is the wide scene's (1.5e-5).
MEASURED = dict(comp=3.305e-7, comp_entry=1.500e-5, color=2.209e-7, depth=1.197e-6, alpha=1.153e-6,      # forward
                means2d=8.049e-7, conics=1.327e-6, colors=6.020e-7, opacity=5.390e-7,                     # entry gradients (blend backward)
                means=2.183e-6, covars=3.168e-6, sh=1.428e-6, opacities=1.418e-6)                         # end to end
GATE = {k: CEILING if v is None else min(2 * v, CEILING) for k, v in MEASURED.items()}

SCENES = dict(wide=(400, 4, 0.25, 64, 48), thin=(400, 4, 0.02, 64, 48), small=(64, 1, 0.05, 17, 33), tail=(70, 1, 0.05, 17, 33))
DEG, KSH, CAMS = 2, 9, 3


def _setup(name, layout):
    U, seed, scale, W, H = SCENES[name]
    means, cov, sh, op = _scene(U, seed, scale=scale, K=KSH)
    view, campos, K = _cams(W, H, CAMS)
    shl = (sh if layout == 1 else sh.permute(0, 2, 1)).contiguous()
    return dict(U=U, W=W, H=H, means=means, cov=cov, sh=sh, shl=shl, op=op, view=view, campos=campos, K=K, layout=layout,
                dev=[t.cuda() for t in (means, cov, shl, op, view, campos, K)])


def _weights(s, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(CAMS, s["H"], s["W"], 3, generator=g), torch.randn(CAMS, s["H"], s["W"], generator=g),
            torch.randn(CAMS, s["H"], s["W"], generator=g))


def _report(parity, test, name, hip, ref64, ref32):
    e, e32 = _rel(hip, ref64), _rel(ref32, ref64)
    print(f"[aa {test}] {name}: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {GATE[name]:.1e}")
    parity(f"raster_aa::{test}", tensor=name, rel_l2=e, oracle_fp32_rel_l2=e32, gate=GATE[name])
    return e


@pytest.fixture(scope="module")
def cases():
    """(scene, layout) -> the set-up, the HIP projection (both modes) and forward with its order, computed once and left unchanged"""
    cache = {}

    def get(name, layout):
        if (name, layout) not in cache:
            from vist3a_amd import ops
            s = _setup(name, layout)
            md, cd, sd, od, vd, pd, kd = s["dev"]
            with torch.no_grad():
                s["pr_classic"] = ops.gs_project(md, cd, sd, vd, pd, kd, s["W"], s["H"], sh_degree=DEG, sh_layout=layout)
                s["pr"] = ops.gs_project(md, cd, sd, vd, pd, kd, s["W"], s["H"], sh_degree=DEG, sh_layout=layout, rasterize_mode="antialiased")
                s["fwd"] = ops.gs_rasterize(s["pr"], od, s["W"], s["H"], background=torch.ones(3, device="cuda"), clamp_rgb=True, return_order=True)
            cache[(name, layout)] = s
        return cache[(name, layout)]
    return get


def _oracle(s, dt, monkeypatch, leaves=None, antialiased=True):
    """per camera (color, depth, alpha, comp) of the oracle in dt, with the HIP forward's masks and order"""
    means, cov, sh, op = leaves if leaves is not None else [t.to(dt) for t in (s["means"], s["cov"], s["sh"], s["op"])]
    ntiles = ((s["W"] + 15) // 16) * ((s["H"] + 15) // 16)
    out = []
    for j in range(CAMS):
        offs, ids = _order_of(s["fwd"], j, s["U"], ntiles)
        mask = (s["pr"]["radii"][j] > 0).cpu()
        out.append(AO.render(dt, means, cov, sh.permute(0, 2, 1), op, s["view"][j], s["campos"][j], s["K"][j], s["W"], s["H"], DEG, mask,
                             offs, ids, monkeypatch, antialiased=antialiased))
    return out


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_matches_oracle(hip_lib, parity, monkeypatch, cases, name, layout):
    s = cases(name, layout)
    pr, prc, fwd = s["pr"], s["pr_classic"], s["fwd"]
    # everything but the compensation is the classic projection, bit for bit
    assert "compensations" not in prc and set(pr) == set(prc) | {"compensations"}
    for k in ("radii", "means2d", "depths", "conics", "colors"):
        assert torch.equal(pr[k], prc[k]), k
    comp = pr["compensations"]
    vis = pr["radii"] > 0
    assert comp.shape == (CAMS, s["U"]) and int(vis.sum()) > 0 and int((~vis).sum()) > 0
    assert float(comp[~vis].abs().max()) == 0.0                                     # culled entries: exactly 0
    assert bool(((comp >= 0) & (comp <= 1)).all())
    r64, r32 = _oracle(s, torch.float64, monkeypatch), _oracle(s, torch.float32, monkeypatch)
    st = lambda r, i: torch.stack([c[i] for c in r])
    c64 = st(r64, 3)
    print(f"[aa forward {name}] visible per camera {vis.sum(1).tolist()} of {s['U']}; compensation min / median / max over visible entries "
          f"{float(c64[vis.cpu()].min()):.3f} / {float(c64[vis.cpu()].median()):.3f} / {float(c64[vis.cpu()].max()):.4f}")
    errs = dict(comp=_report(parity, f"forward[{name},layout{layout}]", "comp", comp, c64, st(r32, 3)))
    worst = float(((comp.cpu().double() - c64).abs() / c64.clamp_min(1e-300))[vis.cpu()].max())   # per visible entry
    print(f"[aa forward {name}] compensation, largest relative error of a visible entry {worst:.3e}")
    parity(f"raster_aa::forward[{name},layout{layout}]", tensor="comp_entry", rel_max=worst, gate=GATE["comp_entry"])
    for key, i in (("color", 0), ("depth", 1), ("alpha", 2)):
        errs[key] = _report(parity, f"forward[{name},layout{layout}]", key, fwd[key], st(r64, i), st(r32, i))
    for k, e in errs.items():
        assert e < GATE[k], (k, e)
    assert worst < GATE["comp_entry"], worst


# ------------------------------------------------------------------------------------------------ 2. entry gradients
@pytest.mark.parametrize("name", ["wide", "thin", "tail"])
def test_blend_backward_matches_oracle(hip_lib, parity, monkeypatch, cases, name):
    from oracle import gsplat_raster as G
    from vist3a_amd import ops
    s = cases(name, 1)
    pr, fwd, od = s["pr"], s["fwd"], s["dev"][3]
    W, H, U = s["W"], s["H"], s["U"]
    dc, dd, da = _weights(s, 100)
    bg = torch.ones(3, device="cuda")
    eg = ops.gs_rasterize_backward(pr, od, W, H, fwd["tile_offsets"], fwd["flatten_ids"].contiguous(), dc.cuda(), dd.cuda(), da.cuda(),
                                   background=bg, clamp_rgb=True)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    ref = {}
    for dt in (torch.float64, torch.float32):
        grads = []
        for j in range(CAMS):
            offs, ids = _order_of(fwd, j, U, ntiles)
            # d_opacity is the gradient with respect to the entry's EFFECTIVE opacity: the leaf is opacity * compensation
            lv = [pr[k][j].cpu().to(dt).requires_grad_(True) for k in ("means2d", "conics", "colors")]
            lv.append((s["op"].to(dt) * pr["compensations"][j].cpu().to(dt)).requires_grad_(True))
            with monkeypatch.context() as m:
                m.setattr(G, "f32", dt)
                img, alpha = G.rasterize(lv[0], lv[1], lv[2], lv[3], W, H, offs, ids, torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=dt))
            loss = (img[..., :3].clamp(0, 1) * dc[j].to(dt)).sum() + (img[..., 3] * dd[j].to(dt)).sum() + (alpha * da[j].to(dt)).sum()
            grads.append(torch.autograd.grad(loss, lv))
        ref[dt] = [torch.stack([g[i] for g in grads]) for i in range(4)]
    errs = {}
    for i, (nm, key) in enumerate((("means2d", "d_means2d"), ("conics", "d_conics"), ("colors", "d_colors"), ("opacity", "d_opacity"))):
        errs[nm] = _report(parity, f"blend[{name}]", nm, eg[key], ref[torch.float64][i], ref[torch.float32][i])
    for nm, e in errs.items():
        assert e < GATE[nm], (nm, e)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _hip_grads(s, weights, scale=1.0, mode="antialiased", **kw):
    from vist3a_amd import ops
    md, cd, sd, od, vd, pd, kd = s["dev"]
    lv = [t.clone().requires_grad_(True) for t in (md, cd, sd, od)]
    col, dep, alp = ops.gs_render(*lv, vd, pd, kd, s["W"], s["H"], sh_degree=DEG, sh_layout=s["layout"], background=torch.ones(3, device="cuda"),
                                  clamp_rgb=True, rasterize_mode=mode, **kw)
    wc, wd, wa = (w.cuda() for w in weights)
    loss = (col * (scale * wc)).sum() + (dep * (scale * wd)).sum() + (alp * (scale * wa)).sum()
    return (col.detach(), dep.detach(), alp.detach()), torch.autograd.grad(loss, lv)


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", list(SCENES))
def test_end_to_end_gradients_match_oracle(hip_lib, parity, monkeypatch, cases, name, layout):
    s = cases(name, layout)
    weights = _weights(s, 200)
    (col, dep, alp), hip = _hip_grads(s, weights)
    for a, k in ((col, "color"), (dep, "depth"), (alp, "alpha")):
        assert torch.equal(a, s["fwd"][k]), k                   # gs_render's forward is gs_rasterize's, bit for bit
    ref = {}
    for dt in (torch.float64, torch.float32):
        rl = [t.clone().to(dt).requires_grad_(True) for t in (s["means"], s["cov"], s["sh"], s["op"])]
        tot = 0
        for j, (c, d, a, _, _) in enumerate(_oracle(s, dt, monkeypatch, leaves=rl)):
            tot = tot + (c * weights[0][j].to(dt)).sum() + (d * weights[1][j].to(dt)).sum() + (a * weights[2][j].to(dt)).sum()
        ref[dt] = list(torch.autograd.grad(tot, rl))
    hip = list(hip)
    if layout == 0:
        hip[2] = hip[2].permute(0, 2, 1)
    errs = {n: _report(parity, f"end_to_end[{name},layout{layout}]", n, h, r64, r32)
            for n, h, r64, r32 in zip(("means", "covars", "sh", "opacities"), hip, ref[torch.float64], ref[torch.float32])}
    for t in hip:
        assert bool(torch.isfinite(t).all())
    for n, e in errs.items():
        assert e < GATE[n], (n, e)


# ------------------------------------------------------------------------------------------------ 4. exact properties
@pytest.mark.parametrize("name", ["thin", "tail"])
def test_exact_properties(hip_lib, cases, name):
    from vist3a_amd import ops
    s = cases(name, 1)
    weights = _weights(s, 300)
    f1, g1 = _hip_grads(s, weights)
    f1b, g1b = _hip_grads(s, weights)
    _, g2 = _hip_grads(s, weights, scale=2.0)
    for a, b, c in zip(g1, g1b, g2):
        assert torch.equal(a, b)                                # bit-identical run to run
        assert torch.equal(c, 2 * a)                            # linear in the incoming gradient, bit for bit
        assert float(a.abs().max()) > 0
    for a, b in zip(f1, f1b):
        assert torch.equal(a, b)
    md, cd, sd, od, vd, pd, kd = s["dev"]
    with torch.no_grad():                                       # the forward under no_grad equals the forward with grad
        plain = ops.gs_render(md, cd, sd, od, vd, pd, kd, s["W"], s["H"], sh_degree=DEG, sh_layout=1, background=torch.ones(3, device="cuda"),
                              rasterize_mode="antialiased")
    for a, b in zip(f1, plain):
        assert torch.equal(a, b) and not b.requires_grad
    # classic through the new keyword = the call without it, forward and gradients
    fc, gc = _hip_grads(s, weights, mode="classic")
    lv = [t.clone().requires_grad_(True) for t in (md, cd, sd, od)]
    col, dep, alp = ops.gs_render(*lv, vd, pd, kd, s["W"], s["H"], sh_degree=DEG, sh_layout=1, background=torch.ones(3, device="cuda"), clamp_rgb=True)
    loss = (col * weights[0].cuda()).sum() + (dep * weights[1].cuda()).sum() + (alp * weights[2].cuda()).sum()
    for a, b in zip(fc + tuple(gc), (col.detach(), dep.detach(), alp.detach()) + tuple(torch.autograd.grad(loss, lv))):
        assert torch.equal(a, b)
    if name == "thin":   # the mode does something: thin Gaussians are dimmed, the image holds less alpha
        a_aa, a_cl = float(f1[2].double().sum()), float(fc[2].double().sum())
        print(f"[aa thin] alpha image sum: antialiased {a_aa:.3f}, classic {a_cl:.3f}")
        assert a_aa < a_cl


def test_zero_covariance_gaussian(hip_lib, cases):
    """One Gaussian with an all-zero covariance among the others: its 2D covariance is the blur alone, compensation exactly 0 - it draws
    nothing (the images are those of the scene with that Gaussian's opacity at 0) and every gradient is finite."""
    from vist3a_amd import ops
    s = dict(_setup("small", 1))
    md, cd, sd, od, vd, pd, kd = [t.clone() for t in s["dev"]]
    z = 5
    md[z] = torch.tensor([0.0, 0.0, 4.0], device="cuda")          # in front of all three cameras
    cd[z] = 0
    od[z] = 0.9
    W, H = s["W"], s["H"]
    pr = ops.gs_project(md, cd, sd, vd, pd, kd, W, H, sh_degree=DEG, sh_layout=1, rasterize_mode="antialiased")
    assert bool((pr["radii"][:, z] > 0).all())
    assert float(pr["compensations"][:, z].abs().max()) == 0.0
    bg = torch.ones(3, device="cuda")
    lv = [t.clone().requires_grad_(True) for t in (md, cd, sd, od)]
    out = ops.gs_render(*lv, vd, pd, kd, W, H, sh_degree=DEG, sh_layout=1, background=bg, rasterize_mode="antialiased")
    o0 = od.clone()
    o0[z] = 0
    with torch.no_grad():
        ref = ops.gs_render(md, cd, sd, o0, vd, pd, kd, W, H, sh_degree=DEG, sh_layout=1, background=bg, rasterize_mode="antialiased")
    for a, b in zip(out, ref):
        assert torch.equal(a.detach(), b)
    g = torch.Generator().manual_seed(7)
    loss = sum((o * torch.randn(o.shape, generator=g).cuda()).sum() for o in out)
    grads = torch.autograd.grad(loss, lv)
    for t in grads:
        assert bool(torch.isfinite(t).all())
    assert float(grads[3][z]) == 0.0 and float(grads[1][z].abs().max()) == 0.0
