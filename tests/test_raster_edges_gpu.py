"""The rasteriser's rarely-taken branches on the GPU: the constructed scenes of tests/raster_edge_scenes.py through gs_project ->
gs_rasterize -> gs_rasterize_backward -> gs_project_backward, every pixel and every Gaussian judged on its own against
torch.autograd through oracle/gsplat_raster.py in fp64 (driven, as in tests/test_raster_bwd_gpu.py, with the HIP forward's radii
mask and composite order).  tests/test_raster_edges_host.py shows, without a GPU, that each scene takes its branch and that an
oracle with that one rule changed misses these gates by more than 10x.

Forward: max over pixels of |hip - ref64| for colour (clamped, over white), depth and alpha; again for alpha over the pixels that
stopped early (the stop index itself cannot be observed: alpha = 1 - T at the stop can).  Nothing excused.
Backward: per tensor, max over Gaussians g of ||hip_g - ref64_g|| / (||ref64_g|| + floor), floor = 1e-3 x the median non-zero
||ref64_g||.  Where the fp64 gradient is exactly zero the HIP gradient is exactly zero, element by element.

Gates: min(4 x the fp32 oracle's own figure on the same metric against fp64, CEILING = 1e-3), formed at run time.  The 4x covers
__expf against expf and the kernels' summation order.  WIDENED lists the (case, tensor) pairs whose HIP figure lies between 4x
and the ceiling with no defect found; those are gated at 2x the figure measured on an MI355X (the MEASURED / GATE convention of
tests/test_raster_bwd_gpu.py).  MEASURED holds (hip, fp32 oracle) for every case and tensor; DESIGN.md section 7a has them per scene (colour_floor: the
largest over its unwidened cases, and the widened cases on rows of their own).

Widened: d_opacities of colour_floor at degree 4, U = 1 (hip 1.79e-7, fp32 oracle 2.3e-8) and U = 65 (hip 3.95e-5, fp32 oracle
3.0e-6), both layouts.  No defect found: a Gaussian's d_opacity is a signed sum over its pixels (random cotangents), and the
maximum over Gaussians of the relative error picks the one whose terms cancel most.  With one Gaussian the HIP figure is 1.5 ulp
of fp32 and the oracle's happened to land at 0.2 ulp; over the other 20 colour_floor cases both sides spread over the same range
(hip 7e-9 .. 1.1e-4, fp32 oracle 3.7e-8 .. 1.3e-4) and the oracle is the larger of the two in 10 of them.  The two summation
orders draw from one distribution; four times one draw does not bound another."""
import pytest
import torch

import raster_edge_scenes as S
from test_raster_bwd_gpu import _oracle_render, _order_of

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
FWD = ("colour", "depth", "alpha", "alpha_at_stops")

# (hip vs fp64, fp32 oracle vs fp64) on an MI355X, every case
MEASURED = {
    "alpha_cap": dict(colour=(1.614e-07, 1.609e-07), depth=(9.389e-07, 9.389e-07), alpha=(1.295e-07, 1.634e-07),
        means=(1.735e-06, 1.803e-06), covars=(1.396e-06, 1.244e-06), sh=(2.162e-06, 1.020e-06),
        opacities=(1.264e-05, 2.538e-05)),
    "round_edges": dict(colour=(7.391e-07, 7.391e-07), depth=(5.668e-06, 5.668e-06), alpha=(3.537e-07, 3.537e-07),
        alpha_at_stops=(2.868e-08, 2.868e-08), means=(1.885e-05, 8.809e-06), covars=(3.552e-05, 3.128e-05),
        sh=(1.498e-05, 9.323e-06), opacities=(5.402e-04, 3.355e-04)),
    "opaque_stack": dict(colour=(2.573e-07, 2.363e-07), depth=(1.476e-06, 8.660e-07), alpha=(3.216e-08, 3.873e-08),
        alpha_at_stops=(2.984e-08, 2.984e-08), means=(1.417e-06, 4.216e-06), covars=(5.210e-06, 2.638e-06),
        sh=(2.172e-06, 2.272e-06), opacities=(5.967e-05, 3.385e-05)),
    "frustum_sides": dict(colour=(3.110e-07, 3.173e-07), depth=(4.983e-07, 5.417e-07), alpha=(2.651e-07, 2.650e-07),
        means=(2.150e-06, 1.409e-06), covars=(1.248e-06, 8.216e-07), sh=(2.416e-06, 1.982e-06),
        opacities=(3.593e-06, 2.135e-06)),
    "culling": dict(colour=(2.825e-07, 2.835e-07), depth=(2.552e-06, 2.552e-06), alpha=(2.367e-07, 2.464e-07),
        means=(3.930e-06, 4.663e-06), covars=(3.468e-06, 4.031e-06), sh=(3.109e-06, 3.050e-06),
        opacities=(6.652e-05, 6.061e-05)),
    "colour_floor[deg0,layout0,U1]": dict(colour=(5.949e-08, 6.639e-08), depth=(1.093e-07, 1.685e-07),
        alpha=(3.965e-08, 4.998e-08), means=(1.817e-07, 1.413e-07), covars=(1.955e-07, 1.914e-07), sh=(1.230e-07, 1.027e-07),
        opacities=(7.071e-09, 1.139e-07)),
    "colour_floor[deg0,layout0,U63]": dict(colour=(2.210e-07, 2.210e-07), depth=(8.054e-07, 6.970e-07),
        alpha=(1.954e-07, 2.275e-07), means=(3.988e-06, 2.415e-06), covars=(1.288e-06, 1.409e-06), sh=(3.409e-06, 2.557e-06),
        opacities=(2.566e-05, 1.029e-05)),
    "colour_floor[deg0,layout0,U64]": dict(colour=(2.200e-07, 2.051e-07), depth=(9.157e-07, 1.085e-06),
        alpha=(1.892e-07, 1.789e-07), means=(1.723e-06, 1.757e-06), covars=(1.560e-06, 1.215e-06), sh=(1.714e-06, 1.237e-06),
        opacities=(1.074e-04, 1.344e-04)),
    "colour_floor[deg0,layout0,U65]": dict(colour=(2.249e-07, 2.519e-07), depth=(7.236e-07, 1.095e-06),
        alpha=(1.880e-07, 1.880e-07), means=(1.391e-06, 1.324e-06), covars=(3.155e-06, 1.213e-06), sh=(9.576e-07, 6.668e-07),
        opacities=(1.104e-04, 9.248e-05)),
    "colour_floor[deg0,layout1,U1]": dict(colour=(5.949e-08, 6.639e-08), depth=(1.093e-07, 1.685e-07),
        alpha=(3.965e-08, 4.998e-08), means=(1.817e-07, 1.413e-07), covars=(1.955e-07, 1.914e-07), sh=(1.230e-07, 1.027e-07),
        opacities=(7.071e-09, 1.139e-07)),
    "colour_floor[deg0,layout1,U63]": dict(colour=(2.210e-07, 2.210e-07), depth=(8.054e-07, 6.970e-07),
        alpha=(1.954e-07, 2.275e-07), means=(3.988e-06, 2.415e-06), covars=(1.288e-06, 1.409e-06), sh=(3.409e-06, 2.557e-06),
        opacities=(2.566e-05, 1.029e-05)),
    "colour_floor[deg0,layout1,U64]": dict(colour=(2.200e-07, 2.051e-07), depth=(9.157e-07, 1.085e-06),
        alpha=(1.892e-07, 1.789e-07), means=(1.723e-06, 1.757e-06), covars=(1.560e-06, 1.215e-06), sh=(1.714e-06, 1.237e-06),
        opacities=(1.074e-04, 1.344e-04)),
    "colour_floor[deg0,layout1,U65]": dict(colour=(2.249e-07, 2.519e-07), depth=(7.236e-07, 1.095e-06),
        alpha=(1.880e-07, 1.880e-07), means=(1.391e-06, 1.324e-06), covars=(3.155e-06, 1.213e-06), sh=(9.576e-07, 6.668e-07),
        opacities=(1.104e-04, 9.248e-05)),
    "colour_floor[deg2,layout0,U1]": dict(colour=(5.702e-08, 5.702e-08), depth=(1.310e-07, 1.054e-07),
        alpha=(5.019e-08, 3.658e-08), means=(2.286e-07, 2.382e-07), covars=(1.808e-07, 2.352e-07), sh=(8.775e-07, 5.703e-07),
        opacities=(3.708e-08, 3.708e-08)),
    "colour_floor[deg2,layout0,U63]": dict(colour=(2.423e-07, 2.806e-07), depth=(6.809e-07, 6.293e-07),
        alpha=(2.376e-07, 2.376e-07), means=(3.257e-06, 1.809e-06), covars=(3.103e-06, 2.183e-06), sh=(1.872e-06, 1.610e-06),
        opacities=(3.732e-05, 3.990e-05)),
    "colour_floor[deg2,layout0,U64]": dict(colour=(2.162e-07, 2.162e-07), depth=(8.787e-07, 1.138e-06),
        alpha=(1.688e-07, 1.688e-07), means=(3.008e-06, 3.341e-06), covars=(2.348e-06, 1.419e-06), sh=(1.300e-06, 2.240e-06),
        opacities=(1.207e-05, 2.043e-05)),
    "colour_floor[deg2,layout0,U65]": dict(colour=(1.920e-07, 2.466e-07), depth=(8.415e-07, 9.148e-07),
        alpha=(1.511e-07, 1.750e-07), means=(2.139e-06, 1.943e-06), covars=(1.038e-06, 2.058e-06), sh=(9.038e-07, 6.936e-07),
        opacities=(1.225e-05, 1.276e-05)),
    "colour_floor[deg2,layout1,U1]": dict(colour=(5.702e-08, 5.702e-08), depth=(1.310e-07, 1.054e-07),
        alpha=(5.019e-08, 3.658e-08), means=(2.286e-07, 2.382e-07), covars=(1.808e-07, 2.352e-07), sh=(8.775e-07, 5.703e-07),
        opacities=(3.708e-08, 3.708e-08)),
    "colour_floor[deg2,layout1,U63]": dict(colour=(2.423e-07, 2.806e-07), depth=(6.809e-07, 6.293e-07),
        alpha=(2.376e-07, 2.376e-07), means=(3.257e-06, 1.809e-06), covars=(3.103e-06, 2.183e-06), sh=(1.872e-06, 1.610e-06),
        opacities=(3.732e-05, 3.990e-05)),
    "colour_floor[deg2,layout1,U64]": dict(colour=(2.162e-07, 2.162e-07), depth=(8.787e-07, 1.138e-06),
        alpha=(1.688e-07, 1.688e-07), means=(3.008e-06, 3.341e-06), covars=(2.348e-06, 1.419e-06), sh=(1.300e-06, 2.240e-06),
        opacities=(1.207e-05, 2.043e-05)),
    "colour_floor[deg2,layout1,U65]": dict(colour=(1.920e-07, 2.466e-07), depth=(8.415e-07, 9.148e-07),
        alpha=(1.511e-07, 1.750e-07), means=(2.139e-06, 1.943e-06), covars=(1.038e-06, 2.058e-06), sh=(9.038e-07, 6.936e-07),
        opacities=(1.225e-05, 1.276e-05)),
    "colour_floor[deg4,layout0,U1]": dict(colour=(6.623e-08, 1.086e-07), depth=(9.925e-08, 2.725e-07),
        alpha=(5.514e-08, 1.086e-07), means=(4.296e-07, 7.158e-07), covars=(8.341e-08, 4.384e-07), sh=(1.786e-07, 6.563e-07),
        opacities=(1.789e-07, 2.314e-08)),
    "colour_floor[deg4,layout0,U63]": dict(colour=(2.118e-07, 2.219e-07), depth=(8.213e-07, 8.486e-07),
        alpha=(1.736e-07, 2.211e-07), means=(3.049e-06, 2.457e-06), covars=(1.642e-06, 2.110e-06), sh=(4.046e-06, 1.321e-06),
        opacities=(2.327e-05, 1.502e-05)),
    "colour_floor[deg4,layout0,U64]": dict(colour=(2.678e-07, 2.090e-07), depth=(8.523e-07, 8.523e-07),
        alpha=(2.102e-07, 1.762e-07), means=(1.178e-06, 2.627e-06), covars=(9.973e-07, 7.519e-07), sh=(2.661e-06, 4.023e-06),
        opacities=(2.224e-05, 8.878e-06)),
    "colour_floor[deg4,layout0,U65]": dict(colour=(1.982e-07, 2.262e-07), depth=(6.747e-07, 8.574e-07),
        alpha=(1.903e-07, 2.070e-07), means=(3.730e-06, 3.669e-06), covars=(1.551e-06, 1.566e-06), sh=(7.978e-07, 1.188e-06),
        opacities=(3.947e-05, 3.019e-06)),
    "colour_floor[deg4,layout1,U1]": dict(colour=(6.623e-08, 1.086e-07), depth=(9.925e-08, 2.725e-07),
        alpha=(5.514e-08, 1.086e-07), means=(4.296e-07, 7.158e-07), covars=(8.341e-08, 4.384e-07), sh=(1.786e-07, 6.563e-07),
        opacities=(1.789e-07, 2.314e-08)),
    "colour_floor[deg4,layout1,U63]": dict(colour=(2.118e-07, 2.219e-07), depth=(8.213e-07, 8.486e-07),
        alpha=(1.736e-07, 2.211e-07), means=(3.049e-06, 2.457e-06), covars=(1.642e-06, 2.110e-06), sh=(4.046e-06, 1.321e-06),
        opacities=(2.327e-05, 1.502e-05)),
    "colour_floor[deg4,layout1,U64]": dict(colour=(2.678e-07, 2.090e-07), depth=(8.523e-07, 8.523e-07),
        alpha=(2.102e-07, 1.762e-07), means=(1.178e-06, 2.627e-06), covars=(9.973e-07, 7.519e-07), sh=(2.661e-06, 4.023e-06),
        opacities=(2.224e-05, 8.878e-06)),
    "colour_floor[deg4,layout1,U65]": dict(colour=(1.982e-07, 2.262e-07), depth=(6.747e-07, 8.574e-07),
        alpha=(1.903e-07, 2.070e-07), means=(3.730e-06, 3.669e-06), covars=(1.551e-06, 1.566e-06), sh=(7.978e-07, 1.188e-06),
        opacities=(3.947e-05, 3.019e-06)),
}

# (case, tensor) -> gate, where the HIP figure lies between 4 x the fp32 oracle's and the ceiling with no defect found (above)
WIDENED = {(c, "opacities"): 2 * MEASURED[c]["opacities"][0]
           for c in (f"colour_floor[deg4,layout{layout},U{U}]" for U in (1, 65) for layout in (0, 1))}


def _dev(ts):
    return [t.contiguous().cuda() for t in ts]


def _run(ops, scene, monkeypatch, seed, layout=1, sh_pad=0):
    """HIP forward + backward of one scene, and the fp64 / fp32 oracle on the function the HIP forward computed"""
    means, cov, sh, op, view, campos, K, W, H, deg = scene
    if sh_pad:                                            # coefficients above the degree: read by nobody, gradient exactly zero
        g = torch.Generator().manual_seed(seed + 1)
        sh = torch.cat([sh, torch.randn(sh.shape[0], 3, sh_pad, generator=g)], -1).contiguous()
    U, Cn = means.shape[0], view.shape[0]
    wc, wd, wa = S.cotangents(scene, seed)
    shl = sh if layout == 1 else sh.permute(0, 2, 1).contiguous()
    md, cd, sd, od, vd, pd, kd = _dev((means, cov, shl, op, view, campos, K))
    bg = torch.ones(3, device="cuda")
    pr = ops.gs_project(md, cd, sd, vd, pd, kd, W, H, sh_degree=deg, sh_layout=layout)
    out = ops.gs_rasterize(pr, od, W, H, background=bg, clamp_rgb=True, return_order=True)
    ids = out["flatten_ids"].contiguous()
    wsp = ops.GsBwdWorkspace()                            # the row buffer is never memset: every slot that is read must have been
    wsp.get(U, Cn, W, H, max(ids.numel(), 1)).fill_(255)  # written by this call, or these NaN bit patterns reach the gradients
    eg = ops.gs_rasterize_backward(pr, od, W, H, out["tile_offsets"], ids, wc.cuda(), wd.cuda(), wa.cuda(), background=bg,
                                   clamp_rgb=True, workspace=wsp)
    dm, dcov, dsh, dop = ops.gs_project_backward(md, cd, sd, vd, pd, kd, W, H, pr["radii"], eg, sh_degree=deg, sh_layout=layout)
    hip = dict(colour=out["color"].cpu(), depth=out["depth"].cpu(), alpha=out["alpha"].cpu(), means=dm.cpu(), covars=dcov.cpu(),
               sh=(dsh if layout == 1 else dsh.permute(0, 2, 1)).cpu(), opacities=dop.cpu())
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    ref = {}
    for dt in (F64, F32):
        lv = [t.clone().to(dt).requires_grad_(True) for t in (means, cov, sh, op)]
        tot, fw = 0, []
        for j in range(Cn):
            offs, ids = _order_of(out, j, U, ntiles)
            c, d, a = _oracle_render(dt, lv[0], lv[1], lv[2].permute(0, 2, 1), lv[3], view[j], campos[j], K[j], W, H, deg,
                                     (pr["radii"][j] > 0).cpu(), offs, ids, monkeypatch)
            tot = tot + (c * wc[j].to(dt)).sum() + (d * wd[j].to(dt)).sum() + (a * wa[j].to(dt)).sum()
            fw.append((c.detach(), d.detach(), a.detach()))
        tot.backward()
        ref[dt] = dict(colour=torch.stack([f[0] for f in fw]), depth=torch.stack([f[1] for f in fw]), alpha=torch.stack([f[2] for f in fw]),
                       **{n: (t.grad if t.grad is not None else torch.zeros_like(t)) for n, t in zip(S.TENSORS, lv)})
    return hip, ref, pr


def _judge(parity, name, hip, ref, census):
    """print every figure beside the fp32 oracle's, log it, then assert all of them"""
    stopped = torch.stack([c["stop"] >= 0 for c in census])
    rows = []
    for n in FWD:
        k = "alpha" if n == "alpha_at_stops" else n
        sel = (lambda t: t[stopped]) if n == "alpha_at_stops" else (lambda t: t)
        if n == "alpha_at_stops" and not bool(stopped.any()):
            continue
        rows.append((n, S.per_pixel_error(sel(hip[k]), sel(ref[F64][k])), S.per_pixel_error(sel(ref[F32][k]), sel(ref[F64][k])), "abs_max"))
    for n in S.TENSORS:
        rows.append((n, S.per_gaussian_error(hip[n], ref[F64][n]), S.per_gaussian_error(ref[F32][n], ref[F64][n]), "per_gaussian_max"))
    bad = []
    for n, e, e32, metric in rows:
        key = "alpha" if n == "alpha_at_stops" else n
        gate = WIDENED.get((name, key), S.gate_from(e32))
        print(f"[{name}] {n}: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {gate:.3e}   ({metric})")
        parity(f"raster_edges::{name}", tensor=n, metric=metric, hip=e, oracle_fp32=e32, gate=gate)
        if not e <= gate:
            bad.append((n, e, e32, gate))
    for n in S.TENSORS:                                   # exact zeros: culled entries, floored channels, capped-only pairs, bands above
        z = ref[F64][n] == 0                              # the degree, the covariance's lower triangle
        nz = int((hip[n][z] != 0).sum())
        print(f"[{name}] d_{n}: {int(z.sum())} of {z.numel()} reference entries are exactly zero, {nz} of them non-zero in HIP")
        if nz:
            bad.append((n, "non-zero where the fp64 gradient is exactly zero", nz))
    if float(hip["covars"][:, [1, 2, 2], [0, 0, 1]].abs().max()) != 0:
        bad.append(("covars", "the lower triangle has a gradient"))
    assert not bad, bad


def _census_matches(pr, census):
    """the HIP radii are the oracle's, bit for bit: the census then speaks for the function the HIP forward computed"""
    for j, c in enumerate(census):
        assert torch.equal(pr["radii"][j].cpu(), c["radii"]), j


# ------------------------------------------------------------------------------------------------ one branch per scene
@pytest.mark.parametrize("name", ["alpha_cap", "round_edges", "opaque_stack", "frustum_sides", "culling"])
def test_scene_matches_oracle_per_pixel_and_per_gaussian(hip_lib, parity, monkeypatch, name):
    from vist3a_amd import ops
    scene = getattr(S, name)()
    census = [S.census(scene, j) for j in range(scene[4].shape[0])]
    hip, ref, pr = _run(ops, scene, monkeypatch, seed=200 + len(name))
    _census_matches(pr, census)
    if name in ("round_edges", "opaque_stack"):
        assert int((census[0]["stop"] >= 0).sum()) > 0
    _judge(parity, name, hip, ref, census)


@pytest.mark.parametrize("U", [1, 63, 64, 65])
@pytest.mark.parametrize("deg,layout", [(0, 0), (0, 1), (2, 0), (2, 1), (4, 0), (4, 1)])
def test_colour_floor_matches_oracle(hip_lib, parity, monkeypatch, deg, layout, U):
    """degree 2 carries 25 coefficients per channel: the 16 above the degree must come back with a gradient of exactly zero"""
    from vist3a_amd import ops
    scene = S.colour_floor(U, deg)
    census = [S.census(scene)]
    hip, ref, pr = _run(ops, scene, monkeypatch, seed=300 + U + deg, layout=layout, sh_pad=16 if deg == 2 else 0)
    _census_matches(pr, census)
    listed = S.colour_floor_listed(U)
    for i in listed:                                      # the floored channel's coefficients: exactly zero, the other two: not
        assert float(hip["sh"][i, i % 3].abs().max()) == 0 and float(hip["sh"][i, (i + 1) % 3].abs().max()) > 0, i
    if deg == 2:
        assert hip["sh"].shape[-1] == 25 and float(hip["sh"][:, :, 9:].abs().max()) == 0
    _judge(parity, f"colour_floor[deg{deg},layout{layout},U{U}]", hip, ref, census)


# ------------------------------------------------------------------------------------------------ exact per-scene assertions
def test_culled_camera_contributes_nothing_bit_for_bit(hip_lib):
    """Random entry gradients on EVERY (camera, Gaussian) entry, the culled ones included: a Gaussian culled by camera 0 gets,
    from the two-camera call, exactly what the call on camera 1 alone gives it; one culled by both gets exactly zero."""
    from vist3a_amd import ops
    means, cov, sh, op, view, campos, K, W, H, deg = scene = S.culling()
    U, n = means.shape[0], 8
    md, cd, sd, vd, pd, kd = _dev((means, cov, sh, view, campos, K))
    pr = ops.gs_project(md, cd, sd, vd, pd, kd, W, H, sh_degree=deg)
    _census_matches(pr, [S.census(scene, 0), S.census(scene, 1)])
    g = torch.Generator().manual_seed(13)
    eg = {k: torch.randn(2, U, m, generator=g).squeeze(-1).contiguous().cuda()
          for k, m in (("d_means2d", 2), ("d_conics", 3), ("d_colors", 4), ("d_opacity", 1))}
    both = ops.gs_project_backward(md, cd, sd, vd, pd, kd, W, H, pr["radii"], eg, sh_degree=deg)
    one = ops.gs_project_backward(md, cd, sd, vd[1:].contiguous(), pd[1:].contiguous(), kd[1:].contiguous(), W, H,
                                  pr["radii"][1:].contiguous(), {k: v[1:].contiguous() for k, v in eg.items()}, sh_degree=deg)
    gone0 = pr["radii"][0] == 0
    seen1 = pr["radii"][1] > 0
    rows = gone0 & seen1
    assert int(rows[:n].sum()) == n                       # the whole "behind camera 0, in front of camera 1" class
    for a, b in zip(both[:3], one[:3]):
        assert torch.equal(a[rows], b[rows]) and float(a[rows].abs().max()) > 0
    nowhere = gone0 & ~seen1
    assert int(nowhere[4 * n:].sum()) == n
    for a in both:
        assert float(a[nowhere].abs().max()) == 0


def test_single_capped_pair_has_no_alpha_gradient(hip_lib):
    """One Gaussian of opacity exactly 1 over a one-pixel image, its mean off the pixel centre: the pair is capped, so d_opacity,
    d_means2d and d_conics are exactly zero while d_colors is not.  The same Gaussian at opacity 0.998 (never capped) has all of
    them non-zero: it is the cap, not the geometry, that zeroes them."""
    from vist3a_amd import ops
    means, cov, sh, op, view, campos, K, W, H, deg = S.alpha_cap_single()
    md, cd, sd, vd, pd, kd = _dev((means, cov, sh, view, campos, K))
    pr = ops.gs_project(md, cd, sd, vd, pd, kd, W, H, sh_degree=deg)
    assert int(pr["radii"][0, 0]) > 0
    bg = torch.ones(3, device="cuda")
    ones = [torch.ones(1, H, W, 3).cuda(), torch.ones(1, H, W).cuda(), torch.ones(1, H, W).cuda()]
    res = {}
    for o in (1.0, 0.998):
        od = torch.full((1,), o, device="cuda")
        out = ops.gs_rasterize(pr, od, W, H, background=bg, clamp_rgb=False, return_order=True)
        assert out["n_isect"] == 1
        res[o] = (out, ops.gs_rasterize_backward(pr, od, W, H, out["tile_offsets"], out["flatten_ids"].contiguous(), *ones,
                                                 background=bg, clamp_rgb=False))
    out, eg = res[1.0]
    assert float(out["alpha"].reshape(-1)[0]) == pytest.approx(0.999, abs=1e-6)          # the capped alpha itself
    for k in ("d_opacity", "d_means2d", "d_conics"):
        assert float(eg[k].abs().max()) == 0, k
    assert float(eg["d_colors"].abs().min()) > 0
    out, eg = res[0.998]
    assert float(out["alpha"].reshape(-1)[0]) < 0.999
    for k in ("d_opacity", "d_means2d", "d_conics"):
        assert float(eg[k].abs().min()) > 0, k
