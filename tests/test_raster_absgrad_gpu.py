"""GPU tests of the rasteriser's absolute-gradient output (gsplat's absgrad: v3a_gs_rasterize_backward's d_means2d_abs, the ABS
instantiations of gs_blend_bwd_kernel / gs_rowsum_kernel) and of gs_render's info_out, on the scenes of tests/test_raster_bwd_gpu.py:
U = 400 at 64 x 48 with one camera and U = 300 at 32 x 20 with three.

With absgrad on, the other four entry gradients keep their bits; d_means2d_abs >= |d_means2d| elementwise and is exactly 0 for
culled entries.  Parity (32 x 20): the fp64 oracle is the sum over pixels of |d L_p / d means2d|, L_p the pixel's share of the loss,
every pixel's gradient taken on its own through oracle.gsplat_raster.rasterize (G.f32 patched to fp64, HIP's radii mask and composite
order): the oracle runs one tile at a time with means2d expanded to [U,2,P], one copy per pixel of the tile, so that one backward
returns every pixel's own gradient.  The error is norm-relative and printed beside the fp32 oracle's own;
the gate is twice the figure measured on the MI355X (MEASURED, also in DESIGN.md section 7f), never above the project's 1e-3."""
import pytest
import torch

from oracle import gsplat_raster as G
from test_raster_bwd_gpu import _cams, _order_of, _rel, _scene

pytestmark = pytest.mark.gpu

CEILING = 1e-3
MEASURED = dict(means2d_abs=1.629e-7)      # the MI355X run recorded in DESIGN.md section 7f (the fp32 oracle's own error: 5.085e-8)
TILE = 16
CASES = [(400, 64, 48, 1, 4), (300, 32, 20, 3, 5)]


def _run(U, W, H, Cn, seed, absgrad):
    from vist3a_amd import ops
    means, cov, sh, op = _scene(U, seed, scale=0.25)
    view, campos, K = _cams(W, H, Cn)
    pr = ops.gs_project(means.cuda(), cov.cuda(), sh.cuda(), view.cuda(), campos.cuda(), K.cuda(), W, H)
    bg = torch.ones(3, device="cuda")
    out = ops.gs_rasterize(pr, op.cuda(), W, H, background=bg, clamp_rgb=True, return_order=True)
    g = torch.Generator().manual_seed(seed + 100)
    d = [torch.randn(Cn, H, W, 3, generator=g), torch.randn(Cn, H, W, generator=g), torch.randn(Cn, H, W, generator=g)]
    eg = ops.gs_rasterize_backward(pr, op.cuda(), W, H, out["tile_offsets"], out["flatten_ids"].contiguous(), *(x.cuda() for x in d),
                                   background=bg, clamp_rgb=True, absgrad=absgrad)
    return pr, out, op, d, eg


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"U{c[0]}_{c[1]}x{c[2]}_C{c[3]}")
def runs(request):
    U, W, H, Cn, seed = request.param
    return request.param, _run(U, W, H, Cn, seed, False), _run(U, W, H, Cn, seed, True)


def test_other_gradients_keep_their_bits(hip_lib, runs):
    _, off, on = runs
    assert set(off[4]) == {"d_means2d", "d_conics", "d_colors", "d_opacity"} and set(on[4]) == set(off[4]) | {"d_means2d_abs"}
    for k in off[4]:
        assert torch.equal(off[4][k], on[4][k]), k
    again = _run(*runs[0], True)[4]
    assert torch.equal(again["d_means2d_abs"], on[4]["d_means2d_abs"])                   # two runs: bit-identical


def test_bounds(hip_lib, runs):
    (U, W, H, Cn, _), _, (pr, _, _, _, eg) = runs
    a, d = eg["d_means2d_abs"], eg["d_means2d"]
    assert a.shape == d.shape == (Cn, U, 2) and a.dtype == torch.float32
    # exact: |v| goes through the very summation tree of v (DPP wave sum, the four waves, the row sum in slot order), and rounding
    # to nearest is monotone, so by induction over that tree |fl-sum(v)| <= fl-sum(|v|)
    assert bool((a >= d.abs()).all())
    assert bool((a > d.abs() * 1.01).any())                                             # and it is not |d_means2d| itself
    culled = pr["radii"] <= 0
    assert bool(culled.any()) and not bool(a[culled].any())                             # exactly 0


def _abs_oracle(dt, pr, op, d, j, mask, offs, ids, W, H, monkeypatch):
    """(sum over the pixels of camera j of |d L_p / d means2d|, the same sum with its signs), in `dt`.  One tile at a time: the
    other tiles' lists are empty and means2d is [U,2,P], a copy per pixel of the tile, which G.rasterize's `means2d[g, k] - px`
    takes lane by lane - so the one backward leaves d L_p / d means2d in lane p."""
    U = mask.shape[0]
    tw, th = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    conics, col4 = pr["conics"][j].cpu().to(dt), pr["colors"][j].cpu().to(dt) * mask[:, None].to(dt)
    absum, plain = torch.zeros(U, 2, dtype=dt), torch.zeros(U, 2, dtype=dt)
    for t in range(tw * th):
        lo, hi = int(offs[t]), int(offs[t + 1])
        if hi == lo:
            continue
        y0, x0 = (t // tw) * TILE, (t % tw) * TILE
        y1, x1 = min(y0 + TILE, H), min(x0 + TILE, W)
        only = torch.zeros_like(offs)
        only[t + 1:] = hi - lo
        m2 = pr["means2d"][j].cpu().to(dt)[:, :, None].repeat(1, 1, (y1 - y0) * (x1 - x0)).requires_grad_(True)
        with monkeypatch.context() as m:
            m.setattr(G, "f32", dt)
            img, alpha = G.rasterize(m2, conics, col4, op.to(dt), W, H, only, ids[lo:hi], torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=dt))
        sl = (slice(y0, y1), slice(x0, x1))
        loss = ((img[sl][..., :3].clamp(0, 1) * d[0][j][sl].to(dt)).sum() + (img[sl][..., 3] * d[1][j][sl].to(dt)).sum()
                + (alpha[sl] * d[2][j][sl].to(dt)).sum())
        g, = torch.autograd.grad(loss, m2)                                               # [U, 2, P]: lane p is pixel p's own gradient
        absum += g.abs().sum(-1)
        plain += g.sum(-1)
    return absum, plain


def test_parity_with_the_per_pixel_oracle(hip_lib, parity, monkeypatch):
    """MEASURED: the figure of the MI355X run; the gate is twice it, capped at 1e-3."""
    U, W, H, Cn, seed = CASES[1]
    pr, out, op, d, eg = _run(U, W, H, Cn, seed, True)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    ref = {}
    for dt in (torch.float64, torch.float32):
        parts = []
        for j in range(Cn):
            offs, ids = _order_of(out, j, U, ntiles)
            parts.append(_abs_oracle(dt, pr, op, d, j, (pr["radii"][j] > 0).cpu(), offs, ids, W, H, monkeypatch))
        ref[dt] = (torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    e, e32 = _rel(eg["d_means2d_abs"], ref[torch.float64][0]), _rel(ref[torch.float32][0], ref[torch.float64][0])
    e_plain = _rel(eg["d_means2d"], ref[torch.float64][1])                              # the same Jacobian summed with its signs
    gate = min(2 * MEASURED["means2d_abs"], CEILING)
    print(f"[absgrad {W}x{H} C={Cn}] d_means2d_abs: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32:.3e}   gate {gate:.1e}   "
          f"(d_means2d against the signed sum of the same Jacobian: {e_plain:.3e})")
    parity("raster_bwd::absgrad", tensor="means2d_abs", rel_l2=e, oracle_fp32_rel_l2=e32, gate=gate, d_means2d_rel_l2=e_plain)
    assert e_plain < 1e-4                                                               # the oracle's pixels are the kernel's pixels
    assert e < gate, (e, gate)


def test_info_out(hip_lib):
    from vist3a_amd import ops
    U, W, H, Cn, seed = CASES[1]
    means, cov, sh, op = _scene(U, seed, scale=0.25)
    view, campos, K = _cams(W, H, Cn)
    bg = torch.ones(3, device="cuda")
    g = torch.Generator().manual_seed(seed + 100)
    d = [torch.randn(Cn, H, W, 3, generator=g).cuda(), torch.randn(Cn, H, W, generator=g).cuda(), torch.randn(Cn, H, W, generator=g).cuda()]

    def render(**kw):
        lv = [t.cuda().requires_grad_(True) for t in (means, cov, sh, op)]
        c, dep, al = ops.gs_render(*lv, view.cuda(), campos.cuda(), K.cuda(), W, H, background=bg, **kw)
        return (c, dep, al), torch.autograd.grad((c * d[0]).sum() + (dep * d[1]).sum() + (al * d[2]).sum(), lv)

    plain = render()
    pr, _, _, _, eg = _run(U, W, H, Cn, seed, True)
    for kw, keys in ((dict(info_out={}), {"radii", "d_means2d"}), (dict(info_out={}, absgrad=True), {"radii", "d_means2d", "d_means2d_abs"})):
        got = render(**kw)
        info = kw["info_out"]
        assert set(info) == keys
        assert torch.equal(info["radii"], pr["radii"]) and all(torch.equal(info[k], eg[k]) for k in keys - {"radii"})
        assert all(torch.equal(a, b) for a, b in zip(plain[0] + plain[1], got[0] + got[1]))      # images and gradients: unchanged bits
    with pytest.raises(ValueError):
        render(absgrad=True)                                                            # nowhere to put it
