"""Small constructed scenes for the 3D-Gaussian rasteriser in which each rarely-taken branch is taken on purpose, a census that
proves the taking from the oracle alone, and the per-Gaussian / per-pixel metrics the edge tests judge with.  Plain module, CPU
only; used by tests/test_raster_edges_host.py (conditions, sensitivity) and tests/test_raster_edges_gpu.py (HIP against fp64).

A scene is the tuple (means [U,3], cov [U,3,3], sh [U,3,K], opacities [U], view [C,4,4], campos [C,3], K [C,3,3], W, H, deg).
Images are 33 x 17 (3 x 2 tiles, ragged on the right and bottom edges) or 48 x 32, U <= 700: the smallest shapes at which the
branch in question can occur, and small enough for fp64 autograd through the oracle to take seconds.

The branches (oracle/gsplat_raster.py; csrc/gs_raster.h and csrc/raster_bwd.hip on the HIP side):
  alpha_cap      alpha = min(0.999, o exp(-sigma)) caps, and the cap blocks the gradient (`raw <= 0.999f` false)
  round_edges    tile lists of 256 k and 256 k + 1 entries, pixels that stop in the first, second and third staging round
  opaque_stack   stop indices that vary widely inside a tile; whole tiles (full and ragged) in which every pixel stops, so that
                 the tile's last stop lies in front of the list's end and the entries behind it get zero rows
  frustum_sides  x / z or y / z beyond each of the four clamp limits, just inside them, and beyond two at once
  culling        near plane, off-screen by radius, zero opacity; two cameras that disagree on which Gaussians they see
  colour_floor   clamp_min(SH + 0.5, 0) holds exactly one channel of a Gaussian"""
import math

import torch

from oracle import gsplat_raster as G

CEILING = 1e-3          # the project's per-kernel parity ceiling
TENSORS = ("means", "covars", "sh", "opacities")


# ------------------------------------------------------------------------------------------------ pieces
def _pinhole(f, cx, cy):
    view = torch.eye(4)[None].clone()
    K = torch.tensor([[[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]]])
    return view, torch.zeros(1, 3), K


def _iso(s):
    """isotropic world covariances of standard deviation s [U]"""
    return torch.diag_embed((s * s)[:, None].expand(-1, 3)).contiguous()


def _place(px, py, z, f, cx, cy):
    """world points (identity camera) that project to pixel coordinates (px, py) at depth z"""
    px, py, z = (torch.as_tensor(t, dtype=torch.float32) for t in (px, py, z))
    return torch.stack([(px - cx) * z / f, (py - cy) * z / f, z.expand_as(px) if z.dim() == 0 else z], -1)


def _sh(U, deg, g, amp=0.1):
    return (torch.randn(U, 3, (deg + 1) ** 2, generator=g) * amp).contiguous()


# ------------------------------------------------------------------------------------------------ scenes
ALPHA_CAP_LISTED = (  # (pixel x, pixel y, depth, opacity, position in its tile's list)
    (4, 4, 2.0, 1.0, "front"), (24, 6, 4.0, 1.0, "middle"), (10, 11, 8.0, 0.9995, "back"), (32, 16, 4.0, 1.0, "middle"),
    (18, 12, 2.0, 0.9995, "front"), (28, 3, 4.0, 0.998, "middle"), (9, 16, 8.0, 1.0, "back"), (20, 16, 4.0, 0.998, "middle"))


def alpha_cap():
    """Identity rotation, depths 2 / 4 / 8, fx = fy = 16, principal point (16.5, 8.5): a listed Gaussian's fx x / z + cx is exactly
    k + 0.5 in fp32 (and in fp64), so sigma is exactly 0 at one pixel.  Listed Gaussians come first (indices 0 .. 7); opacity 1.0
    caps, 0.9995 caps at the centre pixel only, 0.998 never does.  The rest are faint fillers in front of and behind them.
    No listed pixel has |k + 0.5 - cx| = |l + 0.5 - cy|: there the SH basis term x^2 - y^2 is exactly zero in fp64 and a rounding
    residue under fused multiply-add, a zero of the test's making and not of the rasteriser's rules."""
    W, H, f, cx, cy, deg = 33, 17, 16.0, 16.5, 8.5, 2
    g = torch.Generator().manual_seed(41)
    L = ALPHA_CAP_LISTED
    lm = _place([l[0] + 0.5 for l in L], [l[1] + 0.5 for l in L], torch.tensor([l[2] for l in L]), f, cx, cy)
    ls = torch.tensor([0.10 * l[2] for l in L])          # 2D sigma ~1.7 px whatever the depth
    lo = torch.tensor([l[3] for l in L])
    nf = 36
    fz = torch.cat([2.2 + 1.6 * torch.rand(nf // 2, generator=g), 4.3 + 3.4 * torch.rand(nf // 2, generator=g)])
    fm = _place(torch.rand(nf, generator=g) * W, torch.rand(nf, generator=g) * H, fz, f, cx, cy)
    fs = (0.15 + 0.25 * torch.rand(nf, generator=g)) * fz / 4
    fo = 0.05 + 0.20 * torch.rand(nf, generator=g)
    means, op = torch.cat([lm, fm]).contiguous(), torch.cat([lo, fo]).contiguous()
    return (means, _iso(torch.cat([ls, fs])), _sh(means.shape[0], deg, g, 0.3), op, *_pinhole(f, cx, cy), W, H, deg)


def alpha_cap_single():
    """One capped Gaussian covering one pixel: a 1 x 1 image, a wide Gaussian of opacity exactly 1 whose mean is off the pixel
    centre, so dx, dy != 0 and only the cap keeps d_means2d, d_conics and d_opacity at zero."""
    W, H, f, deg = 1, 1, 16.0, 0
    means = _place([0.625], [0.375], 4.0, f, 0.5, 0.5)
    sh = torch.tensor([[[0.4], [-0.2], [0.7]]])
    return (means, _iso(torch.tensor([4.0])), sh, torch.ones(1), *_pinhole(f, 0.5, 0.5), W, H, deg)


ROUND_EDGES_GROUPS = dict(left=256, right=257, centre=87, low=512)   # tile 0: 256, tile 2: 256 + 1, tile 1: all 600, tile 4: 2 x 256


def round_edges():
    """600 faint Gaussians of one size (radius 7) with distinct depths, all over the middle tile of the top row of a 48 x 32
    image.  Where a Gaussian's centre lies decides which neighbouring tiles its radius reaches: 256 reach tile 0, 257 reach tile 2,
    512 reach the row below.  Opacities 0.04 .. 0.09: the middle tile's central pixels stop in the first staging round, the ones
    around them in the second and third, the rim never."""
    W, H, f, cx, cy, deg = 48, 32, 16.0, 24.0, 8.0, 0
    n = ROUND_EDGES_GROUPS
    U = n["left"] + n["right"] + n["centre"]
    g = torch.Generator().manual_seed(43)
    perm = torch.randperm(U, generator=g)                     # depth rank -> role: the groups interleave in every list
    col = torch.empty(U, dtype=torch.long)
    col[perm[:n["left"]]], col[perm[n["left"]:n["left"] + n["right"]]], col[perm[n["left"] + n["right"]:]] = 0, 2, 1
    low = torch.zeros(U, dtype=torch.bool)
    low[torch.randperm(U, generator=g)[:n["low"]]] = True
    u, v = torch.rand(U, generator=g), torch.rand(U, generator=g)
    px = torch.where(col == 0, 21.0 + 1.5 * u, torch.where(col == 2, 25.5 + 1.5 * u, 23.3 + 1.4 * u))
    py = torch.where(low, 9.5 + 1.5 * v, 7.3 + 1.4 * v)
    z = 4.0 + 0.002 * torch.arange(U)
    means = _place(px, py, z, f, cx, cy).contiguous()
    s = math.sqrt(4.2) * z / f                                # 2D variance 4.2 (1 + (x/z)^2) + 0.3: radius ceil(3 sqrt(~4.6)) = 7
    op = 0.04 + 0.05 * torch.rand(U, generator=g)
    return (means, _iso(s), _sh(U, deg, g, 0.5), op, *_pinhole(f, cx, cy), W, H, deg)


OPAQUE_STACK_WIDE = 14


def opaque_stack():
    """40 Gaussians of opacity about 0.9 over a 33 x 17 image.  26 are small (2D sigma 2 .. 5 px) and lie anywhere; 14 are wide
    (sigma 11 .. 14 px) and sit over the right half, at depths interleaved with the small ones.  The right-hand tiles (the full
    tile 1, the ragged tiles 2, 4 and 5) are covered so thickly that every pixel stops, at indices that vary with the small ones in
    front: the tile's last stop lies well in front of the list's end.  In tile 0 the wide ones fade out, so stopped pixels (indices
    varying widely) share the tile with pixels that run through the list."""
    W, H, f, cx, cy, deg, U = 33, 17, 16.0, 16.5, 8.5, 2, 40
    g = torch.Generator().manual_seed(47)
    r = lambda: torch.rand(U, generator=g)
    z = 3.0 + 0.05 * torch.randperm(U, generator=g).float()
    wide = torch.zeros(U, dtype=torch.bool)
    wide[torch.randperm(U, generator=g)[:OPAQUE_STACK_WIDE]] = True
    px = torch.where(wide, 27.0 + 3.0 * r(), 2.0 + 29.0 * r())
    py = torch.where(wide, 6.0 + 5.0 * r(), 1.0 + 15.0 * r())
    means = _place(px, py, z, f, cx, cy).contiguous()
    s = torch.where(wide, 11.0 + 3.0 * r(), 2.0 + 3.0 * r()) * z / f      # 2D sigma in pixels (before the blur)
    op = 0.85 + 0.10 * r()
    return (means, _iso(s), _sh(U, deg, g, 0.3), op, *_pinhole(f, cx, cy), W, H, deg)


FRUSTUM_GROUPS = ("xp", "xn", "yp", "yn", "inside", "two")   # six Gaussians each, in this order


def frustum_limits(W, H, K):
    """the clamp limits of x / z and y / z as oracle.project forms them: (+x, -x, +y, -y), positive numbers"""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    tx, ty = 0.5 * W / fx, 0.5 * H / fy
    return (W - cx) / fx + 0.3 * tx, cx / fx + 0.3 * tx, (H - cy) / fy + 0.3 * ty, cy / fy + 0.3 * ty


def frustum_sides():
    """Wide faint Gaussians whose x / z or y / z lies beyond one of the four clamp limits (a group per side), within 1 % inside a
    limit (fifth group, sides in turn) and beyond two limits at once (sixth group, the four corners).  The principal point is off
    centre, so all four limits differ."""
    W, H, f, cx, cy, deg, n = 33, 17, 16.0, 12.0, 10.5, 2, 6
    view, campos, K = _pinhole(f, cx, cy)
    lxp, lxn, lyp, lyn = frustum_limits(W, H, K[0])
    g = torch.Generator().manual_seed(53)
    r = lambda lo, hi, m=n: lo + (hi - lo) * torch.rand(m, generator=g)
    over, near = r(1.05, 1.4, 6 * n).reshape(6, n), r(0.99, 0.999)
    one = torch.ones(n)
    on_x = torch.tensor([True, True, False, False, True, True])        # the fifth group hugs +x, -x, +y, -y, +x, -x in turn
    xz = torch.stack([lxp * over[0], -lxn * over[1], r(-0.5, 0.8), r(-0.5, 0.8),
                      torch.tensor([lxp, -lxn, 0.3, -0.2, lxp, -lxn]) * torch.where(on_x, near, one),
                      torch.tensor([lxp, lxp, -lxn, -lxn, lxp, -lxn]) * over[4]])
    yz = torch.stack([r(-0.4, 0.3), r(-0.4, 0.3), lyp * over[2], -lyn * over[3],
                      torch.tensor([0.1, -0.2, lyp, -lyn, -0.3, 0.2]) * torch.where(on_x, one, near),
                      torch.tensor([lyp, -lyn, lyp, -lyn, -lyn, lyp]) * over[5]])
    z = 3.0 + 0.1 * torch.randperm(6 * n, generator=g).float()
    means = torch.stack([xz.reshape(-1) * z, yz.reshape(-1) * z, z], -1).contiguous()
    A = torch.randn(6 * n, 3, 3, generator=g) * 0.35
    cov = (A @ A.transpose(1, 2) + _iso(0.35 * z)).contiguous()   # wide: the radius reaches the screen from beyond the limit
    op = 0.05 + 0.10 * torch.rand(6 * n, generator=g)
    return (means, cov, _sh(6 * n, deg, g, 0.3), op, view, campos, K, W, H, deg)


CULLING_CLASSES = ("behind0", "offscreen0", "both", "transparent", "nowhere")   # eight Gaussians each, in this order


def culling():
    """Two cameras facing each other along z (camera 0 at the origin looking at +z, camera 1 at z = 10 looking back).  Classes:
    behind camera 0 but in front of camera 1; beyond camera 0's screen by more than their radius; visible in both; visible but
    of opacity exactly 0; behind camera 0 and off camera 1's screen (culled everywhere)."""
    W, H, f, cx, cy, deg, n = 33, 17, 16.0, 15.0, 9.0, 2, 8
    g = torch.Generator().manual_seed(59)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)
    sgn = lambda: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    behind = torch.stack([r(-1.5, 1.5), r(-0.8, 0.8), r(-3.0, -1.0)], -1)
    zo = r(3.0, 6.0)
    off = torch.stack([sgn() * r(2.6, 3.2) * zo, r(-0.3, 0.3) * zo, zo], -1)
    both = torch.stack([r(-1.0, 1.0), r(-0.5, 0.5), r(4.0, 6.0)], -1)
    clear = torch.stack([r(-1.0, 1.0), r(-0.5, 0.5), r(4.0, 6.0)], -1)
    zn = r(-3.0, -1.0)
    nowhere = torch.stack([sgn() * r(2.6, 3.2) * (10.0 - zn), r(-0.3, 0.3), zn], -1)
    means = torch.cat([behind, off, both, clear, nowhere]).contiguous()
    U = means.shape[0]
    A = torch.randn(U, 3, 3, generator=g) * 0.15
    cov = (A @ A.transpose(1, 2) + 1e-3 * torch.eye(3)).contiguous()
    op = 0.2 + 0.6 * torch.rand(U, generator=g)
    op[3 * n:4 * n] = 0.0
    view = torch.eye(4)[None].repeat(2, 1, 1)
    view[1, :3, :3] = torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    view[1, :3, 3] = torch.tensor([0.0, 0.0, 10.0])
    campos = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 10.0]])
    K = torch.tensor([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])[None].repeat(2, 1, 1).contiguous()
    return (means, cov, _sh(U, deg, g, 0.3), op, view.contiguous(), campos, K, W, H, deg)


def colour_floor_listed(U):
    """the Gaussians whose channel (index % 3) is held by the floor: every other one, and always the first and the last"""
    return sorted(set(range(0, U, 2)) | {U - 1})


def colour_floor(U, deg):
    """U Gaussians spread over a 33 x 17 image.  Small random SH (|SH| well under 0.5), then for the listed Gaussians the DC
    coefficient of ONE channel is set so that SH + 0.5 is about -0.6 there: that channel is floored, the other two are not."""
    W, H, f, cx, cy = 33, 17, 16.0, 16.5, 8.5
    g = torch.Generator().manual_seed(61 + 7 * U + deg)
    z = 3.0 + 2.0 * torch.rand(U, generator=g)
    means = _place(1.0 + 31.0 * torch.rand(U, generator=g), 1.0 + 15.0 * torch.rand(U, generator=g), z, f, cx, cy).contiguous()
    s = (1.0 + 2.0 * torch.rand(U, generator=g)) * z / f
    sh = _sh(U, deg, g, 0.04)
    for i in colour_floor_listed(U):
        sh[i, i % 3, 0] = -1.1 / 0.2820947917738781
    op = 0.1 + 0.3 * torch.rand(U, generator=g)
    return (means, _iso(s), sh, op, *_pinhole(f, cx, cy), W, H, deg)


# ------------------------------------------------------------------------------------------------ census
def census(scene, cam=0):
    """Run the oracle's own projection, binning and compositing (fp32, as it stands) on camera `cam` of a scene and count which
    branches were taken.  Stop indices are positions in the pixel's tile list; -1 = the pixel ran through its list."""
    means, cov, sh, op, view, campos, K, W, H, deg = scene
    v, Kc, cp = view[cam], K[cam], campos[cam]
    U = means.shape[0]
    pr = G.project(means, cov, v, Kc, W, H)
    radii = pr["radii"]
    vis = radii > 0
    z = pr["depths"]
    near = ~((z >= 1e-10) & (z <= 1e10))
    noclip = G.project(means, cov, v, Kc, W, H, radius_clip=0.0)["radii"] > 0
    clipped = noclip & ~vis
    offscreen = ~vis & ~near & ~clipped
    mc = means @ v[:3, :3].T + v[:3, 3]
    rz = 1.0 / torch.where(near, torch.ones_like(z), mc[:, 2])
    xz, yz = mc[:, 0] * rz, mc[:, 1] * rz
    lxp, lxn, lyp, lyn = frustum_limits(W, H, Kc)
    clamped = dict(xp=vis & (xz > lxp), xn=vis & (xz < -lxn), yp=vis & (yz > lyp), yn=vis & (yz < -lyn))
    d = means - cp[None]
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-20)
    raw_col = torch.einsum("uk,ukc->uc", G.sh_basis(d, deg), sh.permute(0, 2, 1)[:, :(deg + 1) ** 2]) + 0.5
    floored = vis[:, None] & (raw_col < 0)
    offs, ids = G.bin_and_sort(pr["means2d"], radii, z, W, H)
    tw, th = (W + 15) // 16, (H + 15) // 16
    stop = torch.full((H, W), -1, dtype=torch.long)
    T_img = torch.ones(H, W)
    capped_by = torch.zeros(U, dtype=torch.long)        # composited pairs capped at 0.999, per Gaussian
    used_by = torch.zeros(U, dtype=torch.long)          # composited pairs, per Gaussian
    capped_at, n_pairs, n_skipped, n_near_cap = {}, 0, 0, 0
    m2, con = pr["means2d"], pr["conics"]
    for ti in range(th):
        for tj in range(tw):
            t = ti * tw + tj
            lst = ids[int(offs[t]):int(offs[t + 1])].tolist()
            y0, x0 = ti * 16, tj * 16
            y1, x1 = min(y0 + 16, H), min(x0 + 16, W)
            py, px = torch.meshgrid(torch.arange(y0, y1, dtype=torch.float32) + 0.5, torch.arange(x0, x1, dtype=torch.float32) + 0.5,
                                    indexing="ij")
            px, py = px.reshape(-1), py.reshape(-1)
            T = torch.ones(px.numel())
            live = torch.ones(px.numel(), dtype=torch.bool)
            st = torch.full((px.numel(),), -1, dtype=torch.long)
            for idx, gi in enumerate(lst):
                dx, dy = m2[gi, 0] - px, m2[gi, 1] - py
                sigma = 0.5 * (con[gi, 0] * dx * dx + con[gi, 2] * dy * dy) + con[gi, 1] * dx * dy
                raw = op[gi] * torch.exp(-sigma)
                a = torch.clamp_max(raw, 0.999)
                cand = live & (sigma >= 0)
                use = cand & (a >= 1.0 / 255.0)
                nT = T * (1.0 - a)
                stp = use & (nT <= 1e-4)
                st[stp] = idx
                live = live & ~stp
                use = use & ~stp
                n_pairs += int(cand.sum())
                n_skipped += int((cand & (a < 1.0 / 255.0)).sum())
                cap = use & (raw > 0.999)
                n_near_cap += int((use & (raw > 0.99) & (raw <= 0.999)).sum())
                used_by[gi] += int(use.sum())
                if cap.any():
                    capped_by[gi] += int(cap.sum())
                    capped_at.setdefault(gi, []).append((t, idx, len(lst)))
                T = torch.where(use, nT, T)
            stop[y0:y1, x0:x1] = st.view(y1 - y0, x1 - x0)
            T_img[y0:y1, x0:x1] = T.view(y1 - y0, x1 - x0)
    return dict(radii=radii, visible=int(vis.sum()), vis=vis, culled_near=near, culled_offscreen=offscreen, culled_radius_clip=clipped,
                clamped=clamped, floored=floored, tile_offsets=offs, flatten_ids=ids, tile_lengths=(offs[1:] - offs[:-1]).tolist(),
                pairs=n_pairs, skipped=n_skipped, capped=int(capped_by.sum()), capped_by=capped_by, capped_at=capped_at,
                near_cap=n_near_cap, used_by=used_by, stop=stop, T=T_img, tw=tw, th=th)


def tile_of(W, t, stop):
    """the block of a per-pixel image that belongs to tile t"""
    tw = (W + 15) // 16
    ti, tj = divmod(t, tw)
    return stop[ti * 16:ti * 16 + 16, tj * 16:tj * 16 + 16]


# ------------------------------------------------------------------------------------------------ metrics
def per_gaussian_error(got, ref64):
    """max over Gaussians g of ||got_g - ref_g|| / (||ref_g|| + floor), floor = 1e-3 x the median of ||ref_g|| over the Gaussians
    whose reference gradient is non-zero.  Both tensors are [U, ...]; nothing is left out."""
    U = ref64.shape[0]
    r = ref64.double().reshape(U, -1)
    d = got.detach().cpu().double().reshape(U, -1) - r
    n = r.norm(dim=1)
    nz = n[n > 0]
    floor = 1e-3 * float(nz.median()) if nz.numel() else 1.0
    return float((d.norm(dim=1) / (n + floor)).max())


def per_pixel_error(got, ref64):
    return float((got.detach().cpu().double() - ref64.double()).abs().max())


def gate_from(oracle_fp32_error):
    """4 x the fp32 oracle's own error on the same metric (the margin for __expf against expf and the kernels' other summation
    order), never above the project's ceiling"""
    return min(4.0 * oracle_fp32_error, CEILING)


def cotangents(scene, seed):
    """seeded random incoming gradients for colour [C,H,W,3], depth and alpha [C,H,W]"""
    Cn, W, H = scene[4].shape[0], scene[7], scene[8]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Cn, H, W, 3, generator=g), torch.randn(Cn, H, W, generator=g), torch.randn(Cn, H, W, generator=g)
