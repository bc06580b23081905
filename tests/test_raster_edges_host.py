"""The constructed scenes of tests/raster_edge_scenes.py judged by the oracle alone, no GPU needed.

  * Conditions: each scene takes the branch it was built for (census of the oracle's own projection, binning and compositing).
  * Sensitivity: a copy of the oracle with exactly ONE rule changed is differentiated on the scene it concerns; the per-Gaussian
    metric of tests/test_raster_edges_gpu.py between that mutant and the true fp64 oracle must exceed the scene's gate by 10x on
    at least one gradient tensor.  The gate is formed as the GPU test forms it, min(4 x the fp32 oracle's own per-Gaussian error
    against fp64, 1e-3), here with the oracle's own composite order (none of the cases the GPU test gates wider is used here).
    So a kernel that got the rule wrong would fail the GPU test, and that is shown without touching a kernel.

The mutants are local restatements: `_project`, `_sh_colors`, `_rasterize` below are oracle/gsplat_raster.py's functions with
switches, and with every switch off they reproduce the oracle's fp64 gradients to 1e-12 per Gaussian (asserted for every scene)."""
import pytest
import torch

import raster_edge_scenes as S
from oracle import gsplat_raster as G

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ restatements with switches
def _straight_through(value, ungated):
    """`value` in the forward, the gradient of `ungated`"""
    return value.detach() + (ungated - ungated.detach())


def _project(means, covars, viewmat, K, W, H, drop_side=None):
    """G.project's differentiable outputs; drop_side in (xp, xn, yp, yn): that side of the clamp mask lets the gradient through"""
    R, t = viewmat[:3, :3], viewmat[:3, 3]
    mc = means @ R.T + t
    cs = torch.triu(covars)
    cs = cs + cs.transpose(1, 2) - torch.diag_embed(torch.diagonal(cs, dim1=1, dim2=2))
    cc = R[None] @ cs @ R.T[None]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = mc[:, 0], mc[:, 1], mc[:, 2]
    in_z = (z >= 1e-10) & (z <= 1e10)
    zs = torch.where(in_z, z, torch.ones_like(z))
    tfx, tfy = 0.5 * W / fx, 0.5 * H / fy
    lxp, lxn = (W - cx) / fx + 0.3 * tfx, cx / fx + 0.3 * tfx
    lyp, lyn = (H - cy) / fy + 0.3 * tfy, cy / fy + 0.3 * tfy
    rz = 1.0 / zs
    rz2 = rz * rz
    xz, yz = x * rz, y * rz
    cxz = torch.minimum(lxp, torch.maximum(-lxn, xz))
    cyz = torch.minimum(lyp, torch.maximum(-lyn, yz))
    if drop_side == "xp":
        cxz = torch.where(xz > lxp, _straight_through(cxz, xz), cxz)
    elif drop_side == "xn":
        cxz = torch.where(xz < -lxn, _straight_through(cxz, xz), cxz)
    elif drop_side == "yp":
        cyz = torch.where(yz > lyp, _straight_through(cyz, yz), cyz)
    elif drop_side == "yn":
        cyz = torch.where(yz < -lyn, _straight_through(cyz, yz), cyz)
    tx, ty = zs * cxz, zs * cyz
    zero = torch.zeros_like(rz)
    J = torch.stack([torch.stack([fx * rz, zero, -fx * tx * rz2], -1), torch.stack([zero, fy * rz, -fy * ty * rz2], -1)], 1)
    c2 = J @ cc @ J.transpose(1, 2)
    m2 = torch.stack([fx * x * rz + cx, fy * y * rz + cy], -1)
    a, b, c = c2[:, 0, 0] + 0.3, c2[:, 0, 1], c2[:, 1, 1] + 0.3
    det = a * c - b * b
    dets = torch.where(in_z & (det > 0), det, torch.ones_like(det))
    return dict(means2d=m2, depths=z, conics=torch.stack([c / dets, -b / dets, a / dets], -1))


def _sh_colors(means, campos, sh_uk3, deg, floor_through=False):
    d = means - campos[None]
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-20)
    B = G.sh_basis(d, deg)
    col = torch.einsum("uk,ukc->uc", B, sh_uk3[:, :B.shape[1]]) + 0.5
    return _straight_through(col.clamp_min(0.0), col) if floor_through else col.clamp_min(0.0)


def _rasterize(m2, con, col, op, W, H, offs, ids, bg, cap="clamp", stop_shift=0):
    """G.rasterize in two passes: the first finds each pixel's stop index, the second composites the entries in front of it.
    cap: "clamp" (the rule), "none" (no cap at all), "through" (capped value, gradient let through).  stop_shift: 0 (the rule:
    the stopping Gaussian is dropped), +1 (it is blended), -1 (the walk ends one composited entry early)."""
    dt = m2.dtype
    img, alpha_img = torch.zeros(H, W, col.shape[1], dtype=dt), torch.zeros(H, W, dtype=dt)
    tw, th = (W + 15) // 16, (H + 15) // 16

    def alpha_of(gi, px, py):
        dx, dy = m2[gi, 0] - px, m2[gi, 1] - py
        sigma = 0.5 * (con[gi, 0] * dx * dx + con[gi, 2] * dy * dy) + con[gi, 1] * dx * dy
        raw = op[gi] * torch.exp(-sigma)
        a = raw if cap == "none" else torch.clamp_max(raw, 0.999)
        if cap == "through":
            a = _straight_through(a, raw)
        return sigma, a

    for ti in range(th):
        for tj in range(tw):
            t = ti * tw + tj
            lst = ids[int(offs[t]):int(offs[t + 1])].tolist()
            y0, x0 = ti * 16, tj * 16
            y1, x1 = min(y0 + 16, H), min(x0 + 16, W)
            py, px = torch.meshgrid(torch.arange(y0, y1, dtype=dt) + 0.5, torch.arange(x0, x1, dtype=dt) + 0.5, indexing="ij")
            px, py = px.reshape(-1), py.reshape(-1)
            P = px.numel()
            with torch.no_grad():                                          # pass 1: where does each pixel stop, and was it used
                T, live = torch.ones(P, dtype=dt), torch.ones(P, dtype=torch.bool)
                bound = torch.full((P,), len(lst), dtype=torch.long)
                used = []
                for idx, gi in enumerate(lst):
                    sigma, a = alpha_of(gi, px, py)
                    use = live & (sigma >= 0) & (a >= 1.0 / 255.0)
                    nT = T * (1.0 - a)
                    stp = use & (nT <= 1e-4)
                    bound[stp] = idx
                    live = live & ~stp
                    use = use & ~stp
                    used.append(use)
                    T = torch.where(use, nT, T)
                if stop_shift == -1 and lst:                               # the last composited entry in front of the stop is lost
                    um = torch.stack(used)                                 # [L, P]
                    pos = torch.arange(len(lst))[:, None]
                    last = torch.where(um, pos, torch.full_like(pos, -1)).max(0).values
                    bound = torch.where((bound < len(lst)) & (last >= 0), last, bound)
                elif stop_shift == 1:
                    bound = bound + 1
            T = torch.ones(P, dtype=dt)
            acc = torch.zeros(P, col.shape[1], dtype=dt)
            for idx, gi in enumerate(lst):
                sigma, a = alpha_of(gi, px, py)
                use = (idx < bound) & (sigma >= 0) & (a >= 1.0 / 255.0)
                nT = T * (1.0 - a)
                vis = torch.where(use, a * T, torch.zeros_like(T))
                acc = acc + vis[:, None] * col[gi][None]
                T = torch.where(use, nT, T)
            acc = acc + T[:, None] * bg[None]
            img[y0:y1, x0:x1] = acc.view(y1 - y0, x1 - x0, -1)
            alpha_img[y0:y1, x0:x1] = (1.0 - T).view(y1 - y0, x1 - x0)
    return img, alpha_img


def _loss(scene, cn, leaves, dt, restated, cot, entry_cot=None, keep_culled=False, **mut):
    """The GPU test's loss: sum over cameras of <cotangents, (clamped colour over white, depth, alpha)>, composite order and
    visibility from the census.  restated=False differentiates the oracle's own functions.  entry_cot: the loss is instead a
    random linear functional of the per-entry projection outputs (means2d, conics, colour + depth) of the visible entries -
    of every entry with keep_culled, which is the "culled entry's gradient kept" mutant."""
    _, _, _, _, view, campos, K, W, H, deg = scene
    means, cov, sh, op = leaves
    wc, wd, wa = cot
    bg = torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=dt)
    total = 0
    for j, c in enumerate(cn):
        v, Kc, cp = view[j].to(dt), K[j].to(dt), campos[j].to(dt)
        mask = c["vis"]
        if restated:
            pr = _project(means, cov, v, Kc, W, H, drop_side=mut.get("drop_side"))
            col = _sh_colors(means, cp, sh.permute(0, 2, 1), deg, floor_through=mut.get("floor_through", False))
        else:
            f32 = G.f32
            G.f32 = dt
            try:
                pr = G.project(means, cov, v, Kc, W, H)
                col = G.sh_colors(means, cp, sh.permute(0, 2, 1), deg)
            finally:
                G.f32 = f32
        col4 = torch.cat([col * mask[:, None], pr["depths"][:, None]], -1)
        if entry_cot is not None:
            mk = torch.ones_like(mask) if keep_culled else mask
            e2, e3, e4 = entry_cot[j]
            out4 = torch.cat([col, pr["depths"][:, None]], -1)
            total = total + (((pr["means2d"] * e2).sum(-1) + (pr["conics"] * e3).sum(-1) + (out4 * e4).sum(-1)) * mk).sum()
            continue
        if restated:
            img, alpha = _rasterize(pr["means2d"], pr["conics"], col4, op, W, H, c["tile_offsets"], c["flatten_ids"], bg,
                                    cap=mut.get("cap", "clamp"), stop_shift=mut.get("stop_shift", 0))
        else:
            f32 = G.f32
            G.f32 = dt
            try:
                img, alpha = G.rasterize(pr["means2d"], pr["conics"], col4, op, W, H, c["tile_offsets"], c["flatten_ids"], bg)
            finally:
                G.f32 = f32
        total = total + (img[..., :3].clamp(0, 1) * wc[j].to(dt)).sum() + (img[..., 3] * wd[j].to(dt)).sum() + (alpha * wa[j].to(dt)).sum()
    return total


def _grads(scene, cn, dt, restated, cot, **kw):
    leaves = [t.detach().clone().to(dt).requires_grad_(True) for t in scene[:4]]
    loss = _loss(scene, cn, leaves, dt, restated, cot, **kw)
    loss.backward()
    return [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves], loss.detach()


_SCENES = dict(alpha_cap=S.alpha_cap, round_edges=S.round_edges, opaque_stack=S.opaque_stack, frustum_sides=S.frustum_sides,
               culling=S.culling, colour_floor=lambda: S.colour_floor(65, 2))
_CACHE = {}


def _prepared(name):
    """scene, census per camera, cotangents, true fp64 gradients and the gates: computed once, shared, never modified"""
    if name not in _CACHE:
        scene = _SCENES[name]()
        cn = [S.census(scene, j) for j in range(scene[4].shape[0])]
        cot = S.cotangents(scene, 1000 + len(name))
        kw = {}
        if name == "culling":                                              # judged on the projection with random entry cotangents
            g = torch.Generator().manual_seed(77)
            U = scene[0].shape[0]
            kw["entry_cot"] = [tuple(torch.randn(U, n, generator=g, dtype=F64) for n in (2, 3, 4)) for _ in cn]
        ref64, _ = _grads(scene, cn, F64, False, cot, **{k: ([tuple(t for t in e) for e in v]) for k, v in kw.items()})
        kw32 = {k: [tuple(t.float() for t in e) for e in v] for k, v in kw.items()}
        ref32, _ = _grads(scene, cn, torch.float32, False, cot, **kw32)
        e32 = {n: S.per_gaussian_error(a, b) for n, a, b in zip(S.TENSORS, ref32, ref64)}
        gate = {n: S.gate_from(e32[n]) for n in S.TENSORS}
        _CACHE[name] = dict(scene=scene, census=cn, cot=cot, ref64=ref64, e32=e32, gate=gate, kw=kw)
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ conditions
def test_alpha_cap_conditions():
    scene = S.alpha_cap()
    c = S.census(scene)
    op = scene[3]
    assert c["visible"] == op.numel()
    for i, (_, _, _, o, _) in enumerate(S.ALPHA_CAP_LISTED):
        assert float(op[i]) == torch.tensor(o).item()
        if o == 1.0:
            assert int(c["capped_by"][i]) >= 1, i                         # every opacity-1 Gaussian has a composited capped pair
        elif o > 0.999:
            assert int(c["capped_by"][i]) == 1, i                         # 0.9995: the centre pixel only
        else:
            assert int(c["capped_by"][i]) == 0 and int(c["used_by"][i]) > 0, i
    assert int(c["capped_by"][len(S.ALPHA_CAP_LISTED):].sum()) == 0       # no filler caps
    assert c["near_cap"] >= 1                                              # raw alpha in (0.99, 0.999]: the branch's other side, close by
    where = [w for ws in c["capped_at"].values() for w in ws]
    assert any(i == 0 and n > 2 for _, i, n in where), "a capped pair at the front of a list"
    assert any(0 < i < n - 1 for _, i, n in where), "a capped pair in the middle of a list"
    assert any(i == n - 1 and n > 2 for _, i, n in where), "a capped pair at the back of a list"
    assert len({t for t, _, _ in where}) >= 4                             # in four tiles, the one-pixel corner tile among them
    assert any(t == c["tw"] * c["th"] - 1 for t, _, _ in where)
    assert int((c["stop"] >= 0).sum()) == 0                                # no pixel stops, so none stops before a capped pair
    one = S.census(S.alpha_cap_single())
    assert one["pairs"] == 1 and one["capped"] == 1 and one["skipped"] == 0


def test_round_edges_conditions():
    scene = S.round_edges()
    c = S.census(scene)
    W, n = scene[7], S.ROUND_EDGES_GROUPS
    U = scene[0].shape[0]
    assert U == 600 and c["visible"] == U and len(set(scene[0][:, 2].tolist())) == U     # distinct depths
    lens = c["tile_lengths"]
    assert lens[1] == U and lens[0] == n["left"] == 256 and lens[2] == n["right"] == 257 and lens[4] == n["low"] == 512
    st = S.tile_of(W, 1, c["stop"])
    s = st[st >= 0]
    assert int((s < 256).sum()) > 0 and int(((s >= 256) & (s < 512)).sum()) > 0 and int((s >= 512).sum()) > 0
    assert int((st < 0).sum()) > 0                                         # and pixels of the same tile that never stop
    assert c["skipped"] > 0 and c["capped"] == 0
    assert float(scene[3].min()) >= 0.03 and float(scene[3].max()) <= 0.09


def test_opaque_stack_conditions():
    scene = S.opaque_stack()
    c = S.census(scene)
    assert scene[0].shape[0] == 40 and c["visible"] == 40
    lens = c["tile_lengths"]
    st = S.tile_of(scene[7], 0, c["stop"])
    s = st[st >= 0]
    assert s.numel() >= 100 and int((st < 0).sum()) >= 50                  # tile 0: stopped and running pixels share the tile,
    assert int(s.max()) - int(s.min()) >= 20 and len(set(s.tolist())) >= 10   # and the stops vary widely
    for t, shape in ((1, (16, 16)), (2, (16, 1)), (4, (1, 16)), (5, (1, 1))):  # a full tile and three ragged ones:
        st = S.tile_of(scene[7], t, c["stop"])
        assert tuple(st.shape) == shape
        assert bool((st >= 0).all()), t                                    # EVERY pixel stops, so the tile's last stop is not the
        assert int(st.max()) < lens[t] - 1, t                              # list's end: entries lie behind it (more than one)
    st = S.tile_of(scene[7], 1, c["stop"])
    assert int(st.max()) - int(st.min()) >= 10 and lens[1] - 1 - int(st.max()) >= 10


def test_frustum_sides_conditions():
    scene = S.frustum_sides()
    c = S.census(scene)
    n = 6
    assert c["visible"] == 6 * n                                           # every group non-empty and visible
    cl = {k: v.reshape(6, n) for k, v in c["clamped"].items()}
    anyc = cl["xp"] | cl["xn"] | cl["yp"] | cl["yn"]
    for gi, side in enumerate(("xp", "xn", "yp", "yn")):
        assert bool(cl[side][gi].all()) and int(anyc[gi].sum()) == n and all(not bool(cl[o][gi].any()) for o in cl if o != side)
    assert not bool(anyc[4].any())                                         # just inside: not clamped ...
    means, K = scene[0], scene[6][0]
    lim = S.frustum_limits(scene[7], scene[8], K)
    r = torch.stack([means[24:30, 0] / means[24:30, 2] / lim[0], -means[24:30, 0] / means[24:30, 2] / lim[1],
                     means[24:30, 1] / means[24:30, 2] / lim[2], -means[24:30, 1] / means[24:30, 2] / lim[3]]).max(0).values
    assert bool(((r > 0.989) & (r < 1.0)).all())                           # ... but within 1 % of a limit
    two = torch.stack([cl[k][5] for k in ("xp", "xn", "yp", "yn")]).sum(0)
    assert bool((two == 2).all()) and all(bool(cl[k][5].any()) for k in cl)
    assert len({round(x, 6) for x in lim}) == 4                            # off-centre principal point: four different limits
    assert int((c["stop"] >= 0).sum()) == 0


def test_culling_conditions():
    scene = S.culling()
    c0, c1 = S.census(scene, 0), S.census(scene, 1)
    n = 8
    cls = lambda t: t.reshape(5, n)
    assert bool(cls(c0["culled_near"])[0].all()) and bool(cls(c1["vis"])[0].all())          # behind camera 0, seen by camera 1
    assert bool(cls(c0["culled_offscreen"])[1].all())                                       # beyond camera 0's screen by their radius
    assert bool(cls(c0["vis"])[2].all()) and bool(cls(c1["vis"])[2].all())                  # visible in both
    assert bool(cls(c0["vis"])[3].all()) and float(scene[3][3 * n:4 * n].abs().max()) == 0  # visible, opacity exactly 0
    assert int(c0["used_by"][3 * n:4 * n].sum()) == 0
    assert not bool(cls(c0["vis"])[4].any()) and not bool(cls(c1["vis"])[4].any())          # culled by every camera
    assert int(c0["culled_radius_clip"].sum()) == 0        # eps2d = 0.3 keeps every radius >= 2: radius_clip = 0.1 cannot cull


@pytest.mark.parametrize("U", [1, 63, 64, 65])
@pytest.mark.parametrize("deg", [0, 2, 4])
def test_colour_floor_conditions(U, deg):
    scene = S.colour_floor(U, deg)
    c = S.census(scene)
    assert c["visible"] == U and scene[2].shape == (U, 3, (deg + 1) ** 2)
    listed = S.colour_floor_listed(U)
    assert 0 in listed and U - 1 in listed
    want = torch.zeros(U, 3, dtype=torch.bool)
    for i in listed:
        want[i, i % 3] = True
    assert torch.equal(c["floored"], want)                                 # exactly one channel of the listed, none of the others
    assert int(c["used_by"][listed].min()) > 0                             # and each of them is composited somewhere


# ------------------------------------------------------------------------------------------------ the restatement is the oracle
@pytest.mark.parametrize("name", list(_SCENES))
def test_restatement_without_mutation_is_the_oracle(name):
    p = _prepared(name)
    got, _ = _grads(p["scene"], p["census"], F64, True, p["cot"], **p["kw"])
    for n, a, b in zip(S.TENSORS, got, p["ref64"]):
        assert S.per_gaussian_error(a, b) < 1e-12, n


# ------------------------------------------------------------------------------------------------ sensitivity
MUTANTS = [("alpha_cap", "cap removed", dict(cap="none")),
           ("alpha_cap", "cap gradient passed through", dict(cap="through")),
           ("round_edges", "stopping Gaussian blended", dict(stop_shift=1)),
           ("round_edges", "stop index off by one", dict(stop_shift=-1)),
           ("opaque_stack", "stopping Gaussian blended", dict(stop_shift=1)),
           ("opaque_stack", "stop index off by one", dict(stop_shift=-1)),
           ("frustum_sides", "+x dropped from the clamp mask", dict(drop_side="xp")),
           ("frustum_sides", "-x dropped from the clamp mask", dict(drop_side="xn")),
           ("frustum_sides", "+y dropped from the clamp mask", dict(drop_side="yp")),
           ("frustum_sides", "-y dropped from the clamp mask", dict(drop_side="yn")),
           ("colour_floor", "floor gradient passed through", dict(floor_through=True)),
           ("culling", "culled entry's gradient kept", dict(keep_culled=True))]


@pytest.mark.parametrize("name,what,mut", MUTANTS, ids=[f"{a}-{b.replace(' ', '_')}" for a, b, _ in MUTANTS])
def test_mutant_oracle_exceeds_the_gate_tenfold(name, what, mut):
    p = _prepared(name)
    got, _ = _grads(p["scene"], p["census"], F64, True, p["cot"], **p["kw"], **mut)
    ratios = {}
    for n, a, b in zip(S.TENSORS, got, p["ref64"]):
        e = S.per_gaussian_error(a, b)
        ratios[n] = e / p["gate"][n] if p["gate"][n] > 0 else (float("inf") if e > 0 else 0.0)
        print(f"[{name}] {what}: d_{n} mutant vs fp64 {e:.3e}   oracle fp32 vs fp64 {p['e32'][n]:.3e}   gate {p['gate'][n]:.3e}")
    assert max(ratios.values()) >= 10.0, (name, what, ratios)
