"""Oracle of the pose optimiser's parametrisation (csrc/post_opt.hip: v3a_camera_adjust; vist3a_amd.post_opt): a torch
restatement, in the dtype of its inputs, of the reference's CameraOptModule.forward followed by what the rasteriser takes from a
camera, inverse(c2w') and c2w'[:3,3].  Pinned to tensors recorded from the reference's own module
(tests/golden/pose_opt_ref.safetensors, written by tests/golden/make_golden_pose_opt.py) by tests/test_pose_opt_host.py.
Differentiable in `deltas`: torch.autograd through it is the gradient reference of the GPU tests."""
import torch


def rotation_6d(d6):
    """[...,6] -> [...,3,3] with ROWS b1, b2, b3: Gram-Schmidt with F.normalize's clamp of the norm at 1e-12"""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    b3 = torch.linalg.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def transform(deltas):
    """deltas [...,9] = (dx[3], drot[6]) -> [Rd | dx] as [...,4,4]"""
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=deltas.dtype, device=deltas.device)
    Rd = rotation_6d(deltas[..., 3:] + ident)
    top = torch.cat([Rd, deltas[..., :3, None]], -1)
    bottom = torch.zeros(*deltas.shape[:-1], 1, 4, dtype=deltas.dtype, device=deltas.device)
    bottom[..., 0, 3] = 1.0
    return torch.cat([top, bottom], -2)


def adjust(c2w, deltas):
    """CameraOptModule.forward: c2w' = c2w [Rd | dx]"""
    return c2w @ transform(deltas)


def camera_adjust(c2w, deltas):
    """-> (viewmat = inverse(c2w'), campos = c2w'[:3,3]): what ops.camera_adjust returns, by the reference's route"""
    c = adjust(c2w, deltas)
    return torch.linalg.inv(c), c[..., :3, 3]


def closed_form(w2c, c2w, deltas):
    """The kernel's route: viewmat = [Rd^T | -Rd^T dx] w2c, campos = c2w[:3,:3] dx + c2w[:3,3]"""
    T = transform(deltas)
    Rt, dx = T[..., :3, :3].transpose(-1, -2), T[..., :3, 3]
    A = torch.zeros_like(T)
    A[..., :3, :3] = Rt
    A[..., :3, 3] = -(Rt @ dx[..., None])[..., 0]
    A[..., 3, 3] = 1.0
    return A @ w2c, (c2w[..., :3, :3] @ dx[..., None])[..., 0] + c2w[..., :3, 3]


def cameras(V, seed, dtype=torch.float64):
    """V rigid camera-to-world matrices: random rotations (QR) and centres a few units from the origin"""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(V, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    q[:, :, 2] *= torch.linalg.det(q)[:, None]
    c2w = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1)
    c2w[:, :3, :3] = q
    c2w[:, :3, 3] = torch.randn(V, 3, generator=g, dtype=torch.float64) * 2.0
    return c2w.to(dtype)


def deltas(V, seed, size, dtype=torch.float64):
    """V x 9 normal deltas of standard deviation `size` (0: zeros)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, 9, generator=g, dtype=torch.float64) * size).to(dtype)


def pose_error(c2w_a, c2w_b):
    """mean translation distance and mean rotation angle (radians) between two sets of cameras, fp64"""
    a, b = c2w_a.detach().cpu().double(), c2w_b.detach().cpu().double()
    dt = (a[:, :3, 3] - b[:, :3, 3]).norm(dim=-1).mean()
    R = a[:, :3, :3].transpose(-1, -2) @ b[:, :3, :3]
    cos = ((torch.diagonal(R, dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1)
    return float(dt), float(torch.acos(cos).mean())


GOLDEN_CASES = {"zero": 0.0, "small": 1e-2, "large": 0.5}   # name -> size of the deltas; V = 3 each


def oracle_render(dt, means, cov, sh, op, view, campos, K, W, H, sh_degree):
    """One camera through oracle/gsplat_raster.py in `dt`, black background, clamped RGB [H,W,3]: project, cull, bin and sort (the
    sort key takes the depth's float32 bits, so that step runs with the module's dtype switch at float32), composite.  sh [U,3,K]."""
    from oracle import gsplat_raster as G
    old = G.f32
    G.f32 = dt
    try:
        p = G.project(means.to(dt), cov.to(dt), view.to(dt), K.to(dt), W, H)
        mask = p["radii"] > 0
        col = G.sh_colors(means.to(dt), campos.to(dt), sh.to(dt).permute(0, 2, 1), sh_degree) * mask[:, None]
        col4 = torch.cat([col, p["depths"][:, None]], -1)
        G.f32 = torch.float32
        offs, ids = G.bin_and_sort(p["means2d"].detach(), p["radii"], p["depths"].detach(), W, H)
        G.f32 = dt
        img, _ = G.rasterize(p["means2d"], p["conics"], col4, op.to(dt), W, H, offs, ids, torch.zeros(4, dtype=dt))
    finally:
        G.f32 = old
    return img[..., :3].clamp(0, 1)


def oracle_pose_loop(dt, means, cov, sh0, logit0, ext, Kpix, targets, order, W, H, *, sh_degree, max_steps, pose_lr, pose_reg,
                     train_scene, grid_of=None, lr_opacities=5e-2, lr_sh=2.5e-3, ssim_lambda=0.2):
    """The pose-optimising loop on the CPU in `dt`, independent of the package: oracle/gsplat_raster.py (which culls, bins and sorts
    for itself every step), tests/ssim_loss_oracle.py, torch.optim.Adam per tensor (eps 1e-15, as the loop) and for the deltas
    torch.optim.Adam(lr=pose_lr, weight_decay=pose_reg) (torch's eps 1e-8) + ExponentialLR(0.01 ** (1 / max_steps)), all stepped once
    per step as the reference steps them.  means [U,3], cov [U,3,3] are fixed; sh0 [U,3,K] and logit0 [U] train when `train_scene`;
    ext: camera-to-world f32 [V,4,4] (the bases are derived as the loop derives them: two float32 inversions); Kpix [V,3,3] in
    pixels; targets [V,H,W,3]; order: the view of every step; grid_of: view -> delta row (default: the identity).
    -> (loss per step, float64 [steps]; the trained deltas [rows,9] in dt)."""
    import ssim_loss_oracle as SO
    w2c = torch.linalg.inv(ext.float())
    c2w = torch.linalg.inv(w2c)
    w2c, c2w = w2c.to(dt), c2w.to(dt)
    rows = len(set(order)) if grid_of is not None else ext.shape[0]
    grid_of = grid_of or {j: j for j in range(ext.shape[0])}
    deltas = torch.zeros(rows, 9, dtype=dt, requires_grad=True)
    lg = logit0.clone().to(dt).requires_grad_(train_scene)
    s0, sN = sh0[..., :1].clone().to(dt).requires_grad_(train_scene), sh0[..., 1:].clone().to(dt).requires_grad_(train_scene)
    opts = []
    if train_scene:
        opts = [torch.optim.Adam([t], lr=lr, eps=1e-15) for t, lr in ((lg, lr_opacities), (s0, lr_sh), (sN, lr_sh / 20))]
    popt = torch.optim.Adam([deltas], lr=pose_lr, weight_decay=pose_reg)
    sched = torch.optim.lr_scheduler.ExponentialLR(popt, gamma=0.01 ** (1.0 / max_steps))
    curve = []
    for j in order:
        view, campos = closed_form(w2c[j], c2w[j], deltas[grid_of[j]])
        img = oracle_render(dt, means, cov, torch.cat([s0, sN], -1), torch.sigmoid(lg), view, campos, Kpix[j], W, H, sh_degree)
        loss = SO.photometric_loss(img[None], targets[j:j + 1].to(dt), ssim_lambda)[0]
        for o in opts + [popt]:
            o.zero_grad()
        loss.backward()
        for o in opts + [popt]:
            o.step()
        sched.step()
        curve.append(float(loss.detach()))
    return torch.tensor(curve, dtype=torch.float64), deltas.detach()
