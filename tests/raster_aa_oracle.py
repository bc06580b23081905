"""Reference for the rasteriser's antialiased mode (gsplat rasterize_mode="antialiased", the Mip-Splatting 2D filter), on top of
oracle/gsplat_raster.py and its dtype switch (G.f32), as tests/test_raster_bwd_gpu.py::_oracle_render wraps the classic mode.

Each camera-Gaussian entry's opacity is multiplied by  comp = sqrt(max(0, det(S) / det(S + eps2d I))),  S = J Cc J^T the projected
2D covariance BEFORE the blur.  Culling, radius, conic, means2d and colours are the classic ones (gsplat culls and sizes on the
blurred covariance in both modes).  In fp64 with torch autograd this is the reference for values and gradients; in fp32 it is the
comparison figure.  Nothing here is read by the package.

  cov2d(means, covars, viewmat, K, W, H)            S [U,2,2] with G.project's arithmetic (tests/test_raster_aa_host.py pins it: the
                                                    inverse of S + eps2d I is G.project's conic)
  compensation(S, eps2d)                            comp [U], by the definition
  dcomp_dcov2d(S, eps2d)                            the closed form the HIP backward uses:
                                                    ((1 - r) B^-1 - eps2d det(B^-1) I) / (2 comp), r = comp^2, B = S + eps2d I; 0 at comp == 0
  render(dtype, ...)                                one camera: clamped RGB over a background + depth + alpha, and comp"""
import torch

from oracle import gsplat_raster as G

EPS2D = 0.3


def cov2d(means, covars, viewmat, K, width, height, near_plane=1e-10, far_plane=1e10):
    """J Cc J^T [U,2,2] of one pinhole camera in G.f32, the steps of G.project up to (not including) the blur."""
    f = G.f32
    means, covars, viewmat, K = means.to(f), covars.to(f), viewmat.to(f), K.to(f)
    U = means.shape[0]
    R, t = viewmat[:3, :3], viewmat[:3, 3]
    mc = means @ R.T + t
    iu = torch.triu_indices(3, 3)
    cs = torch.zeros(U, 3, 3, dtype=f)
    cs[:, iu[0], iu[1]] = covars[:, iu[0], iu[1]]
    cs = cs + cs.transpose(1, 2) - torch.diag_embed(torch.diagonal(cs, dim1=1, dim2=2))
    cc = R[None] @ cs @ R.T[None]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = mc[:, 0], mc[:, 1], mc[:, 2]
    in_z = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(in_z, z, torch.ones_like(z))
    tan_fovx, tan_fovy = 0.5 * width / fx, 0.5 * height / fy
    lim_xp, lim_xn = (width - cx) / fx + 0.3 * tan_fovx, cx / fx + 0.3 * tan_fovx
    lim_yp, lim_yn = (height - cy) / fy + 0.3 * tan_fovy, cy / fy + 0.3 * tan_fovy
    rz = 1.0 / zs
    rz2 = rz * rz
    tx = zs * torch.minimum(lim_xp, torch.maximum(-lim_xn, x * rz))
    ty = zs * torch.minimum(lim_yp, torch.maximum(-lim_yn, y * rz))
    zero = torch.zeros_like(rz)
    J = torch.stack([torch.stack([fx * rz, zero, -fx * tx * rz2], -1), torch.stack([zero, fy * rz, -fy * ty * rz2], -1)], 1)
    return J @ cc @ J.transpose(1, 2)


def compensation(S, eps2d=EPS2D):
    """sqrt(max(0, det S / det(S + eps2d I))) per matrix of S [...,2,2]; exactly 0 (with a zero gradient) where the ratio is <= 0."""
    a, c, bb = S[..., 0, 0], S[..., 1, 1], S[..., 0, 1] * S[..., 1, 0]   # both off-diagonal entries: autograd's gradient is symmetric
    det_orig = a * c - bb
    det_blur = (a + eps2d) * (c + eps2d) - bb
    r = det_orig / det_blur
    pos = r > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, r, torch.ones_like(r))), torch.zeros_like(r))


def dcomp_dcov2d(S, eps2d=EPS2D):
    """d comp / d S as a symmetric [...,2,2] matrix (S01 and S10 taken as independent entries), the closed form of the HIP backward."""
    eye = torch.eye(2, dtype=S.dtype)
    B = S + eps2d * eye
    a, b, c = B[..., 0, 0], B[..., 0, 1], B[..., 1, 1]
    det = a * c - b * b
    X = torch.stack([torch.stack([c, -b], -1), torch.stack([-b, a], -1)], -2) / det[..., None, None]
    comp = compensation(S, eps2d)
    r = comp * comp
    dr = (1 - r)[..., None, None] * X - (eps2d / det)[..., None, None] * eye
    pos = comp > 0
    return torch.where(pos[..., None, None], dr / (2 * torch.where(pos, comp, torch.ones_like(comp)))[..., None, None], torch.zeros_like(dr))


def render(dtype, means, cov, sh_uk3, op, view, campos, K, W, H, deg, mask, offs, ids, monkeypatch, background=(1.0, 1.0, 1.0),
           antialiased=True):
    """One camera in `dtype` with the given radii mask (bool [U]) and composite order (tile offsets, Gaussian ids), as the HIP
    forward chose them: -> (clamped RGB [H,W,3], depth [H,W], alpha [H,W], comp [U] (0 outside the mask), projection dict)."""
    with monkeypatch.context() as m:
        m.setattr(G, "f32", dtype)
        pr = G.project(means, cov, view.to(dtype), K.to(dtype), W, H)
        comp = compensation(cov2d(means, cov, view.to(dtype), K.to(dtype), W, H)) * mask.to(dtype)
        col = G.sh_colors(means, campos.to(dtype), sh_uk3, deg) * mask[:, None]
        col4 = torch.cat([col, pr["depths"][:, None]], -1)
        eff = op * comp if antialiased else op
        bg = torch.tensor([*background, 0.0], dtype=dtype)
        img, alpha = G.rasterize(pr["means2d"], pr["conics"], col4, eff, W, H, offs, ids, bg)
    return img[..., :3].clamp(0, 1), img[..., 3], alpha, comp, dict(pr, colors=col4)
