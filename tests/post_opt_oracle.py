"""Plain-torch restatements for the post-optimisation tests: the splat activation (differentiable, any dtype), its closed-form
backward as csrc/post_opt.hip computes it, and the small scene the loop tests share."""
import math

import torch


def quat_R(q):
    """xyzw, normalised the way v3a_gaussian_adapter normalises it"""
    q = q / (q.norm(dim=-1, keepdim=True) + 1e-8)
    i, j, k, r = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    return torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                        two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], -1).reshape(*q.shape[:-1], 3, 3)


def splat_activate(log_scales, quats, logits):
    R = quat_R(quats)
    s = torch.exp(log_scales)
    return R @ torch.diag_embed(s * s) @ R.transpose(-1, -2), torch.sigmoid(logits)


def splat_activate_backward(log_scales, quats, logits, G, d_op):
    """Closed form, as the kernel: dD_m = r_m^T G r_m, d log s_m = 2 s_m^2 dD_m, dR = (G + G^T) R D, R = I + t M(q), t = 2 / |q|^2."""
    R = quat_R(quats)
    s2 = torch.exp(2 * log_scales)
    dD = torch.einsum("uam,uab,ubm->um", R, G, R)
    g = ((G + G.transpose(-1, -2)) @ R) * s2[:, None, :]
    i, j, k, r = quats.unbind(-1)
    n2 = (quats * quats).sum(-1)
    t = 2.0 / n2
    g = g.reshape(-1, 9).unbind(-1)
    S = (g[0] * -(j * j + k * k) + g[1] * (i * j - k * r) + g[2] * (i * k + j * r) + g[3] * (i * j + k * r) + g[4] * -(i * i + k * k)
         + g[5] * (j * k - i * r) + g[6] * (i * k - j * r) + g[7] * (j * k + i * r) + g[8] * -(i * i + j * j))
    di = j * (g[1] + g[3]) + k * (g[2] + g[6]) + r * (g[7] - g[5]) - 2 * i * (g[4] + g[8])
    dj = i * (g[1] + g[3]) + k * (g[5] + g[7]) + r * (g[2] - g[6]) - 2 * j * (g[0] + g[8])
    dk = i * (g[2] + g[6]) + j * (g[5] + g[7]) + r * (g[3] - g[1]) - 2 * k * (g[0] + g[4])
    dr = i * (g[7] - g[5]) + j * (g[2] - g[6]) + k * (g[3] - g[1])
    c = 2 * t / n2 * S
    d_q = torch.stack([t * di - c * i, t * dj - c * j, t * dk - c * k, t * dr - c * r], -1)
    o = torch.sigmoid(logits)
    return 2 * s2 * dD, d_q, d_op * o * (1 - o)


def activation_case(U, seed, dtype=torch.float64):
    """log-scales, quaternions (rows 0 / 1 of every 3 scaled to norm 0.5 / 2), logits, a full and an upper-triangular d_covars, d_opacities"""
    g = torch.Generator().manual_seed(seed)
    ls = torch.log(0.05 + 0.3 * torch.rand(U, 3, generator=g, dtype=torch.float64))
    q = torch.randn(U, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    q[0::3] *= 0.5
    q[1::3] *= 2.0
    lg = torch.randn(U, generator=g, dtype=torch.float64) * 2
    G = torch.randn(U, 3, 3, generator=g, dtype=torch.float64)
    d_op = torch.randn(U, generator=g, dtype=torch.float64)
    return tuple(t.to(dtype) for t in (ls, q, lg, G, torch.triu(G), d_op))


def loop_scene(U=300, W=64, H=48, K=4, seed=41):
    """~300 Gaussians in front of 3 cameras of 48 x 64, SH degree 1: Gaussians fields as float32 CPU tensors (scales, quaternions,
    opacities in [0.05, 0.95] with the first 10 at 0.005 - under min_opacity), camera-to-world extrinsics and normalised intrinsics."""
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(U, 3, generator=g) * torch.tensor([0.8, 0.8, 1.0]) + torch.tensor([0.0, 0.0, 4.0])
    scales = 0.08 + 0.25 * torch.rand(U, 3, generator=g)
    quats = torch.nn.functional.normalize(torch.randn(U, 4, generator=g), dim=-1)
    sh = torch.randn(U, 3, K, generator=g) * 0.3
    op = 0.05 + 0.9 * torch.rand(U, generator=g)
    op[:10] = 0.005
    views, Ks = [], []
    for i in range(3):
        yaw, f = 0.1 * i - 0.1, 50.0 + 5 * i
        c, s = math.cos(yaw), math.sin(yaw)
        v = torch.eye(4)
        v[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        v[:3, 3] = torch.tensor([0.05 * i, 0.0, 0.1 * i])
        views.append(v)
        Ks.append(torch.tensor([[f / W, 0, 0.5], [0, f * 1.1 / H, 0.5], [0, 0, 1.0]]))
    w2c = torch.stack(views)
    return dict(means=means, scales=scales, quats=quats, sh=sh, op=op, c2w=torch.linalg.inv(w2c), Kn=torch.stack(Ks), W=W, H=H)
