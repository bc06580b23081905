"""Plain-torch restatement of the reference's bilateral grid (third_party_model/anysplat/src/post_opt/lib_bilagrid.py::BilateralGrid /
slice / total_variation_loss, the one-grid-per-image case) in the REFERENCE layout, grids [V,12,L,GY,GX], with the dtype as a parameter:
the oracle of csrc/bilagrid.hip.  tests/test_bilagrid_host.py pins it to tensors recorded from the reference's own module
(tests/golden/bilagrid_ref.safetensors)."""
import torch
import torch.nn.functional as F

GRAY = (0.299, 0.587, 0.114)   # held in float32, as the reference's buffer holds them


def pixel_centres(H, W, dtype):
    """[1,H,W,2]: (x, y) = ((j + 0.5) / W, (i + 0.5) / H), what the loop's meshgrid gives"""
    y, x = torch.meshgrid((torch.arange(H, dtype=dtype) + 0.5) / H, (torch.arange(W, dtype=dtype) + 0.5) / W, indexing="ij")
    return torch.stack([x, y], -1)[None]


def slice_grid(rgb, grids, xy=None, guide=None):
    """rgb [N,H,W,3], grids [N,12,L,GY,GX] (the same dtype) -> rgb_out [N,H,W,3]; `xy` [N,H,W,2] in [0,1] (default: pixel centres);
    `guide` [N,H,W,3]: the colours the guidance axis is computed from (default rgb; rgb.detach() cuts the guidance gradient)"""
    N, H, W, _ = rgb.shape
    dt = rgb.dtype
    if xy is None:
        xy = pixel_centres(H, W, dt).expand(N, H, W, 2)
    gray = (rgb if guide is None else guide) @ torch.tensor(GRAY, dtype=torch.float32).to(dt)[:, None]                       # [N,H,W,1]
    pos = torch.cat([(xy - 0.5) * 2, gray * 2.0 - 1.0], -1)[:, None]                           # [N,1,H,W,3] in [-1,1]
    A = F.grid_sample(grids, pos, mode="bilinear", align_corners=True, padding_mode="border")  # [N,12,1,H,W]
    A = A[:, :, 0].permute(0, 2, 3, 1).reshape(N, H, W, 3, 4)
    return (A[..., :3] @ rgb[..., None])[..., 0] + A[..., 3]


def total_variation(grids):
    """grids [V,12,L,GY,GX] -> scalar"""
    tv = 0
    for d in (2, 3, 4):
        diff = grids.narrow(d, 1, grids.shape[d] - 1) - grids.narrow(d, 0, grids.shape[d] - 1)
        tv = tv + (diff ** 2).sum() / max(diff[0].numel(), 1)
    return tv / grids.shape[0]


def identity(V, GX, GY, L, dtype=torch.float32):
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=dtype)
    return eye[None, :, None, None, None].expand(V, 12, L, GY, GX).contiguous()


def learning_rate(s, lr, warmup, max_steps):
    """the grid Adam's rate at the step with `s` earlier steps: the closed form of ChainedScheduler(LinearLR(0.01, warmup),
    ExponentialLR(0.01 ** (1 / max_steps)))"""
    return lr * (0.01 + 0.99 * min(s, warmup) / warmup) * (0.01 ** (s / max_steps))


def make_inputs(N, H, W, GX, GY, L, seed=0):
    """fp32 CPU inputs of one case -> (rgb [N,H,W,3], grids [N,12,L,GY,GX] in the reference layout, d_out [N,H,W,3]).  Grids are the
    identity plus 0.1 x normal noise; rgb is uniform in [0,1] with (from 8 pixels on) ~10 % exact black pixels, two exact white
    ones, one pixel at -0.2 and one at 1.3 in every channel (both clamps of the guidance axis) and one channel each at -0.2 and 1.3.
    Every pixel that is not clamped keeps gray (L-1) at least 1e-4 away from an integer: fp32 and fp64 stay on one side of the kink."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 5 * H + 3 * W + GX + GY + L)
    grids = identity(N, GX, GY, L) + 0.1 * torch.randn(N, 12, L, GY, GX, generator=g)
    rgb = torch.rand(N, H, W, 3, generator=g)
    d_out = torch.randn(N, H, W, 3, generator=g)
    flat = rgb.view(-1, 3)
    if flat.shape[0] >= 8:
        flat[torch.rand(flat.shape[0], generator=g) < 0.1] = 0.0
        flat[1], flat[-1] = 1.0, 1.0
        flat[2], flat[3] = -0.2, 1.3
        flat[4, 0], flat[5, 1] = -0.2, 1.3
    near = lambda: (lambda gz: (gz > 0) & (gz < L - 1) & ((gz - gz.round()).abs() < 1e-4))(guidance(rgb.double()) * (L - 1))
    rgb[..., 2][near()] += 0.01          # a drawn pixel within 1e-4 of a lattice plane is moved off it (blue: 0.114 x 0.01 x (L-1))
    gz = guidance(rgb.double()) * (L - 1)
    inside = (gz > 0) & (gz < L - 1)
    assert bool(((gz - gz.round()).abs()[inside] >= 1e-4).all()), "a pixel sits on a lattice plane of the guidance axis"
    return rgb, grids.contiguous(), d_out


def guidance(rgb):
    """gray of rgb [...,3] in rgb's dtype, with the float32 weights"""
    return (rgb @ torch.tensor(GRAY, dtype=torch.float32).to(rgb.dtype)[:, None])[..., 0]


def run(rgb, grids, d_out, dtype):
    """-> dict(out, d_rgb, d_grids, tv, d_tv) of the oracle in `dtype` (reference layout)"""
    r, gr = rgb.to(dtype).requires_grad_(True), grids.to(dtype).requires_grad_(True)
    out = slice_grid(r, gr)
    d_rgb, d_grids = torch.autograd.grad(out, (r, gr), d_out.to(dtype))
    tv = total_variation(gr)
    d_tv, = torch.autograd.grad(tv, gr)
    return dict(out=out.detach(), d_rgb=d_rgb, d_grids=d_grids, tv=tv.detach().reshape(1), d_tv=d_tv)


# (N, H, W), (GX, GY, L): the cases recorded from the reference (tests/golden/make_golden_bilagrid.py)
GOLDEN_CASES = (((1, 1, 1), (2, 2, 2)), ((1, 5, 7), (4, 3, 5)), ((2, 13, 37), (5, 3, 4)))
