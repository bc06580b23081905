"""The depth term of the reference's post-optimisation loop in plain torch, any dtype (fp64 is the yardstick, fp32 the comparison
figure), written the reference's way (third_party_model/anysplat/src/post_opt/simple_trainer.py:943-961): the expected depth
(gsplat's "ED": depth / alpha.clamp(min=1e-10)) is sampled with F.grid_sample(align_corners=True) at `points`, turned into a
disparity with where(d > 0, 1 / d, 0), and compared by L1 with 1 / depths_gt, times scene_scale.

Here `points` are the integer pixel coordinates of the used pixels of each camera (mask set, target positive and finite), and
the per-camera sums are divided by the total count, which is what csrc/depth_loss.hip computes on dense maps.  An empty selection
gives 0 (the reference's empty mean is NaN).

One thing is added to the reference's lines.  Its normalisation x / (W - 1) * 2 - 1 and grid_sample's inverse ((g + 1) / 2) * (W - 1)
do not round-trip exactly in binary floating point unless W - 1 is a power of two: at 45 x 70 an integer pixel comes back up to
7e-15 (fp64) or 3.6e-6 (fp32) away from itself and picks up that much of its neighbour.  `sample` therefore zero-pads the map on
the right and at the bottom to 2^k + 1 pixels per axis and normalises with the padded size: every step is then exact, an integer
point returns its pixel bit for bit (tests/test_depth_loss_host.py), the pad is never touched, and an axis of one pixel needs
no special case (the reference's formula is 0 / 0 there).

Where the sampled depth is exactly 0 the reference's own backward is NaN (0 * inf through the unselected branch of torch.where);
the restatement takes the selected branch's gradient, 0.

The reference's lines sit inline in train() and cannot be executed on their own: this is a RESTATEMENT of them, not a golden
vector produced by running the reference."""
import torch
import torch.nn.functional as F


def used_pixels(depth_gt, mask=None):
    u = (depth_gt > 0) & torch.isfinite(depth_gt)
    return u if mask is None else u & mask.bool()


def expected_depth(depth, alpha):
    return depth / alpha.clamp(min=1e-10)


def _padded(size):
    k = 1
    while k + 1 < size:
        k *= 2
    return k + 1


def sample(ed, points):
    """ed [H,W], points [M,2] (x, y) in pixels -> [M], as simple_trainer.py:945-956 on the map padded to 2^k + 1 per axis"""
    H, W = ed.shape
    height, width = _padded(H), _padded(W)
    ed = F.pad(ed, (0, width - W, 0, height - H))
    points = torch.stack([points[:, 0] / (width - 1) * 2 - 1, points[:, 1] / (height - 1) * 2 - 1], dim=-1)   # normalize to [-1, 1]
    grid = points[None].unsqueeze(2)   # [1, M, 1, 2]
    depths = F.grid_sample(ed[None, None], grid, align_corners=True)   # [1, 1, M, 1]
    return depths.squeeze(3).squeeze(1)[0]


def depth_loss(depth, alpha, depth_gt, mask=None, scale=1.0):
    """depth, alpha, depth_gt [C,H,W] of one floating dtype, mask bool / uint8 [C,H,W] or None -> (loss, count)"""
    used = used_pixels(depth_gt, mask)
    ed = expected_depth(depth, alpha)
    total, count = (ed * 0).sum(), 0
    for c in range(depth.shape[0]):
        ys, xs = torch.nonzero(used[c], as_tuple=True)
        if len(ys) == 0:
            continue
        points = torch.stack([xs, ys], -1).to(depth.dtype)
        d = sample(ed[c], points)
        # the reference's where(d > 0, 1 / d, 0) with a safe denominator: where d == 0 exactly (a pixel no Gaussian reaches) autograd
        # through the unselected 1 / d gives 0 * inf = NaN; the gradient of the selected constant branch is 0, and so is the kernel's
        disp = torch.where(d > 0.0, 1.0 / torch.where(d > 0.0, d, torch.ones_like(d)), torch.zeros_like(d))
        disp_gt = 1.0 / depth_gt[c][ys, xs]
        total = total + (disp - disp_gt).abs().sum()
        count += len(ys)
    return (total / count * scale if count else total), count
