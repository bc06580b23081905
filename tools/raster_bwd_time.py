"""Forward and backward time of the 3DGS rasteriser at the production shape of tests/test_raster_gpu.py::test_full_size_properties
(448^2, 1M Gaussians, 12 cameras per launch).  Prints one JSON line: milliseconds (median of --iters runs after --warmup), n_isect,
the backward's row-buffer bytes, and for both directions a byte model and an upper bound of the exponentials per second.

  bytes model   forward : per intersection 8 B key + 4 B id through the sort, 4 B id + 44 B gathered Gaussian at the blend; per
                          entry 44 B of projection output; per pixel 20 B out.
                backward: the forward's blend reads twice (re-walk + back-to-front), one 48 B row written and read per
                          intersection, 40 B of entry gradients written and read, 20 B of pixel gradients read, per Gaussian
                          (48 + 300) B in and the same out at the projection.
  v_exp bound   256 lanes x tile list length, without the early exit (forward: once; backward: twice)."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, default=12)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rasterize_mode", choices=("classic", "antialiased"), default="classic")
    a = ap.parse_args()
    from vist3a_amd import ops
    U, Cn, W, H = a.gaussians, a.cameras, a.size, a.size
    g = torch.Generator().manual_seed(9)
    means = torch.randn(U, 3, generator=g) * torch.tensor([2.0, 2.0, 1.0]) + torch.tensor([0.0, 0.0, 5.0])
    A = torch.randn(U, 3, 3, generator=g) * 0.02
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)
    sh = torch.randn(U, 3, 25, generator=g) * 0.3
    op = torch.rand(U, generator=g)
    views, Ks = [], []
    for i in range(Cn):
        yaw = 0.03 * i - 0.15
        v = torch.eye(4)
        v[:3, :3] = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
        v[:3, 3] = torch.tensor([0.1 + 0.02 * i, -0.2, 0.3 + 0.05 * i])
        views.append(v)
        Ks.append(torch.tensor([[400.0, 0, W / 2], [0, 440.0, H / 2], [0, 0, 1.0]]))
    view, K = torch.stack(views).cuda(), torch.stack(Ks).cuda()
    campos = torch.stack([torch.linalg.inv(v)[:3, 3] for v in views]).contiguous().cuda()
    lv = [t.cuda().requires_grad_(True) for t in (means, cov, sh, op)]
    bg = torch.ones(3, device="cuda")
    ws, n_is = ops.GsWorkspace(), []
    wc, wd, wa = torch.randn(Cn, H, W, 3, device="cuda"), torch.randn(Cn, H, W, device="cuda"), torch.randn(Cn, H, W, device="cuda")
    fwd, bwd = [], []
    for it in range(a.warmup + a.iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        col, dep, alp = ops.gs_render(*lv, view, campos, K, W, H, background=bg, clamp_rgb=True, workspace=ws, n_isect_out=n_is,
                                      rasterize_mode=a.rasterize_mode)
        e[1].record()
        torch.autograd.backward([col, dep, alp], [wc, wd, wa])
        e[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
        for t in lv:
            t.grad = None
    n, f_ms, b_ms = n_is[-1], statistics.median(fwd), statistics.median(bwd)
    px = Cn * H * W
    f_bytes = n * (12 + 48) + Cn * U * 44 + U * 348 + px * 20
    b_bytes = n * (2 * 48 + 2 * 48) + Cn * U * (2 * 40 + 44 + 8) + px * 20 + 2 * U * 348
    print(json.dumps(dict(gaussians=U, cameras=Cn, size=W, rasterize_mode=a.rasterize_mode, n_isect=n, forward_ms=round(f_ms, 3), backward_ms=round(b_ms, 3),
                          backward_over_forward=round(b_ms / f_ms, 2), row_buffer_bytes=48 * n,
                          forward_model_GBps=round(f_bytes / f_ms / 1e6, 1), backward_model_GBps=round(b_bytes / b_ms / 1e6, 1),
                          forward_vexp_bound_per_s=round(256 * n / (f_ms * 1e-3), -6),
                          backward_vexp_bound_per_s=round(2 * 256 * n / (b_ms * 1e-3), -6))))


if __name__ == "__main__":
    main()
