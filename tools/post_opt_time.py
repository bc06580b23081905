"""One post-optimisation step (vist3a_amd/post_opt) at the sizes of tools/raster_bwd_time.py (448^2, 1M Gaussians, SH degree 4), one camera
per step as the loop runs it.  Prints one JSON line: milliseconds (median of --iters after --warmup) of the five parts of a step -
activation, render forward, loss, backward (loss + render + activation), Adam over the five tensors - and the Adam launch on the
harmonics against a `copy_` of the same bytes (28 B per element: p, m, v read and written, g read; the yardstick of tools/norm_time.py).
With --bilateral_grid the step runs as with cfg.use_bilateral_grid (21 views' grids of the default shape): the slice and the
total-variation launches are timed as a part of their own ("bilagrid": both forwards; their backwards fall into "backward", the
grid's Adam into "adam").
A second JSON line times the evaluation-time colour fit on one image pair of the same size (csrc/color_correct.hip, 5 rounds = 12
launches) next to the plain MSE (ops.image_mse, 2 launches): milliseconds, and the fit's bytes read per round (img + one channel
of ref per workgroup row, 3 x 16 B per pixel) over its time.  It runs outside the step: the loop never calls it.
With --mcmc a third JSON line times the MCMC strategy (csrc/mcmc.hip) on the same Gaussians: the per-step noise (ops.mcmc_noise, 44 B
read and 12 B written per Gaussian) against a `copy_` of the same 56 B per Gaussian, and one refine's pieces - the relocation sampler and
relocation with 10 % of the scene dead, the growth sampler for 5 % more rows and the growth itself (the reallocation of the fifteen
tensors is the caller's torch work and is not timed).
With --pose_opt a further JSON line times pose optimisation (cfg.pose_opt) on the same scene and camera: the whole step with the
camera adjusted through ops.camera_adjust and rendered with camera_grad=True (the deltas one more leaf, their Adam included), the
projection-backward call alone without and with camera gradients (the second is the plain kernel + the CAM kernel + the finish
kernel: the projection chain runs twice), and the two camera_adjust launches.  The kernels inside the camera-gradient call are
told apart with a kernel trace of this tool, not here.
With --densify a further JSON line times the densification strategy (csrc/densify.hip, cfg.strategy = "densify") on the same
Gaussians: the per-step accumulate launch (28 B per Gaussian and camera) and one refine's entry points - classify (three launches:
fates and block scans, block prefix, offsets), apply (two launches: the 11-float rows, the harmonics rows) with a third of the scene
above the gradient threshold, and the opacity reset; the bytes apply moves over its time.  With --absgrad also the rasteriser's
backward call without and with the absolute-gradient output (the ABS instantiations of its two kernels).
With --batch B and / or --visible_adam a further JSON line times the step as cfg.batch_size = B and cfg.visible_adam run it: B
cameras (the tool's camera turned by 0.05 rad each) in one render, loss and backward, then the visibility mask and the five Adam
launches (ops.adam_step_visible under --visible_adam): the Adam launches and the whole step, per step and per view.  It also times,
tensor by tensor and at that step's mask, ops.adam_step_visible against ops.adam_step, next to the visible fraction."""
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
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--antialiased", action="store_true", help="the loop's renders in the rasteriser's antialiased mode")
    ap.add_argument("--bilateral_grid", action="store_true")
    ap.add_argument("--mcmc", action="store_true", help="also time the MCMC strategy's noise launch and the pieces of one refine")
    ap.add_argument("--pose_opt", action="store_true", help="also time the step with pose optimisation and the camera-gradient launches")
    ap.add_argument("--reserve_gb", type=int, default=0, metavar="N",
                    help="first take one block of N GB from the driver and hand it to torch's cache, before the library is loaded: every "
                         "buffer is then carved from that block at the same relative place, so that two builds of the library can be "
                         "compared (the harmonics' Adam launch alone moves by 7 %% with where its four 720 MB buffers lie)")
    ap.add_argument("--densify", action="store_true", help="also time the densification strategy's accumulate launch and the pieces of one refine")
    ap.add_argument("--absgrad", action="store_true", help="with --densify: also the rasteriser's backward without and with absgrad")
    ap.add_argument("--batch", type=int, default=1, metavar="B", help="also time the step with B views per step (cfg.batch_size)")
    ap.add_argument("--visible_adam", action="store_true", help="also time the step with the visibility-masked Adam (cfg.visible_adam)")
    a = ap.parse_args()
    if a.reserve_gb > 0:
        block = torch.empty(a.reserve_gb << 30, dtype=torch.uint8, device="cuda")
        del block                                             # back into torch's caching allocator, not to the driver
    from vist3a_amd import ops
    U, W, H = a.gaussians, a.size, a.size
    g = torch.Generator().manual_seed(9)
    p = dict(means=torch.randn(U, 3, generator=g) * torch.tensor([2.0, 2.0, 1.0]) + torch.tensor([0.0, 0.0, 5.0]),
             scales=torch.log(0.005 + 0.03 * torch.rand(U, 3, generator=g)), quats=torch.randn(U, 4, generator=g),
             opacities=torch.randn(U, generator=g), sh=torch.randn(U, 3, 25, generator=g) * 0.3)
    p = {k: t.cuda().requires_grad_(True) for k, t in p.items()}
    m, v = {k: torch.zeros_like(t) for k, t in p.items()}, {k: torch.zeros_like(t) for k, t in p.items()}
    yaw = -0.15
    view = torch.eye(4)
    view[:3, :3] = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    view[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    campos = torch.linalg.inv(view)[:3, 3].contiguous().cuda()[None]
    view, K = view.cuda()[None], torch.tensor([[400.0, 0, W / 2], [0, 440.0, H / 2], [0, 0, 1.0]]).cuda()[None]
    target, bg, ws = torch.rand(1, H, W, 3, device="cuda"), torch.zeros(3, device="cuda"), ops.GsWorkspace()
    names = ("activation", "render_forward", "bilagrid", "loss", "backward", "adam")
    grids = ops.bilagrid_identity(21, 16, 16, 8, "cuda").requires_grad_(True) if a.bilateral_grid else None
    gm, gv = (torch.zeros_like(grids), torch.zeros_like(grids)) if a.bilateral_grid else (None, None)
    ms = {n: [] for n in names}
    for it in range(a.warmup + a.iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        e[0].record()
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        e[1].record()
        col, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view, campos, K, W, H, background=bg, clamp_rgb=True, workspace=ws,
                                  rasterize_mode="antialiased" if a.antialiased else "classic")
        e[2].record()
        tv = None
        if grids is not None:
            col, tv = ops.bilagrid_slice(col, grids[it % 21:it % 21 + 1]), ops.bilagrid_tv(grids)
        e[3].record()
        loss, _, _ = ops.photometric_loss(col, target, 0.2)
        if tv is not None:
            loss = loss + 10.0 * tv
        e[4].record()
        grads = torch.autograd.grad(loss, list(p.values()) + ([grids] if grids is not None else []))
        e[5].record()
        with torch.no_grad():
            for (k, t), gr in zip(p.items(), grads):
                ops.adam_step(t, gr, m[k], v[k], lr=1e-3, step=it + 1, eps=1e-15, lr2=5e-5 if k == "sh" else None, period=25 if k == "sh" else 0)
            if grids is not None:
                ops.adam_step(grids, grads[-1].contiguous(), gm, gv, lr=2e-3, step=it + 1, eps=1e-15)
        e[6].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            for i, n in enumerate(names):
                ms[n].append(e[i].elapsed_time(e[i + 1]))
    med = {n: statistics.median(x) for n, x in ms.items()}
    # the Adam launch on the harmonics alone against a copy of the same bytes
    sh, gr = p["sh"].detach(), torch.randn(U, 3, 25, device="cuda")
    src, dst = torch.empty(sh.numel() * 7 // 2, device="cuda"), torch.empty(sh.numel() * 7 // 2, device="cuda")   # 14 B read + 14 B written per element
    ta, tc = [], []
    for it in range(a.warmup + a.iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        ops.adam_step(sh, gr, m["sh"], v["sh"], lr=1e-3, lr2=5e-5, period=25, step=it + 1, eps=1e-15)
        e[1].record()
        dst.copy_(src)
        e[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            ta.append(e[0].elapsed_time(e[1]))
            tc.append(e[1].elapsed_time(e[2]))
    nbytes = sh.numel() * 28
    a_ms, c_ms = statistics.median(ta), statistics.median(tc)
    print(json.dumps(dict(gaussians=U, size=W, bilateral_grid=bool(a.bilateral_grid), step_ms=round(sum(med.values()), 3), **{n + "_ms": round(x, 3) for n, x in med.items()},
                          adam_sh_elements=sh.numel(), adam_sh_ms=round(a_ms, 3), adam_sh_GBps=round(nbytes / a_ms / 1e6, 1),
                          copy_same_bytes_ms=round(c_ms, 3), copy_GBps=round(nbytes / c_ms / 1e6, 1), adam_over_copy=round(a_ms / c_ms, 2))))
    # the evaluation-time colour fit and the plain MSE on one image pair
    img = (target * 0.85 + 0.05).contiguous()
    tf, tm = [], []
    for it in range(a.warmup + a.iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        ops.color_correct(img, target)
        e[1].record()
        ops.image_mse(img, target)
        e[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            tf.append(e[0].elapsed_time(e[1]))
            tm.append(e[1].elapsed_time(e[2]))
    f_ms, m_ms = statistics.median(tf), statistics.median(tm)
    print(json.dumps(dict(size=W, color_correct_iters=5, color_correct_ms=round(f_ms, 3), color_correct_ms_per_round=round(f_ms / 5, 3),
                          color_correct_read_GBps=round(5 * 48 * W * H / f_ms / 1e6, 1), image_mse_ms=round(m_ms, 3))))
    if a.mcmc:
        print(json.dumps(mcmc_times(ops, {k: t.detach() for k, t in p.items()}, m, v, a.warmup, a.iters)))
    if a.densify:
        print(json.dumps(densify_times(ops, {k: t.detach() for k, t in p.items()}, m, v, view, campos, K, bg, ws, W, H, a.absgrad, a.warmup, a.iters)))
    if a.batch > 1 or a.visible_adam:
        print(json.dumps(batch_times(ops, p, m, v, K, bg, ws, W, H, a.batch, a.visible_adam, a.warmup, a.iters)))
    if a.pose_opt:
        print(json.dumps(pose_times(ops, p, view, K, target, bg, ws, W, H, "antialiased" if a.antialiased else "classic", a.warmup, a.iters)))


def densify_times(ops, p, m, v, view, campos, K, bg, ws, W, H, absgrad, warmup, iters):
    U = p["means"].shape[0]
    timed = {}

    def clock(name, fn):
        ms = []
        for it in range(warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(it)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms.append(e0.elapsed_time(e1))
        timed[name] = statistics.median(ms)
        return out

    with torch.no_grad():
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        pr = ops.gs_project(p["means"], cov, p["sh"], view, campos, K, W, H)
        r = ops.gs_rasterize(pr, op, W, H, background=bg, workspace=ws, return_order=True)
        back = lambda on: ops.gs_rasterize_backward(pr, op, W, H, r["tile_offsets"], r["flatten_ids"].contiguous(), d_color, zero, zero,
                                                    background=bg, absgrad=on)
        d_color, zero = torch.rand(1, H, W, 3, device="cuda"), torch.zeros(1, H, W, device="cuda")
        eg = back(True)
        if absgrad:
            clock("rasterize_backward", lambda it: back(False))
            clock("rasterize_backward_absgrad", lambda it: back(True))
        grad2d, count = torch.zeros(U, device="cuda"), torch.zeros(U, device="cuda", dtype=torch.int32)
        d2 = eg["d_means2d_abs" if absgrad else "d_means2d"]
        clock("accumulate", lambda it: ops.densify_accumulate(grad2d, count, d2, pr["radii"], W, H))
        avg = grad2d / count.clamp(min=1)
        thr = float(avg[count > 0].float().quantile(2.0 / 3.0)) if U <= 16_000_000 else float(avg.mean())
        kw = dict(grow_grad2d=thr, grow_scale3d=0.02, prune_opa=0.005, prune_scale3d=0.1, prune_big=True)
        cls = clock("classify", lambda it: ops.densify_classify(grad2d, count, p["scales"], p["opacities"], **kw))
        totals = cls["totals"].tolist()
        new = clock("apply", lambda it: ops.densify_apply(cls, p, m, v, seed=1, step=it + 1, totals=totals))
        lg, lm, lv = p["opacities"].clone(), m["opacities"].clone(), v["opacities"].clone()
        clock("reset_opacity", lambda it: ops.densify_reset_opacity(lg, lm, lv, 0.01))
    U_out = new[0]["means"].shape[0]
    row = 4 * (11 + 3 * p["sh"].shape[-1])                       # bytes of one row of the five parameter tensors
    # written: params, m and v of every new row; read: params, m and v of an original, the params alone for a clone or a child
    moved = 3 * row * U_out + row * (3 * totals[0] + totals[1] + 2 * totals[2])
    return dict(gaussians=U, size=W, visible=int((pr["radii"] > 0).sum()), absgrad=bool(absgrad), grow_grad2d=thr,
                kept_cloned_split=totals, rows_after=U_out, accumulate_bytes=28 * U, accumulate_GBps=round(28 * U / timed["accumulate"] / 1e6, 1),
                apply_bytes=moved, apply_GBps=round(moved / timed["apply"] / 1e6, 1), **{k + "_ms": round(x, 4) for k, x in timed.items()})


def batch_times(ops, p, m, v, K, bg, ws, W, H, B, visible_adam, warmup, iters):
    U = p["means"].shape[0]
    views = []
    for b in range(B):
        yaw = -0.15 + 0.05 * b
        vm = torch.eye(4)
        vm[:3, :3] = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
        vm[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
        views.append(vm)
    view = torch.stack(views)
    campos = torch.linalg.inv(view)[:, :3, 3].contiguous().cuda()
    view, Kb = view.cuda(), K.expand(B, 3, 3).contiguous()
    target = torch.rand(B, H, W, 3, device="cuda")
    r = math.sqrt(B)
    betas, eps = (1 - B * 0.1, 1 - B * 0.001), 1e-15 / r
    adam_ms, step_ms = [], []
    for it in range(warmup + iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        info = {}
        col, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view, campos, Kb, W, H, background=bg, clamp_rgb=True, workspace=ws,
                                  info_out=info if visible_adam else None)
        loss, _, _ = ops.photometric_loss(col, target, 0.2)
        grads = torch.autograd.grad(loss, list(p.values()))
        e[1].record()
        with torch.no_grad():
            if visible_adam:
                visible = ops.gs_visibility(info["radii"])
            for (k, t), gr in zip(p.items(), grads):
                two = dict(lr2=5e-5 * r, period=25) if k == "sh" else {}
                if visible_adam:
                    ops.adam_step_visible(t, gr, m[k], v[k], visible, lr=1e-3 * r, betas=betas, eps=eps, **two)
                else:
                    ops.adam_step(t, gr, m[k], v[k], lr=1e-3 * r, step=it + 1, betas=betas, eps=eps, **two)
        e[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            adam_ms.append(e[1].elapsed_time(e[2]))
            step_ms.append(e[0].elapsed_time(e[2]))
    a_ms, s_ms = statistics.median(adam_ms), statistics.median(step_ms)
    # tensor by tensor at this batch's mask: the masked launch against the dense one
    with torch.no_grad():
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        visible = ops.gs_visibility(ops.gs_project(p["means"].detach(), cov, p["sh"].detach(), view, campos, Kb, W, H)["radii"])
        ratios = {}
        for k, t in p.items():
            t, gr = t.detach().clone(), torch.randn_like(t)
            two = dict(lr2=5e-5, period=25) if k == "sh" else {}
            td, tv = [], []
            for it in range(warmup + iters):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                ops.adam_step(t, gr, m[k], v[k], lr=1e-3, step=it + 1, eps=1e-15, **two)
                e[1].record()
                ops.adam_step_visible(t, gr, m[k], v[k], visible, lr=1e-3, eps=1e-15, **two)
                e[2].record()
                torch.cuda.synchronize()
                if it >= warmup:
                    td.append(e[0].elapsed_time(e[1]))
                    tv.append(e[1].elapsed_time(e[2]))
            d_ms, v_ms = statistics.median(td), statistics.median(tv)
            ratios[k] = dict(row_bytes=4 * t.numel() // U, adam_ms=round(d_ms, 4), adam_visible_ms=round(v_ms, 4), visible_over_dense=round(v_ms / d_ms, 3))
    return dict(gaussians=U, size=W, batch=B, visible_adam=bool(visible_adam), visible_fraction=round(float(visible.float().mean()), 4),
                adam_ms_per_step=round(a_ms, 3), adam_ms_per_view=round(a_ms / B, 3), step_ms_per_step=round(s_ms, 3),
                step_ms_per_view=round(s_ms / B, 3), per_tensor=ratios)


def pose_times(ops, p, view, K, target, bg, ws, W, H, mode, warmup, iters):
    U = p["means"].shape[0]
    w2c = view.contiguous()
    c2w = torch.linalg.inv(view.cpu()).contiguous().cuda()
    deltas = (torch.randn(1, 9, generator=torch.Generator().manual_seed(3)) * 1e-3).cuda().requires_grad_(True)
    dm, dv = torch.zeros_like(deltas), torch.zeros_like(deltas)
    timed = {}

    def clock(name, fn):
        ms = []
        for it in range(warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(it)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms.append(e0.elapsed_time(e1))
        timed[name] = statistics.median(ms)
        return out

    def step(it):   # forward + backward of a pose-optimising step, and the deltas' Adam (the splat tensors' Adam is the plain step's)
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        v_, c_ = ops.camera_adjust(w2c, c2w, deltas)
        col, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, v_, c_, K, W, H, background=bg, clamp_rgb=True, workspace=ws,
                                  rasterize_mode=mode, camera_grad=True)
        loss, _, _ = ops.photometric_loss(col, target, 0.2)
        grads = torch.autograd.grad(loss, list(p.values()) + [deltas])
        with torch.no_grad():
            ops.adam_step(deltas, (grads[-1] + 1e-6 * deltas).contiguous(), dm, dv, lr=1e-5, step=it + 1, eps=1e-8)

    def step_plain(it):   # the same without pose optimisation and without the splat tensors' Adam: the difference is what pose_opt adds
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        col, _, _ = ops.gs_render(p["means"], cov, p["sh"], op, view, campos_of(view), K, W, H, background=bg, clamp_rgb=True, workspace=ws,
                                  rasterize_mode=mode)
        loss, _, _ = ops.photometric_loss(col, target, 0.2)
        torch.autograd.grad(loss, list(p.values()))

    campos0 = c2w[:, :3, 3].contiguous()
    campos_of = lambda _: campos0
    clock("step_pose_fwd_bwd", step)
    clock("step_plain_fwd_bwd", step_plain)
    with torch.no_grad():
        cov, op = ops.splat_activate(p["scales"], p["quats"], p["opacities"])
        means, sh = p["means"].detach(), p["sh"].detach()
        pr = ops.gs_project(means, cov, sh, view, campos0, K, W, H, rasterize_mode=mode)
        r = ops.gs_rasterize(pr, op, W, H, background=bg, workspace=ws, return_order=True)
        eg = ops.gs_rasterize_backward(pr, op, W, H, r["tile_offsets"], r["flatten_ids"].contiguous(), torch.rand(1, H, W, 3, device="cuda"),
                                       torch.zeros(1, H, W, device="cuda"), torch.zeros(1, H, W, device="cuda"), background=bg)
        aa = dict(rasterize_mode=mode, opacities=op if mode == "antialiased" else None)
        clock("project_backward", lambda it: ops.gs_project_backward(means, cov, sh, view, campos0, K, W, H, pr["radii"], eg, **aa))
        clock("project_backward_cam", lambda it: ops.gs_project_backward(means, cov, sh, view, campos0, K, W, H, pr["radii"], eg,
                                                                         camera_grad=True, **aa))
        d = deltas.detach()
        clock("camera_adjust", lambda it: ops.camera_adjust(w2c, c2w, d))
        lib, p_ = ops.L.load(), ops._ptr
        gv, gc, gd = torch.rand(1, 4, 4, device="cuda"), torch.rand(1, 3, device="cuda"), torch.empty(1, 9, device="cuda")
        clock("camera_adjust_backward", lambda it: lib.v3a_camera_adjust_backward(p_(w2c), p_(c2w), p_(d), p_(gv), p_(gc), 1, p_(gd), ops._stream()))
    return dict(gaussians=U, size=W, visible=int((pr["radii"] > 0).sum()), cam_workspace_bytes=120 * ((U + 63) // 64),
                **{k + "_ms": round(x, 4) for k, x in timed.items()},
                cam_over_plain=round(timed["project_backward_cam"] / timed["project_backward"], 2))


def mcmc_times(ops, p, m, v, warmup, iters):
    U = p["means"].shape[0]
    timed = {}

    def clock(name, fn, setup=None):
        ms = []
        for it in range(warmup + iters):
            state = setup() if setup is not None else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(it, state)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms.append(e0.elapsed_time(e1))
        timed[name] = statistics.median(ms)
        return out

    with torch.no_grad():
        logits = p["opacities"].clone()
        logits[::10] = -7.0                                    # 10 % of the scene dead (opacity 0.0009), and with an open noise gate
        means = p["means"].clone()
        clock("noise", lambda it, _: ops.mcmc_noise(means, p["scales"], p["quats"], logits, scaler=80.0, seed=1, step=it + 1))
        src_b, dst_b = torch.empty(U * 7, device="cuda"), torch.empty(U * 7, device="cuda")      # 28 B read + 28 B written per Gaussian
        clock("copy_same_bytes", lambda it, _: dst_b.copy_(src_b))
        _, op = ops.splat_activate(p["scales"], p["quats"], logits)
        src, counts = clock("relocate_sample", lambda it, _: ops.mcmc_sample(op, min_weight=0.005, alive_only=True, n_slots=U, seed=1, stream=0, step=it + 1))
        fresh = lambda: [dict(p, opacities=logits.clone(), scales=p["scales"].clone()), m, v]
        clock("relocate", lambda it, st: ops.mcmc_relocate(src, counts, *st, dst_offset=0, min_opacity=0.005), setup=fresh)
        n = U // 20
        gsrc, gcounts = clock("grow_sample", lambda it, _: ops.mcmc_sample(op, min_weight=0.005, alive_only=False, n_slots=n, seed=1, stream=1, step=it + 1))
        longer = lambda d: {k: torch.cat([t.detach(), torch.zeros((n,) + tuple(t.shape[1:]), device="cuda")]) for k, t in d.items()}
        grown = [longer(dict(p, opacities=logits)), longer(m), longer(v)]
        clock("grow", lambda it, _: ops.mcmc_relocate(gsrc, gcounts, *grown, dst_offset=U, min_opacity=0.005))
    nbytes = U * 56
    return dict(gaussians=U, mcmc_noise_ms=round(timed["noise"], 4), mcmc_noise_GBps=round(nbytes / timed["noise"] / 1e6, 1),
                noise_bytes=nbytes, copy_same_bytes_ms=round(timed["copy_same_bytes"], 4),
                noise_over_copy=round(timed["noise"] / timed["copy_same_bytes"], 2), dead=int(U // 10 + (U % 10 > 0)), added=n,
                **{k + "_ms": round(timed[k], 4) for k in ("relocate_sample", "relocate", "grow_sample", "grow")})


if __name__ == "__main__":
    main()
