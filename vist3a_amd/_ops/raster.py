"""The 3DGS rasteriser and its backward passes (csrc/raster.hip, csrc/raster_bwd.hip) and the pose parametrisation (csrc/post_opt.hip)."""
import ctypes as C
from typing import Optional

import torch

from .. import lib as L
from .common import _f32_dev, _i32_dev, _ptr, _stream, _workspace, f32


# ------------------------------------------------------------------------------------------------ 3DGS rasteriser
def _gs_scene_args(means, covars, sh, viewmat, campos, K, sh_layout):
    """What gs_project and gs_project_backward check of their tensors -> (cameras, Gaussians, sh_k)."""
    for t, n in ((means, "means"), (covars, "covars"), (sh, "sh"), (viewmat, "viewmat"), (campos, "campos"), (K, "K")):
        _f32_dev(t, n)
    Cn = 1 if viewmat.dim() == 2 else viewmat.shape[0]
    if campos.numel() != 3 * Cn or K.numel() != 9 * Cn or viewmat.numel() != 16 * Cn:
        raise ValueError("viewmat / campos / K disagree on the number of cameras")
    return Cn, means.shape[0], sh.shape[2] if sh_layout == 1 else sh.shape[1]


RASTERIZE_MODES = {"classic": 0, "antialiased": 1}   # gsplat's rasterize_mode -> the C ABI's


def _gs_mode(rasterize_mode: str) -> int:
    if rasterize_mode not in RASTERIZE_MODES:
        raise ValueError(f"rasterize_mode must be one of {sorted(RASTERIZE_MODES)}, got {rasterize_mode!r}")
    return RASTERIZE_MODES[rasterize_mode]


def gs_project(means: torch.Tensor, covars: torch.Tensor, sh: torch.Tensor, viewmat: torch.Tensor, campos: torch.Tensor,
               K: torch.Tensor, width: int, height: int, *, sh_degree: int = 4, sh_layout: int = 1, near_plane: float = 1e-10,
               far_plane: float = 1e10, radius_clip: float = 0.1, eps2d: float = 0.3, rasterize_mode: str = "classic"):
    """fully_fused_projection + SH colours for C cameras at once (viewmat [C,4,4], campos [C,3], K [C,3,3] -> outputs [C,U,...])
    or one camera (viewmat [4,4] -> outputs [U,...]).  sh: [U,3,K] (sh_layout=1, Gaussians.harmonics) or [U,K,3] (0).
    rasterize_mode="antialiased" adds `compensations` [C,U] to the dict (gs_rasterize and gs_rasterize_backward pick it up from
    there): each entry's opacity factor sqrt(det(cov2d) / det(cov2d + eps2d I)); every other output is the classic one."""
    mode = _gs_mode(rasterize_mode)
    Cn, U, sh_k = _gs_scene_args(means, covars, sh, viewmat, campos, K, sh_layout)
    dev = means.device
    lead = () if viewmat.dim() == 2 else (Cn,)
    radii = torch.empty(*lead, U, device=dev, dtype=torch.int32)
    e = lambda *s: torch.empty(*lead, *s, device=dev, dtype=f32)
    m2, dep, con, col = e(U, 2), e(U), e(U, 3), e(U, 4)
    comp = e(U) if mode else None
    a = L.GsProjectArgs(_ptr(means), _ptr(covars), _ptr(sh), sh_layout, sh_k, sh_degree, _ptr(viewmat), _ptr(campos), _ptr(K), U, Cn,
                        width, height, near_plane, far_plane, radius_clip, eps2d, _ptr(radii), _ptr(m2), _ptr(dep), _ptr(con), _ptr(col),
                        mode, _ptr(comp))
    L.check(L.load().v3a_gs_project(C.byref(a), _stream()), "v3a_gs_project")
    out = dict(radii=radii, means2d=m2, depths=dep, conics=con, colors=col)
    if mode:
        out["compensations"] = comp
    return out


class _GsScratch:
    """Grow-only device scratch sized by one of the library's workspace queries, shared by the camera batches of one video."""
    query, min_cap = "", 0

    def __init__(self):
        self.buf, self.cap, self.key = None, 0, None

    def get(self, U, Cn, width, height, need):
        key = (U, Cn, width, height)
        if self.buf is None or self.key != key or need > self.cap:
            self.cap = max(int(need * 1.25), self.min_cap)
            nbytes = getattr(L.load(), self.query)(U, Cn, width, height, self.cap)
            if nbytes < 0:
                L.check(int(nbytes), self.query)
            self.buf, self.key = None, key
            self.buf = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        return self.buf


class GsWorkspace(_GsScratch):
    """Scratch for v3a_gs_rasterize."""
    query, min_cap = "v3a_gs_rasterize_workspace_bytes", 1 << 20

    def __init__(self):
        super().__init__()
        self.bwd = None  # GsBwdWorkspace, created by the first gs_render backward that is handed this workspace


def gs_rasterize(proj: dict, opacities: torch.Tensor, width: int, height: int, *, background: Optional[torch.Tensor] = None,
                 clamp_rgb: bool = True, workspace: Optional[GsWorkspace] = None, return_order: bool = False):
    """isect_tiles + sort + rasterize_to_pixels for the cameras of `proj` -> dict(color [C,H,W,3], depth [C,H,W], alpha [C,H,W],
    n_isect); without the C axis when `proj` came from a single-camera gs_project call.  A `proj` of the antialiased mode carries
    its compensations: entry (c, g) then draws with opacities[g] * compensations[c, g]."""
    U, dev = opacities.shape[0], opacities.device
    _f32_dev(opacities, "opacities", numel=U)
    if U == 0:
        raise ValueError("no Gaussians to draw")
    single = proj["radii"].dim() == 1
    Cn = 1 if single else proj["radii"].shape[0]
    lead = () if single else (Cn,)
    comp = proj.get("compensations")
    if comp is not None:
        _f32_dev(comp, "compensations", numel=Cn * U)
    wsp = workspace or GsWorkspace()
    color = torch.empty(*lead, height, width, 3, device=dev, dtype=f32)
    depth = torch.empty(*lead, height, width, device=dev, dtype=f32)
    alpha = torch.empty(*lead, height, width, device=dev, dtype=f32)
    ntiles = ((width + 15) // 16) * ((height + 15) // 16)
    n_host = C.c_long(0)
    need = max(wsp.cap, 1)
    for _ in range(2):
        buf = wsp.get(U, Cn, width, height, need)
        offs = torch.empty(Cn * ntiles + 1, device=dev, dtype=torch.int32) if return_order else None
        ids = torch.empty(wsp.cap, device=dev, dtype=torch.int32) if return_order else None
        a = L.GsRasterizeArgs(_ptr(proj["radii"]), _ptr(proj["means2d"]), _ptr(proj["depths"]), _ptr(proj["conics"]), _ptr(proj["colors"]),
                              _ptr(opacities), _ptr(background) if background is not None else None, U, Cn, width, height, int(clamp_rgb),
                              _ptr(color), _ptr(depth), _ptr(alpha), _ptr(buf), buf.numel(), wsp.cap, C.pointer(n_host),
                              _ptr(offs) if return_order else None, _ptr(ids) if return_order else None, _ptr(comp))
        rc = L.load().v3a_gs_rasterize(C.byref(a), _stream())
        if rc == -4:  # V3A_ERR_WORKSPACE: the count is known now, grow once and redo
            need = n_host.value
            continue
        L.check(rc, "v3a_gs_rasterize")
        break
    else:
        raise RuntimeError("v3a_gs_rasterize: workspace still too small after growing")
    out = dict(color=color, depth=depth, alpha=alpha, n_isect=int(n_host.value))
    if return_order:
        out["tile_offsets"], out["flatten_ids"] = offs, ids[: n_host.value]
    return out


class GsBwdWorkspace(_GsScratch):
    """Scratch for v3a_gs_rasterize_backward: two counters per camera-Gaussian entry and one 48-byte row per intersection (the
    price of summing without atomics: every (Gaussian, tile) contribution is stored once, then added in order)."""
    query, min_cap = "v3a_gs_rasterize_backward_workspace_bytes", 1 << 16



def gs_rasterize_backward(proj: dict, opacities: torch.Tensor, width: int, height: int, tile_offsets: torch.Tensor,
                          flatten_ids: torch.Tensor, d_color: torch.Tensor, d_depth: torch.Tensor, d_alpha: torch.Tensor, *,
                          background: Optional[torch.Tensor] = None, clamp_rgb: bool = True,
                          workspace: Optional[GsBwdWorkspace] = None, absgrad: bool = False):
    """Backward of gs_rasterize: `proj` and (tile_offsets, flatten_ids) as the forward had / returned them (return_order=True),
    d_color [C,H,W,3], d_depth, d_alpha [C,H,W] -> dict(d_means2d [C,U,2], d_conics [C,U,3], d_colors [C,U,4], d_opacity [C,U])
    per camera-Gaussian entry; without the C axis when `proj` came from a single-camera gs_project call.  With compensations in
    `proj` (antialiased mode) d_opacity is the gradient with respect to the entry's opacities[g] * compensations[c, g].
    absgrad=True adds d_means2d_abs [C,U,2], the sum over pixels of the absolute per-pixel terms of d_means2d (gsplat's absgrad,
    what the densification strategy may read); the other four are the same bits either way."""
    U, dev = opacities.shape[0], opacities.device
    if U == 0:
        raise ValueError("no Gaussians to draw")
    single = proj["radii"].dim() == 1
    Cn = 1 if single else proj["radii"].shape[0]
    lead = () if single else (Cn,)
    ntiles = ((width + 15) // 16) * ((height + 15) // 16)
    _f32_dev(opacities, "opacities", numel=U)
    for k, n in (("means2d", 2), ("conics", 3), ("colors", 4)):
        _f32_dev(proj[k], k, numel=Cn * U * n)
    _i32_dev(proj["radii"], "radii", numel=Cn * U)
    _f32_dev(d_color, "d_color", numel=Cn * height * width * 3)
    _f32_dev(d_depth, "d_depth", numel=Cn * height * width)
    _f32_dev(d_alpha, "d_alpha", numel=Cn * height * width)
    if background is not None:
        _f32_dev(background, "background", numel=3)
    comp = proj.get("compensations")
    if comp is not None:
        _f32_dev(comp, "compensations", numel=Cn * U)
    _i32_dev(tile_offsets, "tile_offsets", numel=Cn * ntiles + 1)
    _i32_dev(flatten_ids, "flatten_ids")
    n_isect = flatten_ids.numel()
    wsp = workspace or GsBwdWorkspace()
    buf = wsp.get(U, Cn, width, height, max(n_isect, 1))
    e = lambda *s: torch.empty(*lead, *s, device=dev, dtype=f32)
    dm2, dcon, dcol, dop = e(U, 2), e(U, 3), e(U, 4), e(U)
    dabs = e(U, 2) if absgrad else None
    a = L.GsRasterizeBackwardArgs(_ptr(proj["radii"]), _ptr(proj["means2d"]), _ptr(proj["conics"]), _ptr(proj["colors"]), _ptr(opacities),
                                  _ptr(background) if background is not None else None, U, Cn, width, height, int(clamp_rgb),
                                  _ptr(tile_offsets), _ptr(flatten_ids) if n_isect else None, n_isect, _ptr(d_color), _ptr(d_depth),
                                  _ptr(d_alpha), _ptr(dm2), _ptr(dcon), _ptr(dcol), _ptr(dop), _ptr(buf), buf.numel(), _ptr(comp), _ptr(dabs))
    L.check(L.load().v3a_gs_rasterize_backward(C.byref(a), _stream()), "v3a_gs_rasterize_backward")
    out = dict(d_means2d=dm2, d_conics=dcon, d_colors=dcol, d_opacity=dop)
    if absgrad:
        out["d_means2d_abs"] = dabs
    return out


def gs_project_backward(means: torch.Tensor, covars: torch.Tensor, sh: torch.Tensor, viewmat: torch.Tensor, campos: torch.Tensor,
                        K: torch.Tensor, width: int, height: int, radii: torch.Tensor, entry_grads: dict, *, sh_degree: int = 4,
                        sh_layout: int = 1, eps2d: float = 0.3, rasterize_mode: str = "classic",
                        opacities: Optional[torch.Tensor] = None, camera_grad: bool = False):
    """Backward of gs_project: the entry gradients of gs_rasterize_backward (or any dict with d_means2d, d_conics, d_colors,
    d_opacity) -> (d_means [U,3], d_covars [U,3,3], d_sh like sh, d_opacities [U]), summed over the cameras in index order.
    Cameras are constants unless camera_grad=True, which calls v3a_gs_project_backward_cam and returns two more tensors,
    d_viewmat (shaped like viewmat, bottom row zero) and d_campos (like campos); the first four are the same bits either way.
    There is no gradient for K.  rasterize_mode="antialiased" needs `opacities` [U]:
    d_opacity is then taken as the gradient of opacity * compensation, and the compensation's share reaches means and covars."""
    mode = _gs_mode(rasterize_mode)
    Cn, U, sh_k = _gs_scene_args(means, covars, sh, viewmat, campos, K, sh_layout)
    if mode:
        if opacities is None:
            raise ValueError("gs_project_backward: rasterize_mode='antialiased' needs opacities [U]")
        _f32_dev(opacities, "opacities", numel=U)
    if covars.numel() != 9 * U or sh.numel() != 3 * sh_k * U:
        raise ValueError("means / covars / sh disagree on the number of Gaussians")
    _i32_dev(radii, "radii", numel=Cn * U)
    for k, n in (("d_means2d", 2), ("d_conics", 3), ("d_colors", 4), ("d_opacity", 1)):
        _f32_dev(entry_grads[k], k, numel=Cn * U * n)
    d_means, d_covars, d_sh = torch.empty_like(means), torch.empty_like(covars), torch.empty_like(sh)
    d_op = torch.empty(U, device=means.device, dtype=f32)
    a = L.GsProjectBackwardArgs(_ptr(means), _ptr(covars), _ptr(sh), sh_layout, sh_k, sh_degree, _ptr(viewmat), _ptr(campos), _ptr(K), U, Cn,
                                width, height, eps2d, _ptr(radii), _ptr(entry_grads["d_means2d"]), _ptr(entry_grads["d_conics"]),
                                _ptr(entry_grads["d_colors"]), _ptr(entry_grads["d_opacity"]), _ptr(d_means), _ptr(d_covars), _ptr(d_sh),
                                _ptr(d_op), mode, _ptr(opacities) if mode else None)
    if camera_grad:
        lib = L.load()
        ws, ws_bytes = _workspace(lib.v3a_gs_project_backward_cam_workspace_bytes(U, Cn),
                                  f"v3a_gs_project_backward_cam_workspace_bytes (U = {U}, C = {Cn})", means.device)
        d_view, d_campos = torch.empty_like(viewmat), torch.empty_like(campos)
        L.check(lib.v3a_gs_project_backward_cam(C.byref(a), _ptr(d_view), _ptr(d_campos), _ptr(ws), ws_bytes, _stream()),
                "v3a_gs_project_backward_cam")
        return d_means, d_covars, d_sh, d_op, d_view, d_campos
    L.check(L.load().v3a_gs_project_backward(C.byref(a), _stream()), "v3a_gs_project_backward")
    return d_means, d_covars, d_sh, d_op


class _GsRender(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, covars, sh, opacities, viewmat, campos, K, width, height, sh_degree, sh_layout, background, clamp_rgb,
                workspace, n_isect_out, rasterize_mode, camera_grad, info_out, absgrad):
        pr = gs_project(means, covars, sh, viewmat, campos, K, width, height, sh_degree=sh_degree, sh_layout=sh_layout,
                        rasterize_mode=rasterize_mode)
        r = gs_rasterize(pr, opacities, width, height, background=background, clamp_rgb=clamp_rgb, workspace=workspace, return_order=True)
        if n_isect_out is not None:
            n_isect_out.append(r["n_isect"])
        ctx.save_for_backward(means, covars, sh, opacities, viewmat, campos, K, pr["radii"], pr["means2d"], pr["conics"], pr["colors"],
                              r["tile_offsets"], r["flatten_ids"].contiguous(), *([pr["compensations"]] if "compensations" in pr else []))
        ctx.cfg = (width, height, sh_degree, sh_layout, background, clamp_rgb, workspace, rasterize_mode)
        ctx.camera_grad = camera_grad
        ctx.info_out, ctx.absgrad = info_out, absgrad
        if info_out is not None:
            info_out["radii"] = pr["radii"]
        return r["color"], r["depth"], r["alpha"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_color, d_depth, d_alpha):
        means, covars, sh, opacities, viewmat, campos, K, radii, means2d, conics, colors, offs, ids, *comp = ctx.saved_tensors
        width, height, sh_degree, sh_layout, background, clamp_rgb, workspace, rasterize_mode = ctx.cfg
        Cn = radii.shape[0]
        z = lambda g, *s: torch.zeros(Cn, height, width, *s, device=means.device, dtype=f32) if g is None else g.float().contiguous()
        if workspace is not None and workspace.bwd is None:
            workspace.bwd = GsBwdWorkspace()
        pr = dict(radii=radii, means2d=means2d, conics=conics, colors=colors)
        if comp:
            pr["compensations"] = comp[0]
        eg = gs_rasterize_backward(pr, opacities, width, height, offs, ids, z(d_color, 3), z(d_depth), z(d_alpha), background=background,
                                   clamp_rgb=clamp_rgb, workspace=workspace.bwd if workspace is not None else None,
                                   absgrad=ctx.absgrad)
        if ctx.info_out is not None:
            ctx.info_out["d_means2d"] = eg["d_means2d"]
            if ctx.absgrad:
                ctx.info_out["d_means2d_abs"] = eg["d_means2d_abs"]
        grads = gs_project_backward(means, covars, sh, viewmat, campos, K, width, height, radii, eg, sh_degree=sh_degree, sh_layout=sh_layout,
                                    rasterize_mode=rasterize_mode, opacities=opacities if comp else None, camera_grad=ctx.camera_grad)
        return grads + (None,) * (19 - len(grads))     # 4 gradients, 6 with the cameras'; none for the other inputs of forward


def gs_render(means: torch.Tensor, covars: torch.Tensor, sh: torch.Tensor, opacities: torch.Tensor, viewmat: torch.Tensor,
              campos: torch.Tensor, K: torch.Tensor, width: int, height: int, *, sh_degree: int = 4, sh_layout: int = 1,
              background: Optional[torch.Tensor] = None, clamp_rgb: bool = True, workspace: Optional[GsWorkspace] = None,
              n_isect_out: Optional[list] = None, rasterize_mode: str = "classic", camera_grad: bool = False,
              info_out: Optional[dict] = None, absgrad: bool = False):
    """Differentiable gs_project + gs_rasterize for C cameras (viewmat [C,4,4], campos [C,3], K [C,3,3]) ->
    (color [C,H,W,3], depth [C,H,W], alpha [C,H,W]) with gradients to means, covars, sh and opacities through the HIP backward
    kernels (csrc/raster_bwd.hip).  The forward values are gs_rasterize's, bit for bit.  By default cameras are constants:
    viewmat / campos / K that require grad are refused.  camera_grad=True (gsplat's optional pose gradients) accepts a viewmat /
    campos that requires grad and hands it its gradient (v3a_gs_project_backward_cam; the other four gradients keep their bits);
    viewmat and campos are independent inputs here, so a pose reaches both through whatever computed them (ops.camera_adjust).
    K that requires grad is refused either way.  First-order only.
    rasterize_mode="antialiased": gsplat's mode of that name, forward and backward (every entry's opacity times its compensation).
    info_out: a dict that receives what the densification strategy reads, as gsplat's `info` does: "radii" [C,U] from the forward,
    "d_means2d" [C,U,2] from the backward, and with absgrad=True "d_means2d_abs" [C,U,2] (see gs_rasterize_backward).  With None
    (and absgrad=False) nothing changes."""
    _gs_mode(rasterize_mode)
    if absgrad and info_out is None:
        raise ValueError("gs_render: absgrad=True needs info_out (the dict that receives d_means2d_abs)")
    for t, n in ((viewmat, "viewmat"), (campos, "campos"), (K, "K")):
        if t.requires_grad and not (camera_grad and n != "K"):
            raise NotImplementedError(f"gs_render: no gradient for {n} (camera pose / intrinsics gradients are not implemented)"
                                      if not camera_grad else "gs_render: no gradient for K (intrinsics are not optimised)")
    if viewmat.dim() != 3:
        raise ValueError("gs_render: viewmat [C,4,4], campos [C,3], K [C,3,3] required")
    return _GsRender.apply(means, covars, sh, opacities, viewmat, campos, K, width, height, sh_degree, sh_layout, background,
                           clamp_rgb, workspace, n_isect_out, rasterize_mode, bool(camera_grad), info_out, bool(absgrad))


class _CameraAdjust(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w2c_base, c2w_base, deltas):
        V = deltas.shape[0]
        viewmat = torch.empty(V, 4, 4, device=deltas.device, dtype=f32)
        campos = torch.empty(V, 3, device=deltas.device, dtype=f32)
        L.check(L.load().v3a_camera_adjust(_ptr(w2c_base), _ptr(c2w_base), _ptr(deltas), V, _ptr(viewmat), _ptr(campos), _stream()),
                "v3a_camera_adjust")
        ctx.save_for_backward(w2c_base, c2w_base, deltas)
        return viewmat, campos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_viewmat, d_campos):
        w2c_base, c2w_base, deltas = ctx.saved_tensors
        V = deltas.shape[0]
        z = lambda g, *s: torch.zeros(V, *s, device=deltas.device, dtype=f32) if g is None else g.float().contiguous()
        d_viewmat, d_campos = z(d_viewmat, 4, 4), z(d_campos, 3)
        d_deltas = torch.empty_like(deltas)
        L.check(L.load().v3a_camera_adjust_backward(_ptr(w2c_base), _ptr(c2w_base), _ptr(deltas), _ptr(d_viewmat), _ptr(d_campos), V,
                                                    _ptr(d_deltas), _stream()), "v3a_camera_adjust_backward")
        return None, None, d_deltas


def camera_adjust(w2c_base: torch.Tensor, c2w_base: torch.Tensor, deltas: torch.Tensor):
    """The pose optimiser's parametrisation (the reference's CameraOptModule): base cameras w2c_base / c2w_base f32 [V,4,4] (each
    other's inverse, computed once on the host) and deltas f32 [V,9] = (translation[3], 6D rotation[6]) -> (viewmat [V,4,4],
    campos [V,3]) of the adjusted cameras c2w_base [Rd | dx], as gs_render takes them, with the gradient to `deltas` (HIP, closed
    form in both directions).  Zero deltas return the base matrices bit for bit.  The bases are constants: refused if they require
    grad."""
    for t, n, shape in ((w2c_base, "w2c_base", (4, 4)), (c2w_base, "c2w_base", (4, 4)), (deltas, "deltas", (9,))):
        _f32_dev(t, f"camera_adjust: {n}", (None,) + shape)
    if not (w2c_base.shape[0] == c2w_base.shape[0] == deltas.shape[0]) or deltas.shape[0] < 1:
        raise ValueError(f"camera_adjust: w2c_base, c2w_base and deltas disagree on the number of cameras: {w2c_base.shape[0]}, "
                         f"{c2w_base.shape[0]}, {deltas.shape[0]}")
    for t, n in ((w2c_base, "w2c_base"), (c2w_base, "c2w_base")):
        if t.requires_grad:
            raise NotImplementedError(f"camera_adjust: no gradient for {n} (the base cameras are constants; the deltas train)")
    return _CameraAdjust.apply(w2c_base, c2w_base, deltas)
