"""Image metrics (csrc/image_metrics.hip), the LPIPS and CLIP passes (csrc/lpips.hip, csrc/clip.hip) and colour correction (csrc/color_correct.hip)."""
import ctypes as C
from typing import Optional

import torch

from .. import lib as L
from .common import _f32_dev, _i32_dev, _ptr, _stream, _tensor, _workspace, bf16, f32


def image_metrics(a_u8: torch.Tensor, b_u8: torch.Tensor):
    """SSIM and MSE of N uint8 image pairs [N,H,W,C] (PNG byte order; pixels scored as u8 / 255) in one call
    (csrc/image_metrics.hip).  -> (ssim [N] f64, mse [N] f64) on the device; PSNR = -10 log10(mse) is the caller's."""
    for name, t in (("a_u8", a_u8), ("b_u8", b_u8)):
        _tensor(t, name, torch.uint8, (None,) * 4)
    if a_u8.shape != b_u8.shape:
        raise ValueError(f"image shapes differ: {tuple(a_u8.shape)} vs {tuple(b_u8.shape)}")
    N, H, W, Cc = a_u8.shape
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_image_metrics_workspace_bytes(N, H, W, Cc),
                              f"v3a_image_metrics_workspace_bytes (shape {tuple(a_u8.shape)})", a_u8.device)
    ssim = torch.empty(N, device=a_u8.device, dtype=torch.float64)
    mse = torch.empty(N, device=a_u8.device, dtype=torch.float64)
    args = L.ImageMetricsArgs(_ptr(a_u8), _ptr(b_u8), N, H, W, Cc, _ptr(ssim), _ptr(mse), _ptr(ws), ws_bytes)
    L.check(lib.v3a_image_metrics(C.byref(args), _stream()), "v3a_image_metrics")
    return ssim, mse


# ------------------------------------------------------------------------------------------------ LPIPS(VGG) passes (csrc/lpips.hip)
def lpips_input(pred: torch.Tensor, gt: torch.Tensor, cin_pad: int = 16) -> torch.Tensor:
    """N pred and N gt images -> ONE pair [2, 2N, H, W, cin_pad] (frames [0,N) = pred, [N,2N) = gt), lpips' input transform
    (ToTensor's u8 / 255 where uint8, 2 x - 1, ScalingLayer) in fp32.  pred / gt: uint8 [N,H,W,3] (PNG bytes) or f32 [N,3,H,W] in [0,1]."""
    for name, t in (("pred", pred), ("gt", gt)):
        _tensor(t, name, (torch.uint8, f32), (None,) * 4)     # uint8 [N,H,W,3] or f32 [N,3,H,W]
    if pred.shape != gt.shape or pred.dtype != gt.dtype:
        raise ValueError(f"pred and gt differ: {pred.dtype} {tuple(pred.shape)} vs {gt.dtype} {tuple(gt.shape)}")
    nchw = pred.dtype == f32
    N, H, W = (pred.shape[0], pred.shape[2], pred.shape[3]) if nchw else pred.shape[:3]
    if (pred.shape[1] if nchw else pred.shape[3]) != 3:
        raise ValueError(f"LPIPS takes 3-channel images, got shape {tuple(pred.shape)}")
    out = torch.empty((2, 2 * N, H, W, cin_pad), device=pred.device, dtype=bf16)
    L.check(L.load().v3a_lpips_input(_ptr(pred), _ptr(gt), int(nchw), N, H, W, cin_pad, _ptr(out[0]), _ptr(out[1]), _stream()),
            "v3a_lpips_input")
    return out


def lpips_pool(x: torch.Tensor) -> torch.Tensor:
    """nn.MaxPool2d(2, 2) (floor mode) of a pair [2, F, H, W, C]: exact, the winning (hi, lo) is copied"""
    _tensor(x, "x", bf16, (2, None, None, None, None))      # a pair [2,F,H,W,C]
    _, F, H, W, Cc = x.shape
    out = torch.empty((2, F, H // 2, W // 2, Cc), device=x.device, dtype=bf16)
    L.check(L.load().v3a_lpips_pool(_ptr(x[0]), _ptr(x[1]), _ptr(out[0]), _ptr(out[1]), F, H, W, Cc, _stream()), "v3a_lpips_pool")
    return out


def lpips_head(x: torch.Tensor, weight: torch.Tensor, out: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """one tapped layer of LPIPS: x pair [2, 2N, h, w, C] (frames [0,N) pred, [N,2N) gt), weight f32 [C] (lin{l}.model.1.weight) ->
    out f64 [N] = the spatial mean of sum_c w (f^_pred - f^_gt)^2, or out += it with accumulate"""
    if x.dim() != 5 or x.shape[0] != 2 or x.shape[1] % 2 or not x.is_contiguous() or x.dtype != bf16 or not x.is_cuda:
        raise ValueError("x must be a contiguous device bf16 pair [2,2N,h,w,C]")
    _, F, h, w, Cc = x.shape
    N = F // 2
    if weight.dtype != f32 or not weight.is_contiguous() or weight.numel() != Cc or weight.device != x.device:
        raise ValueError(f"weight must be a contiguous f32 [{Cc}] tensor on {x.device}")
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != N or out.device != x.device:
        raise ValueError(f"out must be a contiguous f64 [{N}] tensor on {x.device}")
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_lpips_head_workspace_bytes(N, h, w, Cc), f"v3a_lpips_head_workspace_bytes (shape {tuple(x.shape)})",
                              x.device)
    L.check(lib.v3a_lpips_head(_ptr(x[0]), _ptr(x[1]), _ptr(weight), N, h, w, Cc, _ptr(out), int(accumulate), _ptr(ws), ws_bytes,
                               _stream()), "v3a_lpips_head")
    return out



# ------------------------------------------------------------------------------------------------ CLIP score passes (csrc/clip.hip)
def clip_preprocess(frames: torch.Tensor, tables: dict, lut: torch.Tensor, image_size: int, patch: int, *, want_u8: bool = False,
                    want_f32: bool = False):
    """CLIPImageProcessor (Pillow BICUBIC shorter-edge resize, centre crop, rescale, normalise) + patchify for uint8 frames [N,H,W,3].
    tables: device int32 tensors of evaluation.clip.resize_tables(H, W, image_size) - x_bounds / y_bounds [S,2], x_coeffs / y_coeffs
    [S,k] - and the ints row0, rows; lut: f32 [3,256].  -> (patch pair [2, N (S/P)^2, ldk], uint8 crop [N,S,S,3] or None, f32 pixel
    values [N,3,S,S] or None)."""
    _tensor(frames, "frames", torch.uint8, (None,) * 4)
    N, H, W, Cc = frames.shape
    S, P = image_size, patch
    if Cc != 3:
        raise ValueError(f"frames must be RGB [N,H,W,3], got {tuple(frames.shape)}")
    if S % P:
        raise ValueError(f"image_size {S} is not a multiple of the patch size {P}")
    _f32_dev(lut, "lut")
    if lut.numel() != 768:
        raise ValueError("lut must be f32 [3,256]")
    for key in ("x_bounds", "y_bounds", "x_coeffs", "y_coeffs"):
        _i32_dev(tables[key], key, (None, None))
        if tables[key].shape[0] != S:
            raise ValueError(f"{key} must have {S} rows")
    if tuple(tables["size"]) != (H, W, S):
        raise ValueError(f"tables were built for {tables['size']}, frames are {(H, W, S)}")
    row0, rows = int(tables["row0"]), int(tables["rows"])
    ldk = (3 * P * P + 7) // 8 * 8
    G = S // P
    patches = torch.empty((2, N * G * G, ldk), device=frames.device, dtype=bf16)
    u8 = torch.empty((N, S, S, 3), device=frames.device, dtype=torch.uint8) if want_u8 else None
    pix = torch.empty((N, 3, S, S), device=frames.device, dtype=f32) if want_f32 else None
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_clip_preprocess_workspace_bytes(N, rows, S), "v3a_clip_preprocess_workspace_bytes", frames.device)
    args = L.ClipPreprocessArgs(_ptr(frames), _ptr(tables["x_bounds"]), _ptr(tables["x_coeffs"]), _ptr(tables["y_bounds"]),
                                _ptr(tables["y_coeffs"]), _ptr(lut), _ptr(patches[0]), _ptr(patches[1]), _ptr(u8), _ptr(pix),
                                N, H, W, S, P, ldk, tables["x_coeffs"].shape[1], tables["y_coeffs"].shape[1], row0, rows,
                                _ptr(ws), ws_bytes)
    L.check(lib.v3a_clip_preprocess(C.byref(args), _stream()), "v3a_clip_preprocess")
    return patches, u8, pix


def clip_rows(src: torch.Tensor, *, ids: Optional[torch.Tensor] = None, cls: Optional[torch.Tensor] = None,
              pos: Optional[torch.Tensor] = None, S: int = 1, M: Optional[int] = None) -> torch.Tensor:
    """token assembly into the f32 residual stream: out[r] = src[row(r)] + pos[r % S]; row(r) = ids[r] (int32, inside src), or with
    `cls` the class token at r % S == 0 and patch row r - r // S - 1 elsewhere (src [B (S-1), d]) -> f32 [M, d]"""
    _f32_dev(src, "src", (None, None))
    d = src.shape[1]
    if d % 4:
        raise ValueError("row width must be a multiple of 4")
    if ids is not None:
        _i32_dev(ids, "ids")
        M = ids.numel()
    elif cls is not None:
        _f32_dev(cls, "cls")
        if cls.numel() != d or S < 2 or src.shape[0] % (S - 1):
            raise ValueError(f"cls must be f32 [{d}] and src hold whole sequences of {S - 1} patch rows")
        M = src.shape[0] // (S - 1) * S
    elif M is None:
        M = src.shape[0]
    if pos is not None:
        _f32_dev(pos, "pos", (None, None))
        if pos.shape[0] < S or pos.shape[1] != d:
            raise ValueError(f"pos must be f32 [>= {S}, {d}]")
    out = torch.empty((M, d), device=src.device, dtype=f32)
    L.check(L.load().v3a_clip_rows(_ptr(src), src.shape[0], _ptr(ids), _ptr(cls), _ptr(pos), _ptr(out), M, S, d, _stream()), "v3a_clip_rows")
    return out


def attention_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, B: int, S: int, H: int, causal: bool = False,
                  lens: Optional[torch.Tensor] = None, out_f32: bool = False, head_dim: int = 64, scale: Optional[float] = None) -> torch.Tensor:
    """fp32 attention for short sequences (v3a_attention_f32).  q, k, v: f32 [B S, >= H 64] views sharing one row stride (columns of a fused
    qkv buffer), head h at column 64 h.  lens: int32 [B] valid key counts.  -> pair [2, B S, H 64], or f32 [B S, H 64] with out_f32."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda or t.dtype != f32 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != B * S or t.shape[1] < H * head_dim:
            raise ValueError(f"{name} must be a device f32 [B S, >= H hd] view with unit column stride, got {t.dtype} {tuple(t.shape)}")
    if not (q.stride(0) == k.stride(0) == v.stride(0)):
        raise ValueError("q, k, v must share a row stride")
    if lens is not None:
        _i32_dev(lens, "lens", numel=B)
    d = H * head_dim
    out = torch.empty((B * S, d) if out_f32 else (2, B * S, d), device=q.device, dtype=f32 if out_f32 else bf16)
    sc = head_dim ** -0.5 if scale is None else scale
    L.check(L.load().v3a_attention_f32(_ptr(q), _ptr(k), _ptr(v), q.stride(0), None if out_f32 else _ptr(out[0]),
                                       None if out_f32 else _ptr(out[1]), _ptr(out) if out_f32 else None, d, _ptr(lens), B, S, H, head_dim,
                                       sc, int(causal), _stream()), "v3a_attention_f32")
    return out


def clip_score(image_emb: torch.Tensor, text_emb: torch.Tensor):
    """-> (scores f64 [F] = max(100 cos(image_emb[f], text_emb), 0), their mean f64 [1]); fp64 on the device, fixed summation order"""
    _f32_dev(image_emb, "image_emb", (None, None))
    _f32_dev(text_emb, "text_emb")
    F, D = image_emb.shape
    if text_emb.numel() != D:
        raise ValueError(f"text_emb must hold {D} values, got {tuple(text_emb.shape)}")
    scores = torch.empty(F, device=image_emb.device, dtype=torch.float64)
    mean = torch.empty(1, device=image_emb.device, dtype=torch.float64)
    L.check(L.load().v3a_clip_score(_ptr(image_emb), _ptr(text_emb), F, D, _ptr(scores), _ptr(mean), _stream()), "v3a_clip_score")
    return scores, mean


def _image_view(t: torch.Tensor, name: str, what: str, channels: Optional[int] = None):
    """(row stride, image stride) in elements of a float32 device view [N,H,W,C] whose rows of W C elements are contiguous"""
    if t.requires_grad:
        raise NotImplementedError(f"{what}: no gradient ({name} requires grad; detach it - this is a metric, not a loss)")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != f32 or t.dim() != 4 or (channels is not None and t.shape[-1] != channels):
        raise ValueError(f"{what}: {name} must be float32 [N,H,W,{channels or 'C'}], got {t.dtype} {tuple(t.shape)}")
    N, H, W, Cc = t.shape
    if min(N, H, W, Cc) < 1:
        raise ValueError(f"{what}: {name} is empty, shape {tuple(t.shape)}")
    if (Cc > 1 and t.stride(3) != 1) or (W > 1 and t.stride(2) != Cc):
        raise ValueError(f"{what}: the pixels of a row of {name} must be contiguous (strides {t.stride()}); row and image strides are free")
    ld = t.stride(1) if H > 1 else W * Cc
    return ld, (t.stride(0) if N > 1 else H * ld)


def color_correct(img: torch.Tensor, ref: torch.Tensor, num_iters: int = 5, eps: float = 0.5 / 255):
    """The reference's color_correct (lib_bilagrid.py:56-126) per image on csrc/color_correct.hip: `img` f32 [N,H,W,3] is warped
    towards `ref` by `num_iters` rounds of a masked least-squares fit of a quadratic colour transform (10 coefficients per output
    channel), every image on its own; fp64 after the loads, rounded once.  Views with free row / image strides are read in place.
    -> (corrected f32 [N,H,W,3], mse f64 [N] of corrected against ref, status int32 [N,3]).  status[n][c] != 0: in some round channel
    c of image n had fewer than 10 usable pixels (bit 0) or a singular system (bit 1) and kept the identity warp for that round
    (the reference asserts or is undefined there).  PSNR = -10 log10(mse) is the caller's.  No gradient: an input that requires one
    is refused."""
    ld_i, st_i = _image_view(img, "img", "color_correct", 3)
    ld_r, st_r = _image_view(ref, "ref", "color_correct", 3)
    if img.shape != ref.shape:
        raise ValueError(f"color_correct: image shapes differ: {tuple(img.shape)} vs {tuple(ref.shape)}")
    N, H, W, _ = img.shape
    lib = L.load()
    dev = img.device
    ws, ws_bytes = _workspace(lib.v3a_color_correct_workspace_bytes(N, H, W, int(num_iters)),
                              f"v3a_color_correct_workspace_bytes (shape {tuple(img.shape)}, num_iters {num_iters}; 1 <= num_iters <= 16 required)", dev)
    out = torch.empty((N, H, W, 3), device=dev, dtype=f32)
    sse = torch.empty(N, device=dev, dtype=torch.float64)
    status = torch.empty((N, 3), device=dev, dtype=torch.int32)
    args = L.ColorCorrectArgs(_ptr(img), _ptr(ref), _ptr(out), N, H, W, int(num_iters), ld_i, ld_r, 3 * W, st_i, st_r, 3 * W * H,
                              float(eps), _ptr(sse), _ptr(status), _ptr(ws), ws_bytes)
    L.check(lib.v3a_color_correct(C.byref(args), _stream()), f"v3a_color_correct (shape {tuple(img.shape)}, eps {eps})")
    return out, sse / float(H * W * 3), status


def image_mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Per-image mean squared error of two f32 image batches [N,H,W,C] (csrc/color_correct.hip): differences and sums in fp64,
    fixed-order reduction.  -> f64 [N] on the device; PSNR = -10 log10(mse) is the caller's.  Views with free row / image strides
    are read in place.  No gradient: an input that requires one is refused."""
    ld_a, st_a = _image_view(a, "a", "image_mse")
    ld_b, st_b = _image_view(b, "b", "image_mse")
    if a.shape != b.shape:
        raise ValueError(f"image_mse: image shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    N, H, W, Cc = a.shape
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_image_mse_workspace_bytes(N, H, W, Cc), f"v3a_image_mse_workspace_bytes (shape {tuple(a.shape)})", a.device)
    mse = torch.empty(N, device=a.device, dtype=torch.float64)
    args = L.ImageMseArgs(_ptr(a), _ptr(b), N, H, W, Cc, ld_a, ld_b, st_a, st_b, _ptr(mse), _ptr(ws), ws_bytes)
    L.check(lib.v3a_image_mse(C.byref(args), _stream()), f"v3a_image_mse (shape {tuple(a.shape)})")
    return mse
