"""Thin torch-tensor wrappers over the C ABI (include/vist3a_hip.h).

PyTorch supplies device memory and the current HIP stream only; all arithmetic happens inside
libvist3a_hip.so.  Every wrapper validates dtype/device/contiguity and raises on any non-zero return."""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from typing import Optional

import torch

from . import lib as L

bf16 = torch.bfloat16
f32 = torch.float32


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _workspace(need: int, what: str, device):
    """The per-call workspace of a loss / metric entry point from the answer of its *_workspace_bytes query: a negative answer is the
    query's error code and raises as `what`.  -> (float64 tensor, its size in bytes): 8-byte aligned by its dtype, never empty, the
    size rounded up to a multiple of 8.  Not cached: the buffer lives as long as the call's tensors do."""
    need = int(need)
    if need < 0:
        L.check(need, what)
    ws = torch.empty(max((need + 7) // 8, 1), device=device, dtype=torch.float64)
    return ws, ws.numel() * 8


def _chk2d(t: torch.Tensor, name: str, dtypes) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} has dtype {t.dtype}, expected one of {dtypes}")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be 2-D with a contiguous last dim, got shape {tuple(t.shape)} stride {t.stride()}")


class GemmProbe:
    """Optional HIP-event instrumentation of the GEMM launches that resolve to one tile configuration (= one kernel symbol):
    accumulates algorithmic FLOPs and event pairs so bench.py can report that kernel's live roofline numbers."""

    def __init__(self, tile: int, fp8: bool = False, stride: int = 1):
        """stride > 1: only every stride-th matching launch is bracketed by events (an event pair costs ~5 us of stream time; pick a
        stride coprime to the period of the launch sequence so that every shape is sampled)"""
        self.tile, self.fp8, self.flops, self.events, self.active = tile, fp8, 0.0, [], False
        self.stride, self.seen = max(1, int(stride)), 0

    def take(self) -> bool:
        self.seen += 1
        return self.seen % self.stride == 0

    def summary(self):
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.events]
        n = len(ms)
        return dict(launches=n, total_ms=sum(ms), avg_ms=(sum(ms) / n if n else 0.0), flops=self.flops,
                    flops_per_launch=(self.flops / n if n else 0.0))


_probe: Optional[GemmProbe] = None


def set_gemm_probe(p: Optional[GemmProbe]) -> None:
    global _probe
    _probe = p


class FlopMeter:
    """Algorithmic FLOPs of the matrix-pipe launches issued through this module while the meter is installed (`set_flop_meter`), by kind:
    GEMM 2MNK, convolution 2 x output pixels x Cout x taps x Cin (REAL channels; the fp32-equivalent form counts the fp32 convolution once,
    not its three bf16 products), attention 4 B H Nq Nk D over the keys that take part.  bench.py divides a stage's total by the stage's
    time for `stage_roofline`.  Launches replayed from a hipGraph do not pass through Python and are not counted."""

    def __init__(self):
        self.by_kind = {}

    def add(self, kind: str, flops: float) -> None:
        self.by_kind[kind] = self.by_kind.get(kind, 0.0) + float(flops)

    @property
    def total(self) -> float:
        return sum(self.by_kind.values())


_meter: Optional[FlopMeter] = None


def set_flop_meter(m: Optional[FlopMeter]) -> None:
    global _meter
    _meter = m


_gemm_ws = {}   # per (device, thread) split-K partial buffer (see _attn_ws)
# development A/B knob: V3A_TILE_OVERRIDE="MxNxK:tile,..." forces a tile for plain launches (tile = -1, no batch / split-K / transposed tail) of a shape
_tile_override = {tuple(int(v) for v in e.split(":")[0].split("x")): int(e.split(":")[1])
                  for e in os.environ.get("V3A_TILE_OVERRIDE", "").split(",") if ":" in e}


def gemm(
    a: torch.Tensor,
    w: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    *,
    out: Optional[torch.Tensor] = None,
    act: int = L.ACT_NONE,
    residual: Optional[torch.Tensor] = None,
    scale: Optional[torch.Tensor] = None,
    rows_per_batch: int = 0,
    round_after_scale: bool = False,
    out_f32: bool = False,
    bias_row: bool = False,
    tile: int = -1,
    residual2: Optional[torch.Tensor] = None,
    res_row_mod: int = 0,
    relu_out: bool = False,
    out_rows: Optional[tuple] = None,
    a_scale: Optional[torch.Tensor] = None,
    w_scale: Optional[torch.Tensor] = None,
    split_k: int = 1,
    batch: Optional[tuple] = None,
    row_sumsq: Optional[torch.Tensor] = None,
    t_out: Optional[torch.Tensor] = None,
    t_col0: int = 0,
) -> torch.Tensor:
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T); see v3a_gemm_bf16_nt for the epilogue order.
    batch = (count, a_stride, w_stride, out_stride[, residual_stride]) in elements: `count` problems of this shape in one launch, problem z
    offset by z * stride in each operand (0 = shared; residual_stride defaults to out_stride); a / w / out / residual describe problem 0.
    row_sumsq (f32 [M, N // 32], written): per (row, 32-column block) sum of squares of bf16(acc + bias) - the statistics of an RMS norm the
    consumer applies itself (ops.xattn_probs q_row_sumsq); plain bias epilogue only.
    out_rows=(group, skip, off) scatters output row m to m + (m//group)*skip + off (out must be given).
    t_out / t_col0 (transposed tail): output columns n >= t_col0 go to t_out[n - t_col0, m] (bf16 [N - t_col0, >= M]) instead of `out`, which then
    holds the first t_col0 columns only - the fused q | k | v projection: q | k row-major, V^T for the flash kernel, one launch.  Bias only.

    scale: f32 [N] (LayerScale) or [nbatch, N] together with rows_per_batch (AdaLN gate).
    split_k > 1 (bf16 only): K cut into split_k slices computed side by side, summed by a second launch (few output tiles, long K).
    a_scale / w_scale (f32 [M] / [N]): a and w are e4m3 bytes from `quantize_fp8_rows`; runs v3a_gemm_fp8_nt (tile then indexes its tiles)."""
    in_dt = (bf16,) if a_scale is None else (torch.uint8, torch.float8_e4m3fn)
    _chk2d(a, "a", in_dt)
    _chk2d(w, "w", in_dt)
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise ValueError(f"K mismatch: a {tuple(a.shape)} vs w {tuple(w.shape)}")
    if t_out is not None:
        _chk2d(t_out, "t_out", (bf16,))
        if out is None or t_col0 <= 0 or t_col0 % 192 or t_col0 >= N or t_out.shape[0] < N - t_col0 or t_out.shape[1] < M or out.shape[1] < t_col0:
            raise ValueError("t_out needs an explicit out [M, >= t_col0], 0 < t_col0 < N in whole 192-column tiles, t_out [N - t_col0, >= M]")
    if out is None:
        if out_rows is not None:
            raise ValueError("out_rows needs an explicit out tensor")
        out = torch.empty((M, N), device=a.device, dtype=f32 if out_f32 else bf16)
    _chk2d(out, "out", (f32,) if out_f32 else (bf16,))
    # weight-streaming shapes (<= 128 rows against a big matrix) go to the skinny kernel: the tile GEMM would occupy N/128 CUs
    plain = t_out is None and split_k <= 1 and batch is None and row_sumsq is None and a_scale is None and scale is None and residual2 is None and out_rows is None and not relu_out and tile < 0 and res_row_mod == 0
    if plain and K % 512 == 0 and K >= 1024:
        if M <= 128 and N >= 512 and not bias_row:
            return _gemm_skinny(a, w, bias, out, act, residual, out_f32, transposed=False)
        if N <= 128 and M >= 512 and (bias is None or bias_row):
            return _gemm_skinny(w, a, bias, out, act, residual, out_f32, transposed=True)
    flags = L.GEMM_RELU_OUT if relu_out else 0
    if bias is not None:
        if bias.dtype != f32 or not bias.is_contiguous() or bias.numel() != (M if bias_row else N):
            raise ValueError("bias must be contiguous f32 of length N (or M with bias_row)")
        if bias_row:
            flags |= L.GEMM_BIAS_ROW
    sstride = 0
    if scale is not None:
        if scale.dtype != f32 or scale.stride(-1) != 1:
            raise ValueError("scale must be f32 with contiguous last dim")
        if scale.dim() == 2:
            if rows_per_batch <= 0:
                raise ValueError("2-D scale needs rows_per_batch")
            flags |= L.GEMM_SCALE_PER_BATCH
            sstride = scale.stride(0)
        if round_after_scale:
            flags |= L.GEMM_ROUND_AFTER_SCALE
    ldr = 0
    if residual is not None:
        _chk2d(residual, "residual", (bf16, f32))
        if residual.shape[1] != N or (res_row_mod == 0 and residual.shape[0] != M):
            raise ValueError("residual shape mismatch")
        if residual.dtype == f32:
            flags |= L.GEMM_RES_F32
        ldr = residual.stride(0)
    if out_f32:
        flags |= L.GEMM_OUT_F32
    if _tile_override and tile < 0 and batch is None and split_k == 1 and t_out is None and a_scale is None:
        tile = _tile_override.get((M, N, K), tile)
    args = L.GemmArgs(
        _ptr(a), _ptr(w), _ptr(out), _ptr(bias), _ptr(residual), _ptr(scale),
        M, N, K, a.stride(0), w.stride(0), out.stride(0), ldr,
        rows_per_batch, sstride, act, flags, tile,
        _ptr(residual2), residual2.stride(0) if residual2 is not None else 0, res_row_mod,
        *(out_rows if out_rows is not None else (0, 0, 0)),
    )
    if t_out is not None:
        if a_scale is not None:
            raise ValueError("t_out applies to the bf16 GEMM")
        args.C_t, args.ldct, args.t_col0 = t_out.data_ptr(), t_out.stride(0), t_col0
    if row_sumsq is not None:
        nbat = int(batch[0]) if batch is not None else 1
        if a_scale is not None or row_sumsq.dtype != f32 or not row_sumsq.is_contiguous() or row_sumsq.numel() < nbat * M * (N // 32) or N % 32:
            raise ValueError("row_sumsq must be contiguous f32 [batch * M, N // 32] (bf16 GEMM, N % 32 == 0)")
        if residual is not None or residual2 is not None or relu_out or out_rows is not None or act != L.ACT_NONE or scale is not None or bias_row:
            raise ValueError("row_sumsq is a by-product of the plain bias epilogue only")
        args.row_sumsq = row_sumsq.data_ptr()
    nb = 1
    if batch is not None:
        if a_scale is not None or split_k > 1:
            raise ValueError("batch applies to the plain bf16 GEMM")
        nb = int(batch[0])
        args.batch, args.a_batch_stride, args.b_batch_stride, args.c_batch_stride = nb, int(batch[1]), int(batch[2]), int(batch[3])
        args.res_batch_stride = int(batch[4]) if len(batch) > 4 else (int(batch[3]) if residual is not None else 0)
    if split_k > 1:
        if a_scale is not None:
            raise ValueError("split_k applies to the bf16 GEMM")
        nbytes = L.load().v3a_gemm_split_workspace_bytes(M, N, split_k)
        wk = (a.device, threading.get_ident())
        ws = _gemm_ws.get(wk)
        if ws is None or ws.numel() < nbytes:
            ws = _gemm_ws[wk] = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
        args.split_k, args.workspace = split_k, ws.data_ptr()
    if _meter is not None:
        _meter.add("gemm_fp8" if a_scale is not None else "gemm", 2.0 * M * N * K * nb)
    if a_scale is not None:
        for t, n, nm in ((a_scale, M, "a_scale"), (w_scale, N, "w_scale")):
            if t is None or t.dtype != f32 or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"{nm} must be contiguous f32 of length {n}")
        fargs = L.GemmFp8Args(args, _ptr(a_scale), _ptr(w_scale))
        pr = _probe
        timed = pr is not None and pr.active and pr.fp8 and (tile if tile >= 0 else L.load().v3a_gemm_fp8_pick_tile(M, N)) == pr.tile and pr.take()
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        L.check(L.load().v3a_gemm_fp8_nt(C.byref(fargs), _stream()), "v3a_gemm_fp8_nt")
        if timed:
            e1.record()
            pr.events.append((e0, e1))
            pr.flops += 2.0 * M * N * K
        return out
    pr = _probe
    # the tile the C side really runs (batch / split-K slices count towards the tile choice; a transposed tail forces its own tile)
    if pr is not None and pr.active and not pr.fp8 and (tile if tile >= 0 else L.load().v3a_gemm_pick_tile_ex(M, N, act, max(nb, split_k), int(t_out is not None))) == pr.tile and pr.take():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.load().v3a_gemm_bf16_nt(C.byref(args), _stream()), "v3a_gemm_bf16_nt")
        e1.record()
        pr.events.append((e0, e1))
        pr.flops += 2.0 * M * N * K * nb
        return out
    L.check(L.load().v3a_gemm_bf16_nt(C.byref(args), _stream()), "v3a_gemm_bf16_nt")
    return out


_skinny_ws = {}


def _gemm_skinny(x, wbig, bias, out, act, residual, out_f32, transposed):
    """x [Msmall<=128, K] against wbig [Nbig, K]: out[m][n] (or out[n][m] when transposed) through v3a_gemm_skinny_bf16."""
    Ms, K = x.shape
    Nb = wbig.shape[0]
    if bias is not None and (bias.dtype != f32 or not bias.is_contiguous() or bias.numel() != Nb):
        raise ValueError("bias must be contiguous f32 over the weight rows")
    lib = L.load()
    need = lib.v3a_gemm_skinny_workspace_bytes(Ms, Nb, K)
    if need < 0:
        L.check(int(need), "v3a_gemm_skinny_workspace_bytes")
    # per stream and per host thread: the partial sums are live until the finish kernel, and two threads (virtual ranks of
    # seqpar.ThreadWorld) may be inside the two-launch C call at the same time
    key = (x.device.index, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    ws = _skinny_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _skinny_ws[key] = torch.empty(max(need, 1 << 22), device=x.device, dtype=torch.uint8)
    flags, ldr = 0, 0
    if residual is not None:
        _chk2d(residual, "residual", (bf16, f32))
        if tuple(residual.shape) != tuple(out.shape):
            raise ValueError("residual shape mismatch")
        if residual.dtype == f32:
            flags |= L.GEMM_RES_F32
        ldr = residual.stride(0)
    if out_f32:
        flags |= L.GEMM_OUT_F32
    args = L.GemmSkinnyArgs(_ptr(x), _ptr(wbig), _ptr(out), _ptr(bias), _ptr(residual), Ms, Nb, K, x.stride(0), wbig.stride(0),
                            out.stride(0), ldr, act, flags, int(transposed), _ptr(ws), ws.numel())
    if _meter is not None:
        _meter.add("gemm_skinny", 2.0 * Ms * Nb * K)
    L.check(lib.v3a_gemm_skinny_bf16(C.byref(args), _stream()), "v3a_gemm_skinny_bf16")
    return out


class ConvWeight:
    """A convolution weight packed for v3a_conv_bf16: w[CoutPad][Kpad] bf16 (k = tap-major, channel-minor), the
    K-chunk table, f32 bias.  Cin/Cout are padded to multiples of 8 with zeros (activations must carry CinPad)."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, device="cuda", dilation=(1, 1, 1)):
        """dilation (dT, dH, dW): tap (t, h, w) reads the input t dT / h dH / w dW positions from the window origin - the K-chunk table
        carries the scaled offsets (4 bits each: (k - 1) d <= 15), the kernels are unchanged; `k_eff` is the window extent (k - 1) d + 1."""
        w = weight.detach()
        if w.dim() == 4:  # conv2d -> kT = 1
            w = w[:, :, None]
        if w.dim() == 3:  # conv1d
            w = w[:, :, None, None]
        Cout, Cin, kT, kH, kW = w.shape
        self.Cout, self.Cin, self.k = Cout, Cin, (kT, kH, kW)
        self.dil = tuple(int(v) for v in dilation)
        if len(self.dil) != 3 or min(self.dil) < 1 or any((k - 1) * d_ > 15 for k, d_ in zip(self.k, self.dil)):
            raise ValueError(f"dilation {dilation} with kernel {self.k}: every (k - 1) * d must be <= 15 (4-bit tap offsets of the K-chunk table)")
        self.k_eff = tuple((k - 1) * d_ + 1 for k, d_ in zip(self.k, self.dil))
        self.CinP, self.CoutP = (Cin + 7) // 8 * 8, (Cout + 7) // 8 * 8
        K = kT * kH * kW * self.CinP
        self.Kpad = (K + 63) // 64 * 64
        wp = torch.zeros(self.CoutP, kT, kH, kW, self.CinP, dtype=f32)
        wp[:Cout, :, :, :, :Cin] = w.float().permute(0, 2, 3, 4, 1).cpu()
        full = torch.zeros(self.CoutP, self.Kpad, dtype=f32)
        full[:, :K] = wp.reshape(self.CoutP, K)
        self.w = full.to(device=device, dtype=bf16).contiguous()
        tab = torch.zeros(self.Kpad // 8, dtype=torch.int64)
        idx = torch.arange(K // 8)
        tap, c8 = idx // (self.CinP // 8), idx % (self.CinP // 8)
        dt, dh, dw = tap // (kH * kW) * self.dil[0], (tap // kW) % kH * self.dil[1], tap % kW * self.dil[2]
        tab[: K // 8] = (c8 * 8) | (dw << 16) | (dh << 20) | (dt << 24) | (1 << 31)
        tab = torch.where(tab >= 2 ** 31, tab - 2 ** 32, tab)
        self.ktab = tab.to(torch.int32).to(device).contiguous()
        b = torch.zeros(self.CoutP, dtype=f32)
        if bias is not None:
            b[:Cout] = bias.detach().float().cpu()
        self.bias = b.to(device)
        self.has_bias = bias is not None
        # second packing for the halo-tile kernel (csrc/conv_halo.hip; layout documented at v3a_conv_args.w_halo):
        # [Cout/96][kT][Cin/48][9][96][48], the six 16-byte chunks of row n rotated by 3 * ((n >> 3) & 1)
        self.w_halo = None
        if kH == 3 and kW == 3 and kT in (1, 3) and self.CinP % 48 == 0 and self.CoutP % 96 == 0 and self.dil == (1, 1, 1):
            nN, nC = self.CoutP // 96, self.CinP // 48
            h = wp.reshape(nN, 96, kT, 9, nC, 6, 8).permute(0, 2, 4, 3, 1, 5, 6).contiguous()   # [nN, kT, nC, 9, 96, 6 chunks, 8]
            rot = 3 * ((torch.arange(96) >> 3) & 1)
            src = (torch.arange(6)[None, :] - rot[:, None]) % 6                                  # position s of row n holds chunk (s - rot) % 6
            h = torch.gather(h, 5, src.view(1, 1, 1, 1, 96, 6, 1).expand(nN, kT, nC, 9, 96, 6, 8))
            self.w_halo = h.to(device=device, dtype=bf16).contiguous()


def conv(
    x: torch.Tensor, cw: ConvWeight, *, out: Optional[torch.Tensor] = None,
    stride=(1, 1, 1), pad=(0, 0, 0), out_size=None, ups2: bool = False, replicate: bool = False,
    act: int = L.ACT_NONE, residual: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
    out_f32: bool = False, tile: int = -1, residual2: Optional[torch.Tensor] = None, res_row_mod: int = 0,
    relu_out: bool = False, out_rows: Optional[tuple] = None, form_scale: Optional[float] = None,
) -> torch.Tensor:
    """x: channels-last [T,H,W,CinP] bf16 contiguous -> out [oT,oH,oW,CoutP].  pad = LEADING pad per dim.  Spatial
    dims follow PyTorch's symmetric-pad formula; the temporal dim is causal (all padding leading) when
    pad_T == k_T - 1 and symmetric otherwise.  `out_size` overrides.
    tile: -1 = automatic (the halo-tile kernel for wide 3x3(x3) layers, else the implicit GEMM with a heuristic tile), >= 0 = that
    implicit-GEMM tile, -2 = force the halo-tile kernel (error if the layer is not of its form), -3 = never the halo-tile kernel.
    An H-STRIP of a spatially sharded image carries one explicit halo row above and below (the neighbours' boundary rows, zeros at the image
    border) and is convolved VALID in H: pad = (pT, 0, pW) with out_size = (T, H - 2, W) - or, with ups2, pad = (pT, -1, pW) and out_size =
    (T, 2 (H - 2), 2 W) - both forms of the halo-tile kernel as well (v3a_conv_args).
    form_scale (with tile = -1): choose halo-tile vs implicit GEMM as if the layer were form_scale times larger - a rank's strip takes the
    kernel form the whole image would take, which keeps a sharded decode bit-identical to the unsharded one."""
    if x.dim() != 4 or not x.is_contiguous() or x.dtype != bf16 or not x.is_cuda:
        raise ValueError("x must be a contiguous device bf16 tensor [T,H,W,C]")
    T, H, W, Cin = x.shape
    if Cin != cw.CinP:
        raise ValueError(f"x has {Cin} channels, packed weight expects {cw.CinP}")
    kT, kH, kW = cw.k
    eT_, eH_, eW_ = cw.k_eff                      # window extents (= the kernel sizes without dilation)
    eH, eW = (2 * H, 2 * W) if ups2 else (H, W)
    if out_size is None:
        if kT > 1 and pad[0] == eT_ - 1:
            oT = (T + pad[0] - eT_) // stride[0] + 1
        else:
            oT = (T + 2 * pad[0] - eT_) // stride[0] + 1
        oH = (eH + 2 * pad[1] - eH_) // stride[1] + 1
        oW = (eW + 2 * pad[2] - eW_) // stride[2] + 1
    else:
        oT, oH, oW = out_size
    M = oT * oH * oW
    if out is None:
        out = torch.empty((oT, oH, oW, cw.CoutP), device=x.device, dtype=f32 if out_f32 else bf16)
    o2 = out.view(-1, out.shape[-1])
    flags = L.GEMM_RELU_OUT if relu_out else 0
    ldr = 0
    r2 = None
    if residual is not None:
        r2 = residual.view(-1, residual.shape[-1])
        if r2.dtype == f32:
            flags |= L.GEMM_RES_F32
        ldr = r2.stride(0)
    if out_f32:
        flags |= L.GEMM_OUT_F32
    args = L.ConvArgs(
        _ptr(x), _ptr(cw.w), _ptr(cw.ktab), _ptr(o2), _ptr(cw.bias if cw.has_bias else None), _ptr(r2), _ptr(scale),
        T, H, W, Cin, oT, oH, oW, cw.CoutP, cw.Kpad,
        stride[0], stride[1], stride[2], pad[0], pad[1], pad[2],
        int(ups2), int(replicate), o2.stride(0), ldr, act, flags, tile,
        _ptr(residual2), residual2.view(-1, residual2.shape[-1]).stride(0) if residual2 is not None else 0, res_row_mod,
        *(out_rows if out_rows is not None else (0, 0, 0)),
        _ptr(cw.w_halo), kT if cw.w_halo is not None else 0,
    )
    if form_scale is not None and tile == -1 and cw.w_halo is not None:
        args.tile = -2 if L.load().v3a_conv_halo_tiles(C.byref(args)) * form_scale >= 512 else -3
    if _meter is not None:
        _meter.add("conv", 2.0 * M * cw.Cout * kT * kH * kW * cw.Cin)
    L.check(L.load().v3a_conv_bf16(C.byref(args), _stream()), "v3a_conv_bf16")
    return out


# ------------------------------------------------------------------------------------------------ fp32-equivalent ("split bf16") path
# A PAIR is a contiguous bf16 tensor [2, ...]: plane 0 = hi = bf16(x), plane 1 = lo = bf16(x - hi); x = hi + lo (include/vist3a_hip.h,
# v3a_conv_split).  The layers the reference runs with autocast off (anysplat_stitched.py:335) carry their activations in this form.

def pair_value(p: torch.Tensor) -> torch.Tensor:
    """the fp32 value of a pair (tests / glue; the kernels never materialise it)"""
    return p[0].float() + p[1].float()


def split_f32(x: torch.Tensor) -> torch.Tensor:
    """contiguous f32 [...] (numel % 8 == 0) -> pair [2, ...]"""
    if x.dtype != f32 or not x.is_contiguous() or not x.is_cuda or x.numel() % 8:
        raise ValueError("x must be a contiguous device f32 tensor with numel % 8 == 0")
    out = torch.empty((2,) + tuple(x.shape), device=x.device, dtype=bf16)
    L.check(L.load().v3a_split_f32(_ptr(x), _ptr(out[0]), _ptr(out[1]), x.numel(), _stream()), "v3a_split_f32")
    return out


def layernorm_pair(x: torch.Tensor, *, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, eps: float = 1e-5,
                   M: Optional[int] = None, in_rows: tuple = (0, 0, 0)) -> torch.Tensor:
    """F.layer_norm of f32 rows -> pair [2, M, d]; in_rows as in `layernorm`."""
    _chk2d(x, "x", (f32,))
    d = x.shape[1]
    if M is None:
        M = x.shape[0]
    for t in (weight, bias):
        if t is not None and (t.dtype != f32 or not t.is_contiguous() or t.numel() != d):
            raise ValueError("affine weight/bias must be contiguous f32 [d]")
    out = torch.empty((2, M, d), device=x.device, dtype=bf16)
    L.check(L.load().v3a_layernorm_pair(_ptr(x), _ptr(out[0]), _ptr(out[1]), _ptr(weight), _ptr(bias), M, d, x.stride(0), d, eps,
                                        *in_rows, _stream()), "v3a_layernorm_pair")
    return out


def bilinear_cl_pair(x: torch.Tensor, size, *, align_corners: bool, add: Optional[torch.Tensor] = None,
                     table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pair [2,T,h,w,C] -> pair [2,T,H,W,C] (+ pair `add` of the output's shape, + f32 `table` [H*W, C])."""
    if x.dtype != bf16 or not x.is_contiguous() or x.dim() != 5 or x.shape[0] != 2:
        raise ValueError("x must be a contiguous bf16 pair [2,T,h,w,C]")
    _, T, h, w, Cc = x.shape
    H, W = size
    out = torch.empty((2, T, H, W, Cc), device=x.device, dtype=bf16)
    if add is not None and (add.dtype != bf16 or not add.is_contiguous() or tuple(add.shape) != tuple(out.shape)):
        raise ValueError("add must be a contiguous pair with the output's shape")
    if table is not None and (table.dtype != f32 or not table.is_contiguous() or table.numel() != H * W * Cc):
        raise ValueError("table must be contiguous f32 [H*W, C]")
    L.check(L.load().v3a_bilinear_cl_pair(_ptr(x[0]), _ptr(x[1]), _ptr(out[0]), _ptr(out[1]), _ptr(add[0]) if add is not None else None,
                                          _ptr(add[1]) if add is not None else None, _ptr(table), T, h, w, H, W, Cc, int(align_corners),
                                          _stream()), "v3a_bilinear_cl_pair")
    return out


class ConvWeightSplit:
    """An fp32 convolution weight packed for v3a_conv_split: w = wh + wl (bf16 pair), matrix [CoutP][Kpad] = (wh | wl | wh) along K, each
    range tap-major / channel-minor like ConvWeight; the chunk table reads x's LO plane for the first range (bit 28) and its HI plane for
    the other two:  acc = xl.wh + xh.wl + xh.wh  (small terms first).  f32 bias."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, device="cuda"):
        w = weight.detach()
        if w.dim() == 4:
            w = w[:, :, None]
        if w.dim() == 3:
            w = w[:, :, None, None]
        Cout, Cin, kT, kH, kW = w.shape
        self.Cout, self.Cin, self.k = Cout, Cin, (kT, kH, kW)
        self.CinP, self.CoutP = (Cin + 7) // 8 * 8, (Cout + 7) // 8 * 8
        K = kT * kH * kW * self.CinP
        self.Kpad = (3 * K + 63) // 64 * 64
        wp = torch.zeros(self.CoutP, kT, kH, kW, self.CinP, dtype=f32)
        wp[:Cout, :, :, :, :Cin] = w.float().permute(0, 2, 3, 4, 1).cpu()
        wp = wp.reshape(self.CoutP, K)
        wh = wp.to(bf16)
        wl = (wp - wh.float()).to(bf16)
        full = torch.zeros(self.CoutP, self.Kpad, dtype=bf16)
        full[:, :K], full[:, K:2 * K], full[:, 2 * K:3 * K] = wh, wl, wh
        self.w = full.to(device).contiguous()
        tab = torch.zeros(self.Kpad // 8, dtype=torch.int64)
        idx = torch.arange(K // 8)
        tap, c8 = idx // (self.CinP // 8), idx % (self.CinP // 8)
        dt, dh, dw = tap // (kH * kW), (tap // kW) % kH, tap % kW
        e = (c8 * 8) | (dw << 16) | (dh << 20) | (dt << 24) | (1 << 31)
        tab[: K // 8], tab[K // 8: 2 * K // 8], tab[2 * K // 8: 3 * K // 8] = e | (1 << 28), e, e
        tab = torch.where(tab >= 2 ** 31, tab - 2 ** 32, tab)
        self.ktab = tab.to(torch.int32).to(device).contiguous()
        b = torch.zeros(self.CoutP, dtype=f32)
        if bias is not None:
            b[:Cout] = bias.detach().float().cpu()
        self.bias = b.to(device)
        self.has_bias = bias is not None
        # second packing for the halo-tile form (csrc/conv_halo_split.hip; layout at v3a_conv_split_args in the header):
        # [Cout/BN][Cin/16][9][2 planes][BN][2 chunk positions][8], position s of row n holds chunk s ^ ((n >> 3) & 1)
        self.w_halo = None
        BN = 128 if self.CoutP % 128 == 0 else (64 if self.CoutP % 64 == 0 else (32 if self.CoutP % 32 == 0 else 0))
        if kT == 1 and kH == 3 and kW == 3 and self.CinP % 16 == 0 and BN:
            nN, nS = self.CoutP // BN, self.CinP // 16
            planes = torch.stack([wh.float(), wl.float()])                      # [2, CoutP, 9 * CinP] (tap-major, channel-minor)
            h = planes.reshape(2, nN, BN, 9, nS, 2, 8).permute(1, 4, 3, 0, 2, 5, 6).contiguous()   # [nN, nS, 9, 2, BN, 2 chunks, 8]
            rot = (torch.arange(BN) >> 3) & 1
            src = torch.arange(2)[None, :] ^ rot[:, None]                       # position s of row n <- chunk s ^ rot(n)
            h = torch.gather(h, 5, src.view(1, 1, 1, 1, BN, 2, 1).expand(nN, nS, 9, 2, BN, 2, 8))
            self.w_halo = h.to(device=device, dtype=bf16).contiguous()


def conv_split(
    x: torch.Tensor, cw: ConvWeightSplit, *, out: Optional[torch.Tensor] = None, stride=(1, 1, 1), pad=(0, 0, 0), out_size=None,
    act: int = L.ACT_NONE, residual: Optional[torch.Tensor] = None, out_f32: bool = False, tile: int = -1,
    residual2: Optional[torch.Tensor] = None, res_row_mod: int = 0, relu_out: bool = False, out_rows: Optional[tuple] = None,
    form_frames: Optional[int] = None,
) -> torch.Tensor:
    """fp32-equivalent convolution (v3a_conv_split).  x: pair [2,T,H,W,CinP] -> pair [2,oT,oH,oW,CoutP] (or f32 [oT,oH,oW,CoutP] with
    out_f32).  residual: an f32 tensor (table; res_row_mod as in `conv`) or a pair; residual2: a pair.  No bf16 rounding anywhere between
    the accumulator and the store; geometry arguments as in `conv`.
    tile: -1 = automatic (the halo-tile form for wide 3x3 layers, else the implicit GEMM with a heuristic tile), >= 0 = that implicit-GEMM
    tile, -2 = force the halo-tile form, -3 = never the halo-tile form.
    form_frames (with tile = -1): choose between the two forms as if the clip had this many frames - a rank that holds a few views of a
    scene takes the form the whole scene would take, so view-sharded results stay bit-identical to the unsharded ones (the two forms
    differ in fp32 summation order)."""
    if x.dim() != 5 or x.shape[0] != 2 or not x.is_contiguous() or x.dtype != bf16 or not x.is_cuda:
        raise ValueError("x must be a contiguous device bf16 pair [2,T,H,W,C]")
    _, T, H, W, Cin = x.shape
    if Cin != cw.CinP:
        raise ValueError(f"x has {Cin} channels, packed weight expects {cw.CinP}")
    kT, kH, kW = cw.k
    if out_size is None:
        if kT > 1 and pad[0] == kT - 1:
            oT = (T + pad[0] - kT) // stride[0] + 1
        else:
            oT = (T + 2 * pad[0] - kT) // stride[0] + 1
        oH = (H + 2 * pad[1] - kH) // stride[1] + 1
        oW = (W + 2 * pad[2] - kW) // stride[2] + 1
    else:
        oT, oH, oW = out_size
    if out is None:
        if out_rows is not None:
            raise ValueError("out_rows needs an explicit out tensor")
        out = torch.empty((oT, oH, oW, cw.CoutP) if out_f32 else (2, oT, oH, oW, cw.CoutP), device=x.device, dtype=f32 if out_f32 else bf16)
    if out_f32:
        if out.dtype != f32:
            raise ValueError("out must be f32")
        o_hi, o_lo = out.view(-1, out.shape[-1]), None
    else:
        if out.dtype != bf16 or out.shape[0] != 2 or not out.is_contiguous():
            raise ValueError("out must be a contiguous bf16 pair")
        o_hi, o_lo = out[0].view(-1, out.shape[-1]), out[1]
    flags = (L.GEMM_RELU_OUT if relu_out else 0) | (L.GEMM_OUT_F32 if out_f32 else 0)
    r_hi = r_lo = None
    ldr = 0
    if residual is not None:
        if residual.dtype == f32:
            flags |= L.GEMM_RES_F32
            r_hi = residual.view(-1, residual.shape[-1])
        else:
            if residual.dtype != bf16 or residual.shape[0] != 2 or not residual.is_contiguous():
                raise ValueError("residual must be f32 or a contiguous bf16 pair")
            r_hi, r_lo = residual[0].view(-1, residual.shape[-1]), residual[1]
        ldr = r_hi.stride(0)
    q_hi = q_lo = None
    if residual2 is not None:
        if residual2.dtype != bf16 or residual2.shape[0] != 2 or not residual2.is_contiguous():
            raise ValueError("residual2 must be a contiguous bf16 pair")
        q_hi, q_lo = residual2[0].view(-1, residual2.shape[-1]), residual2[1]
    cargs = L.ConvArgs(
        _ptr(x[0]), _ptr(cw.w), _ptr(cw.ktab), _ptr(o_hi), _ptr(cw.bias if cw.has_bias else None), _ptr(r_hi), None,
        T, H, W, Cin, oT, oH, oW, cw.CoutP, cw.Kpad,
        stride[0], stride[1], stride[2], pad[0], pad[1], pad[2],
        0, 0, o_hi.stride(0), ldr, act, flags, tile,
        _ptr(q_hi), q_hi.stride(0) if q_hi is not None else 0, res_row_mod,
        *(out_rows if out_rows is not None else (0, 0, 0)),
        _ptr(cw.w_halo), 1 if cw.w_halo is not None else 0,
    )
    args = L.ConvSplitArgs(cargs, _ptr(x[1]), _ptr(o_lo), _ptr(r_lo), _ptr(q_lo))
    if form_frames is not None and tile == -1 and cw.w_halo is not None:
        per_frame = L.load().v3a_conv_split_halo_tiles(C.byref(args)) // T          # 0: the layer has no halo form
        args.c.tile = -2 if per_frame * form_frames >= 128 else -3
    if _meter is not None:
        _meter.add("conv_f32_equivalent", 2.0 * oT * oH * oW * cw.Cout * kT * kH * kW * cw.Cin)
    L.check(L.load().v3a_conv_split(C.byref(args), _stream()), "v3a_conv_split")
    return out


_attn_ws = {}   # per (device, thread) workspace of the key-split attention: stream-ordered reuse within a thread; virtual ranks
                # (seqpar.ThreadWorld: threads sharing one stream) must not share it - their main / merge launches interleave


def attention(
    q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, *,
    B: int, H: int, Nq: int, Nk: int, D: int,
    q_batch_stride: int, k_batch_stride: int, vt_batch_stride: int, o_batch_stride: int,
    scale: Optional[float] = None, kv_period: int = 0, kv_valid: int = 0,
    rel_bias: Optional[torch.Tensor] = None, rel_bias_center: int = 0, key_bias: Optional[torch.Tensor] = None,
    key_bias_first: int = 0, kv_seg: int = 0, k_seg_stride: int = 0, vt_seg_stride: int = 0, kv_split: int = 1,
) -> torch.Tensor:
    """q,k,out: 2-D views [B*N, >=H*D] (row stride = their stride(0)); vt: 2-D [H*D, >=B*vt_batch_stride].
    rel_bias (D=64 only): fp32 [H, n] table, entry (key - query + rel_bias_center) is added to the scaled score.
    key_bias (D=128 only): fp32 [B, >=Nk], added to the scaled score of every query (log-multiplicity of merged keys).
    kv_seg (D=128 only): k / vt are the FIRST of Nk / kv_seg equally laid out segments k_seg_stride / vt_seg_stride elements apart
    (the per-rank slabs of an all-gather), read in place.
    kv_period / kv_valid: key k takes part only if (k % kv_period) < kv_valid (padded per-view token layout); not together with a bias.
    kv_split > 1 (D=128 only): the keys of every query block are divided among kv_split workgroups whose partial softmaxes a second
    launch merges - for launches with too few query blocks to fill the chip; deterministic, not bit-identical to kv_split = 1."""
    ws = None
    if kv_split > 1:
        nbytes = L.load().v3a_attention_split_workspace_bytes(B, H, Nq, D, kv_split)
        wk = (q.device, threading.get_ident())
        ws = _attn_ws.get(wk)
        if ws is None or ws.numel() < nbytes:
            ws = _attn_ws[wk] = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
    if key_bias is not None and (key_bias.dtype != f32 or key_bias.dim() != 2 or key_bias.shape[0] != B or key_bias.stride(1) != 1):
        raise ValueError("key_bias must be fp32 [B, n] with a contiguous last dim")
    if rel_bias is not None and (rel_bias.dtype != f32 or rel_bias.dim() != 2 or rel_bias.shape[0] != H or not rel_bias.is_contiguous()):
        raise ValueError("rel_bias must be contiguous fp32 [H, n]")
    for t, n in ((q, "q"), (k, "k"), (vt, "vt"), (out, "out")):
        _chk2d(t, n, (bf16,))
    args = L.AttnArgs(
        _ptr(q), _ptr(k), _ptr(vt), _ptr(out),
        q_batch_stride, k_batch_stride, vt_batch_stride, o_batch_stride,
        q.stride(0), k.stride(0), vt.stride(0), out.stride(0),
        B, H, Nq, Nk, D, float(scale if scale is not None else D ** -0.5), kv_period, kv_valid,
        _ptr(rel_bias), rel_bias.shape[1] if rel_bias is not None else 0, rel_bias_center,
        _ptr(key_bias), key_bias.stride(0) if key_bias is not None else 0, key_bias_first,
        kv_seg, k_seg_stride, vt_seg_stride, kv_split, _ptr(ws),
    )
    if _meter is not None:
        _meter.add("attention", 4.0 * B * H * Nq * (Nk * kv_valid / kv_period if kv_period > 0 else Nk) * D)
    L.check(L.load().v3a_attention_fwd_bf16(C.byref(args), _stream()), "v3a_attention_fwd_bf16")
    return out


def xattn_probs(
    q: torch.Tensor, k: torch.Tensor, out: torch.Tensor, *, B: int, H: int, Nq: int, Nk: int, Lkp: int,
    q_batch_stride: int, k_batch_stride: int, p_batch_stride: int, scale: Optional[float] = None,
    key_bias: Optional[torch.Tensor] = None, key_bias_first: int = 0, q_row_sumsq: Optional[torch.Tensor] = None, q_eps: float = 1e-6,
) -> torch.Tensor:
    """Normalised cross-attention probabilities over <= 128 per-prompt keys (csrc/xattn_probs.hip, head_dim 128):
    out[b*p_batch_stride/ld + m, h*Lkp + j] = bf16(softmax_j(scale * q_h . k_h[j] + key_bias[b, j])), zeros for Nk <= j < Lkp.
    q, k, out: 2-D bf16 views with row stride stride(0); key_bias fp32 [B, >= Nk] applies to keys >= key_bias_first.
    q_row_sumsq (f32 [B * Nq, parts], ops.gemm row_sumsq of the projection that made q): q is un-normalised; the scores of a query are
    multiplied by rsqrt(sum(parts) / (H * 128) + q_eps), the row factor of the RMS norm across heads (fold its weight into k)."""
    for t, n in ((q, "q"), (k, "k"), (out, "out")):
        _chk2d(t, n, (bf16,))
    if key_bias is not None and (key_bias.dtype != f32 or key_bias.dim() != 2 or key_bias.shape[0] != B or key_bias.stride(1) != 1):
        raise ValueError("key_bias must be fp32 [B, n] with a contiguous last dim")
    if q_row_sumsq is not None and (q_row_sumsq.dtype != f32 or q_row_sumsq.dim() != 2 or not q_row_sumsq.is_contiguous()
                                    or q_row_sumsq.shape[0] < B * Nq or q_batch_stride != Nq * q.stride(0)):
        raise ValueError("q_row_sumsq must be contiguous f32 [B * Nq, parts] over densely stacked batch items of q")
    args = L.XattnProbsArgs(
        _ptr(q), _ptr(k), _ptr(out), _ptr(key_bias), q_batch_stride, k_batch_stride, p_batch_stride,
        q.stride(0), k.stride(0), out.stride(0), B, H, Nq, Nk, 128, Lkp,
        key_bias.stride(0) if key_bias is not None else 0, key_bias_first, float(scale if scale is not None else 128 ** -0.5),
        _ptr(q_row_sumsq), q_row_sumsq.shape[1] if q_row_sumsq is not None else 0, float(q_eps),
    )
    if _meter is not None:
        _meter.add("attention", 2.0 * B * H * Nq * Nk * 128)   # scores only: P.V is the finishing GEMM's
    L.check(L.load().v3a_xattn_probs_bf16(C.byref(args), _stream()), "v3a_xattn_probs_bf16")
    return out


def quantize_fp8(x: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [rows, cols] (row stride = x.stride(0)) -> e4m3 bytes (uint8 storage) of x / scale, RNE, clamped to +-448."""
    _chk2d(x, "x", (bf16,))
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, cols, device=x.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (rows, cols):
        raise ValueError("out must be a uint8 [rows, cols] tensor with a contiguous last dim")
    L.check(L.load().v3a_quantize_fp8(_ptr(x), _ptr(out), rows, cols, x.stride(0), out.stride(0), float(scale), _stream()), "v3a_quantize_fp8")
    return out


def quantize_fp8_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """(e4m3 bytes [rows, cols], f32 [rows]): per-row dynamic quantisation, scale = max(amax, 1e-12) / 448 (v3a_quantize_fp8_rows)."""
    _chk2d(x, "x", (bf16,))
    rows, cols = x.shape
    out = torch.empty((rows, cols), device=x.device, dtype=torch.uint8) if out is None else out
    scale = torch.empty(rows, device=x.device, dtype=f32) if scale is None else scale
    if out.dtype not in (torch.uint8, torch.float8_e4m3fn) or out.stride(1) != 1 or scale.dtype != f32 or not scale.is_contiguous() or scale.numel() != rows:
        raise ValueError("out must be bytes with unit inner stride, scale contiguous f32 [rows]")
    L.check(L.load().v3a_quantize_fp8_rows(_ptr(x), _ptr(out), _ptr(scale), rows, cols, x.stride(0), out.stride(0), _stream()), "v3a_quantize_fp8_rows")
    return out, scale


def attention_fp8(q8: torch.Tensor, k8: torch.Tensor, vt8: torch.Tensor, out: torch.Tensor, *, B: int, H: int, Nq: int, Nk: int,
                  q_batch_stride: int, k_batch_stride: int, vt_batch_stride: int, o_batch_stride: int, scale: Optional[float] = None,
                  q_scale: float = 1.0, k_scale: float = 1.0, v_scale: float = 1.0, kv_seg: int = 0, k_seg_stride: int = 0,
                  vt_seg_stride: int = 0, kv_split: int = 1) -> torch.Tensor:
    """fp8 (e4m3) flash attention, head dim 128: q8/k8 uint8 [B*N, >=H*128], vt8 uint8 [H*128, >=B*vt_batch_stride], out bf16.
    kv_seg / k_seg_stride / vt_seg_stride (bytes) and kv_split as in `attention`."""
    for t, n in ((q8, "q8"), (k8, "k8"), (vt8, "vt8")):
        _chk2d(t, n, (torch.uint8,))
    _chk2d(out, "out", (bf16,))
    ws = None
    if kv_split > 1:
        nbytes = L.load().v3a_attention_split_workspace_bytes(B, H, Nq, 128, kv_split)
        wk = (q8.device, threading.get_ident())
        ws = _attn_ws.get(wk)
        if ws is None or ws.numel() < nbytes:
            ws = _attn_ws[wk] = torch.empty(nbytes, device=q8.device, dtype=torch.uint8)
    args = L.AttnFp8Args(_ptr(q8), _ptr(k8), _ptr(vt8), _ptr(out), q_batch_stride, k_batch_stride, vt_batch_stride, o_batch_stride,
                         q8.stride(0), k8.stride(0), vt8.stride(0), out.stride(0), B, H, Nq, Nk, 128,
                         float(scale if scale is not None else 128 ** -0.5), float(q_scale), float(k_scale), float(v_scale),
                         kv_seg, k_seg_stride, vt_seg_stride, kv_split, _ptr(ws))
    if _meter is not None:
        _meter.add("attention_fp8", 4.0 * B * H * Nq * Nk * 128)
    L.check(L.load().v3a_attention_fwd_fp8(C.byref(args), _stream()), "v3a_attention_fwd_fp8")
    return out


def layernorm(
    x: torch.Tensor, *, out: Optional[torch.Tensor] = None,
    weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
    scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
    rows_per_batch: int = 0, eps: float = 1e-6, out_dtype: torch.dtype = bf16,
    M: Optional[int] = None, in_rows: tuple = (0, 0, 0), out_rows: tuple = (0, 0, 0), rms: bool = False,
    fp8_scale: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """in_rows/out_rows = (group, skip, off): logical row m maps to physical row m + (m//group)*skip + off.
    rms=True: no mean subtraction (T5LayerNorm).
    fp8_scale (f32 [rows of out]): `out` is e4m3 bytes, the per-row quantisation (ops.quantize_fp8_rows) of the bf16 result."""
    _chk2d(x, "x", (bf16, f32))
    d = x.shape[1]
    if M is None:
        M = x.shape[0]
    if out is None:
        out = torch.empty((M, d), device=x.device, dtype=out_dtype)
    if fp8_scale is not None:
        _chk2d(out, "out", (torch.uint8, torch.float8_e4m3fn))
        if fp8_scale.dtype != f32 or not fp8_scale.is_contiguous() or fp8_scale.numel() < out.shape[0]:
            raise ValueError("fp8_scale must be contiguous f32 with one entry per output row")
    else:
        _chk2d(out, "out", (bf16, f32))
    mstride = 0
    if scale is not None:
        if scale.dtype != f32 or shift is None or shift.dtype != f32 or scale.dim() != 2 or shift.dim() != 2:
            raise ValueError("scale/shift must both be 2-D f32")
        if scale.stride(0) != shift.stride(0) or scale.stride(1) != 1 or shift.stride(1) != 1:
            raise ValueError("scale/shift must share a row stride and be contiguous in the last dim")
        mstride = scale.stride(0)
    for t in (weight, bias):
        if t is not None and (t.dtype != f32 or not t.is_contiguous()):
            raise ValueError("affine weight/bias must be contiguous f32")
    args = L.LayerNormArgs(
        _ptr(x), _ptr(out), _ptr(weight), _ptr(bias), _ptr(scale), _ptr(shift),
        M, d, x.stride(0), out.stride(0), rows_per_batch, mstride, eps,
        int(x.dtype == f32), int(out.dtype == f32), *in_rows, *out_rows, int(rms), _ptr(fp8_scale),
    )
    L.check(L.load().v3a_layernorm(C.byref(args), _stream()), "v3a_layernorm")
    return out


def rmsnorm_rope(
    x: torch.Tensor, weight: torch.Tensor, *, out: Optional[torch.Tensor] = None,
    rope: Optional[torch.Tensor] = None, head_dim: int = 0, tokens_per_batch: int = 0, eps: float = 1e-6,
    weight2: Optional[torch.Tensor] = None, fp8_scale: float = 0.0,
) -> torch.Tensor:
    """weight2: x is [M, 2d] = [q | k] of a fused projection; both halves are normalised (q with weight, k with weight2) in one launch.
    fp8_scale > 0: `out` (required, uint8, same shape) receives e4m3(bf16(result) / fp8_scale) - the fp8 attention's operand format."""
    _chk2d(x, "x", (bf16,))
    M, d = x.shape
    if weight2 is not None:
        if d % 2 or weight2.dtype != f32 or not weight2.is_contiguous() or weight2.numel() != d // 2:
            raise ValueError("weight2 must be contiguous f32 [d] for x [M, 2d]")
        d //= 2
    if out is None:
        out = torch.empty(tuple(x.shape), device=x.device, dtype=torch.uint8 if fp8_scale > 0 else bf16)
    _chk2d(out, "out", (torch.uint8, torch.float8_e4m3fn) if fp8_scale > 0 else (bf16,))
    if tuple(out.shape) != tuple(x.shape):
        raise ValueError("out must have the shape of x")
    if weight.dtype != f32 or not weight.is_contiguous() or weight.numel() != d:
        raise ValueError("weight must be contiguous f32 [d]")
    if rope is not None and (rope.dtype != f32 or not rope.is_contiguous()):
        raise ValueError("rope table must be contiguous f32 [tokens, head_dim/2, 2]")
    args = L.RmsNormRopeArgs(
        _ptr(x), _ptr(out), _ptr(weight), _ptr(rope), M, d, x.stride(0), out.stride(0),
        head_dim, tokens_per_batch, eps, _ptr(weight2), float(fp8_scale),
    )
    L.check(L.load().v3a_rmsnorm_rope(C.byref(args), _stream()), "v3a_rmsnorm_rope")
    return out


def rownorm_act(x: torch.Tensor, weight: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, mode: int = 1, act: int = L.ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    """Channel norm (+SiLU) over the last dim of a channels-last bf16 tensor (any leading dims, contiguous)."""
    if x.dtype != bf16 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be contiguous device bf16")
    d = x.shape[-1]
    M = x.numel() // d
    if out is None:
        out = torch.empty_like(x)
    if weight.dtype != f32 or weight.numel() != d or not weight.is_contiguous():
        raise ValueError("weight must be contiguous f32 [d]")
    args = L.RowNormArgs(_ptr(x), _ptr(out), _ptr(weight), _ptr(bias), M, d, d, d, eps, mode, act)
    L.check(L.load().v3a_rownorm_act(C.byref(args), _stream()), "v3a_rownorm_act")
    return out


def softmax_rows(s: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk2d(s, "s", (f32,))
    M, N = s.shape
    if out is None:
        out = torch.empty((M, N), device=s.device, dtype=bf16)
    _chk2d(out, "out", (bf16,))
    L.check(L.load().v3a_softmax_rows(_ptr(s), _ptr(out), M, N, s.stride(0), out.stride(0), float(scale), _stream()),
            "v3a_softmax_rows")
    return out


def qknorm_rope2d(qk: torch.Tensor, C: int, qw, qb, kw, kb, cos_sin: Optional[torch.Tensor], rows_per_frame: int,
                  n_special: int, n_valid: int, wp: int, eps: float = 1e-5) -> torch.Tensor:
    _chk2d(qk, "qk", (bf16,))
    L.check(L.load().v3a_qknorm_rope2d(_ptr(qk), qk.shape[0], qk.stride(0), C, _ptr(qw), _ptr(qb), _ptr(kw), _ptr(kb),
                                       _ptr(cos_sin), rows_per_frame, n_special, n_valid, wp, eps, _stream()), "v3a_qknorm_rope2d")
    return qk


def latent_upsample_t_cl(z: torch.Tensor) -> torch.Tensor:
    """z [C,Tl,H,W] f32 contiguous -> [4(Tl-1)+1,H,W,C] bf16."""
    if z.dtype != f32 or not z.is_contiguous() or z.dim() != 4:
        raise ValueError("z must be contiguous f32 [C,Tl,H,W]")
    Cc, Tl, H, W = z.shape
    out = torch.empty(((Tl - 1) * 4 + 1, H, W, Cc), device=z.device, dtype=bf16)
    L.check(L.load().v3a_latent_upsample_t_cl(_ptr(z), _ptr(out), Cc, Tl, H, W, _stream()), "v3a_latent_upsample_t_cl")
    return out


def bilinear_cl(x: torch.Tensor, size, *, align_corners: bool, add: Optional[torch.Tensor] = None,
                table: Optional[torch.Tensor] = None, relu: bool = False, out_f32: bool = False) -> torch.Tensor:
    if x.dtype != bf16 or not x.is_contiguous() or x.dim() != 4:
        raise ValueError("x must be contiguous bf16 [T,h,w,C]")
    T, h, w, Cc = x.shape
    H, W = size
    out = torch.empty((T, H, W, Cc), device=x.device, dtype=f32 if out_f32 else bf16)
    if add is not None and (add.dtype != bf16 or not add.is_contiguous() or add.numel() != out.numel()):
        raise ValueError("add must be contiguous bf16 with the output's shape")
    if table is not None and (table.dtype != f32 or not table.is_contiguous() or table.numel() != H * W * Cc):
        raise ValueError("table must be contiguous f32 [H*W, C]")
    L.check(L.load().v3a_bilinear_cl(_ptr(x), _ptr(out), _ptr(add), _ptr(table), T, h, w, H, W, Cc, int(align_corners), int(relu),
                                     int(out_f32), _stream()), "v3a_bilinear_cl")
    return out


def depth_unproject(raw: torch.Tensor, cam: torch.Tensor, S: int, H: int, W: int):
    """raw [S*H*W, ld] f32, cam [S,16] f32 -> depth [S,H,W], conf [S,H,W], pts [S,H,W,3] (all f32)."""
    _chk2d(raw, "raw", (f32,))
    dev = raw.device
    depth = torch.empty(S, H, W, device=dev, dtype=f32)
    conf = torch.empty(S, H, W, device=dev, dtype=f32)
    pts = torch.empty(S, H, W, 3, device=dev, dtype=f32)
    L.check(L.load().v3a_depth_unproject(_ptr(raw), raw.stride(0), _ptr(cam.contiguous()), _ptr(depth), _ptr(conf), _ptr(pts), S, H, W,
                                         _stream()), "v3a_depth_unproject")
    return depth, conf, pts


def voxelize_fuse(pts: torch.Tensor, feat: torch.Tensor, nfeat: int, conf_col: int, voxel_size: float):
    """pts [M,3] f32, feat [M,ld] f32 -> dict(voxel_pts [U,3], voxel_feat [U,nfeat], keys [U,3] i32, inverse [M] i32, counts [U] i32)."""
    _chk2d(pts, "pts", (f32,))
    _chk2d(feat, "feat", (f32,))
    M, dev = pts.shape[0], pts.device
    lib = L.load()
    ws = torch.empty(int(lib.v3a_voxelize_workspace_bytes(M)), device=dev, dtype=torch.uint8)
    keys = torch.empty(M, 3, device=dev, dtype=torch.int32)
    inv = torch.empty(M, device=dev, dtype=torch.int32)
    cnt = torch.empty(M, device=dev, dtype=torch.int32)
    vp = torch.empty(M, 3, device=dev, dtype=f32)
    vf = torch.empty(M, nfeat, device=dev, dtype=f32)
    meta = torch.zeros(2, device=dev, dtype=torch.int32)
    L.check(lib.v3a_voxelize_fuse(_ptr(pts.contiguous()), _ptr(feat), feat.stride(0), nfeat, conf_col, M, float(voxel_size), _ptr(ws), ws.numel(),
                                  _ptr(keys), _ptr(inv), _ptr(cnt), _ptr(vp), _ptr(vf), nfeat, C.c_void_p(meta.data_ptr()),
                                  C.c_void_p(meta.data_ptr() + 4), _stream()), "v3a_voxelize_fuse")
    U, bad = (int(v) for v in meta.tolist())  # one host sync: the Gaussian count sizes every downstream tensor
    if bad:
        raise RuntimeError("voxel coordinate outside [-2^20, 2^20): points too far for the 63-bit key")
    return dict(voxel_pts=vp[:U], voxel_feat=vf[:U], keys=keys[:U], inverse=inv, counts=cnt[:U])


def conf_quantile_compact(conf: torch.Tensor, q: float, pts: torch.Tensor, feat: torch.Tensor, nfeat: int):
    """rows of (pts [M,3], feat[:, :nfeat]) whose confidence exceeds torch.quantile(conf, q), in row-major order ->
    dict(pts [K,3], feat [K,nfeat], threshold (0-dim f32)).  anysplat_stitched.py:381-387, 441-446."""
    _chk2d(pts, "pts", (f32,))
    _chk2d(feat, "feat", (f32,))
    if conf.dtype != f32 or not conf.is_contiguous() or conf.numel() != pts.shape[0]:
        raise ValueError("conf must be contiguous f32 with one value per row")
    M, dev = pts.shape[0], pts.device
    lib = L.load()
    ws = torch.empty(int(lib.v3a_conf_compact_workspace_bytes(M)), device=dev, dtype=torch.uint8)
    op, of = torch.empty(M, 3, device=dev, dtype=f32), torch.empty(M, nfeat, device=dev, dtype=f32)
    thr = torch.empty((), device=dev, dtype=f32)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    L.check(lib.v3a_conf_quantile_compact(_ptr(conf), float(q), _ptr(pts.contiguous()), _ptr(feat), feat.stride(0), nfeat, M, _ptr(ws), ws.numel(),
                                          _ptr(thr), _ptr(op), _ptr(of), nfeat, _ptr(cnt), _stream()), "v3a_conf_quantile_compact")
    K = int(cnt.item())  # one host sync: the Gaussian count sizes every downstream tensor
    return dict(pts=op[:K], feat=of[:K], threshold=thr)


def gaussian_adapter(pts: torch.Tensor, feats: torch.Tensor, sh_mask: torch.Tensor, sh_degree: int = 4, opacity_exponent: float = 1.0):
    _chk2d(feats, "feats", (f32,))
    U, dev, dsh = feats.shape[0], feats.device, (sh_degree + 1) ** 2
    e = lambda *s: torch.empty(*s, device=dev, dtype=f32)
    means, cov, sh, op, sc, rot = e(U, 3), e(U, 3, 3), e(U, 3, dsh), e(U), e(U, 3), e(U, 4)
    L.check(L.load().v3a_gaussian_adapter(_ptr(pts.contiguous()), _ptr(feats), feats.stride(0), U, sh_degree, float(opacity_exponent),
                                          _ptr(sh_mask), _ptr(means), _ptr(cov), _ptr(sh), _ptr(op), _ptr(sc), _ptr(rot), _stream()),
            "v3a_gaussian_adapter")
    return dict(means=means, covariances=cov, harmonics=sh, opacities=op, scales=sc, rotations=rot)


def linear_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: int = L.ACT_NONE,
               residual: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk2d(x, "x", (f32,))
    _chk2d(w, "w", (f32,))
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=f32)
    if _meter is not None:
        _meter.add("linear_f32", 2.0 * M * N * K)
    L.check(L.load().v3a_linear_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), _ptr(residual), _ptr(gamma), M, N, K, x.stride(0), N,
                                    residual.stride(0) if residual is not None else 0, act, _stream()), "v3a_linear_f32")
    return y


def attention_small_f32(qkv: torch.Tensor, H: int) -> torch.Tensor:
    _chk2d(qkv, "qkv", (f32,))
    S, C3 = qkv.shape
    Cc = C3 // 3
    out = torch.empty(S, Cc, device=qkv.device, dtype=f32)
    hd = Cc // H
    L.check(L.load().v3a_attention_small_f32(_ptr(qkv.contiguous()), _ptr(out), S, H, hd, hd ** -0.5, _stream()), "v3a_attention_small_f32")
    return out


def unipc_cfg_step(dit_out: torch.Tensor, tok: Optional[torch.Tensor], sample: torch.Tensor, last_sample: Optional[torch.Tensor],
                   m_prev1: Optional[torch.Tensor], m_prev2: Optional[torch.Tensor], m_out: torch.Tensor, sample_corrected: torch.Tensor,
                   prev: torch.Tensor, *, batch: int, guidance: Optional[float], coeffs: dict) -> None:
    """One launch for unpatchify + CFG + UniPC step + next-step patchify (csrc/denoise_step.hip).  `coeffs` = the host scalars of
    `UniPCMultistepScheduler.plan_step()`; latents [1, C, T, H, W] fp32, token buffers as WanDiT keeps them."""
    if sample.dtype != f32 or not sample.is_contiguous() or sample.dim() != 5 or sample.shape[0] != 1:
        raise ValueError("sample must be contiguous f32 [1, C, T, H, W]")
    _, Cc, T, H, W = sample.shape
    N = T * (H // 2) * (W // 2)
    if batch not in (1, 2) or (guidance is not None and batch != 2):
        raise ValueError("batch must be 1 or 2, and 2 (cond | uncond row blocks) when guidance is given")
    for name, t_ in (("dit_out", dit_out), ("tok", tok), ("last_sample", last_sample), ("m_prev1", m_prev1), ("m_prev2", m_prev2),
                     ("m_out", m_out), ("sample_corrected", sample_corrected), ("prev", prev)):
        if t_ is not None and t_.device != sample.device:
            raise ValueError(f"{name} is on {t_.device}, the latents on {sample.device}")
    for name, t_ in (("m_out", m_out), ("sample_corrected", sample_corrected), ("prev", prev), ("last_sample", last_sample),
                     ("m_prev1", m_prev1), ("m_prev2", m_prev2)):
        if t_ is not None and (t_.dtype != f32 or not t_.is_contiguous() or t_.numel() != sample.numel()):
            raise ValueError(f"{name} must be contiguous f32 with the latents' shape")
    for name, t_ in (("dit_out", dit_out), ("tok", tok)):
        if t_ is not None and (t_.dtype != bf16 or not t_.is_contiguous() or t_.shape != (batch * N, 4 * Cc)):
            raise ValueError(f"{name} must be contiguous bf16 [{batch * N}, {4 * Cc}]")
    c = coeffs
    a = L.UniPCStepArgs(_ptr(dit_out), _ptr(tok), _ptr(sample), _ptr(last_sample), _ptr(m_prev1), _ptr(m_prev2), _ptr(m_out),
                        _ptr(sample_corrected), _ptr(prev), Cc, T, H, W, batch, int(guidance is not None), float(guidance or 0.0), c["sigma"],
                        c["corr_order"], c["cc1"], c["cc2"], c["cc3"], c["c_rho_last"], c["c_rho0"], c["c_inv_rk"],
                        c["pred_order"], c["pc1"], c["pc2"], c["pc3"], c["p_rho0"], c["p_inv_rk"])
    L.check(L.load().v3a_unipc_cfg_step(C.byref(a), _stream()), "v3a_unipc_cfg_step")


# ------------------------------------------------------------------------------------------------ 3DGS rasteriser
def _gs_scene_args(means, covars, sh, viewmat, campos, K, sh_layout):
    """What gs_project and gs_project_backward check of their tensors -> (cameras, Gaussians, sh_k)."""
    for t, n in ((means, "means"), (covars, "covars"), (sh, "sh"), (viewmat, "viewmat"), (campos, "campos"), (K, "K")):
        if t.dtype != f32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{n}: contiguous fp32 device tensor required")
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
    if opacities.dtype != f32 or not opacities.is_contiguous():
        raise ValueError("opacities: contiguous fp32 [U] required")
    if U == 0:
        raise ValueError("no Gaussians to draw")
    single = proj["radii"].dim() == 1
    Cn = 1 if single else proj["radii"].shape[0]
    lead = () if single else (Cn,)
    comp = proj.get("compensations")
    if comp is not None:
        _gs_f32(comp, "compensations", Cn * U)
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


def _gs_f32(t: torch.Tensor, name: str, numel: int) -> None:
    if t.dtype != f32 or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{name}: contiguous fp32 device tensor of {numel} elements required, got {t.dtype} {tuple(t.shape)}")


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
    _gs_f32(opacities, "opacities", U)
    for k, n in (("means2d", 2), ("conics", 3), ("colors", 4)):
        _gs_f32(proj[k], k, Cn * U * n)
    if proj["radii"].dtype != torch.int32 or not proj["radii"].is_contiguous() or proj["radii"].numel() != Cn * U:
        raise ValueError("radii: contiguous int32 [C,U] required")
    _gs_f32(d_color, "d_color", Cn * height * width * 3)
    _gs_f32(d_depth, "d_depth", Cn * height * width)
    _gs_f32(d_alpha, "d_alpha", Cn * height * width)
    if background is not None:
        _gs_f32(background, "background", 3)
    comp = proj.get("compensations")
    if comp is not None:
        _gs_f32(comp, "compensations", Cn * U)
    if tile_offsets.dtype != torch.int32 or not tile_offsets.is_contiguous() or tile_offsets.numel() != Cn * ntiles + 1:
        raise ValueError(f"tile_offsets: contiguous int32 [{Cn * ntiles + 1}] required")
    if flatten_ids.dtype != torch.int32 or not flatten_ids.is_contiguous():
        raise ValueError("flatten_ids: contiguous int32 required")
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
        _gs_f32(opacities, "opacities", U)
    if covars.numel() != 9 * U or sh.numel() != 3 * sh_k * U:
        raise ValueError("means / covars / sh disagree on the number of Gaussians")
    if radii.dtype != torch.int32 or not radii.is_contiguous() or radii.numel() != Cn * U:
        raise ValueError("radii: contiguous int32 [C,U] required")
    for k, n in (("d_means2d", 2), ("d_conics", 3), ("d_colors", 4), ("d_opacity", 1)):
        _gs_f32(entry_grads[k], k, Cn * U * n)
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
        if ctx.camera_grad:
            d_means, d_covars, d_sh, d_op, d_view, d_campos = gs_project_backward(
                means, covars, sh, viewmat, campos, K, width, height, radii, eg, sh_degree=sh_degree, sh_layout=sh_layout,
                rasterize_mode=rasterize_mode, opacities=opacities if comp else None, camera_grad=True)
            return (d_means, d_covars, d_sh, d_op, d_view, d_campos) + (None,) * 13
        d_means, d_covars, d_sh, d_op = gs_project_backward(means, covars, sh, viewmat, campos, K, width, height, radii, eg,
                                                            sh_degree=sh_degree, sh_layout=sh_layout, rasterize_mode=rasterize_mode,
                                                            opacities=opacities if comp else None)
        return (d_means, d_covars, d_sh, d_op) + (None,) * 15


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
        if t.dtype != f32 or not t.is_cuda or not t.is_contiguous() or t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
            raise ValueError(f"camera_adjust: {n} must be a contiguous fp32 device tensor [V,{','.join(map(str, shape))}], got {t.dtype} "
                             f"{tuple(t.shape)}")
    if not (w2c_base.shape[0] == c2w_base.shape[0] == deltas.shape[0]) or deltas.shape[0] < 1:
        raise ValueError(f"camera_adjust: w2c_base, c2w_base and deltas disagree on the number of cameras: {w2c_base.shape[0]}, "
                         f"{c2w_base.shape[0]}, {deltas.shape[0]}")
    for t, n in ((w2c_base, "w2c_base"), (c2w_base, "c2w_base")):
        if t.requires_grad:
            raise NotImplementedError(f"camera_adjust: no gradient for {n} (the base cameras are constants; the deltas train)")
    return _CameraAdjust.apply(w2c_base, c2w_base, deltas)


def image_metrics(a_u8: torch.Tensor, b_u8: torch.Tensor):
    """SSIM and MSE of N uint8 image pairs [N,H,W,C] (PNG byte order; pixels scored as u8 / 255) in one call
    (csrc/image_metrics.hip).  -> (ssim [N] f64, mse [N] f64) on the device; PSNR = -10 log10(mse) is the caller's."""
    for name, t in (("a_u8", a_u8), ("b_u8", b_u8)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
        if t.dtype != torch.uint8 or t.dim() != 4 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint8 [N,H,W,C] tensor, got {t.dtype} {tuple(t.shape)}")
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
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
        if t.dtype not in (torch.uint8, f32) or t.dim() != 4 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint8 [N,H,W,3] or f32 [N,3,H,W] tensor, got {t.dtype} {tuple(t.shape)}")
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
    if x.dim() != 5 or x.shape[0] != 2 or not x.is_contiguous() or x.dtype != bf16 or not x.is_cuda:
        raise ValueError("x must be a contiguous device bf16 pair [2,F,H,W,C]")
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
def _dev(t: torch.Tensor, name: str, dtype, dim: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous() or (dim is not None and t.dim() != dim):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor" + (f" of {dim} dimensions" if dim else "")
                         + f", got {t.dtype} {tuple(t.shape)}")


def clip_preprocess(frames: torch.Tensor, tables: dict, lut: torch.Tensor, image_size: int, patch: int, *, want_u8: bool = False,
                    want_f32: bool = False):
    """CLIPImageProcessor (Pillow BICUBIC shorter-edge resize, centre crop, rescale, normalise) + patchify for uint8 frames [N,H,W,3].
    tables: device int32 tensors of evaluation.clip.resize_tables(H, W, image_size) - x_bounds / y_bounds [S,2], x_coeffs / y_coeffs
    [S,k] - and the ints row0, rows; lut: f32 [3,256].  -> (patch pair [2, N (S/P)^2, ldk], uint8 crop [N,S,S,3] or None, f32 pixel
    values [N,3,S,S] or None)."""
    _dev(frames, "frames", torch.uint8, 4)
    N, H, W, Cc = frames.shape
    S, P = image_size, patch
    if Cc != 3:
        raise ValueError(f"frames must be RGB [N,H,W,3], got {tuple(frames.shape)}")
    if S % P:
        raise ValueError(f"image_size {S} is not a multiple of the patch size {P}")
    _dev(lut, "lut", f32)
    if lut.numel() != 768:
        raise ValueError("lut must be f32 [3,256]")
    for key in ("x_bounds", "y_bounds", "x_coeffs", "y_coeffs"):
        _dev(tables[key], key, torch.int32, 2)
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
    _dev(src, "src", f32, 2)
    d = src.shape[1]
    if d % 4:
        raise ValueError("row width must be a multiple of 4")
    if ids is not None:
        _dev(ids, "ids", torch.int32)
        M = ids.numel()
    elif cls is not None:
        _dev(cls, "cls", f32)
        if cls.numel() != d or S < 2 or src.shape[0] % (S - 1):
            raise ValueError(f"cls must be f32 [{d}] and src hold whole sequences of {S - 1} patch rows")
        M = src.shape[0] // (S - 1) * S
    elif M is None:
        M = src.shape[0]
    if pos is not None:
        _dev(pos, "pos", f32, 2)
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
        _dev(lens, "lens", torch.int32)
        if lens.numel() != B:
            raise ValueError(f"lens must be int32 [{B}]")
    d = H * head_dim
    out = torch.empty((B * S, d) if out_f32 else (2, B * S, d), device=q.device, dtype=f32 if out_f32 else bf16)
    sc = head_dim ** -0.5 if scale is None else scale
    L.check(L.load().v3a_attention_f32(_ptr(q), _ptr(k), _ptr(v), q.stride(0), None if out_f32 else _ptr(out[0]),
                                       None if out_f32 else _ptr(out[1]), _ptr(out) if out_f32 else None, d, _ptr(lens), B, S, H, head_dim,
                                       sc, int(causal), _stream()), "v3a_attention_f32")
    return out


def clip_score(image_emb: torch.Tensor, text_emb: torch.Tensor):
    """-> (scores f64 [F] = max(100 cos(image_emb[f], text_emb), 0), their mean f64 [1]); fp64 on the device, fixed summation order"""
    _dev(image_emb, "image_emb", f32, 2)
    _dev(text_emb, "text_emb", f32)
    F, D = image_emb.shape
    if text_emb.numel() != D:
        raise ValueError(f"text_emb must hold {D} values, got {tuple(text_emb.shape)}")
    scores = torch.empty(F, device=image_emb.device, dtype=torch.float64)
    mean = torch.empty(1, device=image_emb.device, dtype=torch.float64)
    L.check(L.load().v3a_clip_score(_ptr(image_emb), _ptr(text_emb), F, D, _ptr(scores), _ptr(mean), _stream()), "v3a_clip_score")
    return scores, mean


# ------------------------------------------------------------------------------------------------ post-optimisation (csrc/ssim_loss.hip, csrc/post_opt.hip)
def _f32_dev(t: torch.Tensor, name: str, shape=None) -> None:
    if not t.is_cuda or t.dtype != f32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 device tensor, got {t.dtype} on {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, ssim_lambda):
        N, H, W, Cc = pred.shape
        lib = L.load()
        dev = pred.device
        ws, ws_bytes = _workspace(lib.v3a_photometric_loss_workspace_bytes(N, H, W, Cc),
                                  f"v3a_photometric_loss_workspace_bytes (shape {tuple(pred.shape)}; H, W >= 11 and C <= 4 required)", dev)
        planes = None
        if ctx.needs_input_grad[0]:
            planes = torch.empty(int(lib.v3a_photometric_loss_planes_bytes(N, H, W, Cc)) // 8, device=dev, dtype=torch.float64)
        out = torch.empty(3, device=dev, dtype=torch.float64)
        args = L.PhotometricLossArgs(_ptr(pred), _ptr(target), N, H, W, Cc, float(ssim_lambda), _ptr(out), _ptr(ws), ws_bytes,
                                     _ptr(planes), planes.numel() * 8 if planes is not None else 0)
        L.check(lib.v3a_photometric_loss_forward(C.byref(args), _stream()), "v3a_photometric_loss_forward")
        if planes is not None:
            ctx.save_for_backward(pred, target, planes)
        ctx.ssim_lambda = float(ssim_lambda)
        return out[0], out[1], out[2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, d_l1, d_ssim):
        pred, target, planes = ctx.saved_tensors
        N, H, W, Cc = pred.shape
        z = torch.zeros((), device=pred.device, dtype=torch.float64)
        d_out = torch.stack([z if g is None else g.to(torch.float64).reshape(()) for g in (d_loss, d_l1, d_ssim)])
        d_pred = torch.empty_like(pred)
        args = L.PhotometricLossArgs(_ptr(pred), _ptr(target), N, H, W, Cc, ctx.ssim_lambda, None, None, 0, _ptr(planes), planes.numel() * 8)
        L.check(L.load().v3a_photometric_loss_backward(C.byref(args), _ptr(d_out), _ptr(d_pred), _stream()), "v3a_photometric_loss_backward")
        return d_pred, None, None


def photometric_loss(pred: torch.Tensor, target: torch.Tensor, ssim_lambda: float = 0.2):
    """(1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM) of f32 images [N,H,W,C] (C <= 4, H, W >= 11; the layout gs_render emits),
    SSIM as the reference's loss_ssim.py::ssim(data_range=1.0) on the valid map = fused_ssim(padding="valid") (csrc/ssim_loss.hip).
    -> (loss, l1, ssim): float64 scalars on the device, differentiable with respect to `pred` (HIP backward, first order only).
    `target` is a constant: one that requires grad is refused."""
    if target.requires_grad:
        raise NotImplementedError("photometric_loss: no gradient for target (it is a constant of the loss); detach it")
    if pred.dim() != 4:
        raise ValueError(f"photometric_loss: pred must be [N,H,W,C], got {tuple(pred.shape)}")
    _f32_dev(pred, "pred")
    _f32_dev(target, "target", pred.shape)
    return _PhotometricLoss.apply(pred, target, float(ssim_lambda))


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, depth_gt, mask, scale):
        Cc, H, W = depth.shape
        lib = L.load()
        dev = depth.device
        ws, ws_bytes = _workspace(lib.v3a_depth_loss_workspace_bytes(Cc, H, W), f"v3a_depth_loss_workspace_bytes (shape {tuple(depth.shape)})", dev)
        out = torch.empty(2, device=dev, dtype=torch.float64)
        args = L.DepthLossArgs(_ptr(depth), _ptr(alpha), _ptr(depth_gt), _ptr(mask), Cc, H, W, float(scale), _ptr(out), _ptr(ws), ws_bytes)
        L.check(lib.v3a_depth_loss_forward(C.byref(args), _stream()), "v3a_depth_loss_forward")
        ctx.save_for_backward(depth, alpha, depth_gt, mask, out)
        ctx.scale = float(scale)
        loss, count = out[0], out[1]
        ctx.mark_non_differentiable(count)
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, _d_count):
        depth, alpha, depth_gt, mask, out = ctx.saved_tensors
        Cc, H, W = depth.shape
        d_out = d_loss.to(torch.float64).reshape(1).contiguous()
        d_depth, d_alpha = torch.empty_like(depth), torch.empty_like(alpha)
        args = L.DepthLossArgs(_ptr(depth), _ptr(alpha), _ptr(depth_gt), _ptr(mask), Cc, H, W, ctx.scale, _ptr(out), None, 0)
        L.check(L.load().v3a_depth_loss_backward(C.byref(args), _ptr(d_out), _ptr(d_depth), _ptr(d_alpha), _stream()), "v3a_depth_loss_backward")
        return d_depth, d_alpha, None, None, None


def depth_loss(depth: torch.Tensor, alpha: torch.Tensor, depth_gt: torch.Tensor, mask: Optional[torch.Tensor] = None, scale: float = 1.0):
    """The reference loop's depth term (simple_trainer.py:943-961) on dense maps (csrc/depth_loss.hip): `depth`, `alpha` f32 [C,H,W]
    as gs_render returns them (depth = the alpha-weighted z), `depth_gt` f32 [C,H,W], `mask` bool / uint8 [C,H,W] (nonzero = use the
    pixel) or None.  loss = scale * mean over the used pixels of |disp - 1 / depth_gt|, disp = 1 / E where E = depth /
    max(alpha, 1e-10) > 0, else 0; a pixel is used where the mask is set and depth_gt is positive and finite.
    -> (loss, count): float64 scalars on the device, count = the number of used pixels (0 gives loss 0 and zero gradients).
    Differentiable with respect to `depth` and `alpha` (HIP backward, first order only); `depth_gt` and `mask` are constants."""
    if depth_gt.requires_grad or (mask is not None and mask.requires_grad):
        raise NotImplementedError("depth_loss: no gradient for depth_gt / mask (they are constants of the loss); detach them")
    if depth.dim() != 3:
        raise ValueError(f"depth_loss: depth must be [C,H,W], got {tuple(depth.shape)}")
    _f32_dev(depth, "depth")
    _f32_dev(alpha, "alpha", depth.shape)
    _f32_dev(depth_gt, "depth_gt", depth.shape)
    if mask is not None:
        if not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8) or not mask.is_contiguous() or mask.shape != depth.shape:
            raise ValueError(f"mask must be a contiguous bool or uint8 device tensor of shape {tuple(depth.shape)}, got {mask.dtype} "
                             f"{tuple(mask.shape)} on {mask.device}")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)   # the same bytes (a bool is stored as 0 / 1), no copy
    return _DepthLoss.apply(depth, alpha, depth_gt, mask, float(scale))


class _BilagridSlice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, grids):
        N, H, W, _ = rgb.shape
        _, Lz, GY, GX, _ = grids.shape
        out = torch.empty_like(rgb)
        args = L.BilagridSliceArgs(_ptr(rgb), _ptr(grids), N, H, W, GX, GY, Lz)
        L.check(L.load().v3a_bilagrid_slice_forward(C.byref(args), _ptr(out), _stream()),
                f"v3a_bilagrid_slice_forward (rgb {tuple(rgb.shape)}, grids {tuple(grids.shape)})")
        ctx.save_for_backward(rgb, grids)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        rgb, grids = ctx.saved_tensors
        N, H, W, _ = rgb.shape
        _, Lz, GY, GX, _ = grids.shape
        d_out = d_out.float().contiguous()
        d_rgb = torch.empty_like(rgb) if ctx.needs_input_grad[0] else None
        d_grids = torch.empty_like(grids) if ctx.needs_input_grad[1] else None
        args = L.BilagridSliceArgs(_ptr(rgb), _ptr(grids), N, H, W, GX, GY, Lz)
        L.check(L.load().v3a_bilagrid_slice_backward(C.byref(args), _ptr(d_out), _ptr(d_rgb), _ptr(d_grids), _stream()),
                "v3a_bilagrid_slice_backward")
        return d_rgb, d_grids


def _bilagrid_check(grids: torch.Tensor, what: str) -> None:
    if grids.dim() != 5 or grids.shape[-1] != 12:
        raise ValueError(f"{what}: grids must be [V,L,GY,GX,12], got {tuple(grids.shape)}")
    _f32_dev(grids, "grids")


def bilagrid_slice(rgb: torch.Tensor, grids: torch.Tensor) -> torch.Tensor:
    """The reference's bilateral-grid slice (lib_bilagrid.py::slice, one grid per image) on csrc/bilagrid.hip: `rgb` f32 [N,H,W,3]
    as gs_render emits it, `grids` f32 [N,L,GY,GX,12] (coefficient 4c + k = row c, column k of the 3x4 matrix; GX, GY, L >= 2).
    Pixel (i, j) samples its image's grid at ((j + 0.5) / W, (i + 0.5) / H, gray(rgb)) - trilinear, align_corners=True, border -
    and the 3x4 affine matrix it gets is applied to its colour.  -> f32 [N,H,W,3], differentiable with respect to both inputs
    (HIP backward, first order only; deterministic, no atomics)."""
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"bilagrid_slice: rgb must be [N,H,W,3], got {tuple(rgb.shape)}")
    _f32_dev(rgb, "rgb")
    _bilagrid_check(grids, "bilagrid_slice")
    if grids.shape[0] != rgb.shape[0]:
        raise ValueError(f"bilagrid_slice: one grid per image: grids must have shape [{rgb.shape[0]},L,GY,GX,12], got {tuple(grids.shape)}")
    return _BilagridSlice.apply(rgb, grids)


class _BilagridTv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        V, Lz, GY, GX, _ = grids.shape
        lib = L.load()
        ws, ws_bytes = _workspace(lib.v3a_bilagrid_tv_workspace_bytes(V, GX, GY, Lz),
                                  f"v3a_bilagrid_tv_workspace_bytes (grids {tuple(grids.shape)})", grids.device)
        out = torch.empty(1, device=grids.device, dtype=torch.float64)
        args = L.BilagridTvArgs(_ptr(grids), V, GX, GY, Lz, _ptr(out), _ptr(ws), ws_bytes)
        L.check(lib.v3a_bilagrid_tv_forward(C.byref(args), _stream()), "v3a_bilagrid_tv_forward")
        ctx.save_for_backward(grids)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_tv):
        grids, = ctx.saved_tensors
        V, Lz, GY, GX, _ = grids.shape
        d_out = d_tv.to(torch.float64).reshape(1).contiguous()
        d_grids = torch.empty_like(grids)
        args = L.BilagridTvArgs(_ptr(grids), V, GX, GY, Lz, None, None, 0)
        L.check(L.load().v3a_bilagrid_tv_backward(C.byref(args), _ptr(d_out), _ptr(d_grids), _stream()), "v3a_bilagrid_tv_backward")
        return d_grids


def bilagrid_tv(grids: torch.Tensor) -> torch.Tensor:
    """lib_bilagrid.py::total_variation_loss of `grids` f32 [V,L,GY,GX,12] (csrc/bilagrid.hip): per axis L, GY, GX the sum of squared
    forward differences over the number of differences, added and divided by V.  -> a float64 scalar on the device, differentiable
    (HIP backward, first order only)."""
    _bilagrid_check(grids, "bilagrid_tv")
    return _BilagridTv.apply(grids)


def bilagrid_identity(V: int, GX: int, GY: int, L: int, device) -> torch.Tensor:
    """V identity grids f32 [V,L,GY,GX,12]: every vertex holds the 3x4 matrix [I | 0]"""
    if V < 1 or min(GX, GY, L) < 2:
        raise ValueError(f"bilagrid_identity: V >= 1 and GX, GY, L >= 2 required, got V={V}, (GX, GY, L)={(GX, GY, L)}")
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=f32, device=device)
    return eye.repeat(V, L, GY, GX, 1).contiguous()


def bilagrid_from_reference(t: torch.Tensor) -> torch.Tensor:
    """the reference's BilateralGrid.grids [V,12,L,GY,GX] -> this package's [V,L,GY,GX,12] (a copy)"""
    if t.dim() != 5 or t.shape[1] != 12:
        raise ValueError(f"bilagrid_from_reference: expected [V,12,L,GY,GX], got {tuple(t.shape)}")
    return t.permute(0, 2, 3, 4, 1).contiguous()


def bilagrid_to_reference(t: torch.Tensor) -> torch.Tensor:
    """this package's [V,L,GY,GX,12] -> the reference's [V,12,L,GY,GX] (a copy)"""
    if t.dim() != 5 or t.shape[-1] != 12:
        raise ValueError(f"bilagrid_to_reference: expected [V,L,GY,GX,12], got {tuple(t.shape)}")
    return t.permute(0, 4, 1, 2, 3).contiguous()


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


class _SplatActivate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_scales, quats, logits):
        U = logits.shape[0]
        cov = torch.empty(U, 3, 3, device=logits.device, dtype=f32)
        op = torch.empty(U, device=logits.device, dtype=f32)
        L.check(L.load().v3a_splat_activate(_ptr(log_scales), _ptr(quats), _ptr(logits), U, _ptr(cov), _ptr(op), _stream()), "v3a_splat_activate")
        ctx.save_for_backward(log_scales, quats, logits)
        return cov, op

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_cov, d_op):
        log_scales, quats, logits = ctx.saved_tensors
        U = logits.shape[0]
        d_cov = torch.zeros(U, 3, 3, device=logits.device, dtype=f32) if d_cov is None else d_cov.float().contiguous()
        d_op = torch.zeros(U, device=logits.device, dtype=f32) if d_op is None else d_op.float().contiguous()
        d_ls, d_q, d_lg = torch.empty_like(log_scales), torch.empty_like(quats), torch.empty_like(logits)
        L.check(L.load().v3a_splat_activate_backward(_ptr(log_scales), _ptr(quats), _ptr(logits), _ptr(d_cov), _ptr(d_op), U, _ptr(d_ls),
                                                     _ptr(d_q), _ptr(d_lg), _stream()), "v3a_splat_activate_backward")
        return d_ls, d_q, d_lg


def splat_activate(log_scales: torch.Tensor, quats: torch.Tensor, logits: torch.Tensor):
    """(log-scales [U,3], raw quaternions [U,4] xyzw, opacity logits [U]) -> (covariances [U,3,3], opacities [U]), the inverse of
    (log g.scales, g.rotations, logit g.opacities) of gaussian_adapter's output; differentiable (closed-form HIP backward)."""
    U = logits.shape[0]
    if U < 1:
        raise ValueError("splat_activate: no Gaussians")
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(quats, "quats", (U, 4))
    _f32_dev(logits, "logits", (U,))
    return _SplatActivate.apply(log_scales, quats, logits)


class _SplatRegularisers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_scales, logits):
        U = logits.shape[0]
        lib = L.load()
        ws, ws_bytes = _workspace(lib.v3a_splat_reg_workspace_bytes(U), f"v3a_splat_reg_workspace_bytes (U = {U})", logits.device)
        out = torch.empty(2, device=logits.device, dtype=torch.float64)
        L.check(lib.v3a_splat_reg(_ptr(logits), _ptr(log_scales), U, _ptr(out), _ptr(ws), ws_bytes, _stream()), "v3a_splat_reg")
        ctx.save_for_backward(log_scales, logits)
        return out[0], out[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_opacity, d_scale):
        log_scales, logits = ctx.saved_tensors
        z = torch.zeros((), device=logits.device, dtype=torch.float64)
        d_out = torch.stack([z if g is None else g.to(torch.float64).reshape(()) for g in (d_opacity, d_scale)])
        d_ls, d_lg = torch.empty_like(log_scales), torch.empty_like(logits)
        L.check(L.load().v3a_splat_reg_backward(_ptr(logits), _ptr(log_scales), logits.shape[0], _ptr(d_out), _ptr(d_lg), _ptr(d_ls),
                                                _stream()), "v3a_splat_reg_backward")
        return d_ls, d_lg


def splat_regularisers(log_scales: torch.Tensor, logits: torch.Tensor):
    """The reference loop's two regularisers (simple_trainer.py:966-977; csrc/splat_reg.hip) of log-scales [U,3] and opacity logits
    [U] -> (opacity_mean, scale_mean) = (sigmoid(logits).mean(), exp(log_scales).mean()): float64 scalars on the device, summed in
    fp64 in a fixed order (bit-identical run to run), differentiable with respect to both inputs (HIP backward, first order only)."""
    U = logits.shape[0]
    if U < 1:
        raise ValueError("splat_regularisers: no Gaussians")
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(logits, "logits", (U,))
    return _SplatRegularisers.apply(log_scales, logits)


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, step: int, betas=(0.9, 0.999),
              eps: float = 1e-8, lr2: Optional[float] = None, period: int = 0) -> None:
    """One torch.optim.Adam update of p (f32, any shape), in place on p, m, v, reading the gradient g; `step` counts from 1 and
    sets the bias corrections (computed here in double).  period > 0 with lr2: flat element e uses lr where e % period == 0 and lr2
    elsewhere - the harmonics [U,3,K] with period K are the reference's sh0 / shN optimisers in one launch."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _f32_dev(t, name, p.shape)
    if step < 1:
        raise ValueError("adam_step: step counts from 1")
    b1, b2 = float(betas[0]), float(betas[1])
    a = L.AdamArgs(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(lr if lr2 is None else lr2), int(period), b1, b2, float(eps),
                   1.0 - b1 ** step, 1.0 - b2 ** step)
    L.check(L.load().v3a_adam_step(C.byref(a), _stream()), "v3a_adam_step")


def gs_visibility(radii: torch.Tensor) -> torch.Tensor:
    """The step's visibility mask (simple_trainer.py:1111): radii int32 [C,U] as gs_render's info_out holds them -> uint8 [U], 1
    where radii[c,g] > 0 for some camera c: (radii > 0).any(0) in one launch (v3a_gs_visibility), every byte written once."""
    if radii.dim() != 2 or radii.shape[0] < 1:
        raise ValueError(f"gs_visibility: radii [C,U] with C >= 1 required, got {tuple(radii.shape)}")
    Cn, U = radii.shape
    _i32_dev(radii, "radii", (Cn, U))
    visible = torch.empty(U, device=radii.device, dtype=torch.uint8)
    if U > 0:
        L.check(L.load().v3a_gs_visibility(_ptr(radii), Cn, U, _ptr(visible), _stream()), "v3a_gs_visibility")
    return visible


def adam_step_visible(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, visible: torch.Tensor, *, lr: float,
                      betas=(0.9, 0.999), eps: float = 1e-8, lr2: Optional[float] = None, period: int = 0) -> None:
    """gsplat's SelectiveAdam (the reference's visible_adam, simple_trainer.py:449-450) on p, g, m, v f32 [U, ...] and the mask
    `visible` uint8 [U] (gs_visibility), in place on p, m, v: every element of a row with visible != 0 gets
    m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr m / (sqrt(v) + eps) - no bias correction, hence no step argument.  A
    row with visible == 0 keeps the bits of p, m, v, and its g is not loaded (a NaN there reaches nothing).  period / lr2 as in
    adam_step, the element index taken within the whole tensor."""
    if p.dim() < 1 or p.shape[0] < 1 or p.numel() < 1:
        raise ValueError(f"adam_step_visible: p [U, ...] with at least one element required, got {tuple(p.shape)}")
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _f32_dev(t, name, p.shape)
    U = p.shape[0]
    if not isinstance(visible, torch.Tensor) or not visible.is_cuda or visible.device != p.device or visible.dtype != torch.uint8 \
            or not visible.is_contiguous() or tuple(visible.shape) != (U,):
        raise ValueError(f"visible must be a contiguous uint8 tensor of shape {(U,)} on {p.device}, got "
                         f"{getattr(visible, 'dtype', type(visible))} {tuple(getattr(visible, 'shape', ()))} on {getattr(visible, 'device', None)}")
    a = L.AdamVisibleArgs(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(visible), U, p.numel() // U, float(lr), float(lr if lr2 is None else lr2),
                          int(period), float(betas[0]), float(betas[1]), float(eps))
    L.check(L.load().v3a_adam_step_visible(C.byref(a), _stream()), "v3a_adam_step_visible")


# the random streams of the strategies' Philox draws: the sampler's two (2 and 3 are the noise's draws), and the first of the two
# consecutive streams of each split child of the densification (z0, z1 of stream s, z2 = z0 of stream s + 1)
MCMC_STREAMS = dict(relocate=0, grow=1, split0=4, split1=6)


def _mcmc_key(seed: int, step: int, what: str):
    seed, step = int(seed), int(step)
    if not 0 <= seed < 2 ** 64 or not 0 <= step < 2 ** 32:
        raise ValueError(f"{what}: seed must fit 64 bits and step 32 bits, both unsigned, got {seed} and {step}")
    return seed, step


def mcmc_sample(weights: torch.Tensor, *, min_weight: float, alive_only: bool, n_slots: int, seed: int, stream: int, step: int):
    """The MCMC strategy's weighted sampler (csrc/mcmc.hip, v3a_mcmc_sample) over opacities `weights` f32 [U] -> (src int32 [n_slots],
    counts int32 [U]).  alive_only (relocation, n_slots == U): slot s draws iff weights[s] <= min_weight, among the Gaussians above
    it; otherwise (growth) every slot draws among all.  src is the drawn row or -1, counts how often each row was drawn.  Philox
    counter (slot, 0, stream, step) under the key `seed`; fp64 sums in a fixed order: bit-identical run to run and reproducible on
    the host (tests/mcmc_oracle.py).  An empty pool, or no slot that draws, is a no-op (all -1, all 0)."""
    U = weights.shape[0] if weights.dim() == 1 else 0
    if U < 1:
        raise ValueError("mcmc_sample: no Gaussians")
    _f32_dev(weights, "weights", (U,))
    n_slots = int(n_slots)
    if n_slots < 1 or (alive_only and n_slots != U):
        raise ValueError(f"mcmc_sample: n_slots must be positive, and U = {U} with alive_only, got {n_slots}")
    if stream not in (0, 1):
        raise ValueError(f"mcmc_sample: stream is 0 (relocation) or 1 (growth), got {stream!r}")
    seed, step = _mcmc_key(seed, step, "mcmc_sample")
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_mcmc_sample_workspace_bytes(U), f"v3a_mcmc_sample_workspace_bytes (U = {U})", weights.device)
    src = torch.empty(n_slots, device=weights.device, dtype=torch.int32)
    counts = torch.empty(U, device=weights.device, dtype=torch.int32)
    L.check(lib.v3a_mcmc_sample(_ptr(weights), U, float(min_weight), int(bool(alive_only)), n_slots, seed, int(stream), step, _ptr(src),
                                _ptr(counts), _ptr(ws), ws_bytes, _stream()), "v3a_mcmc_sample")
    return src, counts


SPLAT_TENSORS = ("means", "scales", "quats", "opacities", "sh")   # a scene's five tensors, in the order of lib.SPLAT_FIELDS


def _splat_inner(K: int) -> dict:   # the shape of one row of each tensor; K = the last dimension of sh (the DC term included where stored)
    return dict(means=(3,), scales=(3,), quats=(4,), opacities=(), sh=(3, K))


def _splat_dicts(what: str, params: dict, m: dict, v: dict, rows: int) -> int:
    """`params`, `m` and `v` each hold the five SPLAT_TENSORS as contiguous f32 device tensors of `rows` rows -> K of sh [rows,3,K]"""
    sh = params["sh"]
    if sh.dim() != 3 or sh.shape[1] != 3 or sh.shape[2] < 1:
        raise ValueError(f"{what}: sh must be [rows,3,K], got {tuple(sh.shape)}")
    K = sh.shape[2]
    for group, d in (("params", params), ("m", m), ("v", v)):
        for name, inner in _splat_inner(K).items():
            _f32_dev(d[name], f"{group}[{name!r}]", (rows,) + inner)
    return K


def _scene_view(args, tensors: dict, rows: int, K_plus: int, what: str, label: str, pre: str = "") -> None:
    """Sets the five pointers and row strides (`pre` + `field`, `pre` + `ld_field`) of a SplatExportArgs / SplatImportArgs /
    SplatTransformArgs from `tensors`: float32 device tensors [rows, ...], sh [rows,3,K_plus], whose rows may be strided (a row's own
    elements contiguous).  `label` formats a name."""
    for field, (name, inner) in zip(L.SPLAT_FIELDS, _splat_inner(K_plus).items()):
        t, shape, width = tensors[name], (rows,) + inner, math.prod(inner)
        if not t.is_cuda or t.dtype != f32 or tuple(t.shape) != shape:
            raise ValueError(f"{what}: {label.format(name)} must be a float32 device tensor (the HIP path has no CPU fallback) of shape {shape}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if rows > 0 and width > 1 and not t[0].is_contiguous():
            raise ValueError(f"{what}: the elements of a row of {label.format(name)} must be contiguous, got strides {t.stride()}")
        ld = t.stride(0) if rows > 1 else width
        if ld < width:
            raise ValueError(f"{what}: rows of {label.format(name)} overlap (row stride {ld} < {width})")
        setattr(args, pre + field, t.data_ptr())
        setattr(args, pre + "ld_" + field, ld)


def mcmc_relocate(src: torch.Tensor, counts: torch.Tensor, params: dict, m: dict, v: dict, *, dst_offset: int, min_opacity: float) -> None:
    """Relocation (dst_offset = 0) or growth (dst_offset = U) from mcmc_sample's (src, counts), in place on `params` and Adam's
    moments `m`, `v`: dicts of means [R,3], scales (logs) [R,3], quats [R,4], opacities (logits) [R], sh [R,3,K], f32, with R = U
    rows (relocation, src [U]) or R = U + n rows filled up to U (growth, src [n]).  Every drawn row j and its copies get
    compute_relocation's opacity and scales for counts[j] + 1 copies (fp64, csrc/mcmc.hip); copies take means, quats and sh of j.
    Relocation zeroes the moments of j and leaves the dead row's; growth zeroes the new row's and leaves j's."""
    U, n = counts.shape[0], src.shape[0]
    dst_offset = int(dst_offset)
    if dst_offset not in (0, U) or (dst_offset == 0 and n != U):
        raise ValueError(f"mcmc_relocate: dst_offset is 0 with src [U] (relocation) or U (growth), got {dst_offset} with U = {U}, src [{n}]")
    rows = U if dst_offset == 0 else U + n
    for name, t in (("src", src), ("counts", counts)):
        if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"mcmc_relocate: {name} must be a contiguous int32 device vector, got {t.dtype} {tuple(t.shape)} on {t.device}")
    K = _splat_dicts("mcmc_relocate", params, m, v, rows)
    if not 0.0 < float(min_opacity) < 1.0:
        raise ValueError(f"mcmc_relocate: min_opacity must lie in (0, 1), got {min_opacity!r}")
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_mcmc_relocate_workspace_bytes(U), f"v3a_mcmc_relocate_workspace_bytes (U = {U})", src.device)
    a = L.McmcRelocateArgs(_ptr(src), _ptr(counts), *(_ptr(d[name]) for d in (params, m, v) for name in SPLAT_TENSORS), U, n, dst_offset, K,
                           float(min_opacity), _ptr(ws), ws_bytes)
    L.check(lib.v3a_mcmc_relocate(C.byref(a), _stream()), "v3a_mcmc_relocate")


def mcmc_noise(means: torch.Tensor, log_scales: torch.Tensor, quats: torch.Tensor, logits: torch.Tensor, *, scaler: float, seed: int,
               step: int) -> None:
    """The MCMC strategy's per-step noise, in place on means [U,3]: means += cov . (xi * gate * scaler), cov from (log_scales [U,3],
    raw quats [U,4]) as splat_activate forms it, gate = sigmoid(-100 (opacity - 0.005)) of logits [U], xi three standard normals of
    (seed, step, row) (csrc/mcmc.hip, v3a_mcmc_noise: fp64 after the loads, one rounding at the store)."""
    U = logits.shape[0] if logits.dim() == 1 else 0
    if U < 1:
        raise ValueError("mcmc_noise: no Gaussians")
    _f32_dev(means, "means", (U, 3))
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(quats, "quats", (U, 4))
    _f32_dev(logits, "logits", (U,))
    seed, step = _mcmc_key(seed, step, "mcmc_noise")
    L.check(L.load().v3a_mcmc_noise(_ptr(means), _ptr(log_scales), _ptr(quats), _ptr(logits), U, float(scaler), seed, step, _stream()),
            "v3a_mcmc_noise")


# ------------------------------------------------------------------------------------------------ densification (csrc/densify.hip)
def _i32_dev(t: torch.Tensor, name: str, shape) -> None:
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a contiguous int32 device tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def densify_accumulate(grad2d: torch.Tensor, count: torch.Tensor, d_means2d: torch.Tensor, radii: torch.Tensor, width: int,
                       height: int) -> None:
    """The densification strategy's per-step statistics, in place on grad2d f32 [U] and count int32 [U]: for every camera c (index
    order) with radii[c,g] > 0, grad2d[g] += sqrt((gx W/2 C)^2 + (gy H/2 C)^2) with (gx, gy) = d_means2d[c,g], count[g] += 1
    (v3a_densify_accumulate: fp64 norm and sum, one rounding per call).  d_means2d f32 [C,U,2] and radii int32 [C,U] as
    gs_render's info_out holds them."""
    U = grad2d.shape[0] if grad2d.dim() == 1 else -1
    if U < 0 or d_means2d.dim() != 3 or d_means2d.shape[0] < 1:
        raise ValueError("densify_accumulate: grad2d [U] and d_means2d [C,U,2] required")
    Cn = d_means2d.shape[0]
    _f32_dev(grad2d, "grad2d", (U,))
    _i32_dev(count, "count", (U,))
    _f32_dev(d_means2d, "d_means2d", (Cn, U, 2))
    _i32_dev(radii, "radii", (Cn, U))
    if width < 1 or height < 1:
        raise ValueError(f"densify_accumulate: width and height must be positive, got {width} x {height}")
    if U == 0:
        return
    L.check(L.load().v3a_densify_accumulate(_ptr(d_means2d), _ptr(radii), U, Cn, int(width), int(height), _ptr(grad2d), _ptr(count), _stream()),
            "v3a_densify_accumulate")


def densify_classify(grad2d: torch.Tensor, count: torch.Tensor, log_scales: torch.Tensor, logits: torch.Tensor, *, grow_grad2d: float,
                     grow_scale3d: float, prune_opa: float, prune_scale3d: float, grow: bool = True, prune_big: bool = False,
                     revised_opacity: bool = False) -> dict:
    """The fate of every Gaussian at a refine (v3a_densify_classify; fp64 decisions on exactly converted values; the two scale
    thresholds come multiplied by the scene scale) -> dict(fates uint8 [U]: 0 keep, 1 clone, 2 split, + 4 when the rows it leaves
    are pruned; counts int32 [3,U]: the rows it leaves in segment A (the original), B (the clone), C = D (each split child);
    offsets int32 [3,U]: their exclusive prefix sums; totals int64 [3] on the device).  grow=False forces every fate to keep
    (prune only); prune_big adds the scale criterion to the opacity criterion."""
    U = grad2d.shape[0] if grad2d.dim() == 1 else -1
    if U < 0:
        raise ValueError("densify_classify: grad2d [U] required")
    _f32_dev(grad2d, "grad2d", (U,))
    _i32_dev(count, "count", (U,))
    _f32_dev(log_scales, "log_scales", (U, 3))
    _f32_dev(logits, "logits", (U,))
    dev = grad2d.device
    out = dict(fates=torch.empty(U, device=dev, dtype=torch.uint8), counts=torch.empty(3, U, device=dev, dtype=torch.int32),
               offsets=torch.empty(3, U, device=dev, dtype=torch.int32), totals=torch.zeros(3, device=dev, dtype=torch.int64))
    if U == 0:
        return out
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_densify_classify_workspace_bytes(U), f"v3a_densify_classify_workspace_bytes (U = {U})", dev)
    a = L.DensifyClassifyArgs(_ptr(grad2d), _ptr(count), _ptr(log_scales), _ptr(logits), U, float(grow_grad2d), float(grow_scale3d),
                              float(prune_opa), float(prune_scale3d), int(bool(grow)), int(bool(prune_big)), int(bool(revised_opacity)),
                              _ptr(out["fates"]), _ptr(out["counts"]), _ptr(out["offsets"]), _ptr(out["totals"]), _ptr(ws), ws_bytes)
    L.check(lib.v3a_densify_classify(C.byref(a), _stream()), "v3a_densify_classify")
    return out


def densify_apply(cls: dict, params: dict, m: dict, v: dict, *, seed: int, step: int, revised_opacity: bool = False,
                  totals: Optional[list] = None):
    """The refined scene from densify_classify's `cls` and the old tensors (dicts of means [U,3], scales (logs) [U,3], quats [U,4],
    opacities (logits) [U], sh [U,3,K], f32) -> (params, m, v): NEW dicts of tensors with U_out = A + B + 2 C rows in the order
    A surviving non-split originals, B surviving clones, C first children, D second children (v3a_densify_apply; include/vist3a_hip.h
    states a child's values).  The old tensors are read only.  `totals` = cls["totals"].tolist() if the caller has read it already;
    otherwise it is read here: the refine's one read-back, which sizes the new tensors."""
    U = cls["fates"].shape[0]
    K = _splat_dicts("densify_apply", params, m, v, U)
    if cls["fates"].dtype != torch.uint8 or not cls["fates"].is_cuda or not cls["fates"].is_contiguous():
        raise ValueError("densify_apply: cls['fates'] must be a contiguous uint8 device vector")
    _i32_dev(cls["offsets"], "cls['offsets']", (3, U))
    if cls["totals"].dtype != torch.int64 or tuple(cls["totals"].shape) != (3,) or not cls["totals"].is_cuda:
        raise ValueError("densify_apply: cls['totals'] must be int64 [3] on the device")
    seed, step = _mcmc_key(seed, step, "densify_apply")
    nA, nB, nC = (int(x) for x in (cls["totals"].tolist() if totals is None else totals))
    U_out = nA + nB + 2 * nC
    if min(nA, nB, nC) < 0 or nA + nB > 2 * U or nC > U or U_out >= 2 ** 31:
        raise ValueError(f"densify_apply: segment totals {(nA, nB, nC)} do not belong to {U} Gaussians")
    dev = params["sh"].device
    new = [{name: torch.empty((U_out,) + tuple(params[name].shape[1:]), device=dev, dtype=f32) for name in SPLAT_TENSORS} for _ in range(3)]
    if U == 0 or U_out == 0:
        return tuple(new)
    a = L.DensifyApplyArgs(*(_ptr(d[name]) for d in (params, m, v, *new) for name in SPLAT_TENSORS), _ptr(cls["fates"]), _ptr(cls["offsets"]),
                           _ptr(cls["totals"]), U, U_out, K, seed, step, int(bool(revised_opacity)))
    L.check(L.load().v3a_densify_apply(C.byref(a), _stream()), "v3a_densify_apply")
    return tuple(new)


def densify_reset_opacity(logits: torch.Tensor, m: torch.Tensor, v: torch.Tensor, max_opacity: float) -> None:
    """The strategy's opacity reset, in place: logits = min(logits, logit(max_opacity)), Adam's moments m and v of the logits = 0
    (v3a_densify_reset_opacity)."""
    U = logits.shape[0] if logits.dim() == 1 else -1
    if U < 0:
        raise ValueError("densify_reset_opacity: logits [U] required")
    for name, t in (("logits", logits), ("m", m), ("v", v)):
        _f32_dev(t, name, (U,))
    if not 0.0 < float(max_opacity) < 1.0:
        raise ValueError(f"densify_reset_opacity: max_opacity must lie in (0, 1), got {max_opacity!r}")
    if U == 0:
        return
    L.check(L.load().v3a_densify_reset_opacity(_ptr(logits), _ptr(m), _ptr(v), U, float(max_opacity), _stream()), "v3a_densify_reset_opacity")


# ------------------------------------------------------------------------------------------------ scene export (csrc/splat_export.hip)
def _export_scene(scene: dict, quats_xyzw: bool, what: str) -> L.SplatExportArgs:
    """The scene part of v3a_splat_export_args from dict(means [U,3], scales (logs) [U,3], quats [U,4], opacities (logits) [U],
    sh [U,3,K+1]): float32 device tensors whose rows may be strided (a row's own elements contiguous)."""
    means, sh = scene["means"], scene["sh"]
    if means.dim() != 2 or means.shape[1] != 3 or sh.dim() != 3 or sh.shape[1] != 3 or sh.shape[2] < 1:
        raise ValueError(f"{what}: means [U,3] and sh [U,3,K+1] required, got {tuple(means.shape)} and {tuple(sh.shape)}")
    U, K = means.shape[0], sh.shape[2] - 1
    a = L.SplatExportArgs()
    _scene_view(a, scene, U, K + 1, what, "{}")
    a.U, a.K, a.quats_xyzw = U, K, int(bool(quats_xyzw))
    return a


def _export_list(t: torch.Tensor, name: str, n: int, U: int) -> None:
    if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.shape[0] < n or not 0 <= n <= U:
        raise ValueError(f"{name} must be a contiguous int32 device vector of at least n = {n} <= {U} entries, got {t.dtype} {tuple(t.shape)} on {t.device}")


def splat_export_filter(scene: dict, *, quats_xyzw: bool, opacity_threshold: Optional[float] = None):
    """The rows that go into an export (v3a_splat_export_filter): every value finite and, with `opacity_threshold`,
    1 / (1 + exp(-logit)) above it.  -> (rows int32 [U], of which the first `count` are set, in ascending order; count int64 [1] on
    the device - reading it is the caller's one synchronisation)."""
    a = _export_scene(scene, quats_xyzw, "splat_export_filter")
    dev = scene["means"].device
    rows, count = torch.empty(a.U, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int64)
    if a.U == 0:
        return rows, count
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_splat_export_filter_workspace_bytes(a.U, a.K), f"v3a_splat_export_filter_workspace_bytes (U = {a.U})", dev)
    a.filter_opacity, a.opacity_threshold = int(opacity_threshold is not None), float(opacity_threshold or 0.0)
    a.rows, a.count, a.workspace, a.workspace_bytes = rows.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.v3a_splat_export_filter(C.byref(a), _stream()), "v3a_splat_export_filter")
    return rows, count


def splat_export_sort(scene: dict, rows: torch.Tensor, n: int, *, quats_xyzw: bool) -> torch.Tensor:
    """rows[:n] in the Morton order of their means, equal keys in ascending row order (v3a_splat_export_sort) -> int32 [n]."""
    a = _export_scene(scene, quats_xyzw, "splat_export_sort")
    _export_list(rows, "rows", n, a.U)
    order = torch.empty(n, device=rows.device, dtype=torch.int32)
    if n == 0:
        return order
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_splat_export_sort_workspace_bytes(a.U, a.K), f"v3a_splat_export_sort_workspace_bytes (U = {a.U})", rows.device)
    a.rows, a.n, a.order, a.workspace, a.workspace_bytes = rows.data_ptr(), n, order.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.v3a_splat_export_sort(C.byref(a), _stream()), "v3a_splat_export_sort")
    return order


def splat_export_pack_compressed(scene: dict, order: torch.Tensor, n: int, *, quats_xyzw: bool):
    """The compressed PLY's three elements of the splats order[:n] (v3a_splat_export_pack_compressed) -> (chunks f32 [ceil(n/256),18],
    vertices int32 [n,4] (the packed words' bits), sh uint8 [n,3K])."""
    a = _export_scene(scene, quats_xyzw, "splat_export_pack_compressed")
    _export_list(order, "order", n, a.U)
    dev = order.device
    chunks = torch.empty((n + 255) // 256, 18, device=dev, dtype=f32)
    vertices = torch.empty(n, 4, device=dev, dtype=torch.int32)
    sh = torch.empty(n, 3 * a.K, device=dev, dtype=torch.uint8)
    if n:
        a.order, a.n, a.out_chunks, a.out_vertices, a.out_sh = order.data_ptr(), n, chunks.data_ptr(), vertices.data_ptr(), sh.data_ptr()
        L.check(L.load().v3a_splat_export_pack_compressed(C.byref(a), _stream()), "v3a_splat_export_pack_compressed")
    return chunks, vertices, sh


def splat_export_pack_splat(scene: dict, order: torch.Tensor, n: int, *, quats_xyzw: bool) -> torch.Tensor:
    """The .splat records of the splats order[:n] (v3a_splat_export_pack_splat) -> uint8 [n,32]."""
    a = _export_scene(scene, quats_xyzw, "splat_export_pack_splat")
    _export_list(order, "order", n, a.U)
    out = torch.empty(n, 32, device=order.device, dtype=torch.uint8)
    if n:
        a.order, a.n, a.out_splat = order.data_ptr(), n, out.data_ptr()
        L.check(L.load().v3a_splat_export_pack_splat(C.byref(a), _stream()), "v3a_splat_export_pack_splat")
    return out


def splat_export_pack_ply(scene: dict, rows: torch.Tensor, n: int, *, quats_xyzw: bool) -> torch.Tensor:
    """The float PLY's vertex rows of rows[:n] (v3a_splat_export_pack_ply) -> f32 [n, 14 + 3K]."""
    a = _export_scene(scene, quats_xyzw, "splat_export_pack_ply")
    _export_list(rows, "rows", n, a.U)
    out = torch.empty(n, 14 + 3 * a.K, device=rows.device, dtype=f32)
    if n:
        a.rows, a.n, a.out_ply = rows.data_ptr(), n, out.data_ptr()
        L.check(L.load().v3a_splat_export_pack_ply(C.byref(a), _stream()), "v3a_splat_export_pack_ply")
    return out


# ------------------------------------------------------------------------------------------------ scene import (csrc/splat_import.hip)
PLY_COLUMNS = (("x", "y", "z") + tuple(f"f_dc_{j}" for j in range(3)) + ("f_rest_0", "opacity") + tuple(f"scale_{j}" for j in range(3))
               + tuple(f"rot_{j}" for j in range(4)))     # the order of v3a_splat_import_args.offsets


def _import_outputs(n: int, K: int, dev, out: Optional[dict], what: str):
    """The five output tensors of a load - fresh, or the caller's (strided rows allowed, as for the exporter) - and the args struct
    with them, `bad` and the workspace set.  -> (args, scene dict, bad int32 [1], workspace)"""
    if out is None:
        out = {name: torch.empty((n,) + inner, device=dev, dtype=f32) for name, inner in _splat_inner(K + 1).items()}
    a = L.SplatImportArgs()
    _scene_view(a, out, n, K + 1, what, "out[{!r}]")
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = None
    if n > 0:
        ws, a.workspace_bytes = _workspace(L.load().v3a_splat_import_workspace_bytes(n), f"v3a_splat_import_workspace_bytes (n = {n})", dev)
        a.workspace = ws.data_ptr()
    a.n, a.n_rest, a.bad = n, 3 * K, bad.data_ptr()
    return a, {name: out[name] for name in SPLAT_TENSORS}, bad, ws


def _import_payload(payload: torch.Tensor, what: str) -> None:
    if not payload.is_cuda or payload.dtype != torch.uint8 or payload.dim() != 1 or not payload.is_contiguous():
        raise ValueError(f"{what}: the payload must be a contiguous uint8 device vector (the HIP path has no CPU fallback), got {payload.dtype} "
                         f"{tuple(payload.shape)} on {payload.device}")


def splat_import_ply(payload: torch.Tensor, n: int, K: int, table: dict, *, opacity: str = "logit", quats_xyzw: bool = True, out: Optional[dict] = None):
    """The vertex rows of a float PLY (v3a_splat_import_ply): payload uint8 [4 n P] on the device; table = {"P": floats per row,
    name: column of each of PLY_COLUMNS}.  opacity: "logit" (copied) or "linear" (logit of the value clamped to [1e-6, 1 - 1e-6]).
    -> (dict(means, scales (logs), quats, opacities (logits), sh [n,3,K+1]), bad int32 [1] on the device: rows with a NaN or Inf)."""
    if opacity not in ("logit", "linear"):
        raise ValueError(f"splat_import_ply: opacity must be 'logit' or 'linear', got {opacity!r}")
    _import_payload(payload, "splat_import_ply")
    a, scene, bad, ws = _import_outputs(n, K, payload.device, out, "splat_import_ply")
    if n:
        a.payload, a.payload_bytes, a.quats_xyzw = payload.data_ptr(), payload.numel(), int(bool(quats_xyzw))
        a.P, a.opacity_linear = int(table["P"]), int(opacity == "linear")
        for j, name in enumerate(PLY_COLUMNS):
            a.offsets[j] = int(table[name]) if K or name != "f_rest_0" else 0      # K = 0: an empty range, it overlaps nothing
        L.check(L.load().v3a_splat_import_ply(C.byref(a), _stream()), "v3a_splat_import_ply")
    return scene, bad


def splat_import_compressed(payload: torch.Tensor, n: int, K: int, *, quats_xyzw: bool = True, out: Optional[dict] = None):
    """A compressed PLY's three elements, back to back (v3a_splat_import_compressed): payload uint8 [72 ceil(n/256) + 16 n + 3 K n].
    -> (scene dict, bad) as splat_import_ply."""
    _import_payload(payload, "splat_import_compressed")
    a, scene, bad, ws = _import_outputs(n, K, payload.device, out, "splat_import_compressed")
    if n:
        a.payload, a.payload_bytes, a.quats_xyzw, a.nch = payload.data_ptr(), payload.numel(), int(bool(quats_xyzw)), (n + 255) // 256
        L.check(L.load().v3a_splat_import_compressed(C.byref(a), _stream()), "v3a_splat_import_compressed")
    return scene, bad


def splat_import_splat(payload: torch.Tensor, n: int, *, quats_xyzw: bool = True, out: Optional[dict] = None):
    """The 32-byte records of a .splat (v3a_splat_import_splat): payload uint8 [32 n].  -> (scene dict with K = 0, bad)."""
    _import_payload(payload, "splat_import_splat")
    a, scene, bad, ws = _import_outputs(n, 0, payload.device, out, "splat_import_splat")
    if n:
        a.payload, a.payload_bytes, a.quats_xyzw = payload.data_ptr(), payload.numel(), int(bool(quats_xyzw))
        L.check(L.load().v3a_splat_import_splat(C.byref(a), _stream()), "v3a_splat_import_splat")
    return scene, bad


# ------------------------------------------------------------------------------------------------ scene transforms (csrc/splat_transform.hip)
SH_BAND_COUNTS = (1, 4, 9, 16, 25)     # K + 1 of a scene that v3a_splat_transform takes: whole bands up to degree 4


def similarity_parts(T, what: str = "similarity_parts"):
    """A 4x4 similarity [[s R, t], [0, 1]] split on the host in fp64 -> (s, R float64 [3,3], t float64 [3]).  ValueError for what
    is none: a bottom row other than 0 0 0 1, a non-finite entry, det <= 0 (a reflection, s <= 0) or |R R^T - I|_max > 1e-6 (shear,
    unequal scales)."""
    T = torch.as_tensor(T, dtype=torch.float64, device="cpu") if not isinstance(T, torch.Tensor) else T.detach().to("cpu", torch.float64)
    if tuple(T.shape) != (4, 4) or not bool(torch.isfinite(T).all()):
        raise ValueError(f"{what}: T must be a finite 4x4 matrix, got shape {tuple(T.shape)}")
    if not torch.equal(T[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)):
        raise ValueError(f"{what}: the bottom row of T must be 0 0 0 1, got {T[3].tolist()}")
    M = T[:3, :3]
    det = float(torch.linalg.det(M))
    if not det > 0.0:
        raise ValueError(f"{what}: det of the linear part is {det:g}; a similarity needs s > 0 and a proper rotation (no reflection)")
    s = det ** (1.0 / 3.0)
    R = M / s
    off = float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max())
    if not off <= 1e-6:
        raise ValueError(f"{what}: the linear part is not a scaled rotation (|R R^T - I|_max = {off:.3g} > 1e-6): shear or unequal scales")
    return s, R.contiguous(), T[:3, 3].contiguous()


def sh_rotation_matrices(R, deg: int) -> list:
    """D_1(R) .. D_deg(R) of the rasteriser's SH basis, Y_l(R d) = D_l(R) Y_l(d), in fp64 on the host (v3a_sh_rotation_matrices;
    no device needed) -> [float64 [2l+1, 2l+1]]"""
    R = torch.as_tensor(R, dtype=torch.float64, device="cpu").contiguous() if not isinstance(R, torch.Tensor) else R.detach().to("cpu", torch.float64).contiguous()
    if tuple(R.shape) != (3, 3):
        raise ValueError(f"sh_rotation_matrices: R must be 3x3, got {tuple(R.shape)}")
    out = torch.zeros(max(sum((2 * l + 1) ** 2 for l in range(1, max(int(deg), 0) + 1)), 1), dtype=torch.float64)
    dp = C.POINTER(C.c_double)
    rc = L.load().v3a_sh_rotation_matrices(C.cast(R.data_ptr(), dp), int(deg), C.cast(out.data_ptr(), dp))
    if rc == L.V3A_OK:
        mats, o = [], 0
        for l in range(1, deg + 1):
            n = 2 * l + 1
            mats.append(out[o:o + n * n].reshape(n, n).clone())
            o += n * n
        return mats
    if rc == -1:
        raise ValueError("sh_rotation_matrices: R is not a proper rotation (|R R^T - I|_max > 1e-6 or det < 0)")
    L.check(rc, "v3a_sh_rotation_matrices")


def splat_transform(scene: dict, T, out: Optional[dict] = None, *, quats_xyzw: bool = True) -> dict:
    """x' = s R x + t applied to a scene (v3a_splat_transform): `scene` as load_scene / create_splats hold it - means [U,3], scales
    (logs) [U,3], quats [U,4], opacities (logits) [U], sh [U,3,K+1] with K + 1 in SH_BAND_COUNTS; float32 device tensors whose rows
    may be strided.  T: a 4x4 similarity (similarity_parts; ValueError otherwise).  Means move, log-scales gain log s, quaternions
    are multiplied by R's from the left, the harmonics' bands 1.. are rotated in the rasteriser's basis; logits and DC are copied.
    out: None (fresh tensors), another scene dict of the same shapes, or `scene` itself (in place).  -> the five output tensors."""
    s, R, t = similarity_parts(T, "splat_transform")
    means, sh = scene["means"], scene["sh"]
    if means.dim() != 2 or means.shape[1] != 3 or sh.dim() != 3 or sh.shape[1] != 3:
        raise ValueError(f"splat_transform: means [U,3] and sh [U,3,K+1] required, got {tuple(means.shape)} and {tuple(sh.shape)}")
    U, Kp = means.shape[0], sh.shape[2]
    if Kp not in SH_BAND_COUNTS:
        raise ValueError(f"splat_transform: sh holds {Kp} coefficients per channel; whole bands are required, one of {SH_BAND_COUNTS}")
    if out is None:
        out = {name: torch.empty((U,) + inner, device=means.device, dtype=f32) for name, inner in _splat_inner(Kp).items()}
    a = L.SplatTransformArgs()
    _scene_view(a, scene, U, Kp, "splat_transform", "scene[{!r}]")
    _scene_view(a, out, U, Kp, "splat_transform", "out[{!r}]", pre="out_")
    a.rows, a.K, a.quats_xyzw, a.scale = U, Kp - 1, int(bool(quats_xyzw)), s
    for i, x in enumerate(R.reshape(-1).tolist()):
        a.R[i] = x
    for i, x in enumerate(t.tolist()):
        a.t[i] = x
    if U:
        L.check(L.load().v3a_splat_transform(C.byref(a), _stream()), "v3a_splat_transform")
    return {name: out[name] for name in SPLAT_TENSORS}


def splat_moments(means: torch.Tensor, centre) -> torch.Tensor:
    """Count, first and second moments of the rows of `means` (float32 device [n,3], rows may be strided) about `centre` (three host
    floats), in fp64 and in a fixed order (v3a_splat_moments) -> float64 [10] on the device: n, sum (x - c) [3], and
    sum (x - c)(x - c)^T as xx xy xz yy yz zz."""
    if not means.is_cuda or means.dtype != f32 or means.dim() != 2 or means.shape[1] != 3 or (means.shape[0] > 0 and means.stride(1) != 1):
        raise ValueError(f"splat_moments: means must be a float32 device tensor [n,3] with contiguous rows (the HIP path has no CPU fallback), got "
                         f"{means.dtype} {tuple(means.shape)} on {means.device}")
    n = means.shape[0]
    ld = means.stride(0) if n > 1 else 3
    if ld < 3:
        raise ValueError(f"splat_moments: rows of means overlap (row stride {ld} < 3)")
    c = (C.c_double * 3)(*[float(x) for x in (centre.tolist() if isinstance(centre, torch.Tensor) else centre)])
    out = torch.empty(10, device=means.device, dtype=torch.float64)
    lib = L.load()
    ws, ws_bytes = _workspace(lib.v3a_splat_moments_workspace_bytes(n), f"v3a_splat_moments_workspace_bytes (n = {n})", means.device)
    L.check(lib.v3a_splat_moments(_ptr(means) if n else None, ld, n, c, _ptr(out), _ptr(ws), ws_bytes, _stream()), "v3a_splat_moments")
    return out
