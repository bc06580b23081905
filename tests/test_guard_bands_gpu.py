"""Guard bands (`-m gpu`): no entry point reads or writes outside the strided views it is given (include/vist3a_hip.h, "Memory contract").

Every case runs twice on the same seeded values:
  clean    tight contiguous tensors, compared with the reference and under the gate of the kernel's own parity test (imported, not copied);
  guarded  every tensor carved out of an all-0xFF arena (tests/guard.py: NaN in every float format, -1 / 255 in the integer ones), with a row
           stride ld = cols + the smallest pad the entry point accepts wherever the wrapper takes a stride, output regions pre-filled with 0xFF.
and asserts  (a) the guarded output is bit-equal to the clean one,  (b) no byte outside any output / workspace region changed,
(c) every input is bit-unchanged and nothing around it was written,  (d) the output is finite wherever the clean output is.
A load from padding shows as a NaN or a changed bit (a), (d); a store into padding as (b) / (c).

Exceptions to bit-equality: none - no kernel here orders a float sum by stride or alignment.
GEMM operands are small dyadic rationals: every fp32 partial sum is then exact whatever the summation order, so the gates measured on
8192-row outputs apply unchanged to an 8-element output (one bf16 rounding flip in 8 elements would be 1.4e-3 relative L2).

Documented extents beyond [rows, cols] that the cases assert exactly:
  flash attention V^T: readable and FINITE up to the next multiple of 64 keys past each batch item's Nk (loaded with 3.0 in the guarded
  run, zeros in the clean one: bit-equality shows the values never reach the result), poison beyond;
  xattn_probs: columns Nk <= j < Lkp of every head are WRITTEN (zeros) - they lie inside the [rows, H * Lkp] region."""
import math
import sys
import threading
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))
import guard as G                      # noqa: E402
import test_kernels_gpu as TK          # noqa: E402  (references and gates of the kernels' own parity tests)
import test_small_kernels_gpu as TS    # noqa: E402

pytestmark = pytest.mark.gpu
dev = "cuda"
bf16, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
relerr = TK.relerr


# ------------------------------------------------------------------------------------------------------------------ protocol
def cv(values, pad=0, off=0, **kw):
    """an input: carved on the device, ld = cols + pad for 2-D, loaded with `values`; off = offset_bytes past the 256-byte alignment (16 = the
    smallest alignment the `% 8 bf16 elements` / `% 16 bytes` / `% 4 floats` checks of the entry points leave to a pointer)"""
    ld = values.shape[1] + pad if (values.dim() == 2 and pad) else None
    return G.carve_like(values.to(dev), ld=ld, offset_bytes=off, **kw)


def co(shape, dtype, pad=0, off=0, **kw):
    """an output / workspace: carved, every byte still 0xFF"""
    ld = shape[1] + pad if (len(shape) == 2 and pad) else None
    return G.carve(shape, dtype, ld=ld, device=dev, offset_bytes=off, **kw)


def verdict(parity, case, outs, inputs, written=(), **errs):
    """outs: (name, guarded view, clean tensor[, valid rows]); inputs: (name, view, values); written: views updated in place / by-products
    whose padding must stay untouched (their values are compared through `outs`).  Records and asserts (a) - (d)."""
    torch.cuda.synchronize()
    viol, biteq, fin, where = 0, True, True, {}
    for o in outs:
        name, view, clean = o[0], o[1], o[2]
        rows = o[3] if len(o) > 3 else None
        n, w = G.violations(view, rows=rows)
        viol += n
        if n:
            where[name] = w
        got = view if rows is None else view[rows]
        want = clean if rows is None else clean[rows]
        biteq &= bool(torch.equal(G.bits(got), G.bits(want)))
        if want.dtype.is_floating_point and want.element_size() > 1:
            fin &= bool(got.float()[want.float().isfinite()].isfinite().all())
    in_ok = {}
    for name, view, values in inputs:
        in_ok[name] = G.unchanged(view, values)
    for view in written:
        n, w = G.violations(view)
        viol += n
        if n:
            where["written"] = w
    parity("guard_bands", case=case, violations=viol, bit_equal=biteq, inputs_unchanged=all(in_ok.values()), **errs)
    assert viol == 0, (case, "bytes outside the valid region changed at (row, col)", where)
    assert all(in_ok.values()), (case, "inputs changed", [k for k, v in in_ok.items() if not v])
    assert biteq, (case, "guarded run differs from the clean run")
    assert fin, (case, "non-finite output where the clean output is finite")


def dy(g, shape, span=8, div=4, dtype=f32):
    """small dyadic rationals k / div, |k| <= span"""
    return (torch.randint(-span, span + 1, shape, device=dev, generator=g).float() / div).to(dtype)


def tile_dims(name):
    """BM x BN of a tile from its v3a_gemm_tile_name / v3a_gemm_fp8_tile_name (csrc/gemm_bf16.hip: TILE_ENTRY names start with BMxBN, the ping-pong
    forms pp[8]_np<NP>_ra<RA> are 256 x 64 NP when RA (A stays resident) else 64 NP x 256, w4_256x192 carries its shape)"""
    import re
    m = re.match(r"(?:w4_)?(\d+)x(\d+)", name)
    if m:
        return int(m.group(1)), int(m.group(2))
    m = re.match(r"pp8?_np(\d)_ra(true|false)", name)
    assert m, name
    return (256, 64 * int(m.group(1))) if m.group(2) == "true" else (64 * int(m.group(1)), 256)


# ------------------------------------------------------------------------------------------------------------------ tile GEMMs
NT, NT8 = 22, 2      # v3a_gemm_num_tiles() / v3a_gemm_fp8_num_tiles(), tabulated: parametrisation happens at collection, before a library is loaded


def test_gemm_tile_parametrisation_covers_the_table(hip_lib):
    assert (hip_lib.v3a_gemm_num_tiles(), hip_lib.v3a_gemm_fp8_num_tiles()) == (NT, NT8)


def _gemm_guarded(ops, a, w, bias, out_shape, out_dtype, *, res=None, pad=8, off=0, **kw):
    ga, gw = cv(a, pad, off), cv(w, pad, off)
    gb = cv(bias) if bias is not None else None
    gr = cv(res, pad, off) if res is not None else None
    go = co(out_shape, out_dtype, pad, off)
    ops.gemm(ga, gw, gb, out=go, residual=gr, **kw)
    ins = [("a", ga, a), ("w", gw, w)] + ([("bias", gb, bias)] if gb is not None else []) + ([("residual", gr, res)] if gr is not None else [])
    return go, ins


@pytest.mark.parametrize("t", range(NT))
def test_gemm_bf16_tile_ragged_grid(hip_lib, parity, t):
    """M in {1, BM-1, BM+1} x N in {8, BN-8, BN+8} x K in {64, 192}: bias + bf16 residual, strided a / w / out / residual."""
    from vist3a_amd import lib as L, ops
    name = hip_lib.v3a_gemm_tile_name(t).decode()
    BM, BN = tile_dims(name)
    g = torch.Generator(device=dev).manual_seed(100 + t)
    for M in (1, BM - 1, BM + 1):
        for N in (8, BN - 8, BN + 8):
            for K in (64, 192):
                a, w = dy(g, (M, K), dtype=bf16), dy(g, (N, K), div=8, dtype=bf16)
                bias, res = dy(g, (N,), span=16), dy(g, (M, N), dtype=bf16)
                clean = ops.gemm(a, w, bias, residual=res, tile=t)
                r = relerr(clean, TK.gemm_ref(L, a, w, bias, L.ACT_NONE, res, None, 0, False, False, False))
                assert math.isfinite(r) and r < TK.TOL_GEMM, (name, M, N, K, r)
                go, ins = _gemm_guarded(ops, a, w, bias, (M, N), bf16, res=res, tile=t)
                verdict(parity, f"gemm_bf16 {name} {M}x{N}x{K}", [("out", go, clean)], ins, rel_vs_fp32=r)
                if M != 1 and K == 192:      # ... and at the smallest alignment the ABI accepts: 16 bytes, not the allocator's 256
                    go, ins = _gemm_guarded(ops, a, w, bias, (M, N), bf16, res=res, tile=t, off=16)
                    verdict(parity, f"gemm_bf16 {name} {M}x{N}x{K} align16", [("out", go, clean)], ins, rel_vs_fp32=r)


@pytest.mark.parametrize("t", range(NT))
def test_gemm_bf16_tile_epilogue_options(hip_lib, parity, t):
    """Once each on (BM + 1) x (BN + 8) x 64 - the smallest shape that is ragged in both directions with more than one block in each."""
    from vist3a_amd import lib as L, ops
    name = hip_lib.v3a_gemm_tile_name(t).decode()
    BM, BN = tile_dims(name)
    M, N, K = BM + 1, BN + 8, 64
    g = torch.Generator(device=dev).manual_seed(200 + t)
    a, w = dy(g, (M, K), dtype=bf16), dy(g, (N, K), div=8, dtype=bf16)
    bias = dy(g, (N,), span=16)
    ref0 = TK.gemm_ref(L, a, w, bias, L.ACT_NONE, None, None, 0, False, False, False)      # bf16(acc + bias)
    case = lambda what: f"gemm_bf16 {name} {M}x{N}x{K} {what}"

    # out_f32 (+ fp32 residual)
    res32 = dy(g, (M, N))
    clean = ops.gemm(a, w, bias, residual=res32, out_f32=True, tile=t)
    r = relerr(clean, TK.gemm_ref(L, a, w, bias, L.ACT_NONE, res32, None, 0, False, False, True))
    assert r < TK.TOL_GEMM, (name, r)
    go, ins = _gemm_guarded(ops, a, w, bias, (M, N), f32, res=res32, out_f32=True, tile=t)
    verdict(parity, case("out_f32"), [("out", go, clean)], ins, rel_vs_fp32=r)

    # bias_row
    brow = dy(g, (M,), span=16)
    clean = ops.gemm(a, w, brow, bias_row=True, tile=t)
    r = relerr(clean, TK.gemm_ref(L, a, w, brow, L.ACT_NONE, None, None, 0, False, True, False))
    assert r < TK.TOL_GEMM, (name, r)
    go, ins = _gemm_guarded(ops, a, w, brow, (M, N), bf16, bias_row=True, tile=t)
    verdict(parity, case("bias_row"), [("out", go, clean)], ins, rel_vs_fp32=r)

    # per-batch scale, rows_per_batch not dividing M, scale rows strided
    rpb = M // 2 + 3
    sc = dy(g, ((M + rpb - 1) // rpb, N), span=4, div=2)
    clean = ops.gemm(a, w, bias, scale=sc, rows_per_batch=rpb, tile=t)
    r = relerr(clean, TK.gemm_ref(L, a, w, bias, L.ACT_NONE, None, sc, rpb, False, False, False))
    assert r < TK.TOL_GEMM, (name, r)
    gs = cv(sc, 4)
    go, ins = _gemm_guarded(ops, a, w, bias, (M, N), bf16, scale=gs, rows_per_batch=rpb, tile=t)
    verdict(parity, case("scale_per_batch"), [("out", go, clean)], ins + [("scale", gs, sc)], rel_vs_fp32=r)

    # residual table (res_row_mod) + residual2
    mod = 7
    tab, res2 = dy(g, (mod, N), dtype=bf16), dy(g, (M, N), dtype=bf16)
    clean = ops.gemm(a, w, bias, residual=tab, res_row_mod=mod, residual2=res2, tile=t)
    ref = (ref0.float() + tab.float()[torch.arange(M, device=dev) % mod] + res2.float()).to(bf16)
    r = relerr(clean, ref)
    assert r < TK.TOL_GEMM, (name, r)
    g2 = cv(res2, 8)
    go, ins = _gemm_guarded(ops, a, w, bias, (M, N), bf16, res=tab, res_row_mod=mod, residual2=g2, tile=t)
    verdict(parity, case("residual2+res_row_mod"), [("out", go, clean)], ins + [("residual2", g2, res2)], rel_vs_fp32=r)

    # out_rows scatter: the skipped rows of `out` are guard
    grp, skip, off = 16, 5, 2
    rows = torch.arange(M, device=dev)
    rows = rows + (rows // grp) * skip + off
    R = int(rows[-1]) + 1
    clean = torch.zeros(R, N, device=dev, dtype=bf16)
    ops.gemm(a, w, bias, out=clean, out_rows=(grp, skip, off), tile=t)
    r = relerr(clean[rows], ref0)
    assert r < TK.TOL_GEMM, (name, r)
    go, ins = _gemm_guarded(ops, a, w, bias, (R, N), bf16, out_rows=(grp, skip, off), tile=t)
    verdict(parity, case("out_rows"), [("out", go, clean, rows)], ins, rel_vs_fp32=r)

    # batch of 3 with strides larger than a problem (and a shared bias)
    nb, lda, ldc = 3, K + 8, N + 8
    a3, w3 = dy(g, (nb, M, K), dtype=bf16), dy(g, (nb, N, K), div=8, dtype=bf16)
    sa, sw, so = M * lda + 64, N * lda + 40, M * ldc + 24
    clean = torch.stack([ops.gemm(a3[z], w3[z], bias, tile=t) for z in range(nb)])
    r = max(relerr(clean[z], TK.gemm_ref(L, a3[z], w3[z], bias, L.ACT_NONE, None, None, 0, False, False, False)) for z in range(nb))
    assert r < TK.TOL_GEMM, (name, r)
    ga, gw = cv(a3, strides=(sa, lda, 1)), cv(w3, strides=(sw, lda, 1))
    go, gb = co((nb, M, N), bf16, strides=(so, ldc, 1)), cv(bias)
    ops.gemm(ga[0], gw[0], gb, out=go[0], batch=(nb, sa, sw, so), tile=t)
    verdict(parity, case("batch3"), [("out", go, clean)], [("a", ga, a3), ("w", gw, w3), ("bias", gb, bias)], rel_vs_fp32=r)

    # row_sumsq by-product (N % 32 == 0)
    N32 = BN + 32
    w32, b32 = dy(g, (N32, K), div=8, dtype=bf16), dy(g, (N32,), span=16)
    sq_clean = torch.zeros(M, N32 // 32, device=dev)
    clean = ops.gemm(a, w32, b32, row_sumsq=sq_clean, tile=t)
    want = clean.float().view(M, N32 // 32, 32).pow(2).sum(-1)
    rs = ((sq_clean - want).abs() / want.clamp_min(1e-20)).max().item()
    r = relerr(clean, TK.gemm_ref(L, a, w32, b32, L.ACT_NONE, None, None, 0, False, False, False))
    assert r < TK.TOL_GEMM and rs < TK.TOL_ROW_SUMSQ, (name, r, rs)
    gsq = co((M, N32 // 32), f32)
    go, ins = _gemm_guarded(ops, a, w32, b32, (M, N32), bf16, row_sumsq=gsq, tile=t)
    verdict(parity, case("row_sumsq"), [("out", go, clean), ("row_sumsq", gsq, sq_clean)], ins, rel_vs_fp32=r, row_sumsq_max_rel=rs)

    # split_k in {2, 4} at K = 512, workspace of exactly v3a_gemm_split_workspace_bytes
    a5, w5 = dy(g, (M, 512), dtype=bf16), dy(g, (N, 512), div=8, dtype=bf16)
    ref = TK.gemm_ref(L, a5, w5, bias, L.ACT_NONE, None, None, 0, False, False, False)
    wk = (torch.device(dev, torch.cuda.current_device()), threading.get_ident())
    for S in (2, 4):
        ops._gemm_ws.pop(wk, None)
        clean = ops.gemm(a5, w5, bias, split_k=S, tile=t)
        r = relerr(clean, ref)
        assert r < TK.TOL_GEMM_SPLIT_K, (name, S, r)
        ws = co((int(hip_lib.v3a_gemm_split_workspace_bytes(M, N, S)),), u8)
        ops._gemm_ws[wk] = ws
        try:
            go, ins = _gemm_guarded(ops, a5, w5, bias, (M, N), bf16, split_k=S, tile=t)
            assert ops._gemm_ws[wk] is ws
        finally:
            ops._gemm_ws.pop(wk, None)
        verdict(parity, case(f"split_k={S} K=512"), [("out", go, clean)], ins, written=[ws], rel_vs_fp32=r)


@pytest.mark.parametrize("M", [8, 264])
def test_gemm_transposed_tail(hip_lib, parity, M):
    """t_out / t_col0 = 192 (always the transposed-tail tile - v3a_gemm_pick_tile_ex(M, N, act, 1, has_tail=1) returns it whatever M, N; M % 8 == 0): `out` holds 192 columns, t_out [N - 192, M] with row stride > M."""
    from vist3a_amd import lib as L, ops
    N, K, t0 = 192 + 72, 64, 192
    g = torch.Generator(device=dev).manual_seed(300 + M)
    a, w, bias = dy(g, (M, K), dtype=bf16), dy(g, (N, K), div=8, dtype=bf16), dy(g, (N,), span=16)
    ref = TK.gemm_ref(L, a, w, bias, L.ACT_NONE, None, None, 0, False, False, False)
    qk, vt = torch.zeros(M, t0, device=dev, dtype=bf16), torch.zeros(N - t0, M, device=dev, dtype=bf16)
    ops.gemm(a, w, bias, out=qk, t_out=vt, t_col0=t0)
    r = max(relerr(qk, ref[:, :t0]), relerr(vt, ref[:, t0:].t()))
    assert r < TK.TOL_GEMM, r
    ga, gw, gb = cv(a, 8), cv(w, 8), cv(bias)
    go, gt = co((M, t0), bf16, 8), co((N - t0, M), bf16, 8)
    ops.gemm(ga, gw, gb, out=go, t_out=gt, t_col0=t0)
    verdict(parity, f"gemm_bf16 transposed_tail {M}x{N}x{K}", [("out", go, qk), ("t_out", gt, vt)], [("a", ga, a), ("w", gw, w), ("bias", gb, bias)],
            rel_vs_fp32=r)


def _fp8_ref(a8, sa, w8, sw, bias):
    """test_gemm_fp8_every_tile_matches_e4m3_emulation's reference: e4m3 values held in fp32, fp32 matmul, scale product, bias, bf16"""
    qa, qw = a8.view(torch.float8_e4m3fn).float(), w8.view(torch.float8_e4m3fn).float()
    return ((qa @ qw.T) * (sa[:, None] * sw[None, :]) + bias[None, :]).to(bf16)


@pytest.mark.parametrize("t", range(NT8))
def test_gemm_fp8_tile_ragged_grid(hip_lib, parity, t):
    """The e4m3 tiles: M in {1, BM-1, BM+1} x N in {8, BN-8, BN+8} x K in {128, 384}, strides at the `% 16` bytes its checks allow."""
    from vist3a_amd import ops
    name = hip_lib.v3a_gemm_fp8_tile_name(t).decode()
    BM, BN = tile_dims(name)
    g = torch.Generator(device=dev).manual_seed(400 + t)
    for M in (1, BM - 1, BM + 1):
        for N in (8, BN - 8, BN + 8):
            for K in (128, 384):
                a = torch.randn(M, K, device=dev, generator=g).to(bf16)
                w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(bf16)
                bias, res = torch.randn(N, device=dev, generator=g), torch.randn(M, N, device=dev, generator=g).to(bf16)
                (a8, sa), (w8, sw) = ops.quantize_fp8_rows(a), ops.quantize_fp8_rows(w)
                clean0 = ops.gemm(a8, w8, bias, a_scale=sa, w_scale=sw, tile=t)
                r = relerr(clean0, _fp8_ref(a8, sa, w8, sw, bias))
                assert math.isfinite(r) and r < TK.TOL_GEMM_FP8, (name, M, N, K, r)
                clean = ops.gemm(a8, w8, bias, residual=res, a_scale=sa, w_scale=sw, tile=t)
                for off in (0, 16):        # 16: the smallest alignment the `% 16` byte checks leave to a pointer
                    ga, gw, gb, gr = cv(a8, 16, off), cv(w8, 16, off), cv(bias), cv(res, 8, off)
                    gsa, gsw, go = cv(sa), cv(sw), co((M, N), bf16, 8, off)
                    ops.gemm(ga, gw, gb, out=go, residual=gr, a_scale=gsa, w_scale=gsw, tile=t)
                    verdict(parity, f"gemm_fp8 {name} {M}x{N}x{K}" + (" align16" if off else ""), [("out", go, clean)],
                            [("a", ga, a8), ("w", gw, w8), ("bias", gb, bias), ("residual", gr, res), ("a_scale", gsa, sa), ("w_scale", gsw, sw)],
                            rel_vs_e4m3_emulation=r)


# ------------------------------------------------------------------------------------------------------------------ skinny GEMM
@pytest.mark.parametrize("transposed", [False, True], ids=["rows_small", "cols_small"])
@pytest.mark.parametrize("Ms", [1, 13, 128])
@pytest.mark.parametrize("Nb", [512, 520])
def test_gemm_skinny(hip_lib, parity, transposed, Ms, Nb):
    """v3a_gemm_skinny_bf16, both orientations, K = 1024, its workspace of EXACTLY v3a_gemm_skinny_workspace_bytes (through the C ABI:
    ops keeps a larger cached buffer)."""
    import ctypes as C
    from vist3a_amd import lib as L, ops
    K = 1024
    g = torch.Generator(device=dev).manual_seed(500 + Ms + Nb)
    x, wb = dy(g, (Ms, K), dtype=bf16), dy(g, (Nb, K), div=8, dtype=bf16)
    bias = dy(g, (Nb,), span=16)
    a, w = (wb, x) if transposed else (x, wb)                # out[M, N] = a . w^T in both orientations
    oshape = (Nb, Ms) if transposed else (Ms, Nb)
    res = dy(g, oshape, dtype=bf16)
    ref = TK.gemm_ref(L, a, w, bias, L.ACT_NONE, res, None, 0, False, transposed, False)
    need = int(hip_lib.v3a_gemm_skinny_workspace_bytes(Ms, Nb, K))
    assert need > 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(x_, w_, b_, r_, o_, ws_):
        args = L.GemmSkinnyArgs(x_.data_ptr(), w_.data_ptr(), o_.data_ptr(), b_.data_ptr(), r_.data_ptr(), Ms, Nb, K, x_.stride(0), w_.stride(0),
                                o_.stride(0), r_.stride(0), L.ACT_NONE, 0, int(transposed), ws_.data_ptr(), ws_.numel())
        L.check(hip_lib.v3a_gemm_skinny_bf16(C.byref(args), st), "v3a_gemm_skinny_bf16")

    clean = torch.zeros(oshape, device=dev, dtype=bf16)
    run(x, wb, bias, res, clean, torch.empty(need, device=dev, dtype=u8))
    r = relerr(clean, ref)
    assert r < TK.TOL_GEMM, r
    assert torch.equal(clean, ops.gemm(a, w, bias, residual=res, bias_row=transposed))      # ... and it is what ops.gemm dispatches to
    pad_o = 8 if not transposed or Ms % 8 == 0 else 8 - Ms % 8 + 8                           # ldc % 8 == 0
    gx, gw, gb, gr = cv(x, 8), cv(wb, 8), cv(bias), cv(res, pad_o)
    go, ws = co(oshape, bf16, pad_o), co((need,), u8)
    run(gx, gw, gb, gr, go, ws)
    verdict(parity, f"gemm_skinny transposed={transposed} {Ms}x{Nb}x{K}", [("out", go, clean)],
            [("x", gx, x), ("w", gw, wb), ("bias", gb, bias), ("residual", gr, res)], written=[ws], rel_vs_fp32=r)


# ------------------------------------------------------------------------------------------------------------------ flash attention
def _attn_case(hip_lib, parity, case, B, H, Nq, Nk, D, seed, *, opt=None, fp8=False, off=0):
    """One clean + one guarded flash-attention launch.  q, k, out are column slices' worth of wider buffers (ld = H D + pad), V^T has a batch
    stride > Nk (rounded up to 64) and a row stride beyond the last batch item."""
    from vist3a_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    q, k, v, vt, nkp = TK._attn_inputs(B, H, Nq, Nk, D, g)
    HD, opt = H * D, opt or {}
    kw, ref_kw = {}, {}
    if opt.get("kv_period"):
        kw.update(kv_period=opt["kv_period"], kv_valid=opt["kv_valid"])
        ref_kw["mask"] = (torch.arange(Nk, device=dev) % opt["kv_period"]) < opt["kv_valid"]
    if opt.get("key_bias"):
        kb = torch.randn(B, Nk, device=dev, generator=g)
        kw.update(key_bias=kb)
        ref_kw["bias"] = kb
    # ---- clean
    if fp8:
        qs, ks, vs = 0.5, 0.25, 2.0
        q8, k8, vt8 = ops.quantize_fp8(q.view(B * Nq, HD), qs), ops.quantize_fp8(k.view(B * Nk, HD), ks), ops.quantize_fp8(vt, vs)
        clean = torch.empty(B * Nq, HD, device=dev, dtype=bf16)
        ops.attention_fp8(q8, k8, vt8, clean, B=B, H=H, Nq=Nq, Nk=Nk, q_batch_stride=Nq * HD, k_batch_stride=Nk * HD, vt_batch_stride=nkp,
                          o_batch_stride=Nq * HD, q_scale=qs, k_scale=ks, v_scale=vs)
        from oracle import wan_dit as O
        sh = lambda t, n: t.float().cpu().view(B, n, H, D).transpose(1, 2)
        emu = O.attention_fp8_emulated(sh(q, Nq), sh(k, Nk), sh(v, Nk), D ** -0.5, qs, ks, vs).transpose(1, 2)
        errs = dict(rel_vs_e4m3_emulation=relerr(clean.view(B, Nq, H, D).float().cpu(), emu))
        assert errs["rel_vs_e4m3_emulation"] < TK.TOL_ATTN_FP8_EMU, (case, errs)
        qv, kv_, vtv, apad = q8, k8, vt8, 16
    else:
        wk = (torch.device(dev, torch.cuda.current_device()), threading.get_ident())
        ops._attn_ws.pop(wk, None)
        clean = TK._run_attn(q, k, vt, nkp, B, H, Nq, Nk, D, kv_split=opt.get("kv_split", 1), **kw).reshape(B * Nq, HD)
        ref = TK._attn_ref(q, k, v, B, H, D, **ref_kw).reshape(B * Nq, HD)
        errs = dict(rel_vs_fp32=relerr(clean, ref))
        if opt.get("kv_split", 1) > 1:
            assert errs["rel_vs_fp32"] < TK.TOL_ATTN_SPLIT_EXACT, (case, errs)
        else:
            errs["rel_vs_contract"] = relerr(clean, TK._attn_emu(q, k, v, B, H, D, **ref_kw).reshape(B * Nq, HD))
            assert errs["rel_vs_fp32"] < TK.TOL_ATTN_EXACT and errs["rel_vs_contract"] < TK.TOL_ATTN_CONTRACT, (case, errs)
        qv, kv_, vtv, apad = q.view(B * Nq, HD), k.view(B * Nk, HD), vt, 8
    # ---- guarded
    gq, gk, go = cv(qv, apad, off), cv(kv_, apad, off), co((B * Nq, HD), bf16, 8, off)
    vbs = nkp + 64
    ldvt = B * vbs + apad
    vt3 = vtv.view(HD, B, nkp).clone()
    vt3[:, :, Nk:] = torch.tensor(3.0).to(bf16) if not fp8 else ops.quantize_fp8(torch.full((1, 16), 3.0, device=dev, dtype=bf16), vs)[0, 0]
    gvt = cv(vt3, off=off, strides=(ldvt, vbs, 1))
    vt2 = gvt.as_strided((HD, (B - 1) * vbs + nkp), (ldvt, 1))
    ins = [("q", gq, qv), ("k", gk, kv_), ("vt", gvt, vt3)]
    if "key_bias" in kw:
        gkb = cv(kw["key_bias"], 4)
        ins.append(("key_bias", gkb, kw["key_bias"]))
        kw = dict(kw, key_bias=gkb)
    written = []
    common = dict(B=B, H=H, Nq=Nq, Nk=Nk, q_batch_stride=Nq * gq.stride(0), k_batch_stride=Nk * gk.stride(0), vt_batch_stride=vbs,
                  o_batch_stride=Nq * go.stride(0))
    if fp8:
        ops.attention_fp8(gq, gk, vt2, go, q_scale=qs, k_scale=ks, v_scale=vs, **common)
    else:
        if opt.get("kv_split", 1) > 1:
            S = opt["kv_split"]
            ws = co((int(hip_lib.v3a_attention_split_workspace_bytes(B, H, Nq, D, S)),), u8)
            ops._attn_ws[wk] = ws
            written.append(ws)
            kw = dict(kw, kv_split=S)
        try:
            ops.attention(gq, gk, vt2, go, D=D, **common, **kw)
            assert not written or ops._attn_ws[wk] is written[0]
        finally:
            ops._attn_ws.pop(wk, None)
    verdict(parity, case, [("out", go, clean)], ins, written=written, **errs)


RAGGED = [(1, 1), (63, 65), (130, 200)]


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("Nq,Nk", RAGGED + [(64, 64), (128, 128)], ids=lambda v: str(v))
def test_attention_bf16_ragged_and_plain(hip_lib, parity, D, Nq, Nk):
    """(Nq, Nk) ragged against the 64-key tile, and Nk % 64 == 0 (the plain instantiation at D = 128); B = 2, H = 3."""
    _attn_case(hip_lib, parity, f"attention_bf16 D={D} {Nq}x{Nk}", 2, 3, Nq, Nk, D, 600 + Nq + D)
    if (Nq, Nk) in ((63, 65), (64, 64)):      # q / k / vt / out at the smallest alignment the `% 8` element checks leave to a pointer
        _attn_case(hip_lib, parity, f"attention_bf16 D={D} {Nq}x{Nk} align16", 2, 3, Nq, Nk, D, 600 + Nq + D, off=16)


@pytest.mark.parametrize("what,D,opt", [
    ("kv_period", 128, dict(kv_period=50, kv_valid=47)),
    ("kv_period_hd64", 64, dict(kv_period=50, kv_valid=47)),
    ("key_bias", 128, dict(key_bias=True)),                   # stride Nk + 4 > Nk
    ("kv_split3", 128, dict(kv_split=3)),                     # workspace of exactly v3a_attention_split_workspace_bytes, pre-seeded into ops._attn_ws
], ids=lambda v: v if isinstance(v, str) else "")
def test_attention_bf16_options(hip_lib, parity, what, D, opt):
    _attn_case(hip_lib, parity, f"attention_bf16 D={D} 130x200 {what}", 2, 3, 130, 200, D, 700 + D, opt=opt)


def test_attention_bf16_rel_bias_hd64(hip_lib, parity):
    """rel_bias (D = 64): contiguous fp32 [H, n] table, entry (key - query + center)."""
    from vist3a_amd import ops
    B, H, Nq, Nk, D = 2, 3, 63, 65, 64
    g = torch.Generator(device=dev).manual_seed(71)
    q, k, v, vt, nkp = TK._attn_inputs(B, H, Nq, Nk, D, g)
    center, n = Nq - 1, Nq - 1 + Nk
    tab = torch.randn(H, n, device=dev, generator=g)
    clean = TK._run_attn(q, k, vt, nkp, B, H, Nq, Nk, D, rel_bias=tab, rel_bias_center=center).reshape(B * Nq, H * D)
    idx = torch.arange(Nk, device=dev)[None, :] - torch.arange(Nq, device=dev)[:, None] + center
    hs = lambda t: t.float().view(B, -1, H, D).transpose(1, 2)
    s = hs(q) @ hs(k).transpose(-1, -2) * D ** -0.5 + tab[:, idx][None]
    ref = (torch.softmax(s, -1) @ hs(v)).transpose(1, 2).reshape(B * Nq, H * D)
    r = relerr(clean, ref)
    assert r < TK.TOL_ATTN_EXACT, r
    HD = H * D
    gq, gk, go, gt = cv(q.view(B * Nq, HD), 8), cv(k.view(B * Nk, HD), 8), co((B * Nq, HD), bf16, 8), cv(tab)
    vbs, vt3 = nkp + 64, vt.view(HD, B, nkp).clone()
    vt3[:, :, Nk:] = 3.0
    gvt = cv(vt3, strides=(B * vbs + 8, vbs, 1))
    ops.attention(gq, gk, gvt.as_strided((HD, (B - 1) * vbs + nkp), (B * vbs + 8, 1)), go, B=B, H=H, Nq=Nq, Nk=Nk, D=D,
                  q_batch_stride=Nq * gq.stride(0), k_batch_stride=Nk * gk.stride(0), vt_batch_stride=vbs, o_batch_stride=Nq * go.stride(0),
                  rel_bias=gt, rel_bias_center=center)
    verdict(parity, "attention_bf16 D=64 63x65 rel_bias", [("out", go, clean)],
            [("q", gq, q.view(B * Nq, HD)), ("k", gk, k.view(B * Nk, HD)), ("vt", gvt, vt3), ("rel_bias", gt, tab)], rel_vs_fp32=r)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_attention_kv_seg_slabs_with_strides_larger_than_a_slab(hip_lib, parity, fp8):
    """kv_seg = 64 of Nk = 128: K and V^T read in place from two slabs whose strides exceed a slab; between the slabs lies poison.  (The entry
    points require kv_seg % 64 == 0 and Nk % kv_seg == 0, so a segment is never ragged: V^T is read to exactly the segment's end.)"""
    from vist3a_amd import ops
    B, H, Nq, Nk, D, seg = 2, 3, 130, 128, 128, 64
    HD, nseg = H * D, Nk // seg
    g = torch.Generator(device=dev).manual_seed(81)
    q, k, v, vt, nkp = TK._attn_inputs(B, H, Nq, Nk, D, g)
    assert nkp == Nk
    qv, kv_, vtv, pad = q.view(B * Nq, HD), k.view(B * Nk, HD), vt, 8
    if fp8:
        qv, kv_, vtv, pad = ops.quantize_fp8(qv), ops.quantize_fp8(kv_), ops.quantize_fp8(vt), 16
        run, kwd = ops.attention_fp8, {}
    else:
        run, kwd = ops.attention, dict(D=D)
    clean = torch.empty(B * Nq, HD, device=dev, dtype=bf16)
    run(qv, kv_, vtv, clean, B=B, H=H, Nq=Nq, Nk=Nk, q_batch_stride=Nq * HD, k_batch_stride=Nk * HD, vt_batch_stride=nkp, o_batch_stride=Nq * HD, **kwd)
    if fp8:
        from oracle import wan_dit as O
        sh = lambda t, n: t.float().cpu().view(B, n, H, D).transpose(1, 2)
        emu = O.attention_fp8_emulated(sh(q, Nq), sh(k, Nk), sh(v, Nk), D ** -0.5, 1.0, 1.0, 1.0).transpose(1, 2)
        errs = dict(rel_vs_e4m3_emulation=relerr(clean.view(B, Nq, H, D).float().cpu(), emu))
        assert errs["rel_vs_e4m3_emulation"] < TK.TOL_ATTN_FP8_EMU, errs
    else:
        errs = dict(rel_vs_fp32=relerr(clean, TK._attn_ref(q, k, v, B, H, D).reshape(B * Nq, HD)),
                    rel_vs_contract=relerr(clean, TK._attn_emu(q, k, v, B, H, D).reshape(B * Nq, HD)))
        assert errs["rel_vs_fp32"] < TK.TOL_ATTN_EXACT and errs["rel_vs_contract"] < TK.TOL_ATTN_CONTRACT, errs
    ldk = HD + pad
    kbs = seg * ldk + 64
    kss = B * kbs + 128
    k4 = kv_.view(B, nseg, seg, HD).permute(1, 0, 2, 3).contiguous()          # [segment, batch, key, H D]
    gk = cv(k4, strides=(kss, kbs, ldk, 1))
    vbs = seg + 16
    ldvt = B * vbs + pad
    vss = HD * ldvt + 64
    v4 = vtv.view(HD, B, nseg, seg).permute(2, 0, 1, 3).contiguous()          # [segment, H D, batch, key]
    gv = cv(v4, strides=(vss, ldvt, vbs, 1))
    gq, go = cv(qv, pad), co((B * Nq, HD), bf16, 8)
    run(gq, gk.as_strided((seg, HD), (ldk, 1)), gv.as_strided((HD, seg), (ldvt, 1)), go, B=B, H=H, Nq=Nq, Nk=Nk, q_batch_stride=Nq * gq.stride(0),
        k_batch_stride=kbs, vt_batch_stride=vbs, o_batch_stride=Nq * go.stride(0), kv_seg=seg, k_seg_stride=kss, vt_seg_stride=vss, **kwd)
    verdict(parity, f"attention_{'fp8' if fp8 else 'bf16'} kv_seg slabs", [("out", go, clean)], [("q", gq, qv), ("k", gk, k4), ("vt", gv, v4)], **errs)


@pytest.mark.parametrize("Nq,Nk", RAGGED, ids=lambda v: str(v))
def test_attention_fp8_ragged(hip_lib, parity, Nq, Nk):
    """The e4m3 flash kernel at the ragged pairs, strides at the `% 16` bytes its checks allow."""
    _attn_case(hip_lib, parity, f"attention_fp8 {Nq}x{Nk}", 2, 3, Nq, Nk, 128, 900 + Nq, fp8=True)
    if Nq == 63:
        _attn_case(hip_lib, parity, f"attention_fp8 {Nq}x{Nk} align16", 2, 3, Nq, Nk, 128, 900 + Nq, fp8=True, off=16)


@pytest.mark.parametrize("with_sumsq", [False, True], ids=["normalised_q", "q_row_sumsq"])
@pytest.mark.parametrize("Nk", [1, 77, 128])
def test_xattn_probs(hip_lib, parity, Nk, with_sumsq):
    """Nk in {1, 77, 128}, Lkp = Nk rounded up to 16: the padding columns Nk <= j < Lkp of every head are written (zeros) and lie inside the
    [rows, H Lkp] region; everything beyond it, and the key rows past Nk of each batch item, are poison."""
    from vist3a_amd import ops
    B, H, Nq, D = 2, 3, 70, 128
    Lkp, HD = (Nk + 15) // 16 * 16, H * D
    g = torch.Generator(device=dev).manual_seed(1000 + Nk)
    q = (torch.randn(B * Nq, HD, device=dev, generator=g) * (3.0 if with_sumsq else 1.0)).to(bf16)
    k = torch.randn(B, Nk, HD, device=dev, generator=g).to(bf16)
    bias = torch.zeros(B, Nk, device=dev)
    bias[:, Nk - 1] = math.log(512 - (Nk - 1))
    sq = q.float().view(B * Nq, HD // 32, 32).pow(2).sum(-1).contiguous() if with_sumsq else None
    eps = 1e-6
    clean = torch.empty(B * Nq, H * Lkp, device=dev, dtype=bf16)
    ops.xattn_probs(q, k.view(B * Nk, HD), clean, B=B, H=H, Nq=Nq, Nk=Nk, Lkp=Lkp, q_batch_stride=Nq * HD, k_batch_stride=Nk * HD,
                    p_batch_stride=Nq * H * Lkp, key_bias=bias, key_bias_first=Nk - 1, q_row_sumsq=sq, q_eps=eps)
    qf, kf = q.float().view(B, Nq, H, D).transpose(1, 2), k.float().view(B, Nk, H, D).transpose(1, 2)
    s = qf @ kf.transpose(-1, -2) * D ** -0.5
    if with_sumsq:
        s = s * torch.rsqrt(q.float().pow(2).mean(-1) + eps).view(B, 1, Nq, 1)
    ref = torch.softmax(s + bias[:, None, None, :], -1)
    got = clean.float().view(B, Nq, H, Lkp).permute(0, 2, 1, 3)
    r = ((got[..., :Nk] - ref).norm() / ref.norm()).item()
    assert r < TK.TOL_XATTN and (got[..., Nk:] == 0).all(), r
    gq, go, gb = cv(q, 8), co((B * Nq, H * Lkp), bf16, 8), cv(bias, 4)
    ldk = HD + 8
    kbs = Nk * ldk + 5 * ldk                                       # the key buffer has more rows than keys
    gk = cv(k, strides=(kbs, ldk, 1))
    gsq = cv(sq) if with_sumsq else None
    ops.xattn_probs(gq, gk.as_strided((Nk, HD), (ldk, 1)), go, B=B, H=H, Nq=Nq, Nk=Nk, Lkp=Lkp, q_batch_stride=Nq * gq.stride(0), k_batch_stride=kbs,
                    p_batch_stride=Nq * go.stride(0), key_bias=gb, key_bias_first=Nk - 1, q_row_sumsq=gsq, q_eps=eps)
    verdict(parity, f"xattn_probs Nk={Nk} Lkp={Lkp} sumsq={with_sumsq}", [("p", go, clean)],
            [("q", gq, q), ("k", gk, k), ("key_bias", gb, bias)] + ([("q_row_sumsq", gsq, sq)] if with_sumsq else []), rel_vs_fp32=r)


# ------------------------------------------------------------------------------------------------------------------ row kernels
ROWS = [1, 3, 257]
WIDTHS = [8, 520]     # the smallest legal width, and one that is no multiple of (8 elements per lane x 64 lanes)


@pytest.mark.parametrize("off", [0, 16], ids=["align256", "align16"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_layernorm(hip_lib, parity, off, M, d):
    """AdaLN form, bf16 out and e4m3 out (fp8_scale); ldx = d + 8, ldy = d + 16."""
    from vist3a_amd import ops
    g = torch.Generator(device=dev).manual_seed(1100 + M + d)
    x = (torch.randn(M, d, device=dev, generator=g) * 2 + 0.5).to(bf16)
    rpb = M // 2 + 1
    nb = (M + rpb - 1) // rpb
    sc, sh = torch.randn(nb, d, device=dev, generator=g) * 0.3, torch.randn(nb, d, device=dev, generator=g) * 0.3
    clean = ops.layernorm(x, scale=sc, shift=sh, rows_per_batch=rpb, eps=1e-6)
    idx = torch.arange(M, device=dev) // rpb
    ref = (torch.nn.functional.layer_norm(x.float(), (d,), eps=1e-6) * (1 + sc[idx]) + sh[idx]).to(bf16)
    r = relerr(clean, ref)
    assert r < TK.TOL_LN_ADALN, r
    gx, gsc, gsh, go = cv(x, 8, off), cv(sc, 8), cv(sh, 8), co((M, d), bf16, 16, off)
    ops.layernorm(gx, out=go, scale=gsc, shift=gsh, rows_per_batch=rpb, eps=1e-6)
    ins = [("x", gx, x), ("scale", gsc, sc), ("shift", gsh, sh)]
    verdict(parity, f"layernorm adaln bf16 {M}x{d}" + (" align16" if off else ""), [("y", go, clean)], ins, rel_vs_fp32=r)
    # e4m3 out: bit-identical to the bf16 result pushed through v3a_quantize_fp8_rows (test_layernorm_fp8_output_equals_separate_quantisation_pass)
    q_ref, s_ref = ops.quantize_fp8_rows(clean)
    go8, gs8 = co((M, d), u8, 16, off), co((M,), f32)
    ops.layernorm(gx, out=go8, fp8_scale=gs8, scale=gsc, shift=gsh, rows_per_batch=rpb, eps=1e-6)
    verdict(parity, f"layernorm adaln e4m3 {M}x{d}" + (" align16" if off else ""), [("y", go8, q_ref), ("fp8_scale", gs8, s_ref)], ins, rel_vs_fp32=r)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_layernorm_f32_affine(hip_lib, parity, M, d):
    from vist3a_amd import ops
    g = torch.Generator(device=dev).manual_seed(1200 + M + d)
    x = torch.randn(M, d, device=dev, generator=g) * 2.7 + 0.7
    w, b = torch.randn(d, device=dev, generator=g), torch.randn(d, device=dev, generator=g)
    clean = ops.layernorm(x, weight=w, bias=b, eps=1e-5, out_dtype=f32)
    r = relerr(clean, torch.nn.functional.layer_norm(x, (d,), w, b, eps=1e-5))
    assert r < TK.TOL_LN_F32, r
    gx, gw, gb, go = cv(x, 8), cv(w), cv(b), co((M, d), f32, 16)
    ops.layernorm(gx, out=go, weight=gw, bias=gb, eps=1e-5)
    verdict(parity, f"layernorm affine f32 {M}x{d}", [("y", go, clean)], [("x", gx, x), ("weight", gw, w), ("bias", gb, b)], rel_vs_fp32=r)


@pytest.mark.parametrize("off", [0, 16], ids=["align256", "align16"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("H,hd", [(1, 8), (5, 104)], ids=["d8", "d520"])
@pytest.mark.parametrize("form", ["plain", "rope", "rope_weight2"])
def test_rmsnorm_rope(hip_lib, parity, off, M, H, hd, form):
    from vist3a_amd import ops
    d = H * hd
    g = torch.Generator(device=dev).manual_seed(1300 + M + d)
    cols = 2 * d if form == "rope_weight2" else d
    x = torch.randn(M, cols, device=dev, generator=g).to(bf16)
    w, w2 = torch.randn(d, device=dev, generator=g), torch.randn(d, device=dev, generator=g)
    ang = torch.rand(M, hd // 2, device=dev, generator=g, dtype=torch.float64) * 6.28
    rope = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous() if form != "plain" else None
    kw = dict(head_dim=hd, tokens_per_batch=M, eps=1e-6) if rope is not None else dict(eps=1e-6)

    def ref_half(xh, wh):
        xf = xh.float()
        n = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * wh
        if rope is None:
            return n.to(bf16)
        nc = torch.view_as_complex(n.double().view(1, M, H, hd // 2, 2))
        fc = torch.polar(torch.ones_like(ang), ang)[None, :, None, :]
        return torch.view_as_real(nc * fc).reshape(M, d).to(bf16)

    ref = torch.cat([ref_half(x[:, :d], w), ref_half(x[:, d:], w2)], 1) if form == "rope_weight2" else ref_half(x, w)
    clean = ops.rmsnorm_rope(x, w, rope=rope, weight2=w2 if form == "rope_weight2" else None, **kw)
    r = relerr(clean, ref)
    assert r < TK.TOL_RMSNORM_ROPE, r
    gx, gw, gw2, go = cv(x, 8, off), cv(w), cv(w2), co((M, cols), bf16, 16, off)
    grope = cv(rope) if rope is not None else None
    ops.rmsnorm_rope(gx, gw, out=go, rope=grope, weight2=gw2 if form == "rope_weight2" else None, **kw)
    ins = [("x", gx, x), ("weight", gw, w), ("weight2", gw2, w2)] + ([("rope", grope, rope)] if rope is not None else [])
    verdict(parity, f"rmsnorm_rope {form} {M}x{cols}" + (" align16" if off else ""), [("y", go, clean)], ins, rel_vs_fp32=r)


@pytest.mark.parametrize("off", [0, 16], ids=["align256", "align16"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode,silu", [(1, True), (0, False)], ids=["wan_rms_silu", "rmsnorm"])
def test_rownorm_act(hip_lib, parity, off, M, d, mode, silu):
    """Through the C ABI (ops.rownorm_act passes ld = d): ldx = d + 8, ldy = d + 16; reference and gate of test_rownorm_act_matches_wan_rms_norm."""
    import ctypes as C
    from vist3a_amd import lib as L, ops
    F = torch.nn.functional
    g = torch.Generator(device=dev).manual_seed(1350 + M + d)
    x = (torch.randn(M, d, device=dev, generator=g) * 1.7).to(bf16)
    w = 1 + 0.2 * torch.randn(d, device=dev, generator=g)
    b = 0.1 * torch.randn(d, device=dev, generator=g) if mode == 1 else None
    act = L.ACT_SILU if silu else L.ACT_NONE
    clean = ops.rownorm_act(x, w, bias=b, mode=mode, act=act, eps=1e-6)
    xf = x.float()
    ref = F.normalize(xf, dim=-1) * math.sqrt(d) * w + b if mode == 1 else xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    ref = F.silu(ref) if silu else ref
    r = relerr(clean, ref)
    assert r < TS.TOL_ROWNORM, r
    gx, gw, go = cv(x, 8, off), cv(w), co((M, d), bf16, 16, off)
    gb = cv(b) if b is not None else None
    p_ = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    args = L.RowNormArgs(p_(gx), p_(go), p_(gw), p_(gb), M, d, gx.stride(0), go.stride(0), 1e-6, mode, act)
    L.check(hip_lib.v3a_rownorm_act(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v3a_rownorm_act")
    verdict(parity, f"rownorm_act mode={mode} silu={silu} {M}x{d}" + (" align16" if off else ""), [("y", go, clean)],
            [("x", gx, x), ("weight", gw, w)] + ([("bias", gb, b)] if b is not None else []), rel_vs_fp32=r)


@pytest.mark.parametrize("off", [0, 16], ids=["align256", "align16"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N", [4, 260])
def test_softmax_rows(hip_lib, parity, off, M, N):
    from vist3a_amd import ops
    g = torch.Generator(device=dev).manual_seed(1400 + M + N)
    s = torch.randn(M, N, device=dev, generator=g) * 30
    s[0, 3] = 400.0
    clean = ops.softmax_rows(s, 0.05)
    r = relerr(clean, torch.softmax(s * 0.05, -1))
    assert r < TS.TOL_SOFTMAX_ROWS, r
    gs, go = cv(s, 4, off), co((M, N), bf16, 8, off)
    ops.softmax_rows(gs, 0.05, out=go)
    verdict(parity, f"softmax_rows {M}x{N}" + (" align16" if off else ""), [("p", go, clean)], [("s", gs, s)], rel_vs_fp32=r)


@pytest.mark.parametrize("off", [0, 16], ids=["align256", "align16"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("cols", [16, 528])
def test_quantize_fp8(hip_lib, parity, off, M, cols):
    """per-tensor (cols % 16) and per-row (cols % 8: 8 and 520) quantisers: bit-exact against torch's RNE e4m3 conversion, as their own tests ask."""
    from vist3a_amd import ops
    g = torch.Generator(device=dev).manual_seed(1500 + M + cols)
    x = (torch.randn(M, cols, device=dev, generator=g) * 4).to(bf16)
    clean = ops.quantize_fp8(x, 0.5)
    assert torch.equal(clean, x.float().div(0.5).clamp(-448, 448).to(torch.float8_e4m3fn).view(u8))
    gx, go = cv(x, 8, off), co((M, cols), u8, 16, off)
    ops.quantize_fp8(gx, 0.5, out=go)
    verdict(parity, f"quantize_fp8 {M}x{cols}" + (" align16" if off else ""), [("y", go, clean)], [("x", gx, x)], rel_vs_fp32=0.0)
    c8 = cols - 8
    x8 = x[:, :c8].contiguous()
    q, sc = ops.quantize_fp8_rows(x8)
    rq, rsc = TK._quant_rows_emu(x8)
    assert torch.equal(sc, rsc) and torch.equal(q, rq.view(u8))
    gx, go, gs = cv(x8, 8, off), co((M, c8), u8, 8, off), co((M,), f32)
    ops.quantize_fp8_rows(gx, out=go, scale=gs)
    verdict(parity, f"quantize_fp8_rows {M}x{c8}" + (" align16" if off else ""), [("y", go, q), ("scale", gs, sc)], [("x", gx, x8)], rel_vs_fp32=0.0)


@pytest.mark.parametrize("M", [1, 3, 32])       # the entry point takes at most 32 rows
@pytest.mark.parametrize("N,K", [(1, 4), (9, 1028)])
def test_linear_f32(hip_lib, parity, M, N, K):
    """Through the C ABI (ops.linear_f32 allocates y itself): ldx = K + 4, ldy = N + 3, ldr = N + 5."""
    import ctypes as C
    from vist3a_amd import lib as L, ops
    g = torch.Generator(device=dev).manual_seed(1600 + M + N)
    x, w = torch.randn(M, K, device=dev, generator=g), torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)
    b, res, gam = torch.randn(N, device=dev, generator=g) * 0.1, torch.randn(M, N, device=dev, generator=g), 0.3 + 0.1 * torch.randn(N, device=dev, generator=g)
    clean = ops.linear_f32(x, w, b, residual=res, gamma=gam)
    ref = res.double() + gam.double() * (x.double() @ w.double().t() + b.double())
    r = relerr(clean.double(), ref)
    assert r < TS.TOL_LINEAR_F32, r
    gx, gw, gb, gr, gg, go = cv(x, 4), cv(w), cv(b), cv(res, 5), cv(gam), co((M, N), f32, 3)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(hip_lib.v3a_linear_f32(p(gx), p(gw), p(gb), p(go), p(gr), p(gg), M, N, K, gx.stride(0), go.stride(0), gr.stride(0), L.ACT_NONE, st),
            "v3a_linear_f32")
    verdict(parity, f"linear_f32 {M}x{N}x{K}", [("y", go, clean)], [("x", gx, x), ("w", gw, w), ("bias", gb, b), ("residual", gr, res), ("gamma", gg, gam)],
            rel_vs_fp64=r)


@pytest.mark.parametrize("S", [2, 13, 64])
def test_attention_small_f32(hip_lib, parity, S):
    """contiguous-only: bands before and after qkv and out (C ABI: the wrapper allocates out)."""
    import ctypes as C
    from vist3a_amd import lib as L, ops
    H, hd = 2, 16
    g = torch.Generator(device=dev).manual_seed(1700 + S)
    qkv = torch.randn(S, 3 * H * hd, device=dev, generator=g)
    clean = ops.attention_small_f32(qkv, H)
    q, k, v = qkv.double().view(S, 3, H, hd).permute(1, 2, 0, 3)
    ref = (torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1) @ v).permute(1, 0, 2).reshape(S, H * hd)
    r = relerr(clean.double(), ref)
    assert r < TS.TOL_ATTN_SMALL_F32, r
    gq, go = cv(qkv), co((S, H * hd), f32)
    L.check(hip_lib.v3a_attention_small_f32(C.c_void_p(gq.data_ptr()), C.c_void_p(go.data_ptr()), S, H, hd, hd ** -0.5,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v3a_attention_small_f32")
    verdict(parity, f"attention_small_f32 S={S}", [("out", go, clean)], [("qkv", gq, qkv)], rel_vs_fp64=r)


# ------------------------------------------------------------------------------------------------------------------ contiguous-only kernels
@pytest.mark.parametrize("n", [1, 7, 1027])
def test_adam_step(hip_lib, parity, n):
    """Two steps from a zero state, in place on p / m / v (exempt from `unchanged`, not from their bands); g is an input.  Reference, metric and
    gate of test_post_opt_gpu.test_adam_matches_torch: torch.optim.Adam in fp64, largest elementwise relative error of p, m, v."""
    import test_post_opt_gpu as TP
    from vist3a_amd import ops
    gen = torch.Generator().manual_seed(1800 + n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 0.1 for _ in range(2)]
    lr = 2.5e-3
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    gp, gm, gv = cv(p0), cv(torch.zeros(n)), cv(torch.zeros(n))
    ggs = [cv(gr) for gr in grads]
    for t, gr in enumerate(grads, 1):
        ops.adam_step(p, gr.to(dev), m, v, lr=lr, step=t, eps=1e-15)
        ops.adam_step(gp, ggs[t - 1], gm, gv, lr=lr, step=t, eps=1e-15)
    r64 = TP._adam_torch(p0, grads, torch.float64, lr)
    e = max(float(((a.cpu().double() - b) / b).abs().max()) for a, b in zip((p, m, v), r64))
    assert e <= TP.gate("adam"), e
    verdict(parity, f"adam_step n={n}", [("p", gp, p), ("m", gm, m), ("v", gv, v)], [(f"g{i}", gg, gr) for i, (gg, gr) in enumerate(zip(ggs, grads))],
            rel_max_vs_fp64=e)


@pytest.mark.parametrize("n", [8, 1032])
def test_split_f32(hip_lib, parity, n):
    """x f32 [n] (n % 8 == 0) -> (hi, lo) planes, through the C ABI with separately carved planes."""
    import ctypes as C
    from vist3a_amd import lib as L, ops
    g = torch.Generator(device=dev).manual_seed(1900 + n)
    x = torch.randn(n, device=dev, generator=g) * 5
    clean = ops.split_f32(x)
    hi = x.to(bf16)
    assert torch.equal(clean[0], hi) and torch.equal(clean[1], (x - hi.float()).to(bf16))     # the pair encoding (test_split_f32_is_the_pair_encoding)
    gx, ghi, glo = cv(x), co((n,), bf16), co((n,), bf16)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(hip_lib.v3a_split_f32(p(gx), p(ghi), p(glo), n, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v3a_split_f32")
    verdict(parity, f"split_f32 n={n}", [("hi", ghi, clean[0]), ("lo", glo, clean[1])], [("x", gx, x)], rel_vs_fp32=0.0)


# ------------------------------------------------------------------------------------------------------------------ convolutions
def _carve_weights(cw):
    """the packed weight of a ConvWeight / ConvWeightSplit re-homed into arenas (bands only: w [CoutP][Kpad], ktab [Kpad / 8], bias, w_halo are
    read IN FULL, padding chunks included - the extent include/vist3a_hip.h states - and nothing around them) -> the (name, view, values) list"""
    ins = []
    for name in ("w", "ktab", "bias", "w_halo"):
        t = getattr(cw, name)
        if t is not None:
            gt = cv(t.clone())
            setattr(cw, name, gt)
            ins.append((name, gt, t))
    return ins


def _out_cl(shape, dtype, pad):
    """channels-last output [..., C] whose pixel rows are ld = C + pad apart"""
    strides, acc = [1], shape[-1] + pad
    for n in reversed(shape[:-1]):
        strides.append(acc)
        acc *= n
    return co(shape, dtype, strides=tuple(reversed(strides)))


CONV_GUARD = [
    # name, k (T,H,W), T, H, W, conv kwargs, torch reference padding (W-, W+, H-, H+, T-, T+), mode, stride
    ("3x3_pad1_ragged_frame", (1, 3, 3), 2, 5, 7, dict(pad=(0, 1, 1)), (1, 1, 1, 1, 0, 0), "constant", (1, 1, 1)),
    ("3x3_smallest_frame", (1, 3, 3), 1, 1, 1, dict(pad=(0, 1, 1)), (1, 1, 1, 1, 0, 0), "constant", (1, 1, 1)),
    ("stride2_trailing_pad", (1, 3, 3), 2, 6, 10, dict(stride=(1, 2, 2), pad=(0, 0, 0), out_size=(2, 3, 5)), (0, 1, 0, 1, 0, 0), "constant", (1, 2, 2)),
    ("ups2_3x3", (1, 3, 3), 2, 3, 5, dict(pad=(0, 1, 1), ups2=True), (1, 1, 1, 1, 0, 0), "constant", (1, 1, 1)),
    ("replicate_3x3x3_stride2", (3, 3, 3), 3, 5, 7, dict(stride=(1, 2, 2), pad=(1, 1, 1), replicate=True), (1, 1, 1, 1, 1, 1), "replicate", (1, 2, 2)),
    ("causal_3x3x3", (3, 3, 3), 3, 5, 7, dict(pad=(2, 1, 1)), (1, 1, 1, 1, 2, 0), "constant", (1, 1, 1)),
]


def _conv_ref(x, w, b, ups2, refpad, mode, stride):
    """x [T,H,W,C] bf16 (dyadic), w [Cout,Cin,kT,kH,kW]: torch conv3d in fp32 on the same operands, channels-last bf16 (test_conv_variants_match_torch_conv3d)"""
    F = torch.nn.functional
    T, H, W, Cin = x.shape
    xin = x.float().permute(3, 0, 1, 2)[None]
    if ups2:
        xin = F.interpolate(xin.transpose(1, 2).reshape(T, Cin, H, W), scale_factor=2.0, mode="nearest-exact").view(1, T, Cin, 2 * H, 2 * W).transpose(1, 2)
    ref = F.conv3d(F.pad(xin, refpad, mode=mode), w.float(), b, stride=stride)
    return ref[0].permute(1, 2, 3, 0).to(bf16)


@pytest.mark.parametrize("case", CONV_GUARD, ids=[c[0] for c in CONV_GUARD])
def test_conv_implicit_gemm(hip_lib, parity, case):
    """v3a_conv_bf16, implicit-GEMM form (tile = -3): x contiguous between NaN bands - an unmasked halo read shows as a NaN or a changed bit in an
    edge pixel -, y with ldy > Cout, packed weights carved at their exact size.  Dyadic operands: exact sums (see the module docstring)."""
    from vist3a_amd import ops
    name, k, T, H, W, kw, refpad, mode, stride = case
    Cin, Cout = 16, 24
    g = torch.Generator(device=dev).manual_seed(2000 + H * W)
    w, b = dy(g, (Cout, Cin, *k), div=8, dtype=bf16), dy(g, (Cout,), span=16)
    x = dy(g, (T, H, W, Cin), dtype=bf16)
    cw = ops.ConvWeight(w, b)
    clean = ops.conv(x, cw, tile=-3, **kw)
    ref = _conv_ref(x, w, b, kw.get("ups2", False), refpad, mode, stride)
    assert tuple(clean.shape[:3]) == tuple(ref.shape[:3])
    r = relerr(clean[..., :Cout], ref)
    assert r < TK.TOL_CONV, (name, r)
    ins = _carve_weights(cw)
    gx, go = cv(x), _out_cl(tuple(clean.shape), bf16, 8)
    ops.conv(gx, cw, out=go, tile=-3, **kw)
    verdict(parity, f"conv_bf16 implicit {name}", [("y", go, clean)], ins + [("x", gx, x)], rel_vs_fp32=r)


@pytest.mark.parametrize("name,kT,T,ups2", [("3x3", 1, 1, False), ("causal3x3x3", 3, 2, False), ("ups2", 1, 1, True)])
def test_conv_halo_tile_form(hip_lib, parity, name, kT, T, ups2):
    """The halo-tile kernel forced (tile = -2) on the smallest frame it is eligible for - one 16 x 32 output tile, Cin 48, Cout 96: every halo edge
    is a frame edge and the frames before / after are NaN bands.  (A frame that is no multiple of the spatial tile is not of its form: the
    entry point refuses it, test_conv_halo_dispatch_rules.)"""
    from vist3a_amd import ops
    Cin, Cout, oH, oW = 48, 96, 16, 32
    H, W = (oH // 2, oW // 2) if ups2 else (oH, oW)
    g = torch.Generator(device=dev).manual_seed(2100 + kT + ups2)
    w, b = dy(g, (Cout, Cin, kT, 3, 3), div=8, dtype=bf16), dy(g, (Cout,), span=16)
    x = dy(g, (T, H, W, Cin), dtype=bf16)
    cw = ops.ConvWeight(w, b)
    assert cw.w_halo is not None
    kw = dict(pad=(kT - 1, 1, 1), ups2=ups2, tile=-2)
    clean = ops.conv(x, cw, **kw)
    r = relerr(clean, _conv_ref(x, w, b, ups2, (1, 1, 1, 1, kT - 1, 0), "constant", (1, 1, 1)))
    assert tuple(clean.shape) == (T, oH, oW, Cout) and r < TK.TOL_CONV, (name, r)
    ins = _carve_weights(cw)
    gx, go = cv(x), _out_cl(tuple(clean.shape), bf16, 8)
    ops.conv(gx, cw, out=go, **kw)
    verdict(parity, f"conv_bf16 halo {name}", [("y", go, clean)], ins + [("x", gx, x)], rel_vs_fp32=r)


@pytest.mark.parametrize("name,H,W,tile,kw,ckw", [
    ("implicit_3x3_ragged_frame", 5, 7, -3, dict(pad=(0, 1, 1)), dict(padding=1)),
    ("implicit_3x3_smallest_frame", 1, 1, -3, dict(pad=(0, 1, 1)), dict(padding=1)),
    ("implicit_down_s2", 6, 10, -3, dict(stride=(1, 2, 2), pad=(0, 1, 1)), dict(stride=2, padding=1)),
    ("halo_3x3_one_tile", 16, 32, -2, dict(pad=(0, 1, 1)), dict(padding=1)),
])
@pytest.mark.parametrize("out_f32", [False, True], ids=["pair_out", "f32_out_ldy"])
def test_conv_split_forms(hip_lib, parity, name, H, W, tile, kw, ckw, out_f32):
    """v3a_conv_split, implicit-GEMM and halo-tile forms: the input pair contiguous between NaN bands, the packed (wh | wl | wh) weight at its
    exact size, the f32 output with ldy > Cout (a pair output is contiguous by the wrapper's contract: bands only).  Reference and gate of
    test_conv_split_vs_float64."""
    import test_pair_gpu as TP
    from vist3a_amd import ops
    F = torch.nn.functional
    T, Cin, Cout = 2, 16, 32
    g = torch.Generator().manual_seed(2200 + H * W)
    x = torch.randn(T, Cin, H, W, generator=g)
    w, b = torch.randn(Cout, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5, torch.randn(Cout, generator=g) * 0.1
    cw = ops.ConvWeightSplit(w, b)
    assert tile != -2 or cw.w_halo is not None
    xp = TP._pair(TP._cl(x, cw.CinP)).to(dev)
    ref = F.conv2d(ops.pair_value(xp.cpu())[..., :Cin].permute(0, 3, 1, 2).double(), w.double(), b.double(), **ckw)
    clean = ops.conv_split(xp, cw, tile=tile, out_f32=out_f32, **kw)
    y = (clean if out_f32 else ops.pair_value(clean)).cpu()[..., :Cout].permute(0, 3, 1, 2)
    e = TP._rel(y, ref)
    assert e < TP.TOL_SPLIT, (name, e)
    ins = _carve_weights(cw)
    gx = cv(xp)
    go = _out_cl(tuple(clean.shape), f32, 8) if out_f32 else co(tuple(clean.shape), bf16)
    ops.conv_split(gx, cw, out=go, tile=tile, out_f32=out_f32, **kw)
    verdict(parity, f"conv_split {name} out_f32={out_f32}", [("y", go, clean)], ins + [("x", gx, xp)], rel_vs_fp64=e)


# ------------------------------------------------------------------------------------------------------------------ 3DGS rasteriser
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("W,H", [(16, 16), (33, 17)])
@pytest.mark.parametrize("U", [1, 63, 65])
def test_gs_project_rasterize_and_backward(hip_lib, parity, U, W, H, Cn):
    """gs_project -> gs_rasterize -> gs_rasterize_backward -> gs_project_backward through the C ABI, every tensor between bands, the workspaces of
    EXACTLY their query's size: rasterize (i) with cap == n_isect, (ii) first with cap = n_isect - 1, which must return V3A_ERR_WORKSPACE, report
    n_isect and leave the bands of the workspace and of the `ids` buffer untouched, the retry (i) then reproducing the clean run bit for bit.
    SH degree 4 / layout [U,3,K] with the harmonics 4 bytes off a 16-byte boundary (the unaligned-source path of stage_sh_rows), and degree 0 /
    layout [U,K,3] aligned.  Clean run: ops.* on tight tensors; its projection is held to the oracle by test_raster_gpu.check_projection; the
    pixel and gradient parity of these kernels is asserted by test_raster_gpu / test_raster_bwd_gpu on oracle-projected inputs and is not
    re-derived here (the guarded run must equal the clean one bit for bit)."""
    import ctypes as C
    import test_raster_gpu as TR
    from vist3a_amd import lib as L, ops
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    means, cov, sh, op = TR._scene(U, 40 + U, spread=0.6, scale=0.25)
    cams = [TR._camera(W, H, 14.0, yaw=0.1 * c, t=(0.05 * c, -0.1, 0.2)) for c in range(Cn)]
    view, K = torch.stack([c[0] for c in cams]).contiguous(), torch.stack([c[1] for c in cams]).contiguous()
    campos = torch.stack([torch.linalg.inv(v)[:3, 3] for v in view]).contiguous()
    bg = torch.tensor([0.2, 0.5, 0.9])
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    gen = torch.Generator().manual_seed(U + W)
    dcol, ddep, dalp = torch.randn(Cn, H, W, 3, generator=gen), torch.randn(Cn, H, W, generator=gen), torch.randn(Cn, H, W, generator=gen)
    D = lambda t: t.to(dev).contiguous()
    total_viol = 0
    for deg, layout, sh_off in ((4, 1, 4), (0, 0, 0)):
        shl = sh if layout == 1 else sh.permute(0, 2, 1).contiguous()
        sh_k = 25
        case = f"gs U={U} {W}x{H} C={Cn} deg={deg} layout={layout}"
        # ---- clean, through ops
        pr = ops.gs_project(D(means), D(cov), D(shl), D(view), D(campos), D(K), W, H, sh_degree=deg, sh_layout=layout)
        for c in range(Cn):
            TR.check_projection({k: v[c] for k, v in pr.items()}, means, cov, sh, view[c], K[c], W, H, sh_degree=deg)
        out = ops.gs_rasterize(pr, D(op), W, H, background=D(bg), return_order=True)
        n = out["n_isect"]
        bwd = ops.gs_rasterize_backward(pr, D(op), W, H, out["tile_offsets"], out["flatten_ids"], D(dcol), D(ddep), D(dalp), background=D(bg))
        pb = ops.gs_project_backward(D(means), D(cov), D(shl), D(view), D(campos), D(K), W, H, pr["radii"], bwd, sh_degree=deg, sh_layout=layout)
        # ---- guarded: projection
        gm, gc, gs, gv, gp, gk = cv(means), cv(cov), cv(shl, off=sh_off), cv(view), cv(campos), cv(K)
        assert gs.data_ptr() % 16 == sh_off
        names = ("radii", "means2d", "depths", "conics", "colors")
        gpr = {k: co(tuple(pr[k].shape), pr[k].dtype) for k in names}
        a = L.GsProjectArgs(P(gm), P(gc), P(gs), layout, sh_k, deg, P(gv), P(gp), P(gk), U, Cn, W, H, 1e-10, 1e10, 0.1, 0.3,
                            *(P(gpr[k]) for k in names))
        L.check(hip_lib.v3a_gs_project(C.byref(a), st), "v3a_gs_project")
        scene_in = [("means", gm, means), ("covars", gc, cov), ("sh", gs, shl), ("viewmat", gv, view), ("campos", gp, campos), ("K", gk, K)]
        verdict(parity, case + " project", [(k, gpr[k], pr[k]) for k in names], scene_in)
        # ---- guarded: rasterize, (ii) one short, then (i) exact
        gop, gbg = cv(op), cv(bg)
        proj_in = [(k, gpr[k], pr[k]) for k in names] + [("opacities", gop, op), ("background", gbg, bg)]

        def raster(cap):
            nbytes = int(hip_lib.v3a_gs_rasterize_workspace_bytes(U, Cn, W, H, cap))
            assert nbytes > 0
            o = dict(color=co((Cn, H, W, 3), f32), depth=co((Cn, H, W), f32), alpha=co((Cn, H, W), f32), ws=co((nbytes,), u8),
                     offs=co((Cn * ntiles + 1,), torch.int32), ids=co((cap,), torch.int32))
            n_host = C.c_long(0)
            ra = L.GsRasterizeArgs(*(P(gpr[k]) for k in names), P(gop), P(gbg), U, Cn, W, H, 1, P(o["color"]), P(o["depth"]), P(o["alpha"]),
                                   P(o["ws"]), nbytes, cap, C.pointer(n_host), P(o["offs"]), P(o["ids"]))
            rc = hip_lib.v3a_gs_rasterize(C.byref(ra), st)
            torch.cuda.synchronize()
            return rc, int(n_host.value), o

        if n >= 2:
            rc, need, o = raster(n - 1)
            assert rc == -4 and need == n, (case, rc, need, n)            # V3A_ERR_WORKSPACE, and the count the caller must grow to
            short = sum(G.violations(o[k])[0] for k in ("ws", "ids", "offs", "color", "depth", "alpha"))
            parity("guard_bands", case=case + " rasterize cap=n_isect-1", violations=short, bit_equal=True, inputs_unchanged=True)
            assert short == 0, (case, "the refused call wrote outside its buffers", {k: G.violations(o[k]) for k in o})
        rc, need, o = raster(max(n, 1))
        assert rc == 0 and need == n, (case, rc, need, n)
        outs = [("color", o["color"], out["color"]), ("depth", o["depth"], out["depth"]), ("alpha", o["alpha"], out["alpha"]),
                ("tile_offsets", o["offs"], out["tile_offsets"])]
        if n:
            outs.append(("flatten_ids", o["ids"], out["flatten_ids"]))
        verdict(parity, case + " rasterize cap=n_isect", outs, proj_in, written=[o["ws"]] + ([] if n else [o["ids"]]))
        # ---- guarded: rasterize backward at n_isect exactly
        nb = int(hip_lib.v3a_gs_rasterize_backward_workspace_bytes(U, Cn, W, H, max(n, 1)))
        assert nb > 0
        gdc, gdd, gda, wsb = cv(dcol), cv(ddep), cv(dalp), co((nb,), u8)
        bn = ("d_means2d", "d_conics", "d_colors", "d_opacity")
        gb = {k: co(tuple(bwd[k].shape), f32) for k in bn}
        ba = L.GsRasterizeBackwardArgs(P(gpr["radii"]), P(gpr["means2d"]), P(gpr["conics"]), P(gpr["colors"]), P(gop), P(gbg), U, Cn, W, H, 1,
                                       P(o["offs"]), P(o["ids"]) if n else None, n, P(gdc), P(gdd), P(gda), *(P(gb[k]) for k in bn), P(wsb), nb)
        L.check(hip_lib.v3a_gs_rasterize_backward(C.byref(ba), st), "v3a_gs_rasterize_backward")
        verdict(parity, case + " rasterize_backward", [(k, gb[k], bwd[k]) for k in bn],
                proj_in + [("d_color", gdc, dcol), ("d_depth", gdd, ddep), ("d_alpha", gda, dalp), ("tile_offsets", o["offs"], out["tile_offsets"])],
                written=[wsb])
        # ---- guarded: projection backward
        go = [co(tuple(t.shape), f32) for t in pb]
        pa = L.GsProjectBackwardArgs(P(gm), P(gc), P(gs), layout, sh_k, deg, P(gv), P(gp), P(gk), U, Cn, W, H, 0.3, P(gpr["radii"]),
                                     *(P(gb[k]) for k in bn), *(P(t) for t in go))
        L.check(hip_lib.v3a_gs_project_backward(C.byref(pa), st), "v3a_gs_project_backward")
        verdict(parity, case + " project_backward", [(nm, g_, c_) for nm, g_, c_ in zip(("d_means", "d_covars", "d_sh", "d_opacities"), go, pb)],
                scene_in + [(k, gb[k], bwd[k]) for k in bn] + [("radii", gpr["radii"], pr["radii"])])


# ------------------------------------------------------------------------------------------------------------------ wrappers that allocate their own outputs
class _CarvingTorch:
    """Stands in for the `torch` global of vist3a_amd.ops during a guarded run: every tensor a wrapper allocates for itself (outputs, counters,
    autograd gradients, and its workspace - which the wrappers size by the library's workspace query) comes out of an all-0xFF arena with
    bands before and after, at exactly the size the wrapper asked for.  Everything else is torch's.  No wrapper gains a parameter."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, device=None, dtype=None):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        t = co(shape if shape else (1,), dtype or f32)
        self.made.append(t)
        if not shape:
            g_, t = t.guard, t.view(())
            t.guard = g_
        return t

    def zeros(self, *size, device=None, dtype=None):
        t = self.empty(*size, device=device, dtype=dtype)
        t.zero_()
        return t

    def empty_like(self, x):
        return self.empty(tuple(x.shape), dtype=x.dtype)


def _flat(o):
    if isinstance(o, torch.Tensor):
        return [o]
    if isinstance(o, dict):
        return [t for k in sorted(o) for t in _flat(o[k])]
    if isinstance(o, (tuple, list)):
        return [t for v in o for t in _flat(v)]
    return []


def wrapped(parity, case, fn, inputs, pads=None, inplace=(), **errs):
    """The protocol for an ops wrapper that allocates its outputs itself.  fn(**tensors) -> tensors (any nesting); inputs: name -> values;
    pads: name -> row pad of a 2-D input whose wrapper takes a row stride; inplace: names of inputs the call updates (compared with the clean
    run's, exempt from `unchanged`, not from their bands).  Returns the clean result."""
    from vist3a_amd import ops
    pads = pads or {}
    leaf = lambda v: v.clone().to(dev).requires_grad_(v.requires_grad)
    cin = {k: (leaf(v) if v is not None else None) for k, v in inputs.items()}
    clean = _flat(fn(**cin))
    ct = _CarvingTorch()
    gin = {k: (cv(v.detach(), pads.get(k, 0)).requires_grad_(v.requires_grad) if v is not None else None) for k, v in inputs.items()}
    ops.torch = ct
    try:
        guarded = _flat(fn(**gin))
    finally:
        ops.torch = torch
    torch.cuda.synchronize()
    assert len(guarded) == len(clean) and (ct.made or inplace), case
    biteq = all(tuple(a.shape) == tuple(b.shape) and torch.equal(G.bits(a.detach()), G.bits(b.detach())) for a, b in zip(guarded, clean))
    biteq &= all(torch.equal(G.bits(gin[k].detach()), G.bits(cin[k].detach())) for k in inplace)
    fin = all(bool(a.detach().double()[b.detach().double().isfinite()].isfinite().all()) for a, b in zip(guarded, clean) if b.dtype.is_floating_point)
    viol, where = 0, {}
    for i, t in enumerate(ct.made + [gin[k] for k in inplace]):
        n, w = G.violations(t)
        viol += n
        if n:
            where[i] = (tuple(t.shape), w)
    in_ok = {k: G.unchanged(gin[k], inputs[k].detach()) for k in inputs if inputs[k] is not None and k not in inplace}
    parity("guard_bands", case=case, violations=viol, bit_equal=biteq, inputs_unchanged=all(in_ok.values()), **errs)
    assert viol == 0, (case, "bytes outside a wrapper-allocated tensor changed", where)
    assert all(in_ok.values()), (case, "inputs changed", [k for k, v in in_ok.items() if not v])
    assert biteq, (case, "guarded run differs from the clean run")
    assert fin, (case, "non-finite output where the clean output is finite")
    return clean


# The clean runs of the cases below are NOT re-held to a reference here (a named deviation from the protocol, listed in DESIGN.md section 4):
# their parity tests need oracles, golden files or Pillow and live in test_recon_gpu / test_post_opt_gpu / test_depth_loss_gpu /
# test_bilagrid_gpu / test_nvs_gpu / test_lpips_gpu / test_clip_gpu / test_pair_gpu / test_small_kernels_gpu / test_boundary_gpu.  What is asserted is
# the memory contract: guarded == clean bit for bit, bands untouched, inputs unchanged, finite where the clean run is.
def _rn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("M", [1, 63, 65, 1000])
def test_voxelize_fuse_and_conf_quantile_compact(hip_lib, parity, M):
    """ldf > nfeat; the workspaces are the wrappers' own, of exactly v3a_voxelize_workspace_bytes / v3a_conf_compact_workspace_bytes."""
    from vist3a_amd import ops
    nfeat = 11
    pts, feat = _rn(M, M, 3, scale=0.004), _rn(M + 1, M, nfeat + 1)
    wrapped(parity, f"voxelize_fuse M={M}", lambda pts, feat: ops.voxelize_fuse(pts, feat, nfeat, nfeat, 0.002), dict(pts=pts, feat=feat), pads=dict(feat=3))
    conf = torch.rand(M, generator=torch.Generator().manual_seed(M))
    wrapped(parity, f"conf_quantile_compact M={M}", lambda conf, pts, feat: ops.conf_quantile_compact(conf, 0.3, pts, feat, nfeat),
            dict(conf=conf, pts=pts, feat=feat), pads=dict(feat=3))


def _with_grads(loss_fn, names):
    """fn for `wrapped`: the forward value(s) and the gradients of their sum with respect to `names`"""
    def fn(**kw):
        out = loss_fn(**kw)
        tot = sum(o.double().sum() for o in _flat(out) if o.requires_grad)
        return out, torch.autograd.grad(tot, [kw[n] for n in names])
    return fn


@pytest.mark.parametrize("Cn,H,W", [(1, 1, 1), (1, 3, 5), (3, 17, 33)])
def test_depth_loss_forward_backward(hip_lib, parity, Cn, H, W):
    """numel % 4 != 0 and the smallest map; the workspace is the wrapper's, sized by v3a_depth_loss_workspace_bytes."""
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(H * W)
    depth, alpha = (torch.rand(Cn, H, W, generator=g) * 3 + 0.5).requires_grad_(), (torch.rand(Cn, H, W, generator=g) * 0.9 + 0.05).requires_grad_()
    gt, mask = torch.rand(Cn, H, W, generator=g) * 3 + 0.5, (torch.rand(Cn, H, W, generator=g) > 0.2).to(torch.uint8)
    mask.view(-1)[0] = 1
    wrapped(parity, f"depth_loss {Cn}x{H}x{W}", _with_grads(lambda depth, alpha, gt, mask: ops.depth_loss(depth, alpha, gt, mask, 0.7)[0], ("depth", "alpha")),
            dict(depth=depth, alpha=alpha, gt=gt, mask=mask))


@pytest.mark.parametrize("N,H,W,Lz,GY,GX", [(1, 1, 1, 2, 2, 2), (2, 5, 7, 3, 4, 5)])
def test_bilagrid_slice_and_tv_forward_backward(hip_lib, parity, N, H, W, Lz, GY, GX):
    from vist3a_amd import ops
    rgb = torch.rand(N, H, W, 3, generator=torch.Generator().manual_seed(H)).requires_grad_()
    grids = (ops.bilagrid_identity(N, GX, GY, Lz, "cpu") + _rn(GX, N, Lz, GY, GX, 12, scale=0.1)).requires_grad_()
    wrapped(parity, f"bilagrid_slice {N}x{H}x{W} grid {Lz}x{GY}x{GX}", _with_grads(lambda rgb, grids: ops.bilagrid_slice(rgb, grids), ("rgb", "grids")),
            dict(rgb=rgb, grids=grids))
    wrapped(parity, f"bilagrid_tv grid {N}x{Lz}x{GY}x{GX}", _with_grads(lambda grids: ops.bilagrid_tv(grids), ("grids",)), dict(grids=grids))


@pytest.mark.parametrize("N,H,W,Cc", [(1, 11, 11, 3), (2, 13, 12, 3), (1, 11, 14, 3)])
def test_photometric_loss_and_image_metrics(hip_lib, parity, N, H, W, Cc):
    """the smallest legal image (11 x 11) and sizes whose numel % 4 != 0; workspaces at their queries' sizes (the wrappers')."""
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(H * W + Cc)
    pred, target = torch.rand(N, H, W, Cc, generator=g).requires_grad_(), torch.rand(N, H, W, Cc, generator=g)
    wrapped(parity, f"photometric_loss {N}x{H}x{W}x{Cc}", _with_grads(lambda pred, target: ops.photometric_loss(pred, target, 0.2), ("pred",)),
            dict(pred=pred, target=target))
    a, b = torch.randint(0, 256, (N, H, W, Cc), generator=g, dtype=torch.uint8), torch.randint(0, 256, (N, H, W, Cc), generator=g, dtype=torch.uint8)
    wrapped(parity, f"image_metrics {N}x{H}x{W}x{Cc}", lambda a, b: ops.image_metrics(a, b), dict(a=a, b=b))


@pytest.mark.parametrize("N,H,W", [(1, 2, 2), (2, 5, 7)])
def test_lpips_input_pool_head(hip_lib, parity, N, H, W):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(H + W)
    pred, gt = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    x = wrapped(parity, f"lpips_input u8 {N}x{H}x{W}", lambda pred, gt: ops.lpips_input(pred, gt), dict(pred=pred, gt=gt))[0].cpu()
    pf, gf = torch.rand(N, 3, H, W, generator=g), torch.rand(N, 3, H, W, generator=g)
    wrapped(parity, f"lpips_input f32 {N}x{H}x{W}", lambda pred, gt: ops.lpips_input(pred, gt), dict(pred=pf, gt=gf))
    wrapped(parity, f"lpips_pool {N}x{H}x{W}", lambda x: ops.lpips_pool(x), dict(x=x))
    w = torch.rand(x.shape[-1], generator=g)
    for acc in (False, True):
        wrapped(parity, f"lpips_head {N}x{H}x{W} accumulate={acc}", lambda x, w, out: ops.lpips_head(x, w, out, accumulate=acc),
                dict(x=x, w=w, out=torch.full((N,), 0.25, dtype=torch.float64)), inplace=("out",))


def test_clip_preprocess_rows_score(hip_lib, parity):
    import test_clip_gpu as TC
    from vist3a_amd import ops
    from vist3a_amd.evaluation import clip as CL
    H, W, S, P, n = 37, 53, 28, 14, 2
    sc = CL.ClipScorer(TC._Pre(S, P))
    tabs = sc.tables(H, W)
    keys = ("x_bounds", "y_bounds", "x_coeffs", "y_coeffs")
    frames = torch.from_numpy(TC.frames_of(H, W, n))

    def pre(frames, lut, **t):
        return ops.clip_preprocess(frames, dict(tabs, **t), lut, S, P, want_u8=True, want_f32=True)
    wrapped(parity, f"clip_preprocess {n}x{H}x{W} -> {S}", pre, dict(frames=frames, lut=sc.w.lut.cpu(), **{k: tabs[k].cpu() for k in keys}))
    d, seq, B = 12, 5, 3
    src, cls, pos = _rn(1, B * (seq - 1), d), _rn(2, d), _rn(3, seq, d)
    wrapped(parity, "clip_rows cls+pos", lambda src, cls, pos: ops.clip_rows(src, cls=cls, pos=pos, S=seq), dict(src=src, cls=cls, pos=pos))
    ids = torch.tensor([3, 0, 11, 7, 7], dtype=torch.int32)
    wrapped(parity, "clip_rows ids", lambda src, ids: ops.clip_rows(src, ids=ids), dict(src=src, ids=ids))
    wrapped(parity, "clip_score", lambda e, t: ops.clip_score(e, t), dict(e=_rn(4, 7, 20), t=_rn(5, 20)))


@pytest.mark.parametrize("U", [1, 63, 65])
def test_splat_activate_and_gaussian_adapter(hip_lib, parity, U):
    from vist3a_amd import ops
    ls, q, lg = _rn(U, U, 3, scale=0.5).requires_grad_(), _rn(U + 1, U, 4).requires_grad_(), _rn(U + 2, U).requires_grad_()
    wrapped(parity, f"splat_activate U={U}", _with_grads(lambda ls, q, lg: ops.splat_activate(ls, q, lg), ("ls", "q", "lg")), dict(ls=ls, q=q, lg=lg))
    for deg in (0, 4):
        dsh = (deg + 1) ** 2
        mask = torch.ones(dsh)
        mask[1:] = 0.1
        wrapped(parity, f"gaussian_adapter U={U} deg={deg}", lambda pts, feats, mask: ops.gaussian_adapter(pts, feats, mask, deg, 1.0),
                dict(pts=_rn(U, U, 3), feats=_rn(U + 3, U, 8 + 3 * dsh), mask=mask), pads=dict(feats=5))


@pytest.mark.parametrize("S,H,W", [(1, 1, 1), (2, 3, 5)])
def test_depth_unproject_bilinear_upsample(hip_lib, parity, S, H, W):
    from vist3a_amd import ops
    wrapped(parity, f"depth_unproject {S}x{H}x{W}", lambda raw, cam: ops.depth_unproject(raw, cam, S, H, W),
            dict(raw=_rn(H, S * H * W, 2, scale=0.7), cam=_rn(W, S, 16)), pads=dict(raw=3))
    x = _rn(7, S, H, W, 8).to(bf16)
    for ac in (False, True):
        size = (2 * H + 1, 3 * W)
        add, table = _rn(8, S, *size, 8).to(bf16), _rn(9, size[0] * size[1], 8)
        wrapped(parity, f"bilinear_cl {S}x{H}x{W} align_corners={ac}", lambda x, add, table: ops.bilinear_cl(x, size, align_corners=ac, add=add, table=table),
                dict(x=x, add=add, table=table))
        xp, ap = torch.stack([x, (x.float() * 0.01).to(bf16)]), torch.stack([add, (add.float() * 0.01).to(bf16)])
        wrapped(parity, f"bilinear_cl_pair {S}x{H}x{W} align_corners={ac}",
                lambda x, add, table: ops.bilinear_cl_pair(x, size, align_corners=ac, add=add, table=table), dict(x=xp, add=ap, table=table))
    wrapped(parity, f"latent_upsample_t_cl Tl={S} {H}x{W}", lambda z: ops.latent_upsample_t_cl(z), dict(z=_rn(10, 8, S, H, W)))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [1, 77, 257])
def test_attention_f32(hip_lib, parity, S, causal):
    """q, k, v are column slices of one fused qkv buffer with ld = 3 H 64 + 4 (poison between the rows); lens cuts the keys of one item."""
    from vist3a_amd import ops
    B, H = 2, 2
    d = H * 64
    qkv = _rn(S, B * S, 3 * d)
    lens = torch.tensor([S, max(1, S - 3)], dtype=torch.int32)
    for out_f32 in (True, False):
        wrapped(parity, f"attention_f32 S={S} causal={causal} out_f32={out_f32}",
                lambda qkv, lens: ops.attention_f32(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B=B, S=S, H=H, causal=causal, lens=lens, out_f32=out_f32),
                dict(qkv=qkv, lens=lens), pads=dict(qkv=4))


@pytest.mark.parametrize("d", [8, 520])
@pytest.mark.parametrize("M", ROWS)
def test_layernorm_pair(hip_lib, parity, M, d):
    from vist3a_amd import ops
    wrapped(parity, f"layernorm_pair {M}x{d}", lambda x, w, b: ops.layernorm_pair(x, weight=w, bias=b, eps=1e-5),
            dict(x=_rn(M + d, M, d, scale=3.0) + 0.5, w=_rn(1, d), b=_rn(2, d)), pads=dict(x=8))


@pytest.mark.parametrize("S,hp,wp,H", [(1, 1, 1, 1), (3, 2, 3, 2)])
def test_qknorm_rope2d_in_place(hip_lib, parity, S, hp, wp, H):
    """In place on qk [M, 2C] with ld = 2C + 8: the columns it updates are compared with the clean run's, its row padding, the filler rows'
    neighbours and the bands must stay 0xFF."""
    from vist3a_amd import ops
    from vist3a_amd.recon.engine import rope2d_table
    C, nsp = H * 64, 5
    P = hp * wp + nsp
    Pp = (P + 7) // 8 * 8
    tab = rope2d_table(max(hp, wp) + 2).cpu()

    def fn(qk, qw, qb, kw, kb, tab):
        ops.qknorm_rope2d(qk, C, qw, qb, kw, kb, tab, Pp, nsp, P, wp, 1e-5)
        return qk
    wrapped(parity, f"qknorm_rope2d S={S} {hp}x{wp} H={H}", fn,
            dict(qk=_rn(S + H, S * Pp, 2 * C).to(bf16), qw=1 + 0.2 * _rn(1, 64), qb=0.1 * _rn(2, 64), kw=1 + 0.2 * _rn(3, 64), kb=0.1 * _rn(4, 64), tab=tab),
            pads=dict(qk=8), inplace=("qk",))


def test_unipc_cfg_step(hip_lib, parity):
    """Four steps of the fused denoise step (every corrector / predictor order) on tight and on carved buffers: every buffer it updates is compared
    bit for bit, every band must stay 0xFF, dit_out is unchanged."""
    from vist3a_amd import ops
    from vist3a_amd.wan.scheduler import UniPCMultistepScheduler
    Cc, T, H, W = 16, 1, 2, 6
    N = T * (H // 2) * (W // 2)
    worlds = []
    for carved in (False, True):
        sch = UniPCMultistepScheduler(flow_shift=5.0)
        sch.set_timesteps(4)
        mk = (lambda *s, dtype=f32: co(s, dtype)) if carved else (lambda *s, dtype=f32: torch.full(s, float("nan"), device=dev, dtype=dtype))
        cur = mk(1, Cc, T, H, W)
        cur.copy_(_rn(1, 1, Cc, T, H, W))
        last, m_a, m_b, tok = mk(1, Cc, T, H, W), mk(1, Cc, T, H, W), mk(1, Cc, T, H, W), mk(2 * N, 4 * Cc, dtype=bf16)
        m1 = m2 = None
        outs = []
        for i in range(4):
            vals = _rn(20 + i, 2 * N, 4 * Cc).to(bf16)
            out_tok = cv(vals) if carved else vals.to(dev)
            c = sch.plan_step()
            m_out = m_b if m1 is m_a else m_a
            ops.unipc_cfg_step(out_tok, tok, cur, last if c["corr_order"] else None, m1, m2, m_out, last, cur, batch=2, guidance=7.5, coeffs=c)
            m2, m1 = m1, m_out
            outs.append((out_tok, vals))
        worlds.append(dict(cur=cur, last=last, m_a=m_a, m_b=m_b, tok=tok, outs=outs))
    clean, g_ = worlds
    verdict(parity, "unipc_cfg_step 4 steps", [(k, g_[k], clean[k]) for k in ("cur", "last", "m_a", "m_b", "tok")],
            [(f"dit_out{i}", t, v) for i, (t, v) in enumerate(g_["outs"])])
