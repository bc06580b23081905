"""GPU tests of csrc/color_correct.hip: ops.color_correct and ops.image_mse.

Reference: tests/golden/color_correct_ref.safetensors, the reference's own color_correct run in fp64 (and its own fp32 run as the
comparison figure).  Gates, for the output in ||a - a64|| / ||a64|| and for the per-image MSE in relative terms: 2x the largest
error measured on an MI355X (MEASURED, the run recorded in DESIGN.md section 7f), and never above the output error of the
reference's fp32 run on the same case (1.3e-7 .. 1.5e-7).  The MSE error of a rounded image is a sum of signed terms: the fp32
reference's own MSE figure scatters between 2e-9 and 1.1e-7 over the four cases and is printed for comparison only.
Every test prints its figures before it asserts."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch
from safetensors.torch import load_file

sys.path.insert(0, str(Path(__file__).resolve().parent))
import color_correct_oracle as CO  # noqa: E402
import guard as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "color_correct_ref.safetensors"
# largest over the four cases, MI355X: relative L2 error of the output, relative error of the per-image MSE
MEASURED = dict(out=2.401e-8, mse=1.253e-8)


@pytest.fixture(scope="module")
def gold():
    return load_file(str(GOLD))


def _rel(a, b):
    return float((a.detach().cpu().double() - b.double()).norm() / b.double().norm())


def _gate(name, ref32_error):
    return min(2 * MEASURED[name], ref32_error)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", list(CO.GOLDEN_CASES))
def test_matches_reference(hip_lib, parity, gold, case):
    from vist3a_amd import ops
    _, iters = CO.GOLDEN_CASES[case]
    img, ref, o64, o32, m64 = (gold[f"{case}.{k}"] for k in ("img", "ref", "out64", "out32", "mse64"))
    out, mse, status = ops.color_correct(img.cuda(), ref.cuda(), num_iters=iters)
    e, e32 = _rel(out, o64), _rel(o32, o64)
    em = float(((mse.cpu() - m64).abs() / m64).max())
    em32 = float(((CO.mse(o32, ref) - m64).abs() / m64).max())
    print(f"[color_correct {case}] output rel L2: hip vs fp64 {e:.3e} (reference fp32 vs fp64 {e32:.3e}, gate {_gate('out', e32):.3e});  "
          f"mse rel: hip {em:.3e} (reference fp32 {em32:.3e}, gate {_gate('mse', e32):.3e})")
    parity(f"color_correct::parity[{case}]", out_rel_l2=e, ref_fp32_out_rel_l2=e32, mse_rel=em, ref_fp32_mse_rel=em32)
    assert out.dtype == torch.float32 and out.shape == img.shape and mse.dtype == torch.float64 and mse.shape == (img.shape[0],)
    assert status.dtype == torch.int32 and status.shape == (img.shape[0], 3) and int(status.abs().max()) == 0
    assert float(out.min()) >= 0 and float(out.max()) <= 1
    assert e <= _gate("out", e32), (e, e32)
    assert em <= _gate("mse", e32), (em, e32)
    # the returned MSE is that of the stored image: against a fp64 sum over the returned tensor, rounding of the sum only
    assert float(((mse.cpu() - CO.mse(out.cpu(), ref)).abs() / m64).max()) <= 1e-13


def test_image_mse_matches_fp64(hip_lib, parity, gold):
    from vist3a_amd import ops
    for case in CO.GOLDEN_CASES:
        a, b = gold[case + ".img"], gold[case + ".ref"]
        m = ops.image_mse(a.cuda(), b.cuda())
        e = float(((m.cpu() - CO.mse(a, b)).abs() / CO.mse(a, b)).max())
        print(f"[image_mse {case}] relative to torch fp64: {e:.3e}")
        parity(f"color_correct::image_mse[{case}]", rel=e)
        assert m.dtype == torch.float64 and e <= 1e-13      # differences are exact in fp64; a few thousand additions in another order
    z = torch.rand(2, 3, 5, 1, device="cuda")
    assert ops.image_mse(z, z.clone()).tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ independence, determinism
def test_images_are_independent_and_runs_identical(hip_lib, gold):
    from vist3a_amd import ops
    img, ref = gold["2x13x37.it5.img"].cuda(), gold["2x13x37.it5.ref"].cuda()
    both, again = ops.color_correct(img, ref), ops.color_correct(img, ref)
    assert all(torch.equal(p, q) for p, q in zip(both, again))
    for n in range(2):
        one = ops.color_correct(img[n:n + 1], ref[n:n + 1])
        assert all(torch.equal(p[n:n + 1], q) for p, q in zip(both, one)), n
    big_i, big_r = gold["1x45x70.it5.img"].cuda(), gold["1x45x70.it5.ref"].cuda()     # 13 workgroups per channel
    assert all(torch.equal(p, q) for p, q in zip(ops.color_correct(big_i, big_r), ops.color_correct(big_i, big_r)))
    assert torch.equal(ops.image_mse(img, ref), ops.image_mse(img, ref))
    assert torch.equal(ops.image_mse(img, ref)[1:], ops.image_mse(img[1:], ref[1:]))


# ------------------------------------------------------------------------------------------------ rank-deficient channels
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 4)])
def test_fewer_than_ten_rows_keep_the_clipped_input(hip_lib, shape):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    img = torch.rand(*shape, 3, generator=g) * 1.4 - 0.2        # some values outside [0, 1]: the clip is seen
    ref = torch.rand(*shape, 3, generator=g)
    out, mse, status = ops.color_correct(img.cuda(), ref.cuda())
    assert torch.equal(out.cpu(), img.clamp(0, 1))
    assert bool((status & 1).bool().all())
    assert torch.equal(mse.cpu(), CO.mse(img.clamp(0, 1), ref))
    o_ref, s_ref = CO.color_correct_normal(img, ref)
    assert torch.equal(out.cpu().double(), o_ref) and torch.equal(status.cpu() & 1, s_ref & 1)


def test_singular_system_is_flagged(hip_lib):
    """a constant image: 48 usable rows, but every feature column is a multiple of the constant one - the second pivot is 0"""
    from vist3a_amd import ops
    img = torch.full((1, 4, 12, 3), 0.25)
    ref = torch.rand(1, 4, 12, 3, generator=torch.Generator().manual_seed(0)) * 0.8 + 0.1
    out, _, status = ops.color_correct(img.cuda(), ref.cuda())
    assert status.cpu().tolist() == [[2, 2, 2]] and torch.equal(out.cpu(), img)


def test_argument_errors(hip_lib):
    from vist3a_amd import ops
    a = torch.rand(1, 4, 5, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.color_correct(a.clone().requires_grad_(True), a)
    with pytest.raises(NotImplementedError):
        ops.image_mse(a, a.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        ops.color_correct(a, a[:, :, :4])
    with pytest.raises(ValueError):
        ops.color_correct(a.cpu(), a.cpu())
    with pytest.raises(ValueError):
        ops.color_correct(a.permute(0, 2, 1, 3), a.permute(0, 2, 1, 3))      # pixels of a row not contiguous
    for iters in (0, 17):
        with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
            ops.color_correct(a, a, num_iters=iters)
    with pytest.raises(RuntimeError, match="V3A_ERR_ARG"):
        ops.color_correct(a, a, eps=0.5)


# ------------------------------------------------------------------------------------------------ strided views, guard bands
def _cc_raw(img, ref, out, sse, status, ws, ws_bytes, N, H, W, iters):
    from vist3a_amd import lib as L
    stride = lambda t: (t.stride(1) if H > 1 else 3 * W, t.stride(0) if N > 1 else 0)
    (li, si), (lr, sr), (lo, so) = stride(img), stride(ref), stride(out)
    args = L.ColorCorrectArgs(img.data_ptr(), ref.data_ptr(), out.data_ptr(), N, H, W, iters, li, lr, lo, si, sr, so, CO.EPS,
                              sse.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes)
    rc = L.load().v3a_color_correct(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case,pad", [("2x13x37.it5", 5), ("1x45x70.it5", 2)])
def test_color_correct_guard_bands(hip_lib, gold, case, pad):
    """every operand carved out of an all-0xFF arena, rows and images strided (the padding is NaN): results bit-equal to the tight
    run, guard bytes and inputs untouched, the workspace held to its stated size"""
    from vist3a_amd import lib as L, ops
    (N, H, W), iters = CO.GOLDEN_CASES[case]
    img, ref = gold[case + ".img"].cuda(), gold[case + ".ref"].cuda()
    clean = ops.color_correct(img, ref, num_iters=iters)
    need = L.load().v3a_color_correct_workspace_bytes(N, H, W, iters)
    assert need > 0 and need % 8 == 0
    strides = lambda ld, extra: ((H * ld + extra), ld, 3, 1)
    gi = G.carve_like(img, strides=strides(3 * W + pad, 7))
    gr = G.carve_like(ref, strides=strides(3 * W + 1, 0))
    go = G.carve((N, H, W, 3), torch.float32, strides=strides(3 * W + 2 * pad, 3), device="cuda")
    sse, status = G.carve((N,), torch.float64, device="cuda"), G.carve((N, 3), torch.int32, device="cuda")
    ws = G.carve((need,), torch.uint8, device="cuda")
    assert _cc_raw(gi, gr, go, sse, status, ws, need, N, H, W, iters) == 0
    assert torch.equal(G.bits(go), G.bits(clean[0]))
    assert torch.equal(sse / float(H * W * 3), clean[1]) and torch.equal(status, clean[2])
    for name, t in (("out", go), ("sse", sse), ("status", status), ("workspace", ws)):
        assert G.violations(t)[0] == 0, (name, G.violations(t))
    assert G.unchanged(gi, img) and G.unchanged(gr, ref)
    # a workspace one byte short (V3A_ERR_WORKSPACE), a row stride under the row (V3A_ERR_SHAPE): refused before any launch
    assert _cc_raw(gi, gr, go, sse, status, ws, need - 1, N, H, W, iters) == -4
    bad = img.as_strided((N, H, W, 3), (H * 3 * W, 3 * W - 1, 3, 1))
    assert _cc_raw(bad, gr, go, sse, status, ws, need, N, H, W, iters) == -2


@pytest.mark.parametrize("N,H,W,Cc,pad", [(2, 13, 37, 3, 5), (1, 45, 70, 3, 1), (3, 2, 5, 1, 3)])
def test_image_mse_guard_bands(hip_lib, N, H, W, Cc, pad):
    from vist3a_amd import lib as L, ops
    g = torch.Generator().manual_seed(N * H + W)
    a, b = torch.rand(N, H, W, Cc, generator=g).cuda(), torch.rand(N, H, W, Cc, generator=g).cuda()
    clean = ops.image_mse(a, b)
    ga = G.carve_like(a, strides=(H * (W * Cc + pad) + 3, W * Cc + pad, Cc, 1))
    gb = G.carve_like(b, strides=(H * (W * Cc + 2 * pad), W * Cc + 2 * pad, Cc, 1))
    # through the wrapper: strided views are read in place
    assert torch.equal(ops.image_mse(ga, gb), clean)
    assert G.unchanged(ga, a) and G.unchanged(gb, b)
    need = L.load().v3a_image_mse_workspace_bytes(N, H, W, Cc)
    mse, ws = G.carve((N,), torch.float64, device="cuda"), G.carve((need,), torch.uint8, device="cuda")
    args = L.ImageMseArgs(ga.data_ptr(), gb.data_ptr(), N, H, W, Cc, ga.stride(1), gb.stride(1), ga.stride(0), gb.stride(0),
                          mse.data_ptr(), ws.data_ptr(), need)
    assert L.load().v3a_image_mse(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(G.bits(mse), G.bits(clean))
    assert G.violations(mse)[0] == 0 and G.violations(ws)[0] == 0 and G.unchanged(ga, a) and G.unchanged(gb, b)


def test_strided_views_through_the_wrapper(hip_lib, gold):
    """a crop of a larger image is corrected in place: equal to the contiguous copy, bit for bit"""
    from vist3a_amd import ops
    img, ref = gold["1x45x70.it5.img"].cuda(), gold["1x45x70.it5.ref"].cuda()
    ci, cr = img[:, 3:40, 5:61], ref[:, 3:40, 5:61]
    assert not ci.is_contiguous()
    assert all(torch.equal(p, q) for p, q in zip(ops.color_correct(ci, cr), ops.color_correct(ci.contiguous(), cr.contiguous())))
    assert torch.equal(ops.image_mse(ci, cr), ops.image_mse(ci.contiguous(), cr.contiguous()))
