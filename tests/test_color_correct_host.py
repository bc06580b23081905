"""CPU: tests/color_correct_oracle.py against the tensors recorded from the reference's own color_correct
(tests/golden/color_correct_ref.safetensors), and the normal-equations form the kernel uses against the lstsq form."""
import sys
from pathlib import Path

import pytest
import torch
from safetensors.torch import load_file

sys.path.insert(0, str(Path(__file__).resolve().parent))
import color_correct_oracle as CO  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden" / "color_correct_ref.safetensors"


@pytest.fixture(scope="module")
def gold():
    return load_file(str(GOLD))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("case", list(CO.GOLDEN_CASES))
def test_oracle_matches_reference(gold, case):
    (N, H, W), iters = CO.GOLDEN_CASES[case]
    img, ref = gold[case + ".img"], gold[case + ".ref"]
    assert img.shape == (N, H, W, 3) and img.dtype == torch.float32
    i2, r2 = CO.make_inputs(N, H, W, int(gold[case + ".seed"]))
    assert torch.equal(i2, img) and torch.equal(r2, ref)
    masks = []
    out = CO.color_correct(img, ref, iters, masks=masks)
    e = _rel(out, gold[case + ".out64"])
    em = float(((CO.mse(out, ref) - gold[case + ".mse64"]).abs() / gold[case + ".mse64"]).max())
    print(f"[color_correct oracle {case}] vs the reference in fp64: output {e:.3e}, mse {em:.3e}")
    assert e <= 1e-12 and em <= 1e-12
    rows = torch.tensor([int(m.sum()) for m in masks], dtype=torch.int32).reshape(N, iters, 3)
    assert torch.equal(rows, gold[case + ".rows"])
    # the masks matter: some rows are dropped in every fit, and (5 rounds) the set changes between rounds somewhere
    assert int(rows.max()) < H * W and int(rows.min()) >= 10
    # the reference's own float32 run is no closer than float32 allows, no further than a few ulps
    e32 = _rel(gold[case + ".out32"], gold[case + ".out64"])
    assert 1e-9 < e32 < 1e-6


@pytest.mark.parametrize("case", list(CO.GOLDEN_CASES))
def test_normal_equations_match_lstsq(gold, case):
    """what csrc/color_correct.hip solves (fp64 elimination on the Gram matrix) against the reference's lstsq, on the golden cases"""
    _, iters = CO.GOLDEN_CASES[case]
    out, status = CO.color_correct_normal(gold[case + ".img"], gold[case + ".ref"], iters)
    e = _rel(out, gold[case + ".out64"])
    print(f"[color_correct normal equations {case}] vs the reference in fp64: {e:.3e}")
    assert e <= 1e-10 and int(status.abs().max()) == 0


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 4)])
def test_rank_deficient_channels_keep_the_identity(shape):
    """fewer than 10 rows: the clipped input comes back exactly, flag 1 set"""
    g = torch.Generator().manual_seed(sum(shape))
    img = torch.rand(*shape, 3, generator=g) * 1.4 - 0.2
    ref = torch.rand(*shape, 3, generator=g)
    out, status = CO.color_correct_normal(img, ref, 5)
    assert torch.equal(out, img.double().clamp(0, 1)) and bool((status & 1).all())


def test_cast_is_removed():
    """a per-channel gain and bias that clips no pixel has its inverse inside the model: cc_psnr recovers what psnr loses, down to
    the float32 rounding of the cast image (6e-8 of a value: above 120 dB)"""
    _, ref = CO.make_inputs(1, 13, 37, 3)
    ref = ref.clamp(0.05, 0.95)
    img = (ref * torch.tensor([0.8, 0.9, 1.0]) + torch.tensor([0.03, -0.02, 0.01])).clamp(0, 1)
    out = CO.color_correct(img, ref, 5)
    p, cc = float(CO.psnr(CO.mse(img, ref))), float(CO.psnr(CO.mse(out, ref)))
    print(f"[color_correct cast] psnr {p:.2f} dB -> cc_psnr {cc:.2f} dB")
    assert p < 30 and cc > 100


def test_entry_points_reject_bad_arguments_before_any_launch():
    """safe on a GPU-less host: every case returns before a kernel is launched"""
    import ctypes as C
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_color_correct(None, None) == -1 and L.v3a_image_mse(None, None) == -1
    assert L.v3a_color_correct_workspace_bytes(1, 5, 7, 0) == -2 and L.v3a_color_correct_workspace_bytes(1, 5, 7, 17) == -2
    assert L.v3a_color_correct_workspace_bytes(0, 5, 7, 5) == -2 and L.v3a_image_mse_workspace_bytes(1, 0, 7, 3) == -2
    need = L.v3a_color_correct_workspace_bytes(2, 13, 37, 5)
    assert need == 8 * (2 * 3 * 2 * 66 + 2 * 5 * 30 + 2 * 2) + 4 * 30        # 2 workgroups per image at 481 pixels
    assert L.v3a_image_mse_workspace_bytes(2, 13, 37, 3) == 8 * 2 * 6

    def args(**kw):
        a = lib.ColorCorrectArgs()
        a.img = a.ref = a.out = a.sse = a.status = a.workspace = 256
        a.N, a.H, a.W, a.num_iters = 2, 13, 37, 5
        a.ld_img = a.ld_ref = a.ld_out = 111
        a.img_stride = a.ref_stride = a.out_stride = 13 * 111
        a.eps, a.workspace_bytes = 0.5 / 255, need
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    assert L.v3a_color_correct(args(img=None), None) == -1
    assert L.v3a_color_correct(args(out=258), None) == -1               # float pointer not 4-byte aligned
    assert L.v3a_color_correct(args(sse=260), None) == -1               # double pointer not 8-byte aligned
    assert L.v3a_color_correct(args(eps=0.5), None) == -1
    assert L.v3a_color_correct(args(ld_ref=110), None) == -2            # row stride under 3 W
    assert L.v3a_color_correct(args(out_stride=12 * 111), None) == -2   # images would overlap
    assert L.v3a_color_correct(args(num_iters=0), None) == -2
    assert L.v3a_color_correct(args(workspace_bytes=need - 1), None) == -4
    assert L.v3a_color_correct(args(workspace=260), None) == -4
    m = lib.ImageMseArgs()
    m.a = m.b = m.mse = m.workspace = 256
    m.N, m.H, m.W, m.C, m.ld_a, m.ld_b, m.a_stride, m.b_stride, m.workspace_bytes = 1, 4, 5, 3, 15, 14, 0, 0, 8
    assert L.v3a_image_mse(C.byref(m), None) == -2
    m.ld_b, m.workspace_bytes = 15, 7
    assert L.v3a_image_mse(C.byref(m), None) == -4


def test_hold_out_split():
    from vist3a_amd.post_opt import PostOptConfig, train_view_order, train_views, view_order
    assert PostOptConfig().test_every == 0
    assert train_views(5, 0) == [0, 1, 2, 3, 4] and train_views(5, 2) == [1, 3] and train_views(7, 3) == [1, 2, 4, 5]
    assert train_view_order(5, 23, 4, 0) == view_order(5, 23, 4)
    order = train_view_order(5, 23, 4, 2)
    assert len(order) == 23 and set(order) == {1, 3}
    for bad in ((3, 1), (1, 2), (1, 5)):
        with pytest.raises(ValueError, match="no view is left"):
            train_views(*bad)
    with pytest.raises(ValueError):
        train_views(3, -1)
