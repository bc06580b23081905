"""Host-side checks of the bilateral-grid colour compensation (no GPU): the plain-torch oracle of tests/bilagrid_oracle.py against
the tensors recorded from the reference's own module (tests/golden/bilagrid_ref.safetensors), the closed-form learning rate of the
grid Adam against torch's chained scheduler, the layout helpers, the new config fields and the argument errors."""
import sys
from dataclasses import fields
from pathlib import Path

import pytest
import torch
from safetensors.torch import load_file

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bilagrid_oracle as BO  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden" / "bilagrid_ref.safetensors"
KEYS = ("out", "d_rgb", "d_grids", "tv", "d_tv")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def gold():
    return load_file(str(GOLD))


@pytest.mark.parametrize("case", BO.GOLDEN_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])))
def test_oracle_matches_reference_module(gold, case):
    """fp64 against fp64: the same arithmetic up to the order of a few products, 1e-13 relative (measured here: at most 4e-16);
    the oracle's fp32 run is held to 4x the reference's own fp32 error, or 2.4e-7 where that is smaller"""
    (N, H, W), (GX, GY, L) = case
    p = f"{N}x{H}x{W}."
    rgb, grids, d_out = BO.make_inputs(N, H, W, GX, GY, L)
    assert torch.equal(rgb, gold[p + "rgb"]) and torch.equal(grids, gold[p + "grids"]) and torch.equal(d_out, gold[p + "d_out"])
    r64, r32 = BO.run(rgb, grids, d_out, torch.float64), BO.run(rgb, grids, d_out, torch.float32)
    for k in KEYS:
        e, e32, ref32 = _rel(r64[k], gold[p + k + "64"]), _rel(r32[k], gold[p + k + "64"]), _rel(gold[p + k + "32"], gold[p + k + "64"])
        print(f"[bilagrid oracle {p}{k}] fp64 vs reference fp64 {e:.3e} (bound 1e-13)   fp32 {e32:.3e} (reference fp32 {ref32:.3e})")
        assert r64[k].shape == gold[p + k + "64"].shape
        assert e <= 1e-13, (k, e)
        assert e32 <= max(4 * ref32, 2.4e-7), (k, e32, ref32)


def test_oracle_exact_properties():
    rgb, grids, d_out = BO.make_inputs(1, 5, 7, 4, 3, 5)
    ident = BO.identity(1, 4, 3, 5, torch.float64)
    assert _rel(BO.slice_grid(rgb.double(), ident), rgb) <= 1e-15
    assert float(BO.total_variation(ident)) == 0.0
    # the float32 weights sum to more than 1: a white pixel sits on the upper clamp
    assert float(BO.guidance(torch.ones(3, dtype=torch.float64))) > 1.0
    # the guidance gradient vanishes at both clamps (black, white and out-of-range pixels) and nowhere else
    gz = BO.guidance(rgb.double()) * 4
    clamped = (gz <= 0) | (gz >= 4)
    assert int(clamped.sum()) >= 5 and int((~clamped).sum()) >= 5
    for dt in (torch.float64, torch.float32):
        r = rgb.to(dt).requires_grad_(True)
        full, = torch.autograd.grad(BO.slice_grid(r, grids.to(dt)), r, d_out.to(dt))
        matrix_only, = torch.autograd.grad(BO.slice_grid(r, grids.to(dt), guide=r.detach()), r, d_out.to(dt))
        assert torch.equal(full[clamped], matrix_only[clamped])
        assert bool((full[~clamped] != matrix_only[~clamped]).any(-1).all())


def test_learning_rate_matches_chained_scheduler():
    """lr (0.01 + 0.99 min(s, warmup) / warmup) 0.01^(s / max_steps) against ChainedScheduler(LinearLR, ExponentialLR) as the reference
    builds it (simple_trainer.py:831-846): 1e-13 relative over 1200 steps (measured 3.4e-15)"""
    lr, warm, S = 2e-3, 1000, 3000
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr, eps=1e-15)
    sch = torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=warm),
        torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.01 ** (1.0 / S))])
    from vist3a_amd.post_opt.trainer import bilagrid_learning_rate
    from vist3a_amd.post_opt import PostOptConfig
    cfg = PostOptConfig(max_steps=S, bilagrid_lr=lr, bilagrid_warmup_steps=warm)
    worst = 0.0
    for s in range(1200):
        have = opt.param_groups[0]["lr"]
        worst = max(worst, abs(bilagrid_learning_rate(cfg, s) - have) / have, abs(BO.learning_rate(s, lr, warm, S) - have) / have)
        opt.step()
        sch.step()
    print(f"[bilagrid lr] closed form vs torch's chained scheduler over 1200 steps: {worst:.3e} (bound 1e-13)")
    assert worst <= 1e-13


def test_layout_helpers():
    from vist3a_amd import ops
    t = torch.arange(2 * 12 * 4 * 3 * 5, dtype=torch.float32).reshape(2, 12, 4, 3, 5)     # [V,12,L,GY,GX]
    ours = ops.bilagrid_from_reference(t)
    assert ours.shape == (2, 4, 3, 5, 12) and ours.is_contiguous()
    assert float(ours[1, 2, 1, 4, 7]) == float(t[1, 7, 2, 1, 4])
    assert torch.equal(ops.bilagrid_to_reference(ours), t)
    ident = ops.bilagrid_identity(3, 5, 3, 4, "cpu")
    assert ident.shape == (3, 4, 3, 5, 12) and ident.dtype == torch.float32
    assert torch.equal(ops.bilagrid_to_reference(ident), BO.identity(3, 5, 3, 4))
    for bad in ((0, 2, 2, 2), (1, 1, 2, 2), (1, 2, 1, 2), (1, 2, 2, 1)):
        with pytest.raises(ValueError):
            ops.bilagrid_identity(*bad, "cpu")
    with pytest.raises(ValueError):
        ops.bilagrid_from_reference(ours)
    with pytest.raises(ValueError):
        ops.bilagrid_to_reference(t)


def test_config_fields_and_validation():
    from vist3a_amd.post_opt import PostOptConfig
    c = PostOptConfig()
    assert (c.use_bilateral_grid, tuple(c.bilateral_grid_shape), c.bilagrid_lr, c.bilagrid_warmup_steps, c.bilagrid_tv_lambda) == \
        (False, (16, 16, 8), 2e-3, 1000, 10.0)
    assert {"use_bilateral_grid", "bilateral_grid_shape", "bilagrid_lr", "bilagrid_warmup_steps", "bilagrid_tv_lambda"} <= {f.name for f in fields(PostOptConfig)}
    PostOptConfig(use_bilateral_grid=True, bilateral_grid_shape=(4, 4, 3)).check_bilagrid()
    c.check_bilagrid()      # off: nothing is checked
    for bad in (dict(bilateral_grid_shape=(1, 4, 3)), dict(bilateral_grid_shape=(4, 1, 3)), dict(bilateral_grid_shape=(4, 4, 1)),
                dict(bilateral_grid_shape=(4, 4)), dict(bilateral_grid_shape=(4.5, 4, 3)), dict(bilagrid_warmup_steps=0),
                dict(bilagrid_lr=0.0), dict(bilagrid_tv_lambda=-1.0)):
        with pytest.raises(ValueError, match="bila"):
            PostOptConfig(use_bilateral_grid=True, **bad).check_bilagrid()


def test_argument_errors_without_gpu():
    from vist3a_amd import ops
    rgb, grids = torch.zeros(1, 4, 5, 3), torch.zeros(1, 2, 2, 2, 12)
    with pytest.raises(ValueError, match="device"):
        ops.bilagrid_slice(rgb, grids)
    with pytest.raises(ValueError, match="device"):
        ops.bilagrid_tv(grids)
    with pytest.raises(ValueError, match=r"\[N,H,W,3\]"):
        ops.bilagrid_slice(torch.zeros(4, 5, 3), grids)
    with pytest.raises(ValueError, match="grids"):
        ops.bilagrid_tv(torch.zeros(1, 12, 2, 2, 2))
    # the C entry points reject bad arguments before any launch
    import ctypes as C
    from vist3a_amd import lib as L
    lib = L.load()
    assert lib.v3a_bilagrid_slice_forward(None, None, None) == -1 and lib.v3a_bilagrid_tv_forward(None, None) == -1
    assert lib.v3a_bilagrid_slice_backward(None, None, None, None, None) == -1 and lib.v3a_bilagrid_tv_backward(None, None, None, None) == -1
    for shape in ((1, 2, 2), (2, 1, 2), (2, 2, 1)):
        assert lib.v3a_bilagrid_tv_workspace_bytes(1, *shape) == -2
        a = L.BilagridSliceArgs(1, 1, 1, 4, 4, *shape)        # non-null dummies: the shape is refused before they are touched
        assert lib.v3a_bilagrid_slice_forward(C.byref(a), 1, None) == -2
    assert lib.v3a_bilagrid_tv_workspace_bytes(0, 2, 2, 2) == -2 and lib.v3a_bilagrid_tv_workspace_bytes(1, 2, 2, 2) == 3 * 8
    assert lib.v3a_bilagrid_tv_workspace_bytes(1 << 20, 16, 16, 8) == -2
