"""GPU tests of the post-optimisation regularisers (csrc/splat_reg.hip: v3a_splat_reg, v3a_splat_reg_backward; ops.splat_regularisers)
against torch in fp64: (mean sigmoid(logit), mean exp(log_scale)) and their gradients.

Sizes: U = 1 (scalar tails only), 5 (one 16-byte group + a tail of the logits; 15 log-scales), 1027 (several workgroups' worth of
groups and a tail), 70 001 (more groups than the grid's first stride covers in one workgroup each; 3 U % 4 != 0).

Bounds.  Values: 1e-12 relative (fp64 arithmetic on both sides, at most 2.1e5 terms, only the summation order and the last bit of
exp differ).  Gradients: ||g - g64|| / ||g64|| <= 1.2e-7, one fp32 rounding of the stored gradient (6e-8) with a factor 2.
Every test prints its figures before it asserts and logs them through the `parity` fixture."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402

pytestmark = pytest.mark.gpu

VALUE_TOL, GRAD_TOL = 1e-12, 1.2e-7
SIZES = [1, 5, 1027, 70_001]


def _inputs(U):
    g = torch.Generator().manual_seed(U)
    return torch.randn(U, 3, generator=g) * 0.8 - 2.0, torch.randn(U, generator=g) * 2.0      # log-scales, logits


def _reference(ls, lg, g0, g1):
    ls64, lg64 = ls.double().requires_grad_(True), lg.double().requires_grad_(True)
    om, sm = torch.sigmoid(lg64).mean(), torch.exp(ls64).mean()
    d_ls, d_lg = torch.autograd.grad(g0 * om + g1 * sm, [ls64, lg64])
    return om.detach(), sm.detach(), d_ls, d_lg


def _rel(a, b):
    return float((a.detach().cpu().double() - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("U", SIZES)
def test_values_and_gradients_match_fp64(hip_lib, parity, U):
    from vist3a_amd import ops
    ls, lg = _inputs(U)
    g0, g1 = 0.7, -1.3
    om64, sm64, dls64, dlg64 = _reference(ls, lg, g0, g1)
    lsd, lgd = ls.cuda().requires_grad_(True), lg.cuda().requires_grad_(True)
    om, sm = ops.splat_regularisers(lsd, lgd)
    assert om.dtype == sm.dtype == torch.float64 and om.shape == sm.shape == ()
    d_ls, d_lg = torch.autograd.grad(g0 * om + g1 * sm, [lsd, lgd])
    ev = max(abs(float(om) - float(om64)) / float(om64), abs(float(sm) - float(sm64)) / float(sm64))
    e_ls, e_lg = _rel(d_ls, dls64), _rel(d_lg, dlg64)
    print(f"[splat_reg U={U}] values rel {ev:.3e} (bound {VALUE_TOL:.0e}); d_log_scales {e_ls:.3e}, d_logits {e_lg:.3e} (bound {GRAD_TOL:.1e})")
    parity("splat_reg::parity", U=U, value_rel=ev, d_log_scales_rel_l2=e_ls, d_logits_rel_l2=e_lg, value_gate=VALUE_TOL, grad_gate=GRAD_TOL)
    assert d_ls.dtype == d_lg.dtype == torch.float32 and d_ls.shape == (U, 3) and d_lg.shape == (U,)
    assert ev <= VALUE_TOL and e_ls <= GRAD_TOL and e_lg <= GRAD_TOL


@pytest.mark.parametrize("U", SIZES)
def test_linear_and_bit_identical(hip_lib, U):
    from vist3a_amd import ops
    ls, lg = (t.cuda() for t in _inputs(U))

    def run(g0, g1, only=None):
        a, b = ls.clone().requires_grad_(True), lg.clone().requires_grad_(True)
        om, sm = ops.splat_regularisers(a, b)
        loss = g0 * om + g1 * sm if only is None else (g0 * om if only == 0 else g1 * sm)
        return (om.detach(), sm.detach()) + torch.autograd.grad(loss, [a, b], allow_unused=True)

    r1, r1b, r2 = run(0.7, -1.3), run(0.7, -1.3), run(1.4, -2.6)
    for a, b in zip(r1, r1b):
        assert torch.equal(a, b)                                   # bit-identical run to run, values and gradients
    for a, b in zip(r1[2:], r2[2:]):
        assert torch.equal(b, 2 * a)                               # exactly linear in the incoming gradient
    z = run(0.0, 0.0)
    assert float(z[2].abs().max()) == 0 and float(z[3].abs().max()) == 0
    # each mean reaches its own input only: with the other's gradient absent, that input's gradient is exactly zero
    o = run(0.7, 0.0, only=0)
    assert float(o[2].abs().max()) == 0 and torch.equal(o[3], r1[3])
    assert bool((r1[3] > 0).all()) and bool((r1[2] < 0).all())     # d sigmoid > 0 times 0.7; exp > 0 times -1.3


@pytest.mark.parametrize("U,offset", [(1, 0), (5, 4), (1027, 0), (1027, 4), (70_001, 0)])
def test_guard_bands(hip_lib, parity, U, offset):
    """Every tensor carved out of a poisoned arena (tests/guard.py), the workspace at exactly v3a_splat_reg_workspace_bytes; with
    offset 4 the pointers miss 16-byte alignment and the scalar path runs.  No byte outside the views changes, the inputs keep their
    bits, and the results are those of the plain call: bit for bit, except the two sums on the scalar path (another order, 1e-12)."""
    from vist3a_amd import ops
    L = hip_lib
    ls, lg = (t.cuda() for t in _inputs(U))
    om, sm = ops.splat_regularisers(ls, lg)
    d_out = torch.tensor([0.7, -1.3], dtype=torch.float64, device="cuda")
    a, b = ls.clone().requires_grad_(True), lg.clone().requires_grad_(True)
    o2 = ops.splat_regularisers(a, b)
    c_ls, c_lg = torch.autograd.grad(0.7 * o2[0] + -1.3 * o2[1], [a, b])
    need = int(L.v3a_splat_reg_workspace_bytes(U))
    assert need > 0 and need % 16 == 0
    g_ls, g_lg = G.carve_like(ls, offset_bytes=offset), G.carve_like(lg, offset_bytes=offset)
    g_out, g_ws = G.carve((2,), torch.float64, device="cuda"), G.carve((need // 8,), torch.float64, device="cuda")
    g_dout = G.carve_like(d_out)
    g_dls, g_dlg = G.carve((U, 3), torch.float32, offset_bytes=offset, device="cuda"), G.carve((U,), torch.float32, offset_bytes=offset, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.v3a_splat_reg(p(g_lg), p(g_ls), U, p(g_out), p(g_ws), need, stream) == 0
    assert L.v3a_splat_reg(p(g_lg), p(g_ls), U, p(g_out), p(g_ws), need - 8, stream) == -4          # held to its stated size
    assert L.v3a_splat_reg_backward(p(g_lg), p(g_ls), U, p(g_dout), p(g_dlg), p(g_dls), stream) == 0
    torch.cuda.synchronize()
    bad = {n: G.violations(t) for n, t in (("out", g_out), ("workspace", g_ws), ("d_logits", g_dlg), ("d_log_scales", g_dls))}
    counts = {n: v[0] for n, v in bad.items()}
    print(f"[splat_reg guard U={U} offset={offset}] workspace {need} B; violations {counts}")
    parity("splat_reg::guard", U=U, offset=offset, workspace_bytes=need, violations=sum(v[0] for v in bad.values()))
    for n, (cnt, where) in bad.items():
        assert cnt == 0, (n, cnt, where)
    assert G.unchanged(g_ls, ls) and G.unchanged(g_lg, lg) and G.unchanged(g_dout, d_out)
    if offset == 0:
        assert torch.equal(g_out, torch.stack([om, sm]))
    else:   # the scalar path hands each lane other elements than the 16-byte path: the same terms in another order
        assert float(((g_out - torch.stack([om, sm])).abs() / torch.stack([om, sm])).max()) <= VALUE_TOL
    assert torch.equal(g_dls, c_ls) and torch.equal(g_dlg, c_lg)
