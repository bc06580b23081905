"""GPU tests of the step's visibility mask (ops.gs_visibility) and the visibility-masked Adam (ops.adam_step_visible;
csrc/post_opt.hip) against the numpy oracle of tests/visible_adam_oracle.py in fp64.

The parity metric and its gate are those of test_post_opt_gpu.test_adam_matches_torch: the largest elementwise relative error of p,
m, v after 5 steps, at most the recorded `adam` gate and at most 4x what the same update carried in fp32 on the CPU gives on the
same data.  The metric is set where the first moment nearly cancels, that is by the draw and not by the kernel, so the data follow
the recipe the gate was recorded on: p0 = randn, five gradients of 0.1 randn from a generator seeded with the sum of the shape,
lr 2.5e-3, the default betas, eps 1e-15.  Everything else here is exact."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import visible_adam_oracle as VO  # noqa: E402
from test_post_opt_gpu import gate  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000]
SHAPES = {"U": (), "Ux3": (3,), "Ux4": (4,), "Ux3x25": (3, 25)}
MASKS = ["all", "none", "alternating", "block_clear", "last_only"]


def _mask(kind, U):
    m = torch.zeros(U, dtype=torch.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "block_clear":     # one whole 256-row block of the launch clear: the second where the tensor has two full ones
        m[:] = 1
        lo = 256 if U >= 512 else 0
        m[lo:lo + 256] = 0
    elif kind == "last_only":
        m[-1] = 1
    return m


def _kw(tail):
    return dict(lr=2.5e-3, lr2=2.5e-3 / 20, period=25, betas=(0.9, 0.999), eps=1e-15) if tail == (3, 25) else \
        dict(lr=2.5e-3, betas=(0.9, 0.999), eps=1e-15)


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("U", SIZES)
@pytest.mark.parametrize("Cn", [1, 3])
def test_visibility_is_any_positive_radius(hip_lib, Cn, U):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(100 * Cn + U)
    radii = torch.randint(-3, 4, (Cn, U), generator=g, dtype=torch.int32)          # zeros, negatives, small positives
    radii[:, ::7] = 0
    big = torch.rand(Cn, U, generator=g) < 0.05
    radii[big] = 2 ** 31 - 1
    radii[torch.rand(Cn, U, generator=g) < 0.05] = -2 ** 31
    radii[Cn - 1] = 0 if Cn > 1 else radii[0]                                       # one camera sees nothing (with C = 3)
    want = (radii > 0).any(0)
    got = ops.gs_visibility(radii.cuda())
    assert got.dtype == torch.uint8 and got.shape == (U,) and got.is_cuda
    assert torch.equal(got.cpu(), want.to(torch.uint8))
    assert np.array_equal(VO.visibility(radii.numpy()), want.numpy().astype(np.uint8))
    zero = ops.gs_visibility(torch.zeros(Cn, U, dtype=torch.int32, device="cuda"))
    assert not bool(zero.any())
    if U > 1:
        assert bool(want.any()) and not bool(want.all())


def test_visibility_argument_errors(hip_lib):
    from vist3a_amd import ops
    for bad in (torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(2, 5, device="cuda"), torch.zeros(2, 5, dtype=torch.int32),
                torch.zeros(0, 5, dtype=torch.int32, device="cuda"), torch.zeros(5, 2, dtype=torch.int32, device="cuda").t()):
        with pytest.raises(ValueError):
            ops.gs_visibility(bad)


# ------------------------------------------------------------------------------------------------ parity
@pytest.fixture(scope="module")
def data():
    """p0, five gradients, for every (shape, U): drawn once, read only"""
    out = {}
    for name, tail in SHAPES.items():
        for U in SIZES:
            g = torch.Generator().manual_seed(U + sum(tail))                  # test_adam_matches_torch seeds with the sum of the shape
            out[name, U] = (torch.randn(U, *tail, generator=g), [torch.randn(U, *tail, generator=g) * 0.1 for _ in range(5)])
    return out


def _oracle(p0, grads, mask, kw, dtype):
    p, m, v = p0.numpy(), np.zeros(p0.shape), np.zeros(p0.shape)
    for gr in grads:
        p, m, v = VO.adam_step_visible(p, gr.numpy(), m, v, mask.numpy(), dtype=dtype, **kw)
    return p, m, v


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("U", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_the_fp64_oracle(hip_lib, parity, data, name, U, kind):
    from vist3a_amd import ops
    p0, grads = data[name, U]
    tail, mask = SHAPES[name], _mask(kind, U)
    kw = _kw(tail)
    p, m, v = p0.clone().cuda(), torch.zeros_like(p0).cuda(), torch.zeros_like(p0).cuda()
    md = mask.cuda()
    for gr in grads:
        ops.adam_step_visible(p, gr.cuda(), m, v, md, **kw)
    r64, r32 = _oracle(p0, grads, mask, kw, np.float64), _oracle(p0, grads, mask, kw, np.float32)
    rows = mask.numpy().astype(bool)
    # invisible rows: p as it came, zero moments - exactly
    for got, start in ((p, p0), (m, torch.zeros_like(p0)), (v, torch.zeros_like(p0))):
        assert torch.equal(got.cpu()[~mask.bool()], start[~mask.bool()])
    if not rows.any():
        return
    mx = lambda a, b: float(np.abs((np.asarray(a, dtype=np.float64)[rows] - b[rows]) / b[rows]).max())
    e = max(mx(a.cpu().numpy(), b) for a, b in zip((p, m, v), r64))
    e32 = max(mx(a, b) for a, b in zip(r32, r64))
    print(f"[adam_visible {name} U={U} {kind}] max relative error of p, m, v after 5 steps: hip {e:.3e}   numpy fp32 {e32:.3e}   gate {gate('adam'):.1e}")
    parity(f"post_opt::adam_visible[{name},U={U},{kind}]", rel_max=e, cpu_fp32_rel_max=e32, gate=gate("adam"))
    assert e <= gate("adam") and e <= 4 * e32, (e, e32)


# ------------------------------------------------------------------------------------------------ exact properties
def _state(U, tail, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda s=1.0: (torch.randn(U, *tail, generator=g) * s).cuda()
    return r(), r(0.1), r(0.05), (torch.rand(U, *tail, generator=g) * 0.01).cuda()


@pytest.mark.parametrize("name", list(SHAPES))
def test_clear_rows_keep_their_bits_even_under_nan_gradients(hip_lib, name):
    from vist3a_amd import ops
    tail, U = SHAPES[name], 1000
    p, g, m, v = _state(U, tail, 11)
    for kind in ("alternating", "block_clear", "last_only", "none"):
        mask = _mask(kind, U).cuda()
        clear = ~mask.bool()
        gn = g.clone()
        gn[clear] = float("nan")
        a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
        ops.adam_step_visible(a[0], g, a[1], a[2], mask, **_kw(tail))
        ops.adam_step_visible(b[0], gn, b[1], b[2], mask, **_kw(tail))
        for x, y, start in zip(a, b, (p, m, v)):
            assert torch.equal(G.bits(x), G.bits(y)) and bool(torch.isfinite(y).all())      # the NaN reached nothing
            assert torch.equal(G.bits(y[clear]), G.bits(start[clear]))                      # clear rows keep their bits
            if kind != "none":
                assert not bool((y[mask.bool()] == start[mask.bool()]).all())                # the others moved


def test_two_rates_equal_two_calls_on_the_slices(hip_lib):
    from vist3a_amd import ops
    U, K = 1000, 25
    p, g, m, v = _state(U, (3, K), 12)
    mask = _mask("alternating", U).cuda()
    mask[300:600] = 0
    kw = dict(betas=(0.8, 0.998), eps=1e-15)
    whole = [t.clone() for t in (p, m, v)]
    dc = [t[..., :1].contiguous() for t in (p, m, v)]
    rest = [t[..., 1:].contiguous() for t in (p, m, v)]
    for _ in range(3):
        ops.adam_step_visible(whole[0], g, whole[1], whole[2], mask, lr=2.5e-3, lr2=2.5e-3 / 20, period=K, **kw)
        ops.adam_step_visible(dc[0], g[..., :1].contiguous(), dc[1], dc[2], mask, lr=2.5e-3, **kw)
        ops.adam_step_visible(rest[0], g[..., 1:].contiguous(), rest[1], rest[2], mask, lr=2.5e-3 / 20, **kw)
    for w, a, b in zip(whole, dc, rest):
        assert torch.equal(w, torch.cat([a, b], -1))
    assert not torch.equal(whole[0], p)


@pytest.mark.parametrize("name", list(SHAPES))
def test_unaligned_views_take_the_scalar_path_with_the_same_bits(hip_lib, name):
    from vist3a_amd import ops
    tail, U = SHAPES[name], 257
    p, g, m, v = _state(U, tail, 13)
    n = p.numel()
    mask = _mask("alternating", U).cuda()
    pitch = (n + 3) // 4 * 4 + 4
    buf = torch.zeros(4 * pitch + 4, device="cuda")
    views = [buf[i * pitch + 1:i * pitch + 1 + n].view(U, *tail) for i in range(4)]         # each 4 bytes past a 16-byte boundary
    assert all(t.data_ptr() % 16 == 4 for t in views)
    for dst, src in zip(views, (p, g, m, v)):
        dst.copy_(src)
    ops.adam_step_visible(views[0], views[1], views[2], views[3], mask, **_kw(tail))
    ops.adam_step_visible(p, g, m, v, mask, **_kw(tail))
    assert torch.equal(views[0], p) and torch.equal(views[2], m) and torch.equal(views[3], v) and torch.equal(views[1], g)


def test_two_runs_are_bit_identical(hip_lib):
    from vist3a_amd import ops
    out = []
    for _ in range(2):
        p, g, m, v = _state(1000, (3, 25), 14)
        mask = _mask("alternating", 1000).cuda()
        for _ in range(3):
            ops.adam_step_visible(p, g, m, v, mask, **_kw((3, 25)))
        out.append((p, m, v))
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_argument_errors(hip_lib):
    from vist3a_amd import ops
    p, g, m, v = _state(10, (3,), 15)
    ok = torch.ones(10, dtype=torch.uint8, device="cuda")
    ops.adam_step_visible(p, g, m, v, ok, lr=1e-3)
    for bad in (torch.ones(9, dtype=torch.uint8, device="cuda"), torch.ones(10, 3, dtype=torch.uint8, device="cuda"),      # shape
                torch.ones(10, dtype=torch.bool, device="cuda"), torch.ones(10, device="cuda"),                            # dtype
                torch.ones(10, dtype=torch.uint8), torch.ones(20, dtype=torch.uint8, device="cuda")[::2]):                 # device, stride
        with pytest.raises(ValueError, match="visible"):
            ops.adam_step_visible(p, g, m, v, bad, lr=1e-3)
    with pytest.raises(ValueError):
        ops.adam_step_visible(p, g[:5], m, v, ok, lr=1e-3)
    with pytest.raises(ValueError):
        ops.adam_step_visible(p, g.double(), m, v, ok, lr=1e-3)


# ------------------------------------------------------------------------------------------------ guard bands
def _verdict(parity, case, outs, inputs):
    """the protocol of tests/test_guard_bands_gpu.verdict: nothing outside a view changed, inputs unchanged, bit-equal to the tight run"""
    torch.cuda.synchronize()
    viol = sum(G.violations(view)[0] for _, view, _ in outs)
    biteq = all(torch.equal(G.bits(view), G.bits(clean)) for _, view, clean in outs)
    in_ok = {name: G.unchanged(view, values) for name, view, values in inputs}
    parity("guard_bands", case=case, violations=viol, bit_equal=biteq, inputs_unchanged=all(in_ok.values()))
    assert viol == 0, (case, [(n, G.violations(view)[1]) for n, view, _ in outs])
    assert all(in_ok.values()), (case, in_ok)
    assert biteq, case


@pytest.mark.parametrize("U", [1, 257])
@pytest.mark.parametrize("Cn", [1, 3])
def test_guard_bands_visibility(hip_lib, parity, Cn, U):
    from vist3a_amd import ops
    from vist3a_amd import lib as L
    radii = torch.randint(-2, 3, (Cn, U), generator=torch.Generator().manual_seed(U + Cn), dtype=torch.int32).cuda()
    clean = ops.gs_visibility(radii)
    gr = G.carve_like(radii)
    out = G.carve((U,), torch.uint8, device="cuda")
    L.check(L.load().v3a_gs_visibility(ops._ptr(gr), Cn, U, ops._ptr(out), ops._stream()), "v3a_gs_visibility")
    _verdict(parity, f"gs_visibility C={Cn} U={U}", [("visible", out, clean)], [("radii", gr, radii)])


@pytest.mark.parametrize("kind", ["alternating", "block_clear", "last_only"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_guard_bands_adam_visible(hip_lib, parity, name, kind):
    """Two steps in place on carved p / m / v; g and the mask are inputs.  The clear rows of g are the arena's own 0xFF bytes (NaN):
    they are left as carved, so a load of them would show in the result."""
    from vist3a_amd import ops
    tail, U = SHAPES[name], 257
    p, g, m, v = _state(U, tail, 16)
    mask = _mask(kind, U).cuda()
    clear = ~mask.bool()
    gp, gm, gv, gmask = G.carve_like(p), G.carve_like(m), G.carve_like(v), G.carve_like(mask)
    poisoned = g.clone()
    poisoned.view(torch.int32)[clear] = -1                                                  # all-ones bits, as the arena's
    gg = G.carve_like(poisoned)
    for _ in range(2):
        ops.adam_step_visible(p, g, m, v, mask, **_kw(tail))
        ops.adam_step_visible(gp, gg, gm, gv, gmask, **_kw(tail))
    _verdict(parity, f"adam_step_visible {name} {kind}", [("p", gp, p), ("m", gm, m), ("v", gv, v)], [("g", gg, poisoned), ("visible", gmask, mask)])
