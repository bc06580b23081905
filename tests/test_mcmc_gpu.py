"""GPU tests of the MCMC strategy's kernels (csrc/mcmc.hip through ops.mcmc_sample, ops.mcmc_relocate, ops.mcmc_noise) against
tests/mcmc_oracle.py.

Sampler: src and counts equal the oracle's EXACTLY (integers; every sum is fp64 on exactly converted f32 values in a fixed order).
Sizes: U = 1 and 5 (one ragged block), 1024 (one full block), 1025 (a second block of one element), 2049, 70 001 (69 blocks: the
prefix pass stages the block totals through LDS once, the binary search runs 7 levels).  The weights span 14 decades, because f32
values of similar size add exactly in fp64 and would hide a wrong order (tests/test_mcmc_host.py::test_block_tree_order_is_visible).

Relocation, growth and noise: every f32 output is fp64 arithmetic rounded once, so ||a - a64|| / ||a64|| <= 1.2e-7 (2^-23: one
rounding, 6e-8 per element at the most, with the factor 2 of the other section-7f kernels), a64 the oracle's unrounded fp64 value.
The gate of a comparison is never above the oracle's own float32 run of the same case: min(1.2e-7, that run's figure), so that
a kernel computing in single precision does not pass.  Copies, zeroed moments and untouched rows are compared bit
for bit.  Every test prints its figures before it asserts and logs them through the `parity` fixture."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mcmc_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1.2e-7


def gate(fp32_figure):
    """1.2e-7, and never above what the oracle's float32 run of the same case reaches"""
    return min(TOL, fp32_figure)
MIN_OP = 0.005
SIZES = [1, 5, 1024, 1025, 2049, 70_001]


def wide_weights(U, seed=0):
    g = np.random.default_rng(1000 + U + seed)
    w = (g.random(U) * 10 ** (-14 * g.random(U))).astype(np.float32)
    if U > 1:
        w[0], w[-1] = 0.6, 0.001        # at least one alive and one dead, also at U = 5
    return w


def slots_of(U, alive_only):
    return U if alive_only else U // 20 + 3


@functools.lru_cache(maxsize=None)
def oracle_sample(U, alive_only, seed=7, step=13):
    return MO.sample(wide_weights(U), MIN_OP, alive_only, slots_of(U, alive_only), seed, 0 if alive_only else 1, step)


def gpu_sample(w, alive_only, n_slots, seed=7, step=13, min_weight=MIN_OP):
    from vist3a_amd import ops
    src, counts = ops.mcmc_sample(torch.from_numpy(w).cuda(), min_weight=min_weight, alive_only=alive_only, n_slots=n_slots, seed=seed,
                                  stream=0 if alive_only else 1, step=step)
    assert src.dtype == counts.dtype == torch.int32 and src.shape == (n_slots,) and counts.shape == (len(w),)
    return src.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("alive_only", [True, False], ids=["relocation", "growth"])
@pytest.mark.parametrize("U", SIZES)
def test_sampler_equals_oracle(hip_lib, parity, U, alive_only):
    w = wide_weights(U)
    want_src, want_counts = oracle_sample(U, alive_only)
    src, counts = gpu_sample(w, alive_only, slots_of(U, alive_only))
    diff = int((src != want_src).sum()) + int((counts != want_counts).sum())
    print(f"[mcmc sample U={U} {'relocation' if alive_only else 'growth'}] drawn {int((want_src >= 0).sum())} of {len(src)} slots, "
          f"largest count {int(want_counts.max())}; entries that differ from the oracle: {diff}")
    parity("mcmc::sample", U=U, alive_only=alive_only, drawn=int((want_src >= 0).sum()), differing=diff)
    assert np.array_equal(src, want_src) and np.array_equal(counts, want_counts)
    again = gpu_sample(w, alive_only, slots_of(U, alive_only))
    assert np.array_equal(src, again[0]) and np.array_equal(counts, again[1])          # two runs: bit-identical
    assert (want_src >= 0).sum() > (20 if U >= 1024 else 0) or U == 1                  # (one Gaussian alone is dead or alive: nothing to draw)
    if U >= 1024:
        assert not np.array_equal(src, gpu_sample(w, alive_only, slots_of(U, alive_only), seed=8)[0])
        assert not np.array_equal(src, gpu_sample(w, alive_only, slots_of(U, alive_only), step=14)[0])


@pytest.mark.parametrize("alive_only", [True, False], ids=["relocation", "growth"])
def test_sampler_zero_blocks(hip_lib, alive_only):
    """a whole zero block in the middle and one at the end (with a ragged tail): never entered, though P_b <= t holds for them"""
    U = 4 * 1024 + 5
    w = wide_weights(U, seed=1)
    w[::3] = 0.5
    w[::5] = 0.001                                   # dead ones in the live blocks
    w[1024:2048] = 0.0
    w[3072:] = 0.0
    n = slots_of(U, alive_only)
    want = MO.sample(w, MIN_OP, alive_only, n, 3, 0 if alive_only else 1, 21)
    src, counts = gpu_sample(w, alive_only, n, seed=3, step=21)
    assert np.array_equal(src, want[0]) and np.array_equal(counts, want[1])
    drawn = src[src >= 0]
    assert len(drawn) > 100 and {int(i) // 1024 for i in drawn} == {0, 2} and (w[drawn] > (MIN_OP if alive_only else 0)).all()


def heavy_case():
    """one Gaussian with nearly all the weight, 90 dead slots: its count passes the clamp of the relocation ratio (51)"""
    w = np.full(100, 0.006, dtype=np.float32)
    w[7] = 0.99
    w[10:] = 0.001
    return w


def test_sampler_one_heavy_gaussian(hip_lib):
    w = heavy_case()
    want = MO.sample(w, MIN_OP, True, 100, 5, 0, 2)
    src, counts = gpu_sample(w, True, 100, seed=5, step=2)
    assert np.array_equal(src, want[0]) and np.array_equal(counts, want[1])
    assert (src >= 0).sum() == 90 and counts[7] >= 60 and counts.sum() == 90


def test_sampler_no_ops(hip_lib):
    for U in (5, 1500):
        for w, alive_only, n in ((np.zeros(U, np.float32), True, U),                       # nothing alive
                                 (np.full(U, 0.004, np.float32), True, U),                 # all dead, by the threshold
                                 (np.full(U, 0.5, np.float32), True, U),                   # nothing dead: no active slot
                                 (np.zeros(U, np.float32), False, 40)):                    # growth from an empty pool
            src, counts = gpu_sample(w, alive_only, n)
            assert (src == -1).all() and (counts == 0).all(), (U, alive_only)


def test_sampler_rejects_bad_arguments(hip_lib):
    from vist3a_amd import ops
    w = torch.rand(8, device="cuda")
    kw = dict(min_weight=MIN_OP, alive_only=True, n_slots=8, seed=1, stream=0, step=1)
    for bad in (dict(n_slots=7), dict(n_slots=0, alive_only=False), dict(stream=2), dict(seed=-1), dict(step=2 ** 32)):
        with pytest.raises(ValueError):
            ops.mcmc_sample(w, **{**kw, **bad})
    with pytest.raises(ValueError):
        ops.mcmc_sample(w.cpu(), **kw)
    with pytest.raises(ValueError):
        ops.mcmc_sample(w.double(), **kw)


# ------------------------------------------------------------------------------------------------------- relocation and growth

def scene(rows, K, seed, opacities=None):
    g = np.random.default_rng(seed)
    f = lambda *s: g.normal(size=s).astype(np.float32)
    op = g.uniform(0.02, 0.98, rows).astype(np.float32) if opacities is None else opacities
    p = dict(means=f(rows, 3), scales=f(rows, 3) * 0.6 - 2.5, quats=f(rows, 4), opacities=np.log(op / (1 - op)).astype(np.float32), sh=f(rows, 3, K) * 0.3)
    m = {k: f(*x.shape) * 1e-3 for k, x in p.items()}
    v = {k: np.abs(f(*x.shape)) * 1e-6 for k, x in p.items()}
    return p, m, v


def relocation_case(U, K):
    g = np.random.default_rng(50 + U)
    if U == 100:
        op = heavy_case()
    elif U == 5:
        op = np.array([0.7, 0.001, 0.9, 0.002, 0.3], dtype=np.float32)
    else:
        op = g.uniform(0.02, 0.98, U).astype(np.float32)
        op[g.random(U) < 0.3] = 0.001
        op[0], op[U - 1] = 0.7, 0.002
    p, m, v = scene(U, K, U + K, op)
    w = (1.0 / (1.0 + np.exp(-p["opacities"].astype(np.float64)))).astype(np.float32)
    return p, m, v, w


def to_gpu(d):
    return {k: torch.from_numpy(x).cuda() for k, x in d.items()}


def check_move(parity, tag, before, got, src, counts, dst_offset, **info):
    """`got` (params, m, v on the device) against the oracle run on `before` (numpy)."""
    p, m, v = before
    p2, m2, v2, exact = MO.relocate(src, counts, p, m, v, dst_offset, MIN_OP)
    p32, _, _, _ = MO.relocate(src, counts, p, m, v, dst_offset, MIN_OP, values=MO.new_values_f32)
    gp, gm, gv = ({k: x.cpu().numpy() for k, x in d.items()} for d in got)
    touched = np.isfinite(exact["opacities"])
    assert touched.sum() == (counts > 0).sum() + (src >= 0).sum()
    figures = {}
    for name in ("opacities", "scales"):
        a64 = exact[name][touched]
        figures[name] = float(np.linalg.norm(gp[name][touched] - a64) / np.linalg.norm(a64))
        figures[name + "_f32"] = float(np.linalg.norm(p32[name][touched] - a64) / np.linalg.norm(a64))
    print(f"[mcmc {tag}] rows written {int(touched.sum())}, largest count {int(counts.max())}: logits {figures['opacities']:.3e} "
          f"(oracle fp32 {figures['opacities_f32']:.3e}), log-scales {figures['scales']:.3e} (oracle fp32 {figures['scales_f32']:.3e}); gates {gate(figures['opacities_f32']):.3e}, {gate(figures['scales_f32']):.3e}")
    parity(f"mcmc::{tag}", gate=TOL, rows_written=int(touched.sum()), max_count=int(counts.max()), **figures, **info)
    for name in ("opacities", "scales"):       # rows that are neither source nor destination keep their bits
        assert np.array_equal(gp[name][~touched].view(np.int32), p[name][~touched].view(np.int32))
    for name in ("means", "quats", "sh"):      # copies and everything else: bit for bit what the oracle moved
        assert np.array_equal(gp[name].view(np.int32), p2[name].view(np.int32)), name
    for name in MO.NAMES:                      # moments: zeroed or untouched exactly as specified
        assert np.array_equal(gm[name].view(np.int32), m2[name].view(np.int32)) and np.array_equal(gv[name].view(np.int32), v2[name].view(np.int32)), name
    for s, j in enumerate(src.tolist()):       # a copy's new values are its source's, bit for bit
        if j >= 0:
            assert gp["opacities"][dst_offset + s] == gp["opacities"][j] and np.array_equal(gp["scales"][dst_offset + s], gp["scales"][j])
    assert figures["opacities"] <= gate(figures["opacities_f32"]) and figures["scales"] <= gate(figures["scales_f32"]), figures


@pytest.mark.parametrize("U,K", [(5, 1), (5, 25), (1027, 1), (1027, 25), (100, 1)])
def test_relocation_matches_oracle(hip_lib, parity, U, K):
    from vist3a_amd import ops
    p, m, v, w = relocation_case(U, K)
    src, counts = MO.sample(w, MIN_OP, True, U, 11, 0, 5)
    assert (src >= 0).sum() >= 2 and (U != 100 or counts.max() >= 60)                 # U = 100: the ratio is clamped at 51
    gp, gm, gv = to_gpu(p), to_gpu(m), to_gpu(v)
    gsrc, gcounts = ops.mcmc_sample(torch.from_numpy(w).cuda(), min_weight=MIN_OP, alive_only=True, n_slots=U, seed=11, stream=0, step=5)
    assert np.array_equal(gsrc.cpu().numpy(), src) and np.array_equal(gcounts.cpu().numpy(), counts)
    ops.mcmc_relocate(gsrc, gcounts, gp, gm, gv, dst_offset=0, min_opacity=MIN_OP)
    check_move(parity, "relocate", (p, m, v), (gp, gm, gv), src, counts, 0, U=U, K=K)


@pytest.mark.parametrize("U,K", [(5, 1), (5, 25), (1027, 1), (1027, 25)])
def test_growth_matches_oracle(hip_lib, parity, U, K):
    from vist3a_amd import ops
    n = 3 if U == 5 else 51
    p, m, v, w = relocation_case(U, K)
    src, counts = MO.sample(w, MIN_OP, False, n, 11, 1, 5)
    grow = lambda d: {k: np.concatenate([x, np.zeros((n,) + x.shape[1:], np.float32)]) for k, x in d.items()}
    p, m, v = grow(p), grow(m), grow(v)
    gp, gm, gv = to_gpu(p), to_gpu(m), to_gpu(v)
    for d in (gm, gv):                       # the new rows' moments must be WRITTEN: start them off non-zero
        for x in d.values():
            x[U:] = 1.0
    ops.mcmc_relocate(torch.from_numpy(src).cuda(), torch.from_numpy(counts).cuda(), gp, gm, gv, dst_offset=U, min_opacity=MIN_OP)
    check_move(parity, "grow", (p, m, v), (gp, gm, gv), src, counts, U, U=U, K=K)


def test_relocate_twice_is_bit_identical_and_checks_arguments(hip_lib):
    from vist3a_amd import ops
    p, m, v, w = relocation_case(1027, 25)
    src, counts = (torch.from_numpy(x).cuda() for x in MO.sample(w, MIN_OP, True, 1027, 11, 0, 5))
    runs = []
    for _ in range(2):
        g = [to_gpu(p), to_gpu(m), to_gpu(v)]
        ops.mcmc_relocate(src, counts, *g, dst_offset=0, min_opacity=MIN_OP)
        runs.append(g)
    assert all(torch.equal(runs[0][i][k], runs[1][i][k]) for i in range(3) for k in MO.NAMES)
    g = [to_gpu(p), to_gpu(m), to_gpu(v)]
    for bad in (dict(dst_offset=3), dict(min_opacity=0.0), dict(min_opacity=1.0)):
        with pytest.raises(ValueError):
            ops.mcmc_relocate(src, counts, *g, **{**dict(dst_offset=0, min_opacity=MIN_OP), **bad})
    with pytest.raises(ValueError):
        ops.mcmc_relocate(src[:-1], counts, *g, dst_offset=0, min_opacity=MIN_OP)
    with pytest.raises(ValueError):
        ops.mcmc_relocate(src.long(), counts, *g, dst_offset=0, min_opacity=MIN_OP)
    with pytest.raises(ValueError):
        ops.mcmc_relocate(src, counts, g[0], g[1], {**g[2], "sh": g[2]["sh"][:, :, :3].contiguous()}, dst_offset=0, min_opacity=MIN_OP)
    with pytest.raises(ValueError):          # growth wants U + n rows
        ops.mcmc_relocate(src[:4].contiguous(), counts, *g, dst_offset=1027, min_opacity=MIN_OP)


# --------------------------------------------------------------------------------------------------------------------- noise

SCALER = 5e5 * 1.6e-4    # the reference's noise_lr times the means' initial rate


def noise_case(U, zero_means):
    g = np.random.default_rng(300 + U)
    means = np.zeros((U, 3), np.float32) if zero_means else (g.normal(size=(U, 3)) * [0.8, 0.8, 1.0] + [0, 0, 4.0]).astype(np.float32)
    ls = np.log(0.02 + 0.2 * g.random((U, 3))).astype(np.float32)
    quats = (g.normal(size=(U, 4)) * g.uniform(0.2, 3.0, (U, 1))).astype(np.float32)         # raw: any length
    logits = (g.normal(size=U) * 2.0 - 5.0).astype(np.float32)                                   # opacities around 0.007: the gate is half open
    return means, ls, quats, logits


@pytest.mark.parametrize("zero_means", [True, False], ids=["displacement", "means"])
@pytest.mark.parametrize("U", [1, 5, 1027, 70_001])
def test_noise_matches_oracle(hip_lib, parity, U, zero_means):
    from vist3a_amd import ops
    means, ls, quats, logits = noise_case(U, zero_means)
    a64 = MO.noise(means, ls, quats, logits, SCALER, 9, 33)
    a32 = MO.noise(means, ls, quats, logits, SCALER, 9, 33, dt=np.float32)
    runs = []
    for _ in range(2):
        gm = torch.from_numpy(means).cuda()
        ops.mcmc_noise(gm, *(torch.from_numpy(x).cuda() for x in (ls, quats, logits)), scaler=SCALER, seed=9, step=33)
        runs.append(gm)
    got = runs[0].cpu().numpy()
    e, e32 = (float(np.linalg.norm(x.astype(np.float64) - a64) / np.linalg.norm(a64)) for x in (got, a32))
    moved = float(np.abs(a64 - means).max())
    print(f"[mcmc noise U={U} {'means = 0' if zero_means else 'real means'}] largest displacement {moved:.3e}; ||a - a64|| / ||a64|| = {e:.3e} "
          f"(oracle fp32 {e32:.3e}); gate {gate(e32):.3e}")
    parity("mcmc::noise", U=U, zero_means=zero_means, rel_l2=e, oracle_fp32_rel_l2=e32, gate=gate(e32), max_displacement=moved)
    assert got.dtype == np.float32 and np.isfinite(got).all() and moved > 1e-6
    assert torch.equal(runs[0], runs[1])                                                        # two runs: bit-identical
    assert e <= gate(e32), (e, e32)
    other = torch.from_numpy(means).cuda()
    ops.mcmc_noise(other, *(torch.from_numpy(x).cuda() for x in (ls, quats, logits)), scaler=SCALER, seed=9, step=34)
    assert not torch.equal(other, runs[0])


def test_noise_leaves_visible_gaussians_alone(hip_lib):
    """opacity >= 0.5, |means| >= 0.1, scales <= 1: the gate is <= e^-49 and the displacement far below half an ulp of any mean"""
    from vist3a_amd import ops
    U = 1027
    g = np.random.default_rng(4)
    means = (g.uniform(0.1, 5.0, (U, 3)) * g.choice([-1.0, 1.0], (U, 3))).astype(np.float32)
    ls = np.log(g.uniform(0.01, 1.0, (U, 3))).astype(np.float32)
    ls[0] = 0.0
    quats = g.normal(size=(U, 4)).astype(np.float32)
    logits = g.uniform(0.0, 9.0, U).astype(np.float32)
    logits[0] = 0.0
    gm = torch.from_numpy(means).cuda()
    ops.mcmc_noise(gm, *(torch.from_numpy(x).cuda() for x in (ls, quats, logits)), scaler=SCALER, seed=1, step=1)
    assert np.array_equal(gm.cpu().numpy().view(np.int32), means.view(np.int32))
    with pytest.raises(ValueError):
        ops.mcmc_noise(gm, torch.from_numpy(ls).cuda(), torch.from_numpy(quats[:, :3].copy()).cuda(), torch.from_numpy(logits).cuda(), scaler=1.0, seed=1, step=1)
