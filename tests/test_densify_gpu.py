"""GPU tests of the densification kernels (csrc/densify.hip through ops.densify_accumulate, densify_classify, densify_apply,
densify_reset_opacity) against tests/densify_oracle.py.

Sizes: U = 1 and 5 (one ragged block), 1027 (five scan blocks of 256), 70 001 (274 blocks: the block-prefix pass takes two rounds of
256 with a carry); K = 1, 4, 25 (harmonics rows of 3, 12 and 75 floats: never, always, and one time in four on the 16-byte path).

Decisions are integers: the inputs keep every compared quantity at least 1e-6 (relative) from its threshold - asserted on the CPU
first - so fates, counts, offsets and totals EQUAL the oracle's.  Copied rows, kept moments and zeroed moments are compared bit for
bit.  Computed values (child means, child log-scales, revised logits, grad2d, reset logits) are fp64 arithmetic rounded once:
||a - a64|| / ||a64|| <= min(2^-23, the oracle's own float32 run of the same case), the rule of tests/test_mcmc_gpu.py."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import densify_oracle as DO  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -23
TH = dict(grow_grad2d=2e-4, grow_scale3d=0.01, prune_opa=0.005, prune_scale3d=0.1)
SIZES = [1, 5, 1027, 70_001]


def gate(fp32_figure):
    return min(TOL, fp32_figure)


def rel(a, a64):
    return float(np.linalg.norm(a.astype(np.float64) - a64) / np.linalg.norm(a64)) if a64.size else 0.0


@functools.lru_cache(maxsize=None)
def scene(U, K, seed=0):
    """params, m, v and the running statistics: a third of the Gaussians above the gradient threshold, scales spread over both
    scale thresholds, one in ten transparent.  Values that come within 1e-5 of a threshold are moved off it."""
    g = np.random.default_rng(100 + U + 7 * K + seed)
    f = lambda *s: g.normal(size=s).astype(np.float32)
    count = g.integers(0, 6, U).astype(np.int32)
    avg = TH["grow_grad2d"] * 10 ** g.uniform(-1.0, 0.6, U)
    grad = (avg * np.maximum(count, 1)).astype(np.float32)
    smax = 10 ** g.uniform(-3.0, -0.5, U)
    ls = np.log(smax[:, None] * g.uniform(0.2, 1.0, (U, 3)))
    ls[np.arange(U), g.integers(0, 3, U)] = np.log(smax)
    op = g.uniform(0.01, 0.99, U)
    op[g.random(U) < 0.1] = 0.002
    op[g.random(U) < 0.1] = 0.008                     # pruned as revised children only
    if U >= 5:
        grad[:5] = [1e-4, 1e-3, 1e-3, 1e-3, 1e-4]      # keep, clone, split, split with oversized children, oversized keep
        count[:5] = 1
        ls[:5] = np.log([0.004, 0.004, 0.05, 0.2, 0.3])[:, None]
        op[:5] = 0.6
    p = dict(means=f(U, 3), scales=ls.astype(np.float32), quats=(f(U, 4) * g.uniform(0.2, 3.0, (U, 1))).astype(np.float32),
             opacities=np.log(op / (1 - op)).astype(np.float32), sh=f(U, 3, K) * 0.3)
    for name, t, scale in (("scales", "grow_scale3d", 1.0), ("scales", "prune_scale3d", 1.0), ("scales", "prune_scale3d", 1.6)):
        near = np.abs(np.exp(p["scales"].astype(np.float64)).max(1) / scale / TH[t] - 1) < 1e-5
        p["scales"][near] += np.float32(0.01)
    m = {k: f(*x.shape) * 1e-3 for k, x in p.items()}
    v = {k: np.abs(f(*x.shape)) * 1e-6 for k, x in p.items()}
    return grad, count, p, m, v


def to_gpu(d):
    return {k: torch.from_numpy(x).cuda() for k, x in d.items()}


def gpu_classify(grad, count, p, **kw):
    from vist3a_amd import ops
    kw = dict(kw)
    kw["revised_opacity"] = kw.pop("revised", False)
    c = ops.densify_classify(torch.from_numpy(grad).cuda(), torch.from_numpy(count).cuda(), torch.from_numpy(p["scales"]).cuda(),
                             torch.from_numpy(p["opacities"]).cuda(), **TH, **kw)
    assert c["fates"].dtype == torch.uint8 and c["counts"].dtype == c["offsets"].dtype == torch.int32 and c["totals"].dtype == torch.int64
    return c


def same_cls(c, want):
    return all(np.array_equal(c[k].cpu().numpy(), want[k]) for k in ("fates", "counts", "offsets", "totals"))


# -------------------------------------------------------------------------------------------------------------- accumulate

@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("U", SIZES)
def test_accumulate(hip_lib, parity, U, Cn):
    from vist3a_amd import ops
    g = np.random.default_rng(U + Cn)
    d = (g.normal(size=(Cn, U, 2)) * 10 ** g.uniform(-7, -3, (Cn, U, 1))).astype(np.float32)
    radii = g.integers(-1, 4, (Cn, U)).astype(np.int32)                                 # a third of the entries culled (radius <= 0)
    grad0 = (g.random(U) * 1e-3).astype(np.float32)
    count0 = g.integers(0, 5, U).astype(np.int32)
    a64, cnt = DO.accumulate(grad0, count0, d, radii, 64, 48)
    a32, _ = DO.accumulate(grad0, count0, d, radii, 64, 48, dt=np.float32)
    runs = []
    for _ in range(2):
        gg, gc = torch.from_numpy(grad0).cuda(), torch.from_numpy(count0).cuda()
        ops.densify_accumulate(gg, gc, torch.from_numpy(d).cuda(), torch.from_numpy(radii).cuda(), 64, 48)
        runs.append((gg, gc))
    got = runs[0][0].cpu().numpy()
    e, e32 = rel(got, a64), rel(a32, a64)
    print(f"[densify accumulate U={U} C={Cn}] ||a - a64|| / ||a64|| = {e:.3e} (oracle fp32 {e32:.3e}); gate {gate(e32):.3e}")
    parity("densify::accumulate", U=U, C=Cn, rel_l2=e, oracle_fp32_rel_l2=e32, gate=gate(e32))
    assert np.array_equal(runs[0][1].cpu().numpy(), cnt) and (cnt > count0).any()
    culled = (radii <= 0).all(0)
    assert np.array_equal(got[culled].view(np.int32), grad0[culled].view(np.int32))     # never visible: the sum keeps its bits
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert e <= gate(e32), (e, e32)


# ------------------------------------------------------------------------------------------------------- classify and apply

def check_refine(parity, tag, U, K, seed=5, t=9, **kw):
    """classify + apply on scene(U, K) against the oracle -> the GPU's new tensors"""
    from vist3a_amd import ops
    grad, count, p, m, v = scene(U, K)
    revised = kw.get("revised", False)
    mg = DO.margin(grad, count, p["scales"], p["opacities"], revised=revised, **TH)
    assert mg >= 1e-6, mg                                                               # on the CPU, before anything runs
    want = DO.classify(grad, count, p["scales"], p["opacities"], **TH, **kw)
    cls = gpu_classify(grad, count, p, **kw)
    differing = sum(int((cls[k].cpu().numpy() != want[k]).sum()) for k in ("fates", "counts", "offsets", "totals"))
    fate = want["fates"] & 3
    print(f"[densify {tag} U={U} K={K}] margin {mg:.2e}; keep/clone/split {[int((fate == f).sum()) for f in range(3)]}, pruned "
          f"{int((want['fates'] & 4 > 0).sum())}, totals {want['totals'].tolist()}; entries that differ from the oracle: {differing}")
    assert same_cls(cls, want)
    P64, M, V, computed = DO.apply(want, p, m, v, seed, t, revised=revised)
    P32, _, _, _ = DO.apply(want, p, m, v, seed, t, revised=revised, dt=np.float32)
    new = ops.densify_apply(cls, to_gpu(p), to_gpu(m), to_gpu(v), seed=seed, step=t, revised_opacity=revised)
    gp, gm, gv = ({k: x.cpu().numpy() for k, x in d.items()} for d in new)
    U_out = int(want["totals"][0] + want["totals"][1] + 2 * want["totals"][2])
    assert all(gp[k].shape[0] == gm[k].shape[0] == gv[k].shape[0] == U_out for k in DO.NAMES)
    bits = lambda x: np.ascontiguousarray(x).view(np.int32)
    for k in DO.NAMES:                                  # moments: kept or zero, bit for bit
        assert np.array_equal(bits(gm[k]), bits(M[k])) and np.array_equal(bits(gv[k]), bits(V[k])), k
    for k in ("quats", "sh"):                           # copied everywhere
        assert np.array_equal(bits(gp[k]), bits(P64[k].astype(np.float32))), k
    for k in ("means", "scales", "opacities"):          # copied outside the children's rows
        assert np.array_equal(bits(gp[k][~computed]), bits(P64[k][~computed].astype(np.float32))), k
    figures = {}
    names = ("means", "scales") + (("opacities",) if revised else ())
    for k in names:
        figures[k], figures[k + "_f32"] = rel(gp[k][computed], P64[k][computed]), rel(P32[k][computed], P64[k][computed])
    if not revised:
        assert np.array_equal(bits(gp["opacities"]), bits(P64["opacities"].astype(np.float32)))
    print(f"[densify {tag} U={U} K={K}] rows {U} -> {U_out}, children {int(computed.sum())}: " +
          ", ".join(f"{k} {figures[k]:.3e} (oracle fp32 {figures[k + '_f32']:.3e})" for k in names))
    parity(f"densify::{tag}", U=U, K=K, U_out=U_out, differing=differing, margin=mg, gate=TOL, **figures)
    for k in names:
        assert figures[k] <= gate(figures[k + "_f32"]), (k, figures)
    return new, (p, m, v), want


@pytest.mark.parametrize("U,K", [(1, 1), (5, 4), (5, 25), (1027, 1), (1027, 4), (1027, 25), (70_001, 4)])
def test_refine_matches_oracle(hip_lib, parity, U, K):
    _, _, want = check_refine(parity, "refine", U, K, prune_big=True)
    if U >= 1027:
        fate, pruned = want["fates"] & 3, want["fates"] & 4 > 0
        assert all(((fate == f) & ~pruned).sum() > 20 and ((fate == f) & pruned).sum() > 5 for f in range(3))   # every fate, pruned and not
    if U == 5:
        assert want["fates"].tolist() == [0, 1, 2, 6, 4]


@pytest.mark.parametrize("U,K", [(5, 4), (1027, 25)])
def test_refine_before_the_first_reset_and_revised(hip_lib, parity, U, K):
    _, _, early = check_refine(parity, "refine_early", U, K, prune_big=False)
    _, _, rev = check_refine(parity, "refine_revised", U, K, prune_big=True, revised=True)
    if U == 5:
        assert early["fates"].tolist() == [0, 1, 2, 2, 0]
    else:
        grad, count, p, _, _ = scene(U, K)
        plain = DO.classify(grad, count, p["scales"], p["opacities"], prune_big=True, **TH)
        assert (rev["fates"] != plain["fates"]).sum() > 5 and (early["fates"] != plain["fates"]).sum() > 5


@pytest.mark.parametrize("U,K", [(5, 1), (1027, 25), (70_001, 1)])
def test_grow_off_prunes_only(hip_lib, parity, U, K):
    new, (p, m, v), want = check_refine(parity, "prune_only", U, K, prune_big=True, grow=False)
    assert (want["fates"] & 3 == 0).all() and want["totals"][1] == want["totals"][2] == 0
    alive = want["fates"] == 0
    assert 0 < alive.sum() < U or U == 5
    for d, src in zip(new, (p, m, v)):                  # what is left is the old rows, in order, with their moments
        for k in DO.NAMES:
            assert np.array_equal(d[k].cpu().numpy().view(np.int32), np.ascontiguousarray(src[k][alive]).view(np.int32))


def test_all_pruned_and_nothing_changes(hip_lib):
    from vist3a_amd import ops
    for U, K in ((5, 4), (1027, 25)):
        grad, count, p, m, v = scene(U, K)
        dead = dict(p, opacities=np.full(U, -9.0, np.float32))                          # sigmoid(-9) = 1.2e-4 < prune_opa
        cls = gpu_classify(grad, count, dead, prune_big=True)
        assert cls["totals"].tolist() == [0, 0, 0] and bool((cls["fates"] & 4 > 0).all())
        new = ops.densify_apply(cls, to_gpu(dead), to_gpu(m), to_gpu(v), seed=1, step=1)
        assert all(d[k].shape[0] == 0 and d[k].shape[1:] == torch.Size(p[k].shape[1:]) for d in new for k in DO.NAMES)
        # nothing to do: no gradient above the threshold, everything opaque and small -> the outputs equal the inputs
        calm = dict(p, opacities=np.full(U, 2.0, np.float32), scales=np.full((U, 3), -4.0, np.float32))
        cls = gpu_classify(np.zeros(U, np.float32), count, calm, prune_big=True)
        assert cls["totals"].tolist() == [U, 0, 0] and not bool(cls["fates"].any()) and cls["offsets"][0].tolist() == list(range(U))
        new = ops.densify_apply(cls, to_gpu(calm), to_gpu(m), to_gpu(v), seed=1, step=1)
        for d, src in zip(new, (calm, m, v)):
            for k in DO.NAMES:
                assert torch.equal(d[k].cpu(), torch.from_numpy(src[k])), k


def test_two_runs_are_bit_identical_and_seeded(hip_lib):
    from vist3a_amd import ops
    grad, count, p, m, v = scene(1027, 25)
    runs = []
    for seed, step in ((5, 9), (5, 9), (6, 9), (5, 10)):
        cls = gpu_classify(grad, count, p, prune_big=True)
        runs.append((cls, ops.densify_apply(cls, to_gpu(p), to_gpu(m), to_gpu(v), seed=seed, step=step)))
    assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in ("fates", "counts", "offsets", "totals"))
    assert all(torch.equal(runs[0][1][i][k], runs[1][1][i][k]) for i in range(3) for k in DO.NAMES)
    for other in (2, 3):                                # the seed and the step move the children's means and nothing else
        assert not torch.equal(runs[0][1][0]["means"], runs[other][1][0]["means"])
        assert all(torch.equal(runs[0][1][i][k], runs[other][1][i][k]) for i in range(3) for k in DO.NAMES if (i, k) != (0, "means"))


def test_wrappers_check_their_arguments(hip_lib):
    from vist3a_amd import ops
    grad, count, p, m, v = scene(5, 4)
    cls = gpu_classify(grad, count, p)
    gp, gm, gv = to_gpu(p), to_gpu(m), to_gpu(v)
    with pytest.raises(ValueError):
        ops.densify_apply(cls, {**gp, "sh": gp["sh"][:, :, :3].contiguous()}, gm, gv, seed=1, step=1)
    with pytest.raises(ValueError):
        ops.densify_apply(cls, gp, gm, gv, seed=-1, step=1)
    with pytest.raises(ValueError):
        ops.densify_apply(cls, gp, gm, gv, seed=1, step=1, totals=(11, 0, 0))
    with pytest.raises(ValueError):
        ops.densify_classify(torch.from_numpy(grad).cuda(), torch.from_numpy(count).cuda().long(), gp["scales"], gp["opacities"], **TH)
    with pytest.raises(ValueError):
        ops.densify_accumulate(torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda", dtype=torch.int32), torch.zeros(1, 4, 2, device="cuda"),
                               torch.zeros(1, 5, device="cuda", dtype=torch.int32), 8, 8)
    with pytest.raises(ValueError):
        ops.densify_reset_opacity(gp["opacities"], gm["opacities"], gv["opacities"], 1.0)


# ------------------------------------------------------------------------------------------------------------------- reset

@pytest.mark.parametrize("U", SIZES)
def test_reset_opacity(hip_lib, parity, U):
    from vist3a_amd import ops
    g = np.random.default_rng(U)
    lg = (g.normal(size=U) * 3.0).astype(np.float32)
    if U == 1:
        lg[0] = 1.0
    a64, a32 = DO.reset_opacity(lg, 0.01), DO.reset_opacity(lg, 0.01, dt=np.float32)
    t, m, v = torch.from_numpy(lg).cuda(), torch.ones(U, device="cuda"), torch.ones(U, device="cuda")
    ops.densify_reset_opacity(t, m, v, 0.01)
    got = t.cpu().numpy()
    low = lg.astype(np.float64) <= a64
    e, e32 = rel(got, a64), rel(a32, a64)
    print(f"[densify reset U={U}] capped {int((~low).sum())} of {U}: ||a - a64|| / ||a64|| = {e:.3e} (oracle fp32 {e32:.3e})")
    parity("densify::reset", U=U, rel_l2=e, oracle_fp32_rel_l2=e32, gate=gate(e32))
    assert np.array_equal(got[low].view(np.int32), lg[low].view(np.int32))              # below the cap: untouched bits
    assert (~low).any() and (got[~low] == got[~low][0]).all()
    assert not bool(m.any()) and not bool(v.any())
    assert e <= gate(e32), (e, e32)
