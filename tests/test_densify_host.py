"""Host tests of the densification strategy (cfg.strategy = "densify"): the numpy oracle (tests/densify_oracle.py) on a hand-built
case whose fates, prune reasons and row order are written out here; its random numbers against tests/mcmc_oracle.py and the library's
host Philox; the schedule helpers against gsplat's three conditions; config validation; the command line; the C ABI's refusals and
its workspace query.  No GPU."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import densify_oracle as DO  # noqa: E402
import mcmc_oracle as MO  # noqa: E402

TH = dict(grow_grad2d=2e-4, grow_scale3d=0.01, prune_opa=0.005, prune_scale3d=0.1)

# (grad2d, count, largest scale, opacity): what each of the 12 is there for
CASE = [
    (1e-4, 1, 0.005, 0.5),     # 0  keep
    (1e-4, 1, 0.005, 0.001),   # 1  keep, pruned: transparent
    (1e-4, 1, 0.2, 0.5),       # 2  keep, pruned once i > reset_every: oversized
    (4e-4, 1, 0.005, 0.5),     # 3  clone
    (4e-4, 1, 0.005, 0.002),   # 4  clone, pruned with its clone: transparent
    (4e-4, 1, 0.05, 0.5),      # 5  split
    (4e-4, 1, 0.05, 0.001),    # 6  split, both children pruned: transparent
    (4e-4, 1, 0.2, 0.5),       # 7  split; children of 0.125 pruned once i > reset_every
    (4e-4, 1, 0.15, 0.5),      # 8  split; the parent is oversized, the children (0.09375) are not: they stay
    (0.0, 0, 0.005, 0.5),      # 9  never visible: count 0 divides by 1, keep
    (1e-3, 10, 0.005, 0.5),    # 10 a large sum over ten views is a small average: keep
    (4e-4, 1, 0.05, 0.008),    # 11 split; children of 1 - sqrt(0.992) = 0.004008 pruned with revised opacities only
]


def case(K=4, seed=0):
    g = np.random.default_rng(seed)
    U = len(CASE)
    f = lambda *s: g.normal(size=s).astype(np.float32)
    grad = np.array([c[0] for c in CASE], np.float32)
    count = np.array([c[1] for c in CASE], np.int32)
    ls = np.log(np.array([[c[2], c[2] * 0.5, c[2] * 0.25] for c in CASE])).astype(np.float32)
    ls = np.stack([np.roll(r, i % 3) for i, r in enumerate(ls)])                       # the largest scale sits on any axis
    op = np.array([c[3] for c in CASE])
    p = dict(means=f(U, 3), scales=ls, quats=f(U, 4), opacities=np.log(op / (1 - op)).astype(np.float32), sh=f(U, 3, K))
    m = {k: f(*x.shape) * 1e-3 for k, x in p.items()}
    v = {k: np.abs(f(*x.shape)) * 1e-6 for k, x in p.items()}
    return grad, count, p, m, v


def parents_of(cls):
    fate, alive = cls["fates"] & 3, (cls["fates"] & 4) == 0
    A = [g for g in range(len(fate)) if alive[g] and fate[g] != 2]
    B = [g for g in range(len(fate)) if alive[g] and fate[g] == 1]
    S = [g for g in range(len(fate)) if alive[g] and fate[g] == 2]
    return A, B, S


@pytest.mark.parametrize("prune_big,revised,fates,A,B,S", [
    (False, False, [0, 4, 0, 1, 5, 2, 6, 2, 2, 0, 0, 2], [0, 2, 3, 9, 10], [3], [5, 7, 8, 11]),
    (True, False, [0, 4, 4, 1, 5, 2, 6, 6, 2, 0, 0, 2], [0, 3, 9, 10], [3], [5, 8, 11]),
    (True, True, [0, 4, 4, 1, 5, 2, 6, 6, 2, 0, 0, 6], [0, 3, 9, 10], [3], [5, 8]),
])
def test_oracle_fates_and_order(prune_big, revised, fates, A, B, S):
    grad, count, p, m, v = case()
    assert DO.margin(grad, count, p["scales"], p["opacities"], revised=revised, **TH) > 1e-3
    cls = DO.classify(grad, count, p["scales"], p["opacities"], prune_big=prune_big, revised=revised, **TH)
    assert cls["fates"].tolist() == fates
    assert parents_of(cls) == (A, B, S)
    assert cls["totals"].tolist() == [len(A), len(B), len(S)] and cls["counts"].sum(1).tolist() == [len(A), len(B), len(S)]
    for s, rows in enumerate((A, B, S)):
        assert [int(cls["offsets"][s][g]) for g in rows] == list(range(len(rows)))
    P, M, V, computed = DO.apply(cls, p, m, v, seed=3, t=7, revised=revised)
    order = A + B + S + S
    assert P["means"].shape[0] == len(order) and computed.tolist() == [False] * (len(A) + len(B)) + [True] * (2 * len(S))
    for k in DO.NAMES:                                   # segment A: rows and moments bit for bit; B: rows copied, moments zero
        assert np.array_equal(P[k][:len(A)].astype(np.float32), p[k][A]) and np.array_equal(M[k][:len(A)], m[k][A]) and np.array_equal(V[k][:len(A)], v[k][A])
        assert np.array_equal(P[k][len(A):len(A) + len(B)].astype(np.float32), p[k][B])
        assert not M[k][len(A):].any() and not V[k][len(A):].any()
    for k in ("quats", "sh"):                            # children keep the parent's quats and sh
        assert np.array_equal(P[k][len(A) + len(B):].astype(np.float32), p[k][S + S])
    # every fate and every prune reason occurs in the three cases together
    if prune_big and revised:
        assert set(fates) == {0, 1, 2, 4, 5, 6}


def test_oracle_cap_pass_and_empty():
    grad, count, p, m, v = case()
    cls = DO.classify(grad, count, p["scales"], p["opacities"], grow=False, prune_big=True, **TH)
    assert cls["fates"].tolist() == [0, 4, 4, 0, 4, 0, 4, 4, 4, 0, 0, 0] and cls["totals"].tolist() == [6, 0, 0]   # prune only: 7, 8 judged as parents
    none = DO.classify(grad, count, p["scales"], p["opacities"], **{**TH, "prune_opa": 0.9})
    assert none["totals"].tolist() == [0, 0, 0]
    P, M, V, computed = DO.apply(none, p, m, v, seed=1, t=1)
    assert P["means"].shape == (0, 3) and M["sh"].shape == (0, 3, 4) and computed.shape == (0,)


@pytest.mark.parametrize("revised", [False, True])
def test_oracle_split_children(revised):
    grad, count, p, m, v = case()
    cls = DO.classify(grad, count, p["scales"], p["opacities"], revised=revised, **TH)
    A, B, S = parents_of(cls)
    P, _, _, _ = DO.apply(cls, p, m, v, seed=3, t=7, revised=revised)
    base = len(A) + len(B)
    for child in (0, 1):
        for j, g in enumerate(S):
            r = base + child * len(S) + j
            ls = p["scales"][g].astype(np.float64)
            assert np.allclose(np.exp(P["scales"][r]), np.exp(ls) / 1.6, rtol=1e-14, atol=0)
            o = 1 / (1 + math.exp(-float(p["opacities"][g])))
            want = 1 - math.sqrt(1 - o) if revised else o
            assert abs(1 / (1 + math.exp(-P["opacities"][r])) - want) <= 1e-14
            if not revised:
                assert P["opacities"][r] == float(p["opacities"][g])                   # the parent's logit itself
            # means: the offset, taken back through R^T and the scales, is the child's three normals
            R = DO.quat_R(p["quats"][g])
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-7) and abs(np.linalg.det(R) - 1) < 1e-7
            z = (R.T @ (P["means"][r] - p["means"][g].astype(np.float64))) / np.exp(ls)
            s = 4 + 2 * child
            z0, z1 = MO.normals(MO.draw(3, g, s, 7))
            z2, _ = MO.normals(MO.draw(3, g, s + 1, 7))
            assert np.allclose(z, [z0, z1, z2], rtol=0, atol=1e-6)
    first, second = P["means"][base:base + len(S)], P["means"][base + len(S):]
    assert not np.allclose(first, second)                                             # the two children are different draws


def test_oracle_random_numbers():
    from vist3a_amd import lib, ops
    assert {k: ops.MCMC_STREAMS[k] for k in ("relocate", "grow")} == dict(relocate=0, grow=1)          # not renumbered
    assert (ops.MCMC_STREAMS["split0"], ops.MCMC_STREAMS["split1"]) == (DO.STREAMS["split0"], DO.STREAMS["split1"]) == (4, 6)
    assert (MO.STREAM_NOISE_A, MO.STREAM_NOISE_B) == (2, 3)
    L = lib.load()
    for seed, g, t in ((0, 0, 1), (3, 11, 7), (2 ** 40 + 5, 70_000, 15_000)):
        for child in (0, 1):
            s = DO.STREAMS[f"split{child}"]
            z = DO.child_draws(seed, g, t, child)
            z0, z1 = MO.normals(MO.draw(seed, g, s, t))
            z2, _ = MO.normals(MO.draw(seed, g, s + 1, t))
            assert z.tolist() == [z0, z1, z2]
            for stream in (s, s + 1):                                                   # the counter and key assignment, in the library
                ctr, key, out = (C.c_uint32 * 4)(g, 0, stream, t), (C.c_uint32 * 2)(*MO.key_of(seed)), (C.c_uint32 * 4)()
                assert L.v3a_mcmc_philox(ctr, key, out) == 0 and list(out) == list(MO.draw(seed, g, stream, t))
    assert not np.array_equal(DO.child_draws(1, 5, 2, 0), DO.child_draws(1, 5, 2, 1))


def test_oracle_accumulate_and_reset():
    g = np.random.default_rng(0)
    d = g.normal(size=(3, 7, 2)).astype(np.float32) * 1e-4
    radii = g.integers(0, 3, (3, 7)).astype(np.int32)
    radii[:, 0] = 0
    grad, count = DO.accumulate(np.ones(7, np.float32), np.full(7, 2, np.int32), d, radii, 64, 48)
    assert grad[0] == 1.0 and count[0] == 2
    want = 1.0 + sum(math.hypot(float(d[c, 3, 0]) * 32 * 3, float(d[c, 3, 1]) * 24 * 3) for c in range(3) if radii[c, 3] > 0)
    assert abs(grad[3] - want) < 1e-15 and count[3] == 2 + int((radii[:, 3] > 0).sum())
    lg = np.array([-9.0, -4.0, 0.0, 5.0], np.float32)
    cap = math.log(0.01 / 0.99)
    assert DO.reset_opacity(lg, 0.01).tolist() == [-9.0, cap, cap, cap]


def test_schedule_helpers():
    from vist3a_amd.post_opt import PostOptConfig, densify_active_at, densify_refines_at, densify_resets_at
    start, stop, every, reset, pause = 50, 600, 25, 200, 30
    cfg = PostOptConfig(strategy="densify", densify_refine_start_iter=start, densify_refine_stop_iter=stop, densify_refine_every=every,
                        densify_reset_every=reset, densify_pause_refine_after_reset=pause)
    cfg.check_strategy()
    n_refines = n_resets = 0
    for i in range(0, 701):
        # gsplat's DefaultStrategy.step_post_backward, spelled out
        active = not i >= stop
        refines = active and (i > start and i % every == 0 and i % reset >= pause)
        resets = active and i % reset == 0 and i > 0
        assert (densify_active_at(cfg, i), densify_refines_at(cfg, i), densify_resets_at(cfg, i)) == (active, refines, resets), i
        assert DO.schedule(i, start, stop, every, reset, pause) == (active, refines, resets)
        n_refines += refines
        n_resets += resets
    assert n_resets == 2 and [i for i in range(701) if densify_resets_at(cfg, i)] == [200, 400]
    assert not densify_refines_at(cfg, 200) and not densify_refines_at(cfg, 225) and densify_refines_at(cfg, 250)   # the pause after a reset
    assert not densify_refines_at(cfg, 50) and densify_refines_at(cfg, 75) and densify_refines_at(cfg, 575) and not densify_refines_at(cfg, 600)
    assert n_refines == len([i for i in range(75, 600, 25) if i % 200 >= 30])
    assert not densify_resets_at(cfg, 0) and densify_active_at(cfg, 0)                  # the reset at i = 0 does not fire
    d = PostOptConfig()
    assert [i for i in range(16_000) if densify_refines_at(d, i)] == list(range(600, 15_000, 100))
    assert [i for i in range(16_000) if densify_resets_at(d, i)] == [3000, 6000, 9000, 12_000]


def test_config_validation():
    from vist3a_amd.post_opt import PostOptConfig
    d = PostOptConfig()
    assert (d.strategy, d.densify_prune_opa, d.densify_grow_grad2d, d.densify_grow_scale3d, d.densify_prune_scale3d,
            d.densify_refine_start_iter, d.densify_refine_stop_iter, d.densify_reset_every, d.densify_refine_every,
            d.densify_pause_refine_after_reset, d.densify_absgrad, d.densify_revised_opacity, d.densify_cap_max) == (
        "none", 0.005, 2e-4, 0.01, 0.1, 500, 15_000, 3000, 100, 0, False, False, 0)
    PostOptConfig(strategy="densify").check_strategy()
    PostOptConfig(strategy="none", densify_refine_every=0).check_strategy()             # not looked at while it is off
    PostOptConfig(strategy="mcmc", densify_refine_every=0).check_strategy()
    for kw in (dict(densify_refine_every=0), dict(densify_reset_every=0), dict(densify_refine_start_iter=-1), dict(densify_refine_stop_iter=1.5),
               dict(densify_pause_refine_after_reset=-1), dict(densify_cap_max=-1), dict(densify_cap_max=True), dict(densify_prune_opa=0.0),
               dict(densify_prune_opa=0.5), dict(densify_grow_grad2d=0.0), dict(densify_grow_scale3d=-1.0), dict(densify_prune_scale3d=0.0),
               dict(scene_scale=0.0), dict(densify_absgrad=1), dict(densify_revised_opacity="yes"), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            PostOptConfig(strategy="densify", **kw).check_strategy()
    for name in ("Densify", "default"):                                                 # "default" stays refused, as before the strategy existed
        with pytest.raises(ValueError, match="strategy"):
            PostOptConfig(strategy=name).check_strategy()


def test_cli_options():
    import inference_t23d as I
    from vist3a_amd.utils.argument import inference_vist3a_argument
    req = ["--checkpoint_path", "c", "--transformer_lora_path", "l", "--input_texts_path", "t"]
    parse = lambda *x: inference_vist3a_argument().parse_args(req + list(x))
    ns = parse()
    assert (ns.post_opt_densify, ns.post_opt_densify_refine, ns.post_opt_densify_grad, ns.post_opt_densify_absgrad,
            ns.post_opt_densify_cap_max) == (False, "500,15000,100,3000", 2e-4, False, 0)
    assert I.densify_options(ns) is None
    assert I.densify_options(parse("--post_opt_densify", "--post_opt_steps", "3")) == dict(
        densify_refine_start_iter=500, densify_refine_stop_iter=15_000, densify_refine_every=100, densify_reset_every=3000,
        densify_grow_grad2d=2e-4, densify_absgrad=False, densify_cap_max=0)
    got = I.densify_options(parse("--post_opt_densify", "--post_opt_steps", "3", "--post_opt_densify_refine", "1,100,3,6", "--post_opt_densify_grad",
                                  "8e-4", "--post_opt_densify_absgrad", "--post_opt_densify_cap_max", "400"))
    assert got == dict(densify_refine_start_iter=1, densify_refine_stop_iter=100, densify_refine_every=3, densify_reset_every=6,
                       densify_grow_grad2d=8e-4, densify_absgrad=True, densify_cap_max=400)
    on = ("--post_opt_densify", "--post_opt_steps", "3")
    for bad in (("--post_opt_densify",), on + ("--post_opt_mcmc",), on + ("--post_opt_densify_refine", "1,100,3"),
                on + ("--post_opt_densify_refine", "1,100,0,6"), on + ("--post_opt_densify_refine", "1,100,3,0"),
                on + ("--post_opt_densify_refine", "1,100,x,6"), on + ("--post_opt_densify_refine=-1,100,3,6",),
                on + ("--post_opt_densify_grad", "0"), on + ("--post_opt_densify_cap_max", "-1")):
        with pytest.raises(ValueError):
            I.densify_options(parse(*bad))
    assert I.mcmc_options(parse("--post_opt_mcmc", "--post_opt_steps", "3")) is not None    # the other strategy alone still parses


def test_c_abi_and_queries():
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_abi_version() == lib.EXPECTED_ABI >= 33
    assert [f for f, _ in lib.GsRasterizeBackwardArgs._fields_][-1] == "d_means2d_abs"
    q = L.v3a_densify_classify_workspace_bytes
    assert q(-1) == -2 and q(1 << 31) == -2 and q(0) == 0
    assert q(1) == q(256) == 16 and q(257) == 24 and q(70_001) == ((3 * 274 * 4 + 7) // 8) * 8 and q((1 << 31) - 1) == 3 * (1 << 23) * 4
    acc = lambda d=8, r=8, U=4, Cn=1, w=8, h=8, g=8, c=8: L.v3a_densify_accumulate(d, r, U, Cn, w, h, g, c, None)
    assert acc(d=None) == acc(r=None) == acc(g=None) == acc(c=None) == -1
    assert acc(U=-1) == acc(U=1 << 31) == acc(Cn=0) == acc(w=0) == acc(h=0) == -2 and acc(U=0) == 0
    assert L.v3a_densify_classify(None, None) == -1
    a = lib.DensifyClassifyArgs()
    for name in ("grad2d", "count", "log_scales", "logits", "fates", "counts", "offsets", "totals", "workspace"):
        setattr(a, name, 8)
    a.U, a.workspace_bytes = 300, 24
    bad = lambda **kw: [setattr(a, k, x) for k, x in kw.items()] and L.v3a_densify_classify(C.byref(a), None)
    assert bad(U=-1) == -2 and bad(U=1 << 31) == -2 and bad(U=0) == 0
    assert bad(U=300, workspace_bytes=23) == -4 and bad(workspace_bytes=24, workspace=4) == -4 and bad(workspace=None) == -4
    assert bad(workspace=8, totals=None) == -1
    assert L.v3a_densify_apply(None, None) == -1
    b = lib.DensifyApplyArgs()
    fields = [f for f, _ in lib.DensifyApplyArgs._fields_]
    assert len(fields) == 39 and fields[:5] == ["means", "log_scales", "quats", "logits", "sh"] and fields[15] == "new_means"
    for i, name in enumerate(fields[:30]):
        setattr(b, name, (i + 1) << 20)                                                  # 1 MiB apart: no two tensors overlap
    b.fates = b.offsets = b.totals = 8
    b.U, b.U_out, b.K = 100, 150, 4
    bad = lambda **kw: [setattr(b, k, x) for k, x in kw.items()] and L.v3a_densify_apply(C.byref(b), None)
    assert bad(U=-1) == -2 and bad(U=100, U_out=201) == -2 and bad(U_out=150, K=0) == -2 and bad(K=4, U_out=1 << 31) == -2
    assert bad(U_out=0) == 0 and bad(U_out=150, U=0) == -2                              # nothing to write; 150 rows cannot come from 0
    assert bad(U=100, new_sh=b.sh) == -2                                                 # old and new alias
    assert bad(new_sh=b.sh + 4 * 1199) == -2 and bad(new_sh=b.new_m_sh - 4 * 1799) == -2   # by one float, an old and a new one
    assert bad(new_sh=20 << 20, new_v_logits=None) == -1 and bad(new_v_logits=30 << 20, fates=None) == -1
    r = lambda lg=8, m=8, v=8, U=4, o=0.01: L.v3a_densify_reset_opacity(lg, m, v, U, o, None)
    assert r(lg=None) == r(m=None) == r(v=None) == -1
    assert r(o=0.0) == r(o=1.0) == r(o=float("nan")) == r(U=-1) == r(U=1 << 31) == -2 and r(U=0) == 0
