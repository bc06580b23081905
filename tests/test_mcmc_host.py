"""CPU tests of the MCMC strategy's host side: the oracle of tests/mcmc_oracle.py against known answers and against itself, the
library's host entry points for the generator (the device code's own source, compiled for the host), argument validation of the
C ABI, PostOptConfig's validation, the refine-step predicate and the growth arithmetic."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mcmc_oracle as MO  # noqa: E402

KNOWN = [   # counter, key, output (Random123's known-answer vectors for philox4x32-10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert tuple(MO.philox(counter, key)) == want
    assert tuple(int(x) for x in MO.philox_np(*counter, *key)) == want
    from vist3a_amd import lib
    L = lib.load()
    c, k, out = (C.c_uint32 * 4)(*counter), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    assert L.v3a_mcmc_philox(c, k, out) == 0
    assert tuple(out) == want                                         # the library's generator, compiled for the host


def test_philox_addressing_and_vectorised_form():
    seed = 0x123456789abcdef0
    assert MO.key_of(seed) == (0x9abcdef0, 0x12345678)                # low word first
    slots = np.array([0, 1, 77, 70_000, 2 ** 31 - 1])
    w = MO.draw_np(seed, slots, 3, 41)
    for n, s in enumerate(slots.tolist()):
        assert [int(x[n]) for x in w] == MO.draw(seed, s, 3, 41) == MO.philox((s, 0, 3, 41), (0x9abcdef0, 0x12345678))
    assert MO.draw(seed, 5, 0, 41) != MO.draw(seed, 5, 1, 41) != MO.draw(seed, 5, 1, 42)


def test_uniforms_lie_in_the_half_open_interval():
    from vist3a_amd import lib
    L = lib.load()
    top = MO.uniform(0xffffffff, 0xffffffff)
    assert top == 1.0 - 2.0 ** -53 < 1.0 and MO.uniform(0, 0) == 0.0
    assert MO.uniform(1 << 5, 0) == 2.0 ** -27 and MO.uniform(0, 1 << 6) == 2.0 ** -53 and MO.uniform(31, 63) == 0.0
    g = np.random.default_rng(3)
    x = g.integers(0, 2 ** 32, size=(2, 4096), dtype=np.uint64)
    u = MO.uniform_np(x[0], x[1])
    assert u.min() >= 0.0 and u.max() < 1.0
    for a, b, want in [(0xffffffff, 0xffffffff, top), (0, 0, 0.0)] + [(int(x[0, i]), int(x[1, i]), float(u[i])) for i in range(64)]:
        assert MO.uniform(a, b) == want == L.v3a_mcmc_uniform(a, b)
    z = MO.normals((0xffffffff,) * 4)                                  # u1 at its largest: the radius is finite
    assert all(math.isfinite(v) for v in z) and abs(math.hypot(*z) - math.sqrt(2 * 53 * math.log(2))) < 1e-12


def test_normals_have_unit_moments():
    z0, z1 = MO.normals_np(MO.draw_np(11, np.arange(200_000), 2, 7))
    for z in (z0, z1):
        assert abs(z.mean()) < 5 / math.sqrt(200_000) and abs(z.var() - 1) < 5 * math.sqrt(2 / 200_000)
    assert abs(float((z0 * z1).mean())) < 5 / math.sqrt(200_000)
    assert (MO.normals(MO.draw(11, 5, 2, 7))[0], MO.normals(MO.draw(11, 5, 2, 7))[1]) == pytest.approx((z0[5], z1[5]), rel=1e-14)


def test_sampler_frequencies_follow_the_weights():
    w = np.array([0.05, 0.9, 0.0, 0.3, 0.6], dtype=np.float32)
    n = 200_000
    src, counts = MO.sample(w, 0.0, False, n, seed=5, stream=1, step=9)
    assert counts.sum() == n and (src >= 0).all() and np.array_equal(np.bincount(src, minlength=5), counts)
    assert counts[2] == 0                                              # a zero weight is never drawn
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    sigma = np.sqrt(n * p * (1 - p))
    assert (np.abs(counts - n * p) <= 5 * sigma).all(), (counts, n * p, sigma)


def test_sampler_relocation_mode():
    g = np.random.default_rng(8)
    w = g.uniform(0.0, 1.0, 3000).astype(np.float32)
    dead = g.random(3000) < 0.3
    w[dead] = g.uniform(0.0, 0.005, int(dead.sum())).astype(np.float32)
    w[17] = np.float32(0.005)                                          # at the threshold: dead
    src, counts = MO.sample(w, 0.005, True, 3000, seed=1, stream=0, step=3)
    is_dead = w <= np.float32(0.005)
    assert is_dead[17] and (src[~is_dead] == -1).all() and (src[is_dead] >= 0).all()
    assert not is_dead[src[is_dead]].any()                             # only live Gaussians are drawn
    assert counts.sum() == is_dead.sum() and (counts[is_dead] == 0).all()
    slow = MO.sample(w, 0.005, True, 3000, seed=1, stream=0, step=3, slow=True)
    assert np.array_equal(src, slow[0]) and np.array_equal(counts, slow[1])      # the vectorised search is the written-out rule
    other = MO.sample(w, 0.005, True, 3000, seed=2, stream=0, step=3)[0]
    assert not np.array_equal(src, other)


def test_sampler_zero_blocks_and_the_fallback():
    # every block but the first is all zero: P_b <= t holds for the empty blocks too, and none of their entries may be picked
    w = np.zeros(5000, dtype=np.float32)
    w[3:1000:7] = 0.25
    for slow in (False, True):
        src, counts = MO.sample(w, 0.0, False, 4000, seed=4, stream=1, step=1, slow=slow)
        assert (w[src] > 0).all() and src.max() < 1000 and counts.sum() == 4000
    # a zero block in the middle and one at the end
    w = np.full(1024 * 4 + 5, 0.5, dtype=np.float32)
    w[1024:2048] = 0.0
    w[3072:] = 0.0
    a, b = MO.sample(w, 0.0, False, 3000, 9, 1, 2), MO.sample(w, 0.0, False, 3000, 9, 1, 2, slow=True)
    assert np.array_equal(a[0], b[0]) and (w[a[0]] > 0).all() and {int(x) // 1024 for x in a[0]} == {0, 2}
    # t at or past the running sum of the whole block (u total rounded up to total): the block's last weighted entry
    pool = np.array([0.25, 0.0, 0.5, 0.0])
    T, (P, total) = MO.block_totals(pool), MO.prefix(MO.block_totals(pool))
    assert total == 0.75 and MO.pick(pool, T, P, 0.75) == 2 and MO.pick(pool, T, P, 0.2) == 0 and MO.pick(pool, T, P, 0.25) == 2


def test_sampler_degenerate_cases_are_no_ops():
    w = np.zeros(1500, dtype=np.float32)
    src, counts = MO.sample(w, 0.005, True, 1500, 1, 0, 1)             # nothing alive
    assert (src == -1).all() and (counts == 0).all()
    src, counts = MO.sample(w, 0.0, False, 40, 1, 1, 1)                # growth from an all-zero pool
    assert (src == -1).all() and (counts == 0).all()
    w[:] = 0.5
    src, counts = MO.sample(w, 0.005, True, 1500, 1, 0, 1)             # nothing dead: no active slot
    assert (src == -1).all() and (counts == 0).all()


def test_block_tree_order_is_visible():
    """The emulated tree must differ from a sum in index order in the bits, or the GPU test could pass with any order.  f32 values
    of similar size add exactly in fp64 (24-bit significands), so the weights span 14 decades: wide_weights of test_mcmc_gpu.py."""
    g = np.random.default_rng(2)
    pool = (g.random(5000) * 10 ** (-14 * g.random(5000))).astype(np.float32).astype(np.float64)
    T = MO.block_totals(pool)
    blocks = [pool[b * 1024:(b + 1) * 1024] for b in range(len(T))]
    exact = np.array([math.fsum(x) for x in blocks])
    in_index_order = np.array([np.cumsum(x)[-1] for x in blocks])
    assert np.allclose(T, exact, rtol=1e-13, atol=0) and (T != in_index_order).any()


@pytest.mark.parametrize("op", [0.006, 0.5, 0.99, 1 - 1e-6])
def test_relocation_oracle(op):
    o2, sc, o1 = MO.relocation(op, 0.37, 0, min_opacity=1e-9)         # r = 1: the Gaussian as it is
    # 1 - (1 - op) rounds twice near 1: an absolute 2^-52 at the most, which op / o' carries into the scale
    assert abs(o1 - op) <= 2.0 ** -52 and abs(sc - 0.37) <= 0.37 * (2.0 ** -52 / op + 4e-16) and o2 == min(o1, 1 - 2.0 ** -23)
    _, sc, o1 = MO.relocation(op, 0.37, 1, min_opacity=1e-9)          # r = 2: den = 2 o' - o'^2 / sqrt 2
    want = op / (2 * o1 - o1 * o1 / math.sqrt(2)) * 0.37
    assert abs(o1 - (1 - math.sqrt(1 - op))) <= 1e-15 and abs(sc - want) <= 1e-14 * want
    for count in (6, 50, 51, 400):                                     # the ratio is clamped at 51; the copies stay dimmer and smaller
        o2, sc, o1 = MO.relocation(op, 0.37, count)
        assert 0 < o1 < op and o2 >= 0.005 and 0 < sc and math.isfinite(sc)
    assert MO.relocation(op, 0.37, 50) == MO.relocation(op, 0.37, 51) == MO.relocation(op, 0.37, 400)
    assert MO.relocation(0.001, 1.0, 3)[0] == 0.005                    # the floor


def test_relocate_oracle_moves_rows_as_specified():
    g = np.random.default_rng(6)
    U, K = 6, 2
    mk = lambda rows: dict(means=g.normal(size=(rows, 3)), scales=g.normal(size=(rows, 3)) - 2, quats=g.normal(size=(rows, 4)),
                           opacities=g.normal(size=rows), sh=g.normal(size=(rows, 3, K)))
    f32 = lambda d: {k: x.astype(np.float32) for k, x in d.items()}
    p, m, v = f32(mk(U)), f32(mk(U)), f32(mk(U))
    src, counts = np.array([-1, 4, -1, -1, -1, 4], dtype=np.int32), np.array([0, 0, 0, 0, 2, 0], dtype=np.int32)
    p2, m2, v2, exact = MO.relocate(src, counts, p, m, v, 0, 0.005)
    for d in (1, 5):
        assert all(np.array_equal(p2[k][d], p[k][4]) for k in ("means", "quats", "sh"))
        assert p2["opacities"][d] == p2["opacities"][4] and np.array_equal(p2["scales"][d], p2["scales"][4])
        assert all(np.array_equal(m2[k][d], m[k][d]) and np.array_equal(v2[k][d], v[k][d]) for k in MO.NAMES)      # dead rows keep their moments
    assert all(not m2[k][4].any() and not v2[k][4].any() for k in MO.NAMES)
    for r in (0, 2, 3):
        assert all(np.array_equal(p2[k][r], p[k][r]) and np.array_equal(m2[k][r], m[k][r]) for k in MO.NAMES)
    assert np.isnan(exact["opacities"][[0, 2, 3]]).all() and np.isfinite(exact["opacities"][[1, 4, 5]]).all()
    # growth: two new rows from row 2
    grow = lambda d: {k: np.concatenate([x, np.zeros((2,) + x.shape[1:], np.float32)]) for k, x in d.items()}
    src, counts = np.array([2, 2], dtype=np.int32), np.array([0, 0, 2, 0, 0, 0], dtype=np.int32)
    p3, m3, v3, _ = MO.relocate(src, counts, grow(p), grow(m), grow(v), U, 0.005)
    for d in (6, 7):
        assert all(np.array_equal(p3[k][d], p[k][2]) for k in ("means", "quats", "sh")) and p3["opacities"][d] == p3["opacities"][2]
        assert all(not m3[k][d].any() and not v3[k][d].any() for k in MO.NAMES)
    assert all(np.array_equal(m3[k][2], m[k][2]) for k in MO.NAMES) and p3["opacities"][2] != p["opacities"][2]


def test_noise_oracle_gate_and_shape():
    g = np.random.default_rng(12)
    U = 50
    means, ls = g.normal(size=(U, 3)).astype(np.float32), (g.normal(size=(U, 3)) - 2).astype(np.float32)
    quats = g.normal(size=(U, 4)).astype(np.float32)
    R = MO.rotation(quats)
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-7)             # (|q| + 1e-8 in the normalisation: not exactly 1)
    dead = np.full(U, -12.0, dtype=np.float32)
    assert np.all(MO.noise_gate(dead) > 0.37) and np.all(MO.noise_gate(np.zeros(U, np.float32)) <= math.exp(-49))
    out = MO.noise(np.zeros_like(means), ls, quats, dead, 2.0, 3, 4)
    cov = R @ (np.exp(2 * ls.astype(np.float64))[:, :, None] * R.transpose(0, 2, 1))
    want = np.einsum("uab,ub->ua", cov, MO.noise_draws(U, 3, 4) * (MO.noise_gate(dead) * 2.0)[:, None])
    assert np.allclose(out, want, rtol=1e-12, atol=1e-300)
    assert not np.array_equal(out, MO.noise(np.zeros_like(means), ls, quats, dead, 2.0, 3, 5))
    live = MO.noise(means, ls, quats, np.zeros(U, np.float32), 80.0, 3, 4)       # opacity 0.5: the gate shuts
    assert np.array_equal(live.astype(np.float32), means)


def test_c_abi_rejects_bad_arguments():
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_abi_version() == lib.EXPECTED_ABI >= 31
    assert L.v3a_mcmc_philox(None, None, None) == -1
    assert L.v3a_mcmc_sample_workspace_bytes(0) == -2 and L.v3a_mcmc_sample_workspace_bytes(1 << 31) == -2
    assert L.v3a_mcmc_sample_workspace_bytes(1) == L.v3a_mcmc_sample_workspace_bytes(1024) == 24
    assert L.v3a_mcmc_sample_workspace_bytes(1025) == 40 and L.v3a_mcmc_sample_workspace_bytes(70_001) == (2 * 69 + 1) * 8
    assert L.v3a_mcmc_relocate_workspace_bytes(0) == -2 and L.v3a_mcmc_relocate_workspace_bytes(1027) == 16 * 1027
    sample = lambda w=8, U=4, alive=1, n=4, src=8, counts=8, ws=8, nbytes=1024: L.v3a_mcmc_sample(w, U, 0.005, alive, n, 1, 0, 1, src, counts, ws, nbytes, None)
    assert sample(w=None) == sample(src=None) == sample(counts=None) == -1
    assert sample(U=0) == sample(n=0) == sample(n=5) == -2              # relocation draws for the U rows themselves
    assert sample(ws=None) == sample(ws=4) == sample(nbytes=16) == -4
    assert L.v3a_mcmc_noise(None, 8, 8, 8, 4, 1.0, 1, 1, None) == -1 and L.v3a_mcmc_noise(8, 8, 8, 8, 0, 1.0, 1, 1, None) == -2
    assert L.v3a_mcmc_relocate(None, None) == -1
    a = lib.McmcRelocateArgs()
    for name, _ in lib.McmcRelocateArgs._fields_[:17]:
        setattr(a, name, 8)
    a.U, a.n_slots, a.dst_offset, a.K, a.min_opacity, a.workspace, a.workspace_bytes = 4, 4, 0, 1, 0.005, 8, 64
    bad = lambda **kw: [setattr(a, k, x) for k, x in kw.items()] and L.v3a_mcmc_relocate(C.byref(a), None)
    assert bad(n_slots=3) == -2 and bad(n_slots=4, dst_offset=2) == -2 and bad(dst_offset=0, K=0) == -2        # neither relocation nor growth
    assert bad(K=1, min_opacity=0.0) == -2 and bad(min_opacity=0.005, workspace_bytes=63) == -4 and bad(workspace_bytes=64, workspace=4) == -4
    assert bad(workspace=8, v_sh=None) == -1


def test_config_validation_and_schedule():
    from vist3a_amd.post_opt import PostOptConfig, mcmc_refines_at
    d = PostOptConfig()
    assert (d.strategy, d.mcmc_cap_max, d.mcmc_noise_lr, d.mcmc_refine_start_iter, d.mcmc_refine_stop_iter, d.mcmc_refine_every,
            d.mcmc_min_opacity) == ("none", 1_000_000, 5e5, 500, 25_000, 100, 0.005)
    assert (d.opacity_reg, d.scale_reg) == (0.0, 0.0)                  # the strategy does not move the regularisers' defaults
    d.check_strategy()
    PostOptConfig(strategy="mcmc").check_strategy()
    PostOptConfig(strategy="none", mcmc_refine_every=0).check_strategy()          # the fields are not looked at while it is off
    for kw in (dict(strategy="default"), dict(strategy="MCMC"), dict(strategy="mcmc", mcmc_refine_every=0), dict(strategy="mcmc", mcmc_cap_max=0),
               dict(strategy="mcmc", mcmc_cap_max=1.5), dict(strategy="mcmc", mcmc_min_opacity=0.0), dict(strategy="mcmc", mcmc_min_opacity=1.0),
               dict(strategy="mcmc", mcmc_noise_lr=-1.0), dict(strategy="mcmc", seed=-1), dict(strategy="mcmc", mcmc_refine_start_iter=2.0)):
        with pytest.raises(ValueError):
            PostOptConfig(**kw).check_strategy()
    # the predicate at its edges: strictly inside (start, stop), on multiples of `every`
    assert [i for i in range(0, 26_000) if mcmc_refines_at(d, i)] == list(range(600, 25_000, 100))
    c = PostOptConfig(strategy="mcmc", mcmc_refine_start_iter=1, mcmc_refine_stop_iter=100, mcmc_refine_every=4)
    assert [i for i in range(0, 120) if mcmc_refines_at(c, i)] == list(range(4, 100, 4))
    c = PostOptConfig(strategy="mcmc", mcmc_refine_start_iter=4, mcmc_refine_stop_iter=12, mcmc_refine_every=4)
    assert [i for i in range(0, 40) if mcmc_refines_at(c, i)] == [8]
    assert mcmc_refines_at(PostOptConfig(mcmc_refine_start_iter=-1), 0)           # step 0 is a multiple of everything


def test_growth_arithmetic():
    from vist3a_amd.post_opt import PostOptConfig, mcmc_growth
    c = PostOptConfig(strategy="mcmc", mcmc_cap_max=340)
    rows, U = [300], 300
    for _ in range(5):
        U += mcmc_growth(c, U)
        rows.append(U)
    assert rows == [300, 315, 330, 340, 340, 340]
    assert mcmc_growth(c, 341) == 0 and mcmc_growth(c, 5000) == 0       # a scene above the cap only relocates
    assert mcmc_growth(c, 339) == 1 and mcmc_growth(PostOptConfig(), 1) == 0 and mcmc_growth(PostOptConfig(), 19) == 0
    assert mcmc_growth(PostOptConfig(), 20) == 1 and mcmc_growth(PostOptConfig(), 2_400_000) == 0
    assert mcmc_growth(PostOptConfig(), 960_000) == 40_000


def test_cli_options():
    import inference_t23d as I
    from vist3a_amd.utils.argument import inference_vist3a_argument
    req = ["--checkpoint_path", "c", "--transformer_lora_path", "l", "--input_texts_path", "t"]
    parse = lambda *x: inference_vist3a_argument().parse_args(req + list(x))
    ns = parse()
    assert (ns.post_opt_mcmc, ns.post_opt_mcmc_cap_max, ns.post_opt_mcmc_refine) == (False, 1_000_000, "500,25000,100")
    assert (ns.post_opt_opacity_reg, ns.post_opt_scale_reg) == (0.0, 0.0) and I.mcmc_options(ns) is None
    ns = parse("--post_opt_mcmc", "--post_opt_steps", "3")
    assert (ns.post_opt_opacity_reg, ns.post_opt_scale_reg) == (0.0, 0.0)          # the switch leaves the regularisers alone
    assert I.mcmc_options(ns) == (1_000_000, (500, 25_000, 100))
    assert I.mcmc_options(parse("--post_opt_mcmc", "--post_opt_steps", "3", "--post_opt_mcmc_cap_max", "340", "--post_opt_mcmc_refine", "1,100,4")) == (340, (1, 100, 4))
    for bad in (("--post_opt_mcmc",), ("--post_opt_mcmc", "--post_opt_steps", "3", "--post_opt_mcmc_refine", "1,100"),
                ("--post_opt_mcmc", "--post_opt_steps", "3", "--post_opt_mcmc_refine", "1,100,x"),
                ("--post_opt_mcmc", "--post_opt_steps", "3", "--post_opt_mcmc_refine", "1,100,0"),
                ("--post_opt_mcmc", "--post_opt_steps", "3", "--post_opt_mcmc_cap_max", "0")):
        with pytest.raises(ValueError):
            I.mcmc_options(parse(*bad))
    help_text = inference_vist3a_argument().format_help()
    assert "--post_opt_opacity_reg 0.01 --post_opt_scale_reg 0.01" in " ".join(help_text.split()) and "only relocates" in " ".join(help_text.split())
