"""GPU: similarity transforms of a scene (csrc/splat_transform.hip) against the fp64 oracle of tests/splat_transform_oracle.py.

Every output element of v3a_splat_transform is held to a DERIVED bound (the oracle's docstring): (n + 2) 2^-24 sum_j |A_ij| |x_j|
with n the length of the dot product - 3 for the means (plus the same factor times |t|), 4 for the quaternion, 2l + 1 for band l -
and 2 * 2^-24 (|v| + |log s|) for the log-scales; logits and band 0 are copies.  Identity, in-place, run-to-run and guard-band cases
are exact.  v3a_splat_moments is held to n 2^-53 sum |terms| against numpy fp64 and to bit-identity over runs and row paddings.
The render test moves a degree-4 scene and its cameras and compares the rasteriser's images; its gate is twice what the same
comparison gives for the oracle-moved scene rounded to fp32 (mean absolute colour difference, measured on an MI355X and recorded in
DESIGN.md 7i: random similarity yardstick 1.26e-7, kernel 1.34e-7; quarter turn about x yardstick 6.11e-8, kernel 5.95e-8; with the
harmonics left unrotated 0.16)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import splat_transform_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = (1, 63, 64, 65, 257)
NAMES = ("means", "scales", "quats", "opacities", "sh")


def _similarity(seed):
    rng = np.random.default_rng(seed)
    s, R, t = float(np.exp(rng.uniform(-1, 1))), O.random_rotation(rng), rng.standard_normal(3) * 2
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * R, t
    return T, s, R, t


def _dev(scene):
    return {k: torch.from_numpy(v).cuda() for k, v in scene.items()}


def _check(got, scene, s, R, t, xyzw, what):
    val, bnd = O.transform_scene(scene, s, R, t, xyzw)
    worst = {}
    for k in NAMES:
        g = got[k].detach().cpu().double().numpy()
        err = np.abs(g - val[k])
        assert g.shape == val[k].shape and np.isfinite(g).all(), (what, k)
        over = err > bnd[k]
        assert not over.any(), (what, k, int(over.sum()), float(err[over].max()), np.argwhere(over)[:4].tolist())
        worst[k] = float((err / np.maximum(bnd[k], 1e-300)).max()) if err.size and bnd[k].max() > 0 else 0.0
    assert np.array_equal(got["opacities"].cpu().numpy(), scene["opacities"])
    assert np.array_equal(got["sh"][:, :, 0].cpu().numpy(), scene["sh"][:, :, 0])
    return worst


@pytest.mark.parametrize("Kp", O.BAND_COUNTS)
@pytest.mark.parametrize("rows", ROWS)
def test_every_element_within_the_derived_bound(hip_lib, rows, Kp):
    from vist3a_amd import ops
    for xyzw in (True, False):
        T, s, R, t = _similarity(1000 * rows + Kp + int(xyzw))
        scene = O.make_scene(rows, Kp, rows + Kp)
        got = ops.splat_transform(_dev(scene), T, quats_xyzw=xyzw)
        worst = _check(got, scene, s, R, t, xyzw, (rows, Kp, xyzw))
        print(f"[splat transform] rows {rows} K+1 {Kp} xyzw {xyzw}: worst error / bound {worst}")


@pytest.mark.parametrize("Kp", (1, 4, 16, 25))
def test_padded_rows_in_guard_bands(hip_lib, Kp):
    """strided inputs and outputs carved out of poisoned arenas: bound held, inputs untouched, nothing written outside the views;
    then the same call in place on the padded views equals it bit for bit"""
    from vist3a_amd import ops
    rows = 257
    T, s, R, t = _similarity(77 + Kp)
    scene = O.make_scene(rows, Kp, 5 + Kp)
    host = {k: torch.from_numpy(v).cuda() for k, v in scene.items()}
    pad = dict(means=5, scales=4, quats=7, opacities=3, sh=3 * Kp + 6)

    def carve(values=True):
        out = {}
        for k in NAMES:
            flat = host[k].reshape(rows, -1)
            v = G.carve(flat.shape, torch.float32, ld=pad[k], device="cuda")
            if values:
                G.load(v, flat)
            out[k] = v
        return out

    def views(c):
        return dict(means=c["means"], scales=c["scales"], quats=c["quats"], opacities=c["opacities"][:, 0],
                    sh=c["sh"].as_strided((rows, 3, Kp), (pad["sh"], Kp, 1)))

    src, dst = carve(), carve(values=False)
    got = ops.splat_transform(views(src), T, views(dst), quats_xyzw=True)
    _check(got, scene, s, R, t, True, ("padded", Kp))
    for k in NAMES:
        assert G.unchanged(src[k], host[k].reshape(rows, -1)), k
        assert G.violations(dst[k])[0] == 0, (k, G.violations(dst[k]))
    ops.splat_transform(views(src), T, views(src), quats_xyzw=True)                 # in place, padded
    for k in NAMES:
        assert torch.equal(G.bits(src[k]), G.bits(dst[k])), k
        assert G.violations(src[k])[0] == 0, (k, G.violations(src[k]))


@pytest.mark.parametrize("Kp", O.BAND_COUNTS)
def test_identity_in_place_and_repeat(hip_lib, Kp):
    from vist3a_amd import ops
    rows = 257
    scene = O.make_scene(rows, Kp, 31 + Kp)
    scene["means"][3] = [0.0, -0.0, 1e-38]                                          # zeros of both signs, a denormal-range value
    scene["sh"][5] = 0.0
    dev = _dev(scene)
    same = ops.splat_transform(dev, np.eye(4))
    for k in NAMES:
        assert bool((same[k] == dev[k]).all()), k                                   # the identity: every finite input back, under ==
    T, *_ = _similarity(9)
    a, b = ops.splat_transform(dev, T), ops.splat_transform(dev, T)
    work = {k: v.clone() for k, v in dev.items()}
    c = ops.splat_transform(work, T, work)
    for k in NAMES:
        assert torch.equal(G.bits(a[k]), G.bits(b[k])), k                           # two runs
        assert torch.equal(G.bits(a[k]), G.bits(c[k])) and c[k] is work[k], k       # in place
        assert torch.equal(dev[k].cpu(), torch.from_numpy(scene[k])), k             # out of place left the input alone


@pytest.mark.parametrize("Kp", (1, 9, 25))
def test_layout_does_not_change_a_bit(hip_lib, Kp):
    """contiguous 16-byte-aligned harmonics take the 16-byte staging path, the same rows 4 bytes off a 16-byte boundary or padded
    take the per-float walk: one result"""
    from vist3a_amd import ops
    rows = 257
    T, *_ = _similarity(5)
    dev = _dev(O.make_scene(rows, Kp, 8 + Kp))
    want = ops.splat_transform(dev, T)

    def shifted(t):
        buf = torch.full((t.numel() + 1,), float("nan"), device="cuda")
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)
    off_in = dict(dev, sh=shifted(dev["sh"]))
    off_out = {k: torch.empty_like(v) for k, v in dev.items()}
    off_out["sh"] = shifted(dev["sh"])
    wide = torch.full((rows, 3 * Kp + 1), float("nan"), device="cuda")
    wide[:, :3 * Kp] = dev["sh"].reshape(rows, -1)
    pad_in = dict(dev, sh=wide.as_strided((rows, 3, Kp), (3 * Kp + 1, Kp, 1)))
    for what, got in (("unaligned in", ops.splat_transform(off_in, T)), ("unaligned out", ops.splat_transform(dev, T, off_out)),
                      ("padded in", ops.splat_transform(pad_in, T))):
        for k in NAMES:
            assert torch.equal(G.bits(got[k]), G.bits(want[k])), (what, k)


def test_quarter_turn_permutes_band_one(hip_lib):
    """R = a quarter turn about x: D_1 is a signed permutation, so the kernel's band 1 is the input's, reordered, exactly"""
    from vist3a_amd import ops
    T = np.eye(4)
    T[:3, :3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    scene = O.make_scene(65, 4, 2)
    got = ops.splat_transform(_dev(scene), T)["sh"].cpu().numpy()
    D1 = O.band_matrices(T[:3, :3], 1)[0].round()
    assert np.array_equal(got[:, :, 1:], (scene["sh"][:, :, 1:].astype(np.float64) @ D1.T).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ moments
@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(5)
    return (rng.standard_normal((70001, 3)) * np.array([3.0, 0.5, 1.0]) + np.array([10.0, -4.0, 0.25])).astype(np.float32)


@pytest.mark.parametrize("n", (1, 255, 256, 257, 70001))
def test_moments_against_fp64(hip_lib, cloud, n):
    from vist3a_amd import ops
    x, c = cloud[:n], np.array([9.5, -4.25, 0.125])
    d = x.astype(np.float64) - c
    terms = np.concatenate([np.ones((n, 1)), d, d[:, [0, 0, 0, 1, 1, 2]] * d[:, [0, 1, 2, 1, 2, 2]]], axis=1)
    want, bound = terms.sum(0), n * 2.0 ** -53 * np.abs(terms).sum(0)
    dev = torch.from_numpy(x).cuda()
    got = ops.splat_moments(dev, c)
    err = np.abs(got.cpu().numpy() - want)
    print(f"[splat moments] n {n}: worst error / bound {float((err[1:] / np.maximum(bound[1:], 1e-300)).max()):.3g}")
    assert got.cpu().numpy()[0] == n and (err <= bound).all(), (err, bound)
    again = ops.splat_moments(dev, c)
    assert torch.equal(G.bits(got), G.bits(again))                                  # two runs
    for ld in (4, 7):                                                               # two row paddings
        wide = torch.full((n, ld), float("nan"), device="cuda")
        wide[:, :3] = dev
        assert torch.equal(G.bits(ops.splat_moments(wide[:, :3], torch.from_numpy(c))), G.bits(got)), ld


def test_moments_of_nothing(hip_lib):
    from vist3a_amd import ops
    assert not ops.splat_moments(torch.empty(0, 3, device="cuda"), (1.0, 2.0, 3.0)).any()


# ------------------------------------------------------------------------------------------------------ world normalisation
@pytest.mark.parametrize("V", (2, 13, 21))
def test_world_normalisation_with_means(hip_lib, V):
    """the whole normalize() against the reference's record: T1 exactly its T1 route, the covariance of the moved cloud and its
    eigenvalues to 1e-10, the result a similarity whose rows are the reference's axes up to their signs"""
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_transform import covariance_of, principal_axes, world_normalisation
    g = {k.split(".", 1)[1]: v.numpy() for k, v in load_file(str(ROOT / "tests" / "golden" / "world_normalize_ref.safetensors")).items()
         if k.startswith(f"v{V}.")}
    pts = torch.from_numpy(g["points"]).float().cuda()
    assert np.array_equal(pts.cpu().double().numpy(), g["points"])
    T = world_normalisation(g["cams"], pts)
    s, R, t = ops.similarity_parts(T)
    T2 = T @ np.linalg.inv(g["T1"])
    assert np.abs(np.abs(T2[:3, :3]) - np.abs(g["T2"][:3, :3])).max() <= 1e-8
    assert abs(abs(np.linalg.det(T2[:3, :3])) - 1) <= 1e-10 and np.linalg.det(T2[:3, :3]) > 0
    moved = g["points"] @ T[:3, :3].T + T[:3, 3]
    # the point that align_principal_axes centres on - the per-axis median of the cloud in T1's frame - lands on the origin (the
    # per-axis median of the TURNED cloud does not: medians do not commute with rotations, in the reference either)
    assert np.abs(T2[:3, :3] @ np.median(g["points1"], axis=0) + T2[:3, 3]).max() <= 1e-10
    assert np.abs(moved - g["points2"] * np.sign(T2[:3, :3] @ g["T2"][:3, :3].T).diagonal()).max() <= 1e-8
    cov = np.cov(moved, rowvar=False)
    assert np.abs(np.sort(np.diag(cov)) - g["eigenvalues"]).max() <= 1e-10
    assert np.abs(cov - np.diag(np.diag(cov))).max() <= 1e-10
    # the one-pass covariance itself, about the reference's centroid of the cloud it saw
    c1 = np.median(g["points1"], axis=0)
    pts1 = torch.from_numpy(g["points1"]).float().cuda()
    got = covariance_of(pts1, c1)
    ref = np.cov(pts1.cpu().double().numpy(), rowvar=False)
    assert np.abs(got - ref).max() <= 1e-10
    w, _ = principal_axes(got)
    assert np.abs(w - g["eigenvalues"][::-1]).max() <= 1e-6                         # points1 rounded to fp32 here


# ------------------------------------------------------------------------------------------------------- render invariance
def _render_scene():
    rng = np.random.default_rng(42)
    U = 200
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    means = np.concatenate([rng.uniform(-1.2, 1.2, (U, 2)), rng.uniform(2.0, 4.0, (U, 1))], axis=1).astype(np.float32)
    sh = f(U, 3, 25) * 0.25
    sh[:, :, 0] += 0.5
    scene = dict(means=means, scales=np.log(rng.uniform(0.05, 0.25, (U, 3))).astype(np.float32), quats=f(U, 4),
                 opacities=rng.uniform(-1.0, 2.0, U).astype(np.float32), sh=sh)
    c2w = np.tile(np.eye(4), (2, 1, 1))
    a = 0.25
    c2w[1, :3, :3] = [[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]
    c2w[1, :3, 3] = [0.8, -0.1, 0.2]
    return scene, c2w


def _render(scene, c2w):
    from vist3a_amd import ops
    W = H = 32
    view = torch.from_numpy(np.linalg.inv(c2w)).float().cuda().contiguous()
    campos = torch.from_numpy(c2w[:, :3, 3].copy()).float().cuda().contiguous()
    K = torch.tensor([[32.0, 0, 16.0], [0, 32.0, 16.0], [0, 0, 1.0]]).repeat(2, 1, 1).cuda().contiguous()
    with torch.no_grad():
        cov, op = ops.splat_activate(scene["scales"].contiguous(), scene["quats"].contiguous(), scene["opacities"].contiguous())
        color, _, alpha = ops.gs_render(scene["means"].contiguous(), cov, scene["sh"].contiguous(), op, view, campos, K, W, H)
    return color.double().cpu().numpy(), alpha.double().cpu().numpy()


@pytest.mark.parametrize("which", ("random", "quarter_turn_x"))
def test_render_is_invariant(hip_lib, which):
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_transform import transform_cameras
    scene, c2w = _render_scene()
    if which == "random":
        T, s, R, t = _similarity(2024)
    else:
        T, s, t = np.eye(4), 1.0, np.zeros(3)
        R = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
        T[:3, :3] = R
    base, alpha = _render(_dev(scene), c2w)
    assert alpha.mean() > 0.2 and base.std() > 0.05                                 # the images show the scene
    moved_cams = transform_cameras(T, c2w)
    kernel, _ = _render(ops.splat_transform(_dev(scene), T), moved_cams)
    val, _ = O.transform_scene(scene, s, R, t, True)
    oracle, _ = _render(_dev({k: v.astype(np.float32) for k, v in val.items()}), moved_cams)
    yardstick, figure = float(np.abs(oracle - base).mean()), float(np.abs(kernel - base).mean())
    # a wrong component order or sign in any band is a gross error: the unrotated harmonics, for comparison
    wrong = dict(_dev({k: v.astype(np.float32) for k, v in val.items()}), sh=_dev(scene)["sh"])
    gross = float(np.abs(_render(wrong, moved_cams)[0] - base).mean())
    print(f"[splat transform render] {which}: yardstick {yardstick:.3g}, kernel {figure:.3g}, harmonics left unrotated {gross:.3g}")
    assert gross > 100 * max(yardstick, 1e-9)
    assert figure <= 2 * yardstick
