"""Host checks of the scene transforms (csrc/splat_transform.hip, vist3a_amd/utils/splat_transform.py; no GPU needed): the band
matrices of v3a_sh_rotation_matrices against the fit of tests/splat_transform_oracle.py and against their own algebra, the float
basis of the rasteriser's oracle, the camera side of the world normalisation against the reference's recorded outputs
(tests/golden/world_normalize_ref.safetensors), the ctypes struct against the header, and every refusal."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import splat_transform_oracle as O  # noqa: E402
from c_layout import assert_mirrors  # noqa: E402

OK, ARG, SHAPE = 0, -1, -2
SETS = (2, 13, 21)


def _mats(R, deg=4):
    from vist3a_amd import ops
    return [m.numpy() for m in ops.sh_rotation_matrices(R, deg)]


@pytest.fixture(scope="module")
def rotations():
    rng = np.random.default_rng(7)
    return [O.random_rotation(rng) for _ in range(6)]


@pytest.fixture(scope="module")
def golden():
    return {k: v.numpy() for k, v in load_file(str(ROOT / "tests" / "golden" / "world_normalize_ref.safetensors")).items()}


# ------------------------------------------------------------------------------------------------------------ band matrices
def test_band_matrices_match_the_oracle_fit(rotations):
    for R in rotations:
        for l, (D, Do) in enumerate(zip(_mats(R), O.band_matrices(R)), start=1):
            assert D.shape == (2 * l + 1, 2 * l + 1)
            assert np.abs(D - Do).max() <= 1e-12, l


def test_band_matrices_are_orthogonal(rotations):
    for R in rotations:
        for D in _mats(R):
            assert np.abs(D @ D.T - np.eye(len(D))).max() <= 1e-12


def test_band_matrices_compose(rotations):
    for R1, R2 in zip(rotations[:3], rotations[3:]):
        for D12, D1, D2 in zip(_mats(R1 @ R2), _mats(R1), _mats(R2)):
            assert np.abs(D12 - D1 @ D2).max() <= 1e-12


def test_band_matrices_of_the_identity_are_exact():
    for D in _mats(np.eye(3)):
        assert np.array_equal(D, np.eye(len(D)))


def test_lower_degrees_are_prefixes(rotations):
    full = _mats(rotations[0], 4)
    for deg in range(0, 4):
        got = _mats(rotations[0], deg)
        assert len(got) == deg and all(np.array_equal(a, b) for a, b in zip(got, full))


def test_band_matrices_turn_the_float_basis(rotations):
    """Y_l(R d) = D_l Y_l(d) with Y the fp32 basis of the rasteriser's oracle (oracle/gsplat_raster.py: sh_eval's polynomials)"""
    from oracle.gsplat_raster import sh_basis
    rng = np.random.default_rng(11)
    d = rng.standard_normal((100, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for R in rotations:
        Y = sh_basis(torch.from_numpy(d).float(), 4).double().numpy()
        YR = sh_basis(torch.from_numpy(d @ R.T).float(), 4).double().numpy()
        for l, D in enumerate(_mats(R), start=1):
            sl = slice(l * l, (l + 1) * (l + 1))
            assert np.abs(YR[:, sl] - Y[:, sl] @ D.T).max() <= 1e-5, l


def test_quarter_turn_about_x_permutes_band_one():
    Rx = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    D1 = _mats(Rx, 1)[0]
    assert np.abs(np.abs(D1).sum(0) - 1).max() <= 1e-12 and np.abs(np.abs(D1).sum(1) - 1).max() <= 1e-12
    assert sorted(np.abs(D1).round(12).reshape(-1).tolist()) == [0.0] * 6 + [1.0] * 3


def test_sh_rotation_matrices_refusals():
    from vist3a_amd import lib, ops
    L = lib.load()
    I = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    out = (C.c_double * 164)()
    assert L.v3a_sh_rotation_matrices(None, 1, out) == ARG and L.v3a_sh_rotation_matrices(I, 1, None) == ARG
    assert L.v3a_sh_rotation_matrices(I, -1, out) == SHAPE and L.v3a_sh_rotation_matrices(I, 5, out) == SHAPE
    assert L.v3a_sh_rotation_matrices(I, 0, None) == OK and L.v3a_sh_rotation_matrices(I, 4, out) == OK
    mirror = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, -1)
    sheared = (C.c_double * 9)(1, 1e-5, 0, 0, 1, 0, 0, 0, 1)
    assert L.v3a_sh_rotation_matrices(mirror, 1, out) == ARG and L.v3a_sh_rotation_matrices(sheared, 1, out) == ARG
    with pytest.raises(ValueError, match="proper rotation"):
        ops.sh_rotation_matrices(np.diag([1.0, 1.0, -1.0]), 2)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_struct_matches_the_header():
    from vist3a_amd import lib
    assert_mirrors(lib.SplatTransformArgs, "v3a_splat_transform_args")
    assert lib.EXPECTED_ABI >= 37


def _args(rows=0, K=0):
    from vist3a_amd import lib
    a = lib.SplatTransformArgs()
    a.rows, a.K, a.scale = rows, K, 1.0
    for i in (0, 4, 8):
        a.R[i] = 1.0
    return a


def _point(a, K, pre):
    from vist3a_amd import lib
    for f in lib.SPLAT_FIELDS:
        setattr(a, pre + f, 256)
    for f, ld in dict(means=3, log_scales=3, quats=4, logits=1, sh=3 * (K + 1)).items():
        setattr(a, pre + "ld_" + f, ld)


@pytest.mark.parametrize("K", [4, 2, 5, 23, 25, 63])
def test_partial_bands_are_refused(K):
    """K + 1 = 5 and every other count that is not a whole number of bands; no pointer is looked at (rows = 0, all null)"""
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_splat_transform(C.byref(_args(K=K)), None) == SHAPE
    a = _args(rows=4, K=K)
    _point(a, K, "")
    _point(a, K, "out_")
    assert L.v3a_splat_transform(C.byref(a), None) == SHAPE


def test_transform_refusal_order():
    from vist3a_amd import lib
    L = lib.load()
    call = lambda a: L.v3a_splat_transform(C.byref(a), None)
    assert L.v3a_splat_transform(None, None) == ARG
    for K in (0, 3, 8, 15, 24):
        assert call(_args(K=K)) == OK                                               # rows = 0, every pointer null: nothing to do
    assert call(_args(rows=-1)) == SHAPE and call(_args(K=-1)) == SHAPE
    a = _args(rows=4, K=3)
    assert call(a) == ARG                                                           # null inputs
    _point(a, 3, "")
    assert call(a) == ARG                                                           # null outputs
    _point(a, 3, "out_")
    for pre in ("", "out_"):
        for f in lib.SPLAT_FIELDS:
            setattr(a, pre + f, None)
            assert call(a) == ARG, pre + f
            setattr(a, pre + f, 256)
        for f, ld in dict(means=3, log_scales=3, quats=4, logits=1, sh=12).items():
            setattr(a, pre + "ld_" + f, ld - 1)
            assert call(a) == SHAPE, pre + f
            setattr(a, pre + "ld_" + f, ld)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        a.scale = bad
        assert call(a) == ARG, bad
    a.scale = 2.0
    a.R[8] = -1.0                                                                   # a reflection
    assert call(a) == ARG
    a.R[8], a.R[1] = 1.0, 1e-5                                                      # shear: |R R^T - I| = 1e-5
    assert call(a) == ARG
    a.R[1] = 0.0
    a.t[2] = float("nan")
    assert call(a) == ARG


def test_moments_refusals():
    from vist3a_amd import lib
    L = lib.load()
    c = (C.c_double * 3)(0, 0, 0)
    assert L.v3a_splat_moments_workspace_bytes(-1) == SHAPE and L.v3a_splat_moments_workspace_bytes(1 << 31) == SHAPE
    assert L.v3a_splat_moments_workspace_bytes(0) == 0 and L.v3a_splat_moments_workspace_bytes(1024) == 256
    assert L.v3a_splat_moments_workspace_bytes(70001) == 69 * 80 + (256 - 69 * 80 % 256) % 256
    assert L.v3a_splat_moments(256, 3, -1, c, 256, 256, 256, None) == SHAPE
    assert L.v3a_splat_moments(256, 3, 4, None, 256, 256, 256, None) == ARG
    assert L.v3a_splat_moments(256, 3, 4, c, None, 256, 256, None) == ARG
    assert L.v3a_splat_moments(None, 3, 4, c, 256, 256, 256, None) == ARG
    assert L.v3a_splat_moments(256, 2, 4, c, 256, 256, 256, None) == SHAPE
    assert L.v3a_splat_moments(256, 3, 4, c, 256, None, 256, None) == -4 and L.v3a_splat_moments(256, 3, 4, c, 256, 256, 8, None) == -4
    bad = (C.c_double * 3)(0, float("nan"), 0)
    assert L.v3a_splat_moments(256, 3, 4, bad, 256, 256, 256, None) == ARG


# ------------------------------------------------------------------------------------------------------------ similarities
def test_similarity_parts_splits_and_refuses():
    from vist3a_amd import ops
    rng = np.random.default_rng(3)
    R, t = O.random_rotation(rng), rng.standard_normal(3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 1.7 * R, t
    s, Rg, tg = ops.similarity_parts(T)
    assert abs(s - 1.7) <= 1e-14 and np.abs(Rg.numpy() - R).max() <= 1e-14 and np.array_equal(tg.numpy(), t)
    s, Rg, tg = ops.similarity_parts(torch.eye(4))
    assert s == 1.0 and torch.equal(Rg, torch.eye(3, dtype=torch.float64)) and not tg.any()

    def moved(f):
        X = T.copy()
        f(X)
        return X
    mirror = moved(lambda X: X.__setitem__((slice(0, 3), 0), -X[:3, 0]))
    shear = moved(lambda X: X.__setitem__((0, 1), X[0, 1] + 0.01))
    for bad, what in ((mirror, "reflection"), (shear, "not a scaled rotation"), (moved(lambda X: X.__setitem__((slice(0, 3), slice(0, 3)), -X[:3, :3])), "reflection"),
                      (moved(lambda X: X.__setitem__((slice(0, 3), slice(0, 3)), 0.0)), "reflection"),
                      (moved(lambda X: X.__setitem__((slice(0, 3), slice(0, 3)), X[:3, :3] * np.array([1.0, 1.0, 1.1]))), "not a scaled rotation"),
                      (moved(lambda X: X.__setitem__((3, 0), 0.1)), "bottom row"), (np.eye(3), "4x4"),
                      (moved(lambda X: X.__setitem__((0, 3), np.nan)), "finite")):
        with pytest.raises(ValueError, match=what):
            ops.similarity_parts(bad)
    with pytest.raises(ValueError, match="reflection"):
        ops.splat_transform({}, mirror)                                             # refused before the scene is looked at


def test_wrappers_refuse_host_tensors_and_partial_bands():
    from vist3a_amd import ops
    s = {k: torch.from_numpy(v) for k, v in O.make_scene(4, 5, 0).items()}
    with pytest.raises(ValueError, match="whole bands"):
        ops.splat_transform(s, np.eye(4))
    s = {k: torch.from_numpy(v) for k, v in O.make_scene(4, 4, 0).items()}
    with pytest.raises(ValueError, match="device tensor"):
        ops.splat_transform(s, np.eye(4))
    with pytest.raises(ValueError, match="device tensor"):
        ops.splat_moments(torch.zeros(4, 3), (0, 0, 0))


# ------------------------------------------------------------------------------------------------------ world normalisation
@pytest.mark.parametrize("V", SETS)
def test_camera_similarity_matches_the_reference(golden, V):
    from vist3a_amd.utils.splat_transform import transform_cameras, world_normalisation
    g = lambda k: golden[f"v{V}.{k}"]
    T1 = world_normalisation(g("cams"))
    assert np.abs(T1 - g("T1")).max() <= 1e-10
    assert np.abs(transform_cameras(T1, g("cams")) - g("cams1")).max() <= 1e-10
    assert np.abs(transform_cameras(g("T"), torch.from_numpy(g("cams"))) - g("cams2")).max() <= 1e-10      # any similarity, tensors too
    assert np.array_equal(world_normalisation(torch.from_numpy(g("cams"))), T1)


@pytest.mark.parametrize("V", SETS)
def test_principal_axes_convention(golden, V):
    """eigenvalues as the reference's eigh saw them (descending here), a proper rotation, every axis with its largest-magnitude
    component positive except where the determinant rule flipped axis 0; the reference's own T2 differs by row signs at most"""
    from vist3a_amd.utils.splat_transform import principal_axes
    g = lambda k: golden[f"v{V}.{k}"]
    w, rot = principal_axes(g("cov"))
    assert np.abs(w - g("eigenvalues")[::-1]).max() <= 1e-10
    assert abs(abs(np.linalg.det(rot)) - 1) <= 1e-10 and np.linalg.det(rot) > 0
    assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-10
    assert np.abs(rot @ g("cov") @ rot.T - np.diag(w)).max() <= 1e-10
    lead = [rot[j, np.argmax(np.abs(rot[j]))] for j in range(3)]
    assert lead[1] > 0 and lead[2] > 0
    assert np.abs(np.abs(rot) - np.abs(g("T2")[:3, :3])).max() <= 1e-8
    assert np.abs(np.cov(g("points1"), rowvar=False) - g("cov")).max() <= 1e-10                            # the fixture is what np.cov gives


def test_world_transform_json_round_trip(golden, tmp_path):
    from vist3a_amd.utils.splat_transform import read_transform, transform_cameras, write_world_transform
    import json
    T, cams = golden["v13.T"], golden["v13.cams"]
    write_world_transform(tmp_path / "world_transform.json", T, cams)
    data = json.loads((tmp_path / "world_transform.json").read_text())
    assert sorted(data) == ["extrinsics", "transform"]
    assert np.array_equal(read_transform(tmp_path / "world_transform.json"), T)
    assert np.array_equal(np.asarray(data["extrinsics"]), transform_cameras(T, cams))
    (tmp_path / "bare.json").write_text(json.dumps(T.tolist()))
    assert np.array_equal(read_transform(tmp_path / "bare.json"), T)
    (tmp_path / "bad.json").write_text(json.dumps({"matrix": T.tolist()}))
    with pytest.raises(ValueError, match="transform"):
        read_transform(tmp_path / "bad.json")
