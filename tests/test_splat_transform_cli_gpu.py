"""GPU: `inference_t23d.py --export_frame {camera,normalized}` on the synthetic reference-layout checkpoints of tests/test_cli_gpu.py.
`camera` (the default) writes what a run without the flag writes, byte for byte.  `normalized` adds world_transform.json and writes
gaussians.ply and the --export_format files in the normalised frame: moving that gaussians.ply back by the inverse of the recorded
transform (ops.splat_transform) lands on the camera-frame file within the bounds of two fp32 passes, and the moved cloud is centred
and axis-aligned.

Bounds of the round trip (u = 2^-24; e(.) the per-element bound of one pass, tests/splat_transform_oracle.py):
  means       |A^-1| e(forward) + e(inverse): the first pass's bound carried through the second, plus the second's own.
  quaternions the same with the Hamilton matrices; both files hold unit quaternions (the writer normalises in fp64 and rounds once,
              which the bounds' spare u per pass covers), compared up to the common sign of a row: q and -q are one rotation.
  log-scales  e(inverse) + what the WRITER adds, which no kernel pass contains: the normalised file stores logf(sigma * s), one
              rounded product (u, absolute in the log) and a logf of 1 ulp (2 u |v'|), the camera file logf(sigma) (2 u |v|).
  opacity, DC copies: equal."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import splat_export_oracle as SO  # noqa: E402
import splat_transform_oracle as O  # noqa: E402
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu
U32 = O.U32


def test_export_frame_flag(hip_lib, tmp_path):
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_import import load_scene
    from vist3a_amd.utils.splat_transform import transform_cameras, world_normalisation
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text("a red chair in a white room\n")
    common = ("--no_video", "--export_format", "ply_compressed,splat", "--export_sh_rest")
    runs = {}
    for name, extra in (("plain", ()), ("camera", ("--export_frame", "camera")), ("normalized", ("--export_frame", "normalized"))):
        r = CLI._cli(a, tmp_path / name, extra=(*common, *extra))
        assert r.returncode == 0, (name, r.stderr[-3000:])
        runs[name] = tmp_path / name / "a red chair in a white room"
    files = ["gaussians.compressed.ply", "gaussians.ply", "gaussians.splat", "prompt.txt"]
    assert sorted(p.name for p in runs["plain"].iterdir()) == files and sorted(p.name for p in runs["camera"].iterdir()) == files
    for f in files:
        assert (runs["camera"] / f).read_bytes() == (runs["plain"] / f).read_bytes(), f
    assert sorted(p.name for p in runs["normalized"].iterdir()) == sorted(files + ["world_transform.json"])
    for f in files[:3]:
        assert (runs["normalized"] / f).read_bytes() != (runs["plain"] / f).read_bytes(), f

    world = json.loads((runs["normalized"] / "world_transform.json").read_text())
    assert sorted(world) == ["extrinsics", "transform"]
    T, moved_cams = np.asarray(world["transform"]), np.asarray(world["extrinsics"])
    s, R, t = ops.similarity_parts(T)
    R, t = R.numpy(), t.numpy()
    Tinv = np.linalg.inv(T)
    cam = load_scene(runs["plain"] / "gaussians.ply", opacity="linear")
    nrm = load_scene(runs["normalized"] / "gaussians.ply", opacity="linear")
    back = ops.splat_transform(nrm, Tinv)
    host = lambda d: {k: v.cpu().double().numpy() for k, v in d.items()}
    cam_h, nrm_h, back_h = host(cam), host(nrm), host(back)
    n = cam_h["means"].shape[0]
    assert nrm_h["means"].shape[0] == n and cam_h["sh"].shape == (n, 3, 1)

    _, e1 = O.transform_scene(cam_h, s, R, t, True)
    _, e2 = O.transform_scene(nrm_h, 1 / s, R.T, Tinv[:3, 3], True)
    bound = e1["means"] @ np.abs(Tinv[:3, :3]).T + e2["means"]
    err = np.abs(back_h["means"] - cam_h["means"])
    print(f"[export frame] {n} Gaussians, s = {s:.4f}; means: worst error / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all()
    H = np.abs(O.hamilton_matrix(O.quat_of_rotation(R.T)))
    sign = np.sign((back_h["quats"] * cam_h["quats"]).sum(1, keepdims=True))
    wxyz, xyzw = [3, 0, 1, 2], [1, 2, 3, 0]
    bound = (e1["quats"][:, wxyz] @ H.T)[:, xyzw] + e2["quats"]
    err = np.abs(sign * back_h["quats"] - cam_h["quats"])
    print(f"[export frame] quaternions: worst error / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all()
    bound = e2["scales"] + U32 * (1 + 2 * np.abs(nrm_h["scales"]) + 2 * np.abs(cam_h["scales"]))
    err = np.abs(back_h["scales"] - cam_h["scales"])
    print(f"[export frame] log-scales: worst error / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all()
    assert np.array_equal(back_h["opacities"], cam_h["opacities"]) and np.array_equal(back_h["sh"], cam_h["sh"])

    # centred and axis-aligned.  The centre is the one the reference's align_principal_axes uses: the per-axis median of the cloud in
    # the frame of the camera similarity T1, which T2 = T T1^-1 sends to the origin (the per-axis median of the turned cloud is
    # printed, not asserted: medians do not commute with rotations)
    cams = transform_cameras(Tinv, moved_cams)
    T1 = world_normalisation(cams)
    T2 = T @ np.linalg.inv(T1)
    p1 = cam_h["means"] @ T1[:3, :3].T + T1[:3, 3]
    centre = T2[:3, :3] @ np.median(p1, axis=0) + T2[:3, 3]
    cov = np.cov(nrm_h["means"], rowvar=False)
    off = np.abs(cov - np.diag(np.diag(cov))).max() / np.trace(cov)
    print(f"[export frame] median mean lands at {np.abs(centre).max():.3g}; per-axis median of the moved cloud "
          f"{np.abs(np.median(nrm_h['means'], axis=0)).max():.3g}; off-diagonal covariance / trace {off:.3g}")
    assert np.abs(centre).max() <= 1e-4 and off <= 1e-4
    assert np.all(np.diff(np.diag(cov)) <= 0)                                       # x, y, z in descending variance
    # the extra files are in the same frame: the .splat holds the same means
    sp = SO.decode_splat((runs["normalized"] / "gaussians.splat").read_bytes())
    assert np.array_equal(np.sort(sp["means"], axis=0), np.sort(nrm_h["means"], axis=0))
