"""GPU: `inference_t23d.py --post_opt_pose_opt` on the synthetic reference-layout checkpoints of tests/test_cli_gpu.py (5 views; with
--post_opt_eval_every 2 the views 1 and 3 train).  With the flag, post_opt_cameras.json next to gaussians.ply holds "extrinsics"
(the camera-to-world matrix of every view), "deltas" (one row of 9 per TRAINING view) and "train_views"; without it the file is
absent and gaussians.ply is byte for byte the plain run's - which runs the loop as it stood - whatever --post_opt_pose_lr says."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu

PROMPT = "a red chair in a white room"
BASE = ("--no_video", "--post_opt_steps", "6", "--post_opt_eval_every", "2")


def test_pose_opt_writes_the_refined_cameras(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text(PROMPT + "\n")

    def run(name, extra=()):
        r = CLI._cli(a, tmp_path / name, extra=BASE + tuple(extra))
        assert r.returncode == 0, r.stderr[-3000:]
        return tmp_path / name / PROMPT

    plain = run("plain")
    off = run("off", ("--post_opt_pose_lr", "1e-3"))
    on = run("on", ("--post_opt_pose_opt", "--post_opt_pose_lr", "1e-3"))
    for d in (plain, off):
        assert not (d / "post_opt_cameras.json").exists()
    assert (off / "gaussians.ply").read_bytes() == (plain / "gaussians.ply").read_bytes()
    assert json.loads((off / "post_opt_stats.json").read_text())["after"]["per_view"] == \
        json.loads((plain / "post_opt_stats.json").read_text())["after"]["per_view"]
    cams = json.loads((on / "post_opt_cameras.json").read_text())
    assert sorted(cams) == ["deltas", "extrinsics", "train_views"]
    ext, deltas = np.asarray(cams["extrinsics"]), np.asarray(cams["deltas"])
    assert cams["train_views"] == [1, 3] and ext.shape == (5, 4, 4) and deltas.shape == (2, 9)
    assert np.isfinite(ext).all() and np.isfinite(deltas).all() and (np.abs(deltas).max(axis=1) > 0).all()
    assert np.allclose(ext[:, 3], [0, 0, 0, 1], atol=1e-6)
    R = ext[:, :3, :3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-4)             # still rigid
    # scene and cameras were refined together: the exported scene is not the plain run's
    assert (on / "gaussians.ply").read_bytes() != (plain / "gaussians.ply").read_bytes()
    assert np.isfinite(CLI._read_ply(on / "gaussians.ply")[2]).all()
