"""GPU: `inference_t23d.py --post_opt_steps 3 --post_opt_depth_lambda X` on the synthetic reference-layout checkpoints of
tests/test_cli_gpu.py.  0 (the default) changes nothing: gaussians.ply is byte-identical to a run without the flag; 0.05 completes,
writes every output and a different .ply (the depth head's maps and confidence mask of the scene supervise the loop)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu


def test_post_opt_depth_lambda_flag(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    prompt = "a red chair in a white room"
    a.prompts.write_text(prompt + "\n")
    runs = {}
    for name, extra in (("plain", ("--no_video",)), ("zero", ("--no_video", "--post_opt_depth_lambda", "0")), ("depth", ("--post_opt_depth_lambda", "0.05"))):
        r = CLI._cli(a, tmp_path / name, extra=("--post_opt_steps", "3", *extra))   # each child under _cli's own time limit
        assert r.returncode == 0, (name, r.stderr[-3000:])
        runs[name] = tmp_path / name / prompt
    ply = {k: (d / "gaussians.ply").read_bytes() for k, d in runs.items()}
    assert ply["plain"] == ply["zero"]
    assert ply["depth"] != ply["zero"]
    assert sorted(p.stem for p in runs["depth"].iterdir()) == ["depth", "gaussians", "gs", "prompt"]      # the two videos too
    assert all(p.stat().st_size > 0 for p in runs["depth"].iterdir())
    _, props, data = CLI._read_ply(runs["depth"] / "gaussians.ply")
    n0 = CLI._read_ply(runs["zero"] / "gaussians.ply")[2].shape[0]
    assert 0 < data.shape[0] <= n0 and np.isfinite(data).all()
    assert np.allclose(np.linalg.norm(data[:, 13:17], axis=1), 1.0, atol=1e-4)
