"""GPU: `inference_t23d.py --post_opt_steps N --post_opt_bilateral_grid` on the synthetic reference-layout checkpoints of
tests/test_cli_gpu.py (5 views).  With `--post_opt_steps 4` the run completes and writes the same files as a run without the flag.
A different gaussians.ply needs a view to come round again: every grid starts as the identity, whose slice returns the render bit
for bit and whose total variation has a zero gradient, so a grid first moves at the step that shows its view and the scene sees it
at that view's NEXT step - with 5 views never within 4 steps (the reference's loop has the same property up to the rounding of its
fp32 slice).  The difference is therefore asserted at 10 steps, two passes over the views, against the run without the flag."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu


def test_post_opt_bilateral_grid_flag(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    prompt = "a red chair in a white room"
    a.prompts.write_text(prompt + "\n")
    runs = {}
    for name, extra in (("plain", ("--post_opt_steps", "10")), ("grid", ("--post_opt_steps", "10", "--post_opt_bilateral_grid")),
                        ("grid4", ("--post_opt_steps", "4", "--post_opt_bilateral_grid"))):
        r = CLI._cli(a, tmp_path / name, extra=("--no_video", *extra))   # each child under _cli's own time limit
        assert r.returncode == 0, (name, r.stderr[-3000:])
        runs[name] = tmp_path / name / prompt
    files = sorted(p.name for p in runs["plain"].iterdir())
    for name in ("grid", "grid4"):
        assert sorted(p.name for p in runs[name].iterdir()) == files
        assert all(p.stat().st_size > 0 for p in runs[name].iterdir())
    assert (runs["grid"] / "gaussians.ply").read_bytes() != (runs["plain"] / "gaussians.ply").read_bytes()
    n0 = CLI._read_ply(runs["plain"] / "gaussians.ply")[2].shape[0]
    for name in ("grid", "grid4"):
        _, props, data = CLI._read_ply(runs[name] / "gaussians.ply")
        assert data.shape[0] == n0 and np.isfinite(data).all()
        assert np.allclose(np.linalg.norm(data[:, 13:17], axis=1), 1.0, atol=1e-4)
