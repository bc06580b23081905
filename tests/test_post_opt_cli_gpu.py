"""GPU: `inference_t23d.py --post_opt_steps N` on the synthetic reference-layout checkpoints of tests/test_cli_gpu.py.  0 (the default)
changes nothing: gaussians.ply is byte-identical to a run without the flag; 3 steps complete and write a .ply with at most as
many vertices (Gaussians at or below min_opacity are dropped)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu


def test_post_opt_steps_flag(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text("a red chair in a white room\n")
    runs = {}
    for name, extra in (("plain", ()), ("zero", ("--post_opt_steps", "0")), ("three", ("--post_opt_steps", "3"))):
        r = CLI._cli(a, tmp_path / name, extra=("--no_video", *extra))
        assert r.returncode == 0, (name, r.stderr[-3000:])
        runs[name] = tmp_path / name / "a red chair in a white room" / "gaussians.ply"
    assert runs["plain"].read_bytes() == runs["zero"].read_bytes()
    n0 = CLI._read_ply(runs["plain"])[2].shape[0]
    _, props, data = CLI._read_ply(runs["three"])
    assert 0 < data.shape[0] <= n0 and np.isfinite(data).all()
    assert np.allclose(np.linalg.norm(data[:, 13:17], axis=1), 1.0, atol=1e-4)
    assert runs["three"].read_bytes() != runs["plain"].read_bytes()
