"""GPU: `inference_t23d.py --post_opt_batch_size B --post_opt_visible_adam` on the synthetic reference-layout checkpoints of
tests/test_cli_gpu.py (5 views: batches of 4 and 1).  The run writes gaussians.ply, a second run writes the same bytes, and a batch size of 10 is refused with the validation's message before anything loads."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu

PROMPT = "a red chair in a white room"
BASE = ("--no_video", "--post_opt_steps", "6")


def test_batched_visible_adam_run_is_reproducible(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text(PROMPT + "\n")

    def run(name, extra=()):
        r = CLI._cli(a, tmp_path / name, extra=BASE + tuple(extra))
        assert r.returncode == 0, r.stderr[-3000:]
        ply = tmp_path / name / PROMPT / "gaussians.ply"
        return ply.read_bytes(), CLI._read_ply(ply)[2]

    flags = ("--post_opt_batch_size", "4", "--post_opt_visible_adam")
    first, data = run("first", flags)
    second, _ = run("second", flags)
    assert first == second
    assert data.shape[0] > 0 and np.isfinite(data).all()


def test_batch_size_ten_is_refused(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text(PROMPT + "\n")
    r = CLI._cli(a, tmp_path / "ten", extra=BASE + ("--post_opt_batch_size", "10"))
    assert r.returncode != 0 and "--post_opt_batch_size" in r.stderr and "at most 9" in r.stderr and "unresolved" in r.stderr
    assert not (tmp_path / "ten" / PROMPT / "gaussians.ply").exists()
