"""GPU: `inference_t23d.py --post_opt_densify` on the synthetic reference-layout checkpoints of tests/test_cli_gpu.py (5 views; with
--post_opt_eval_every 2 the views 1 and 3 train and post_opt_stats.json reports the scene's size).  With the strategy on (one refine
after the step with 4 steps before it, a gradient threshold every visible Gaussian passes) gaussians.ply holds as many vertices as
num_GS says, and not as many as the run without the switch."""
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
OPTIONS = ("--post_opt_densify_refine", "1,100,4,100", "--post_opt_densify_grad", "1e-9")


def test_post_opt_densify_changes_the_exported_count(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text(PROMPT + "\n")

    def run(name, extra=()):
        r = CLI._cli(a, tmp_path / name, extra=BASE + tuple(extra))
        assert r.returncode == 0, r.stderr[-3000:]
        save = tmp_path / name / PROMPT
        return (save / "gaussians.ply").read_bytes(), json.loads((save / "post_opt_stats.json").read_text()), CLI._read_ply(save / "gaussians.ply")[2]

    _, stats, data = run("plain", OPTIONS)               # without the switch the strategy's other options are not looked at
    U = stats["after"]["num_GS"]
    assert data.shape[0] == U
    _, stats_on, data_on = run("on", ("--post_opt_densify",) + OPTIONS)
    n = stats_on["after"]["num_GS"]
    print(f"[densify cli] num_GS {stats_on['before']['num_GS']} -> {n} (without the switch {U})")
    assert data_on.shape[0] == n and n != U and stats_on["before"]["num_GS"] == stats["before"]["num_GS"]
    assert np.isfinite(data_on).all()
