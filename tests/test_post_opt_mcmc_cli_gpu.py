"""GPU: `inference_t23d.py --post_opt_mcmc` on the synthetic reference-layout checkpoints of tests/test_cli_gpu.py (5 views; with
--post_opt_eval_every 2 the views 1 and 3 train and post_opt_stats.json reports the scene's size).  With the strategy on and a cap
just above the scene's count, the exported PLY and num_GS hold exactly the cap; without the switch the output is byte for byte the
plain run's, whatever the strategy's other options say."""
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


def test_post_opt_mcmc_grows_the_scene_to_the_cap(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text(PROMPT + "\n")

    def run(name, extra=()):
        r = CLI._cli(a, tmp_path / name, extra=BASE + tuple(extra))
        assert r.returncode == 0, r.stderr[-3000:]
        save = tmp_path / name / PROMPT
        return (save / "gaussians.ply").read_bytes(), json.loads((save / "post_opt_stats.json").read_text()), CLI._read_ply(save / "gaussians.ply")[2]

    ply, stats, data = run("plain")
    U = stats["after"]["num_GS"]
    assert data.shape[0] == U >= 200                     # 5 % of it is more than the 7 rows the cap leaves room for
    cap = U + 7
    # the switch off: the strategy's other options change nothing
    ply_off, stats_off, _ = run("off", ("--post_opt_mcmc_cap_max", str(cap), "--post_opt_mcmc_refine", "1,100,4"))
    assert ply_off == ply and stats_off["after"]["per_view"] == stats["after"]["per_view"] and stats_off["after"]["num_GS"] == U
    # on: one refine after the step with 4 steps before it; the scene grows to the cap and is exported and scored at that size
    _, stats_on, data_on = run("on", ("--post_opt_mcmc", "--post_opt_mcmc_cap_max", str(cap), "--post_opt_mcmc_refine", "1,100,4"))
    assert data_on.shape[0] == cap and stats_on["after"]["num_GS"] == cap and stats_on["before"]["num_GS"] == stats["before"]["num_GS"]
    # the Gaussians that were drawn gave opacity and scale to their copies: the old rows are not all what the plain run exported
    assert np.isfinite(data_on).all() and not np.array_equal(data_on[:U], data)
