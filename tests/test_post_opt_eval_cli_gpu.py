"""GPU: `inference_t23d.py --post_opt_steps 4 --post_opt_eval_every 2` on the synthetic reference-layout checkpoints of
tests/test_cli_gpu.py (5 views: 0, 2 and 4 are held out, 1 and 3 train).  post_opt_stats.json appears next to gaussians.ply with the
reference's keys and finite values; cc_psnr is there exactly when --post_opt_bilateral_grid is."""
import json
import math
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("grid", [False, True])
def test_post_opt_eval_every_writes_stats(hip_lib, tmp_path, grid):
    a = CLI._write_assets(tmp_path)
    prompt = "a red chair in a white room"
    a.prompts.write_text(prompt + "\n")
    extra = ("--no_video", "--post_opt_steps", "4", "--post_opt_eval_every", "2") + (("--post_opt_bilateral_grid",) if grid else ())
    r = CLI._cli(a, tmp_path / "run", extra=extra)
    assert r.returncode == 0, r.stderr[-3000:]
    save = tmp_path / "run" / prompt
    assert (save / "gaussians.ply").stat().st_size > 0
    stats = json.loads((save / "post_opt_stats.json").read_text())
    assert sorted(stats) == ["after", "before", "held_out"] and stats["held_out"] == [0, 2, 4]
    keys = {"psnr", "ssim", "num_GS", "ellipse_time", "per_view"} | ({"cc_psnr"} if grid else set())
    for when in ("before", "after"):
        s = stats[when]
        assert set(s) == keys, (when, sorted(s))
        assert all(math.isfinite(s[k]) for k in keys - {"per_view"}), s
        assert s["num_GS"] > 0 and s["ellipse_time"] > 0 and -1 <= s["ssim"] <= 1 and s["psnr"] > 0
        assert len(s["per_view"]) == 3
        for v in s["per_view"]:
            assert all(math.isfinite(v[k]) for k in keys - {"per_view", "num_GS", "ellipse_time"}), v
        assert abs(sum(v["psnr"] for v in s["per_view"]) / 3 - s["psnr"]) < 1e-9
    assert stats["after"]["num_GS"] <= stats["before"]["num_GS"]          # rows at or below min_opacity are dropped
    assert stats["after"]["per_view"] != stats["before"]["per_view"]       # four steps moved the scene
