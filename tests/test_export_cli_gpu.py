"""GPU: `inference_t23d.py --export_format ply_compressed,splat` on the synthetic reference-layout checkpoints of tests/test_cli_gpu.py.
Without the flag the directory holds what it held; with it gaussians.compressed.ply and gaussians.splat appear next to a
gaussians.ply that is byte for byte the plain run's, DC colour only, and decode to its Gaussians: all of them in the .splat, those
with an opacity above 1/255 in the compressed PLY (the format's own filter)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import splat_export_oracle as SO  # noqa: E402
import test_cli_gpu as CLI  # noqa: E402

pytestmark = pytest.mark.gpu


def test_export_format_flag(hip_lib, tmp_path):
    a = CLI._write_assets(tmp_path)
    a.prompts.write_text("a red chair in a white room\n")
    runs = {}
    for name, extra in (("plain", ()), ("export", ("--export_format", "ply_compressed,splat"))):
        r = CLI._cli(a, tmp_path / name, extra=("--no_video", *extra))
        assert r.returncode == 0, (name, r.stderr[-3000:])
        runs[name] = tmp_path / name / "a red chair in a white room"
    assert sorted(p.name for p in runs["plain"].iterdir()) == ["gaussians.ply", "prompt.txt"]
    assert sorted(p.name for p in runs["export"].iterdir()) == ["gaussians.compressed.ply", "gaussians.ply", "gaussians.splat", "prompt.txt"]
    assert (runs["export"] / "gaussians.ply").read_bytes() == (runs["plain"] / "gaussians.ply").read_bytes()
    _, props, data = CLI._read_ply(runs["plain"] / "gaussians.ply")
    N, opacity = data.shape[0], data[:, props.index("opacity")].astype(np.float64)
    s = SO.decode_splat((runs["export"] / "gaussians.splat").read_bytes())
    assert s["n"] == N
    assert np.array_equal(np.sort(s["means"], axis=0), np.sort(data[:, :3].astype(np.float64), axis=0))     # the same Gaussians, Morton order
    c = SO.decode_compressed((runs["export"] / "gaussians.compressed.ply").read_bytes())
    sure, maybe = int((opacity > 1 / 255 + 1e-6).sum()), int((opacity > 1 / 255 - 1e-6).sum())
    print(f"[export cli] {N} Gaussians, {c['n']} in the compressed PLY ({sure}..{maybe} above 1/255)")
    assert sure <= c["n"] <= maybe and c["n"] > 0 and c["K"] == 0
    lo, hi = data[:, :3].min(axis=0), data[:, :3].max(axis=0)
    assert (c["means"] >= lo - 1e-5).all() and (c["means"] <= hi + 1e-5).all()
