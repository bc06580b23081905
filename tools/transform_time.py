"""The scene transform (csrc/splat_transform.hip) on a synthetic scene of the benchmark's size, 2.4 M Gaussians, for every band count
K + 1 = 25, 16, 9, 4, 1, out of place and in place, and the second-moment reduction of the principal-axes step, each beside the COPY
YARDSTICK of tools/norm_time.py: a plain `copy_` that moves the same number of bytes (half read, half written).  Stream events around
`inner` back-to-back calls, 10 warm-up calls, 7 repeats: the median and the spread (min .. max) in microseconds.  The byte counts are
the algorithm's: every parameter of a row read once and written once (11 + 3 (K + 1) floats each way); the moments read the means.
The host's part of a transform call (the fp64 band matrices, 164 coefficients) is inside the timed calls.

    python tools/transform_time.py [--n 2400000] [--json OUT]     one JSON line per case"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from tools.export_time import copy_us, scene, timed
from vist3a_amd import ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_400_000)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transform_time.py measures on the GPU; none is visible")
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    rng = np.random.default_rng(0)
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 0.7 * q, [0.3, -1.0, 2.0]
    N = args.n
    for Kp in (25, 16, 9, 4, 1):
        s = scene(N, Kp - 1)
        out = {k: torch.empty_like(v) for k, v in s.items()}
        nbytes = 2 * N * (3 + 3 + 4 + 1 + 3 * Kp) * 4
        cu = copy_us(nbytes)
        for name, dst in (("transform", out), ("transform_in_place", s)):
            med, lo, hi = timed(lambda: ops.splat_transform(s, T, dst))
            row(stage=name, coefficients=Kp, N=N, us=round(med, 1), us_min=round(lo, 1), us_max=round(hi, 1), MB=round(nbytes / 1e6, 1),
                TBps=round(nbytes / med / 1e6, 3), copy_same_bytes_us=round(cu, 1), vs_copy=round(med / cu, 2))
    means = scene(N, 0)["means"]
    nbytes = N * 12
    med, lo, hi = timed(lambda: ops.splat_moments(means, (0.1, -0.2, 0.3)))
    cu = copy_us(2 * nbytes)       # a copy that READS as many bytes
    row(stage="moments", N=N, us=round(med, 1), us_min=round(lo, 1), us_max=round(hi, 1), MB=round(nbytes / 1e6, 1),
        TBps=round(nbytes / med / 1e6, 3), copy_reading_same_bytes_us=round(cu, 1), vs_copy=round(med / cu, 2))
    if args.json:
        Path(args.json).parent.mkdir(exist_ok=True, parents=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
