"""The unpack kernels of the scene import (csrc/splat_import.hip) on a synthetic scene of the benchmark's size, 2.4 M Gaussians, with
K = 24 and K = 0 higher-order coefficients, each beside the COPY YARDSTICK of tools/export_time.py: a plain `copy_` that moves the
same number of bytes (half read, half written).  Stream events around `inner` back-to-back calls, 10 warm-up calls, 7 repeats: the
median and the spread (min .. max) in microseconds.  The byte counts are the algorithm's: the payload read once, every output
element written once.  The outputs are allocated once, outside the timed region.

    python tools/import_time.py [--n 2400000] [--json OUT]     one JSON line per format and K"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import torch

from export_time import copy_us, scene, timed
from vist3a_amd import ops
from vist3a_amd.utils.splat_export import export_scene
from vist3a_amd.utils.splat_import import parse_header


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_400_000)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("import_time.py measures on the GPU; none is visible")
    rows = []
    for K in (24, 0):
        s = scene(args.n, K)
        for fmt in ("ply", "ply_compressed", "splat"):
            data = export_scene(s, fmt, quats_xyzw=True)
            _, n, k, table, off = parse_header(data)
            payload = torch.frombuffer(bytearray(data), dtype=torch.uint8)[off:].cuda()
            out = {name: torch.empty_like(t[:n]) if fmt != "splat" else torch.empty_like(t[:n, :, :1] if name == "sh" else t[:n]) for name, t in s.items()}
            fn = {"ply": lambda: ops.splat_import_ply(payload, n, k, table, out=out),
                  "ply_compressed": lambda: ops.splat_import_compressed(payload, n, k, out=out),
                  "splat": lambda: ops.splat_import_splat(payload, n, out=out)}[fmt]
            nbytes = payload.numel() + sum(t.numel() * 4 for t in out.values())
            med, lo, hi = timed(fn)
            cu = copy_us(nbytes)
            row = dict(format=fmt, K=k, n=n, us=round(med, 1), us_min=round(lo, 1), us_max=round(hi, 1), MB=round(nbytes / 1e6, 1),
                       TBps=round(nbytes / med / 1e6, 3), copy_same_bytes_us=round(cu, 1), vs_copy=round(med / cu, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del payload, out
    if args.json:
        Path(args.json).parent.mkdir(exist_ok=True, parents=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
