"""The stages of the scene export (csrc/splat_export.hip) on a synthetic scene of the benchmark's size, 2.4 M Gaussians, with K = 24
and K = 0 higher-order coefficients, each beside the COPY YARDSTICK of tools/norm_time.py: a plain `copy_` that moves the same
number of bytes (half read, half written).  Stream events around `inner` back-to-back calls, 10 warm-up calls, 7 repeats: the
median and the spread (min .. max) in microseconds.  The byte counts are the algorithm's (what a stage must read and write once),
computed from the shapes below; the radix sort's internal passes are not counted, so its ratio shows their cost.

    python tools/export_time.py [--n 2400000] [--json OUT]     one JSON line per stage and K, then the end-to-end file times"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from vist3a_amd import ops
from vist3a_amd.utils.splat_export import OPACITY_THRESHOLD, export_scene


def timed(fn, inner=20, warm=10, repeats=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / inner * 1e3)
    return statistics.median(us), min(us), max(us)


def copy_us(nbytes_moved):
    a = torch.empty(max(int(nbytes_moved) // 2, 1), device="cuda", dtype=torch.uint8)
    b = torch.empty_like(a)
    return timed(lambda: b.copy_(a))[0]


def scene(N, K, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return dict(means=rn(N, 3) * 3, scales=rn(N, 3) * 0.8 - 3, quats=rn(N, 4), opacities=rn(N) * 2 + 1, sh=rn(N, 3, K + 1) * 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_400_000)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("export_time.py measures on the GPU; none is visible")
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for K in (24, 0):
        N = args.n
        s = scene(N, K)
        kw = dict(quats_xyzw=True)
        in_row = (3 + 3 + 4 + 1 + 3 * (K + 1)) * 4             # bytes of one Gaussian's parameters
        r, c = ops.splat_export_filter(s, opacity_threshold=OPACITY_THRESHOLD, **kw)
        n = int(c.item())
        order = ops.splat_export_sort(s, r, n, **kw)
        stages = {
            # every parameter read once; a flag byte written and read, a row index written
            "filter": (lambda: ops.splat_export_filter(s, opacity_threshold=OPACITY_THRESHOLD, **kw), N * (in_row + 2) + n * 4),
            # means gathered twice (range, keys); key written; (key, row) read and written once by an ideal sort
            "sort": (lambda: ops.splat_export_sort(s, r, n, **kw), n * (4 + 12) * 2 + n * 4 + n * 16),
            # index + means, log-scales, DC (3 floats of the row), quaternion, logit, the K harmonics; 16 + 3K bytes out, 72 per chunk
            "pack_compressed": (lambda: ops.splat_export_pack_compressed(s, order, n, **kw), n * (4 + 12 + 12 + 12 + 16 + 4 + 12 * K + 16 + 3 * K) + (n + 255) // 256 * 72),
            "pack_splat": (lambda: ops.splat_export_pack_splat(s, order, n, **kw), n * (4 + 12 + 12 + 12 + 16 + 4 + 32)),
            "pack_ply": (lambda: ops.splat_export_pack_ply(s, r, n, **kw), n * (4 + 2 * in_row)),
        }
        for name, (fn, nbytes) in stages.items():
            med, lo, hi = timed(fn)
            cu = copy_us(nbytes)
            row(stage=name, K=K, N=N, survivors=n, us=round(med, 1), us_min=round(lo, 1), us_max=round(hi, 1), MB=round(nbytes / 1e6, 1),
                TBps=round(nbytes / med / 1e6, 3), copy_same_bytes_us=round(cu, 1), vs_copy=round(med / cu, 2))
        for fmt in ("ply_compressed", "splat", "ply"):          # end to end: kernels, the count's read-back, the copy to the host, bytes()
            export_scene(s, fmt, **kw)
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                data = export_scene(s, fmt, **kw)
                ts.append((time.perf_counter() - t0) * 1e3)
            row(end_to_end=fmt, K=K, N=N, file_MB=round(len(data) / 1e6, 1), ms=round(statistics.median(ts), 1), ms_min=round(min(ts), 1), ms_max=round(max(ts), 1))
    if args.json:
        Path(args.json).parent.mkdir(exist_ok=True, parents=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
