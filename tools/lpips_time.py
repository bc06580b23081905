"""Time LPIPS(VGG) on 448^2 pairs (seeded weights): ms per pair at N = 4 and N = 16, the per-stage split (trunk convolutions, pools, head)
and the trunk's executed TFLOP/s (three bf16 products per split convolution, conv1_1 at its padded width), for conv1_1 padded to 16
channels (halo-tile form) and to 8 (implicit GEMM).  Prints one JSON object; `--json PATH` also writes it to PATH.

    python tools/lpips_time.py [reps] [--json PATH]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
import torch  # noqa: E402

import lpips_oracle as LO  # noqa: E402
from vist3a_amd import lib as L  # noqa: E402
from vist3a_amd import ops  # noqa: E402
from vist3a_amd.evaluation.lpips import LPIPS, LPIPSWeights, VGG_STAGES, _conv_tile  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (spec)


def _cli():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("reps", type=int, nargs="?", default=10, help="timed repetitions (after two warm-ups)")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args()


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def med(xs):
    return sorted(xs)[len(xs) // 2]


def staged(w: LPIPSWeights, pred, gt, out):
    """LPIPS.forward_chunk with an event after every launch group -> {stage: ms}, executed trunk FLOPs"""
    t = {"input": 0.0, "conv": 0.0, "pool": 0.0, "head": 0.0}
    flops = 0.0
    e0 = ev()
    x = ops.lpips_input(pred, gt, w.cin_pad)
    e1 = ev()
    marks = [("input", e0, e1)]
    k = 0
    for s, idx in enumerate(VGG_STAGES):
        if s > 0:
            a = ev()
            x = ops.lpips_pool(x)
            marks.append(("pool", a, ev()))
        for _ in idx:
            cw = w.convs[k]
            k += 1
            F, h, wd = x.shape[1], x.shape[2], x.shape[3]
            flops += 3 * 2.0 * F * h * wd * cw.CoutP * 9 * cw.CinP
            a = ev()
            x = ops.conv_split(x, cw, pad=(0, 1, 1), act=L.ACT_RELU, tile=_conv_tile(cw, h, wd))
            marks.append(("conv", a, ev()))
        a = ev()
        ops.lpips_head(x, w.lins[s], out, accumulate=s > 0)
        marks.append(("head", a, ev()))
    torch.cuda.synchronize()
    for kind, a, b in marks:
        t[kind] += a.elapsed_time(b)
    return t, flops


def main():
    cli = _cli()
    vgg, lin = LO.make_weights(seed=0)
    g = torch.Generator().manual_seed(0)
    res = {"size": 448}
    for cin_pad in (16, 8):
        w = LPIPSWeights.from_state_dicts(vgg, lin, device="cuda", cin_pad=cin_pad)
        m = LPIPS(w)
        for N in (4, 16):
            pred = torch.randint(0, 256, (N, 448, 448, 3), generator=g, dtype=torch.uint8).cuda()
            gt = torch.randint(0, 256, (N, 448, 448, 3), generator=g, dtype=torch.uint8).cuda()
            out = torch.empty(N, dtype=torch.float64, device="cuda")
            for _ in range(2):
                m.forward_chunk(pred, gt, out)
            torch.cuda.synchronize()
            whole = []
            for _ in range(cli.reps):
                a = ev()
                m.forward_chunk(pred, gt, out)
                b = ev()
                torch.cuda.synchronize()
                whole.append(a.elapsed_time(b))
            stages = [staged(w, pred, gt, out) for _ in range(cli.reps)]
            split = {k: med([s[0][k] for s in stages]) for k in stages[0][0]}
            flops = stages[0][1]
            r = dict(ms_total=med(whole), ms_per_pair=med(whole) / N, stage_ms=split,
                     trunk_tflops_executed=flops / (split["conv"] * 1e-3) / 1e12)
            r["trunk_frac_bf16_peak"] = r["trunk_tflops_executed"] / BF16_PEAK_TFLOPS
            r["pool_head_share"] = (split["pool"] + split["head"]) / sum(split.values())
            res[f"cin{cin_pad}_N{N}"] = r
            del pred, gt
    s = json.dumps(res, indent=1)
    print(s)
    if cli.json:
        Path(cli.json).write_text(s)


if __name__ == "__main__":
    main()
