"""Time one synthetic full-size RE10K sequence of the NVS evaluation (12 views: 9-view context forward, 13-view pose pass, 4 renders
at 448^2) stage by stage, the poses-only pass against a full second forward, and the metric launch on the four 448^2 pairs.
Prints one JSON object; `--json PATH` also writes it to PATH.

    python tools/nvs_time.py [reps] [--json PATH]"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from vist3a_amd import ops  # noqa: E402
from vist3a_amd.evaluation.argument import stitching_nvs_evaluation_argument  # noqa: E402
from vist3a_amd.evaluation.nvs import inference_nvs, load_nvs_model, quantize, split_views  # noqa: E402


def _cli():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("reps", type=int, nargs="?", default=5, help="timed repetitions (after one warm-up)")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args()


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    cli = _cli()
    reps = cli.reps
    args = stitching_nvs_evaluation_argument().parse_args(["--dataset", "re10k:.", "--seq_id_map", "x", "--checkpoint_path", "synthetic",
                                                            "--model_id", "none"])
    t0 = time.time()
    model = load_nvs_model(args)
    torch.cuda.synchronize()
    print(f"build {time.time() - t0:.1f} s", flush=True)
    g = torch.Generator().manual_seed(0)
    images, vae_images = torch.rand(12, 3, 448, 448, generator=g), torch.rand(12, 3, 512, 512, generator=g)
    target, source = split_views(12)
    stages = []
    with torch.no_grad():
        for it in range(reps + 1):
            t, w0 = {}, time.time()
            pred = inference_nvs(images, vae_images, model, target, generator=torch.Generator(device="cuda").manual_seed(0), timings=t)
            torch.cuda.synchronize()
            t["wall_ms"] = (time.time() - w0) * 1e3
            if it:
                stages.append(t)
        # pose pass vs a full second forward on the same 13 views
        ctx = [*source, source[-1]]
        allv = images[ctx + target][None].cuda().permute(0, 2, 1, 3, 4) * 2 - 1
        allv_vae = vae_images[ctx + target][None].cuda().permute(0, 2, 1, 3, 4) * 2 - 1
        pose_ms, full_ms = [], []
        for it in range(reps + 1):
            e0 = ev()
            model.predict_poses(allv_vae, allv, generator=torch.Generator(device="cuda").manual_seed(1))
            e1 = ev()
            model(images=allv_vae, feedforward_image=allv, train=False, generator=torch.Generator(device="cuda").manual_seed(1))
            e2 = ev()
            e2.synchronize()
            if it:
                pose_ms.append(e0.elapsed_time(e1))
                full_ms.append(e1.elapsed_time(e2))
        # metric launch on the four 448^2 pairs of the sequence
        gt = torch.stack([torch.from_numpy(quantize(images[i])) for i in target]).cuda()
        pr = torch.stack([torch.from_numpy(quantize(p)) for p in pred]).cuda()
        ops.image_metrics(gt, pr)
        torch.cuda.synchronize()
        m = []
        for _ in range(20):
            e0 = ev()
            ops.image_metrics(gt, pr)
            e1 = ev()
            e1.synchronize()
            m.append(e0.elapsed_time(e1))
    res = dict(stages={k: med([s[k] for s in stages]) for k in stages[0]}, pose_pass_13v_ms=med(pose_ms), full_forward_13v_ms=med(full_ms),
               metric_4x448_ms=med(m), reps=reps)
    print(json.dumps(res, indent=1))
    if cli.json:
        Path(cli.json).parent.mkdir(parents=True, exist_ok=True)
        Path(cli.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
