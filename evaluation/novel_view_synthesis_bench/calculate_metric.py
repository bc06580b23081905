"""PSNR / SSIM / LPIPS of rendered novel views — drop-in for the reference's evaluation/novel_view_synthesis_bench/calculate_metric.py
(same flags; reads `<output_dir>/images/<seq>/{gt,pred}/*.png`, writes `_all_samples.csv` and `overall-metric.csv`), scored by the
HIP kernels (vist3a_amd.evaluation.metrics).  LPIPS(VGG) needs two weight files the reference's packages ship:
`--lpips_vgg_weights` (torchvision's vgg16-397923af.pth) and `--lpips_lin_weights` (lpips' weights/v0.1/vgg.pth).  Without them
LPIPS is not computed and the CSVs hold PSNR and SSIM only."""
from __future__ import annotations

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from vist3a_amd.evaluation.argument import calculate_metric_argument  # noqa: E402
from vist3a_amd.evaluation.metrics import main  # noqa: E402

if __name__ == "__main__":
    args = calculate_metric_argument().parse_args()
    main(args.output_dir, getattr(args, "save_suffix", None), lpips_vgg_weights=args.lpips_vgg_weights,
         lpips_lin_weights=args.lpips_lin_weights)
