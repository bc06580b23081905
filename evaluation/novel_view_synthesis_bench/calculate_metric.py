"""PSNR / SSIM of rendered novel views — drop-in for the reference's evaluation/novel_view_synthesis_bench/calculate_metric.py
(same flags; reads `<output_dir>/images/<seq>/{gt,pred}/*.png`, writes `_all_samples.csv` and `overall-metric.csv`), scored by the
HIP metric kernel (vist3a_amd.evaluation.metrics).  LPIPS is not computed."""
from __future__ import annotations

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from vist3a_amd.evaluation.argument import stitching_nvs_evaluation_argument  # noqa: E402
from vist3a_amd.evaluation.metrics import main  # noqa: E402

if __name__ == "__main__":
    args = stitching_nvs_evaluation_argument().parse_args()
    main(args.output_dir, getattr(args, "save_suffix", None))
