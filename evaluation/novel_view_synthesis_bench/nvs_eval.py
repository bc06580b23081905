"""RE10K novel-view rendering — drop-in for the reference's evaluation/novel_view_synthesis_bench/nvs_eval.py (same flags, same
output layout `<output_dir>/images/<seq>/{gt,pred}/NNNNNN.png`), on the HIP path (vist3a_amd.evaluation.nvs).

    PYTHONPATH=$(pwd) python evaluation/novel_view_synthesis_bench/nvs_eval.py --dataset re10k:<root> \
        --seq_id_map re10k_indexmap.json --output_dir <out> --checkpoint_path <stitched.pth> --anysplat_weights <...> --model_id <wan>"""
from __future__ import annotations

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from vist3a_amd.evaluation.argument import stitching_nvs_evaluation_argument  # noqa: E402
from vist3a_amd.evaluation.nvs import main  # noqa: E402

if __name__ == "__main__":
    args = stitching_nvs_evaluation_argument().parse_args()
    with torch.no_grad():
        main(args)
