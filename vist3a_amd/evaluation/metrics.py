"""Scores of rendered novel views: the reference's evaluation/novel_view_synthesis_bench/calculate_metric.py.

Walks <output_dir>/images/<seq>/{gt,pred}/NNNNNN.png (sequences and files in sorted order), scores each sequence's pairs with
ONE `ops.image_metrics` launch (SSIM as skimage computes it, PSNR from the MSE of uint8 / 255), averages per sequence and then
over sequences.  Writes `_all_samples.csv` (seq,PSNR,SSIM; rewritten, where the reference appends to an existing file) and
`overall-metric[-<save_suffix>].csv`.  LPIPS is not computed: it needs the `lpips` package's VGG and linear weights."""
from __future__ import annotations

import csv
import math
import os
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

LPIPS_NOTE = "LPIPS not computed: it needs the lpips package's VGG-16 and linear-layer weights, which this installation does not have"


def read_png_u8(path: Path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    return a[..., None] if a.ndim == 2 else a


def psnr_from_mse(mse: float) -> float:
    """compute_psnr (metrics.py:11-19): -10 log10(mse); identical images give +inf"""
    return math.inf if mse == 0 else -10.0 * math.log10(mse)


def score_sequence(seq_path: Path, device="cuda") -> Dict[str, object]:
    """one sequence: all gt / pred pairs in one launch -> {psnr: [..], ssim: [..]}"""
    import torch
    from .. import ops
    names = sorted(os.listdir(seq_path / "gt"))
    if sorted(os.listdir(seq_path / "pred")) != names:
        raise ValueError(f"{seq_path}: gt/ and pred/ hold different files")
    gt = np.stack([read_png_u8(seq_path / "gt" / n) for n in names])
    pred = np.stack([read_png_u8(seq_path / "pred" / n) for n in names])
    ssim, mse = ops.image_metrics(torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device))
    ssim, mse = ssim.cpu().tolist(), mse.cpu().tolist()
    return dict(psnr=[psnr_from_mse(m) for m in mse], ssim=ssim)


def write_csv(path: Path, rows: List[dict]) -> None:
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


def main(output_dir: str, save_suffix: Optional[str] = None, device="cuda") -> Dict[str, float]:
    image_path = Path(output_dir) / "images"
    seqs = sorted(d for d in os.listdir(image_path) if (image_path / d).is_dir())
    if not seqs:
        raise FileNotFoundError(f"no sequences under {image_path}")
    rows = []
    for seq in seqs:
        s = score_sequence(image_path / seq, device)
        rows.append(dict(seq=seq, PSNR=float(np.mean(s["psnr"])), SSIM=float(np.mean(s["ssim"]))))
    write_csv(Path(output_dir) / "_all_samples.csv", rows)
    overall = dict(PSNR=float(np.mean([r["PSNR"] for r in rows])), SSIM=float(np.mean([r["SSIM"] for r in rows])))
    name = "overall-metric" + (f"-{save_suffix}" if save_suffix is not None else "") + ".csv"
    write_csv(Path(output_dir) / name, [overall])
    print(LPIPS_NOTE)
    print(f"[metric] {len(rows)} sequences: PSNR {overall['PSNR']:.4f}  SSIM {overall['SSIM']:.4f}")
    return overall
