"""Scores of rendered novel views: the reference's evaluation/novel_view_synthesis_bench/calculate_metric.py.

Walks <output_dir>/images/<seq>/{gt,pred}/NNNNNN.png (sequences and files in sorted order), scores each sequence's pairs with
ONE `ops.image_metrics` launch (SSIM as skimage computes it, PSNR from the MSE of uint8 / 255), averages per sequence and then
over sequences.  Writes `_all_samples.csv` (seq,PSNR,SSIM; rewritten, where the reference appends to an existing file) and
`overall-metric[-<save_suffix>].csv`.  LPIPS needs torchvision's VGG-16 and the `lpips` package's linear weights: given both files,
each sequence's pairs are also scored by `evaluation.lpips.LPIPS` (HIP, in chunks) and both CSVs gain the reference's LPIPS column;
without them LPIPS is not computed and the output is PSNR / SSIM only."""
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


def score_sequence(seq_path: Path, device="cuda", lpips=None) -> Dict[str, object]:
    """one sequence: all gt / pred pairs in one launch -> {psnr: [..], ssim: [..]} (+ lpips: [..] with an `evaluation.lpips.LPIPS`)"""
    import torch
    from .. import ops
    names = sorted(os.listdir(seq_path / "gt"))
    if sorted(os.listdir(seq_path / "pred")) != names:
        raise ValueError(f"{seq_path}: gt/ and pred/ hold different files")
    gt = np.stack([read_png_u8(seq_path / "gt" / n) for n in names])
    pred = np.stack([read_png_u8(seq_path / "pred" / n) for n in names])
    ssim, mse = ops.image_metrics(torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device))
    ssim, mse = ssim.cpu().tolist(), mse.cpu().tolist()
    out = dict(psnr=[psnr_from_mse(m) for m in mse], ssim=ssim)
    if lpips is not None:
        out["lpips"] = lpips(torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device)).cpu().tolist()
    return out


def write_csv(path: Path, rows: List[dict]) -> None:
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


def main(output_dir: str, save_suffix: Optional[str] = None, device="cuda", lpips_vgg_weights: Optional[str] = None,
         lpips_lin_weights: Optional[str] = None) -> Dict[str, float]:
    if (lpips_vgg_weights is None) != (lpips_lin_weights is None):
        raise ValueError("LPIPS needs both weight files: lpips_vgg_weights and lpips_lin_weights")
    image_path = Path(output_dir) / "images"
    seqs = sorted(d for d in os.listdir(image_path) if (image_path / d).is_dir())
    if not seqs:
        raise FileNotFoundError(f"no sequences under {image_path}")
    lpips = None
    if lpips_vgg_weights is not None:
        from .lpips import get_lpips
        lpips = get_lpips(lpips_vgg_weights, lpips_lin_weights, device)
    rows = []
    for seq in seqs:
        s = score_sequence(image_path / seq, device, lpips)
        rows.append(dict(seq=seq, PSNR=float(np.mean(s["psnr"])), SSIM=float(np.mean(s["ssim"]))))
        if lpips is not None:
            rows[-1]["LPIPS"] = float(np.mean(s["lpips"]))
    write_csv(Path(output_dir) / "_all_samples.csv", rows)
    overall = {k: float(np.mean([r[k] for r in rows])) for k in rows[0] if k != "seq"}
    name = "overall-metric" + (f"-{save_suffix}" if save_suffix is not None else "") + ".csv"
    write_csv(Path(output_dir) / name, [overall])
    if lpips is None:
        print(LPIPS_NOTE)
        print(f"[metric] {len(rows)} sequences: PSNR {overall['PSNR']:.4f}  SSIM {overall['SSIM']:.4f}")
    else:
        print(f"[metric] {len(rows)} sequences: PSNR {overall['PSNR']:.4f}  SSIM {overall['SSIM']:.4f}  LPIPS {overall['LPIPS']:.4f}")
    return overall
