"""RE10K test-split reader: the reference's evaluation/datasets/re10k_nvs.py (`rescale_image_w_crop` :25-89, `Re10KNVSDataset`,
`get_data` :172-227).

Layout: <root>/<seq>/annotations.json = [{idx, filepath, intrinsics [3,3], extrinsics [4,4]}, ...], `filepath` relative to <root>.
Differences from the reference: no `re10k_nvs_cache.npy` is written next to the code, and sequences that are missing from the
frame-id map or whose annotations do not load are skipped (and counted) instead of raising a KeyError later."""
from __future__ import annotations

import json
import os.path as osp
from typing import Iterable, List, Optional

import numpy as np
import torch
from PIL import Image, ImageFile

ImageFile.LOAD_TRUNCATED_IMAGES = True
LANCZOS = Image.Resampling.LANCZOS


def to_tensor(img: Image.Image) -> torch.Tensor:
    """torchvision ToTensor for an 8-bit PIL image: [C,H,W] float32 = uint8 / 255"""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[..., None]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255)


def rescale_image_w_crop(image: Image.Image, intrinsic, output_width_1: int, output_width_2: int, pixel_center: bool = True):
    """Lanczos resize so the short side is output_width_1, centre crop to a square (the VAE image), Lanczos resize to
    output_width_2 (the feed-forward image); intrinsics follow with the +-0.5 pixel-centre shifts.  The arithmetic is the
    reference's, in the dtype of `intrinsic` (float32 when it comes from annotations.json through torch.tensor).
    -> (feed-forward image, intrinsic, VAE image)"""
    # PIL's size is (width, height): `H` holds the width here, so a non-square image comes out of the first resize with its
    # aspect transposed before the square crop.  That is what the reference computes (and what its published numbers used): kept.
    H, W = map(float, image.size)
    scale = output_width_1 / min(H, W)
    new_h, new_w = round(H * scale), round(W * scale)
    image_first = image.resize((new_w, new_h), resample=LANCZOS)
    intrinsic = np.copy(np.asarray(intrinsic))
    if pixel_center:
        intrinsic[0, 2] = intrinsic[0, 2] + 0.5
        intrinsic[1, 2] = intrinsic[1, 2] + 0.5
    intrinsic[:2, :] = intrinsic[:2, :] * scale
    if pixel_center:
        intrinsic[0, 2] = intrinsic[0, 2] - 0.5
        intrinsic[1, 2] = intrinsic[1, 2] - 0.5
    x0 = max((new_w - output_width_1) // 2, 0)
    y0 = max((new_h - output_width_1) // 2, 0)
    l, t, r, b = x0, y0, x0 + output_width_1, y0 + output_width_1  # noqa: E741
    image_first = image_first.crop((l, t, r, b))
    intrinsic = intrinsic.copy()
    intrinsic[0, 2] -= l
    intrinsic[1, 2] -= t
    H, W = map(float, image_first.size)
    scale = output_width_2 / min(H, W)
    image_second = image_first.resize((round(W * scale), round(H * scale)), resample=LANCZOS)
    intrinsic = intrinsic.copy()
    if pixel_center:
        intrinsic[0, 2] = intrinsic[0, 2] + 0.5
        intrinsic[1, 2] = intrinsic[1, 2] + 0.5
    intrinsic[:2, :] = intrinsic[:2, :] * scale
    if pixel_center:
        intrinsic[0, 2] = intrinsic[0, 2] - 0.5
        intrinsic[1, 2] = intrinsic[1, 2] - 0.5
    return image_second, intrinsic, image_first


class Re10KNVSDataset:
    def __init__(self, root, seq_id_map: dict, load_img_size: int = 512, feedforward_img_size: int = 448,
                 seq_file: Optional[str] = None, verbose: bool = True):
        """seq_id_map: {sequence: [frame positions]} (re10k_indexmap.json).  seq_file: one sequence per line (re10k_test.txt);
        default: the keys of `seq_id_map` in file order.  `sequence_list` keeps the listed order, minus the skipped sequences."""
        self.root = str(root)
        self.load_img_size, self.feedforward_img_size = load_img_size, feedforward_img_size
        if seq_file is not None:
            with open(seq_file) as f:
                listed = [x.strip() for x in f if x.strip()]
        else:
            listed = list(seq_id_map)
        self.metadata, self.sequence_list = {}, []
        self.skipped_missing, self.skipped_unreadable = [], []
        for seq in listed:
            if seq not in seq_id_map:
                self.skipped_missing.append(seq)
                continue
            try:
                with open(osp.join(self.root, seq, "annotations.json")) as f:
                    annos = json.load(f)
                info = [dict(idx=a["idx"], filepath=a["filepath"], intrinsics=torch.tensor(a["intrinsics"]),
                             extrinsics=torch.tensor(a["extrinsics"])) for a in annos]
            except Exception:  # noqa: BLE001  (the reference prints and moves on as well)
                self.skipped_unreadable.append(seq)
                continue
            self.metadata[seq] = info
            self.sequence_list.append(seq)
        if verbose and (self.skipped_missing or self.skipped_unreadable):
            print(f"[Re10K-test] skipped {len(self.skipped_missing) + len(self.skipped_unreadable)} of {len(listed)} sequences "
                  f"({len(self.skipped_missing)} not in the frame-id map, {len(self.skipped_unreadable)} without readable annotations)")

    def __len__(self) -> int:
        return len(self.sequence_list)

    def get_data(self, sequence_name: str, ids: Optional[Iterable[int]] = None) -> dict:
        """ids: positions in the sequence's annotation list, used in the given order (not sorted)"""
        metadata = self.metadata[sequence_name]
        ids = list(range(len(metadata))) if ids is None else [int(i) for i in ids]
        annos = [metadata[i] for i in ids]
        n = len(annos)
        images: List[torch.Tensor] = []
        vae_images: List[torch.Tensor] = []
        extrinsics = torch.eye(4, 4)[None].repeat(n, 1, 1)
        intrinsics = torch.eye(3, 3)[None].repeat(n, 1, 1)
        paths = []
        for k, anno in enumerate(annos):
            impath = osp.join(self.root, anno["filepath"])
            with Image.open(impath) as im:
                rgb, intr, vae = rescale_image_w_crop(im, anno["intrinsics"].numpy(), self.load_img_size, self.feedforward_img_size)
            paths.append(impath)
            extrinsics[k] = anno["extrinsics"]
            intrinsics[k] = torch.from_numpy(intr)
            images.append(to_tensor(rgb))
            vae_images.append(to_tensor(vae))
        return {"seq_id": sequence_name, "n": len(metadata), "ind": torch.tensor(ids), "image_paths": paths, "extrs": extrinsics,
                "intrs": intrinsics, "images": torch.stack(images), "vae_images": torch.stack(vae_images)}


def load_seq_id_map(path: str) -> dict:
    with open(path) as f:
        return json.load(f)
