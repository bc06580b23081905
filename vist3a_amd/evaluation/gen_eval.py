"""Generated-scene evaluation, host side: the reference's evaluation/gen_eval/t3_scene_evaluation.py - the folder walk (:50-77), the
frame sampling (:28-47) and the JSON layout (:138-160) - for the metrics this package computes (clip_score, longclip_score;
vist3a_amd.evaluation.clip).  `gs.avi` is the Motion-JPEG AVI our own CLI writes (misc/image_io.py) and is decoded with PIL; `gs.mp4`
needs OpenCV."""
from __future__ import annotations

import io
import json
import os
import struct
from pathlib import Path
from typing import Callable, Dict, List, Optional

import numpy as np

NUM_SAMPLES = 8
VIDEO_NAMES = ("gs.mp4", "gs.avi")


def sample_indices(total_frames: int, num_samples: int = NUM_SAMPLES) -> List[int]:
    """t3_scene_evaluation.py:35"""
    return [int(i * total_frames / num_samples) for i in range(num_samples)]


def mjpeg_avi_chunks(path) -> List[bytes]:
    """the JPEG byte strings of a Motion-JPEG AVI, in order: every `00dc` chunk of the RIFF `movi` list"""
    data = Path(path).read_bytes()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    frames: List[bytes] = []

    def walk(lo: int, hi: int, in_movi: bool) -> None:
        p = lo
        while p + 8 <= hi:
            cid, size = data[p: p + 4], struct.unpack("<I", data[p + 4: p + 8])[0]
            body = p + 8
            if body + size > hi:
                raise ValueError(f"{path}: chunk {cid!r} at {p} runs past its parent")
            if cid == b"LIST":
                walk(body + 4, body + size, data[body: body + 4] == b"movi")
            elif in_movi and cid == b"00dc":
                frames.append(data[body: body + size])
            p = body + size + (size & 1)
    walk(12, min(len(data), 8 + struct.unpack("<I", data[4:8])[0]), False)
    return frames


def read_mjpeg_avi(path, indices: Optional[List[int]] = None) -> np.ndarray:
    """-> uint8 [n, H, W, 3] RGB: all frames, or those at `indices` (indices past the end are skipped, as the reference skips a failed
    read)"""
    from PIL import Image
    chunks = mjpeg_avi_chunks(path)
    if not chunks:
        raise ValueError(f"{path}: no video frames (`00dc` chunks) found")
    pick = range(len(chunks)) if indices is None else [i for i in indices if 0 <= i < len(chunks)]
    return np.stack([np.asarray(Image.open(io.BytesIO(chunks[i])).convert("RGB")) for i in pick])


def sample_video_frames(video_path, num_samples: int = NUM_SAMPLES) -> np.ndarray:
    """t3_scene_evaluation.py:28-47 -> uint8 [n, H, W, 3]"""
    video_path = str(video_path)
    if video_path.lower().endswith(".avi"):
        n = len(mjpeg_avi_chunks(video_path))
        return read_mjpeg_avi(video_path, sample_indices(n, num_samples))
    try:
        import cv2
    except ImportError as e:
        raise RuntimeError(f"{video_path}: reading an H.264 .mp4 needs OpenCV (cv2), which is not installed; "
                           "write the videos as Motion-JPEG .avi instead") from e
    cap = cv2.VideoCapture(video_path)
    if not cap.isOpened():
        raise ValueError(f"Cannot open video: {video_path}")
    total = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
    out = []
    for idx in sample_indices(total, num_samples):
        cap.set(cv2.CAP_PROP_POS_FRAMES, idx)
        ret, frame = cap.read()
        if ret:
            out.append(cv2.cvtColor(frame, cv2.COLOR_BGR2RGB))
    cap.release()
    return np.stack(out)


def get_file_list_with_pair(folder_path) -> Dict[str, str]:
    """t3_scene_evaluation.py:50-77: prompt (first line of prompt.txt) -> video path; incomplete sequences are skipped with the
    reference's message.  Sequences are visited in sorted order; two sequences with the same prompt collapse into one entry, the later
    one, as in the reference.  Where a sequence holds both videos, gs.mp4 is taken when OpenCV can read it and gs.avi otherwise."""
    import importlib.util
    try:
        have_cv2 = importlib.util.find_spec("cv2") is not None
    except (ImportError, ValueError):   # a module table entry of None
        have_cv2 = False
    names = VIDEO_NAMES if have_cv2 else tuple(reversed(VIDEO_NAMES))
    pairs: Dict[str, str] = {}
    for sequence in sorted(os.listdir(folder_path)):
        seq = os.path.join(folder_path, sequence)
        if not os.path.isdir(seq):
            continue
        video = next((os.path.join(seq, n) for n in names if os.path.exists(os.path.join(seq, n))), None)
        prompt_file = os.path.join(seq, "prompt.txt")
        if video is None or not os.path.exists(prompt_file):
            print(f"Skipping {sequence}: missing gs.mp4 or prompt.txt")
            continue
        with open(prompt_file, "r") as f:
            prompt = f.readline().strip()
        pairs[prompt] = video
    return pairs


def evaluate_folder(folder_path, scorers: Dict[str, Callable[[np.ndarray, str], float]], eval_save_path=None) -> dict:
    """scorers: metric name -> f(frames uint8 [n,H,W,3], prompt) -> float.  -> the reference's JSON layout, holding the given metrics
    only; written to eval_save_path when given."""
    pairs = get_file_list_with_pair(folder_path)
    print(f"Found {len(pairs)} prompt-video pairs.")
    results = []
    for prompt, video in pairs.items():
        frames = sample_video_frames(video)
        row = {"prompt": prompt}
        for name, fn in scorers.items():
            row[name] = float(fn(frames, prompt))
        results.append(row)
    avg = {name: (float(np.mean([r[name] for r in results])) if results else float("nan")) for name in scorers}
    out = {"all_average": avg, "eval_results": results}
    if eval_save_path is not None:
        with open(eval_save_path, "w") as f:
            json.dump(out, f, indent=4)
        print(f"Results saved to {eval_save_path}")
    print(f"Average scores: {json.dumps(avg, indent=2)}")
    return out
