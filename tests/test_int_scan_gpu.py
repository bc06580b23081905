"""Pins the contract of csrc/int_scan.h - block_exclusive_scan over 256 lanes, block_totals_to_prefix over the blocks' totals, 256
blocks per round with a carry - through its two users: ops.splat_export_filter (the survivors' row list and count) and
ops.densify_classify (three offset arrays and their totals).  Integers only, so every judgment is equality.

Sizes: U = 1 (one lane), 255 / 256 / 257 (one block short of, exactly, and one row past a block), 65 536 (exactly 256 blocks: one
full round of the second stage, no carry), 65 537 (257 blocks: the second round has one live lane, and its one row sits right
after the carry), 70 001 (274 blocks, the last one ragged).

The export keep patterns are random (60 % kept) with these structures forced in where U has the blocks for them:
  three blocks or more   block 0 entirely kept (a block total of 256), block 1 entirely dropped (a total of 0)
  U > 65 792             block 256, the first of the second round (rows 65 536 .. 65 791), entirely dropped
  a last block of >= 2   mixed: its last row kept (the end of the list), the row before it dropped
  a last block of 1 row  kept: at 257 and 65 537 its place in the list is the whole carry
U = 1 cannot hold both outcomes in one pattern and runs twice, its row kept and its row dropped.  The fates, counts and thresholds
of the classify inputs are judged by tests/test_densify_gpu.py; here only offsets and totals against the counts."""
import functools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_densify_gpu import TH, scene  # noqa: E402

THREADS = 256
ROUND = THREADS * THREADS           # rows that one round of block_totals_to_prefix holds
SIZES = [1, 255, 256, 257, 65_536, 65_537, 70_001]
PATTERNS = [(1, True), (1, False)] + [(U, True) for U in SIZES[1:]]     # (U, what a one-row last block gets)
pattern_id = lambda p: f"{p[0]}" + ("" if p[0] > 1 else "-kept" if p[1] else "-dropped")


def forced(U):
    """the forced structures U has room for -> dict(kept=block or None, dropped=[blocks], last=(first row, rows))"""
    nb = (U + THREADS - 1) // THREADS
    first = (nb - 1) * THREADS
    return dict(kept=0 if nb >= 3 else None, dropped=([1] if nb >= 3 else []) + ([THREADS] if U > ROUND + THREADS else []),
                last=(first, U - first))


@functools.lru_cache(maxsize=None)
def keep_pattern(U, lone=True):
    keep = torch.rand(U, generator=torch.Generator().manual_seed(4000 + U)) < 0.6
    f = forced(U)
    if f["kept"] is not None:
        keep[f["kept"] * THREADS:(f["kept"] + 1) * THREADS] = True
    for b in f["dropped"]:
        keep[b * THREADS:(b + 1) * THREADS] = False
    if f["last"][1] >= 2:
        keep[U - 1], keep[U - 2] = True, False
    else:
        keep[U - 1] = lone
    return keep


def scene_nonfinite(keep):
    """K = 0; a dropped row has one nan / inf / -inf, in means, scales, quats, opacities, sh in rotation"""
    U = keep.shape[0]
    g = torch.Generator().manual_seed(7)
    s = dict(means=torch.randn(U, 3, generator=g), scales=torch.randn(U, 3, generator=g) - 3, quats=torch.randn(U, 4, generator=g),
             opacities=torch.randn(U, generator=g), sh=torch.randn(U, 3, 1, generator=g))
    bad = (float("nan"), float("inf"), float("-inf"))
    for n, i in enumerate(torch.nonzero(~keep).flatten().tolist()):
        t = s[("means", "scales", "quats", "opacities", "sh")[i % 5]]
        t[i].view(-1)[n % t[i].numel()] = bad[n % 3]
    return s, None


def scene_opacity(keep):
    """K = 0, everything finite; logits of exactly +-4 (sigmoid 0.982 / 0.018) against a threshold of 0.5"""
    s, _ = scene_nonfinite(torch.ones_like(keep))
    s["opacities"] = torch.where(keep, 4.0, -4.0)
    return s, 0.5


def test_patterns_hold_the_forced_structures():
    """without this the GPU tests could pass on patterns that never fill or empty a block"""
    assert [bool(keep_pattern(1, lone)[0]) for _, lone in PATTERNS[:2]] == [True, False]
    seen = dict(kept=0, dropped=0, second_round=0, mixed=0)
    for U, lone in PATTERNS[2:]:
        keep, f = keep_pattern(U, lone), forced(U)
        blocks = keep.split(THREADS)
        assert 0.1 * U <= int(keep.sum()) <= 0.9 * U, (U, int(keep.sum()))
        if f["kept"] is not None:
            assert bool(blocks[f["kept"]].all()) and blocks[f["kept"]].numel() == THREADS
            seen["kept"] += 1
        for b in f["dropped"]:
            assert not bool(blocks[b].any()) and blocks[b].numel() == THREADS and b != len(blocks) - 1
            seen["dropped"] += 1
            seen["second_round"] += b == THREADS
        last = blocks[-1]
        assert last.numel() == f["last"][1] and bool(last[-1])
        if last.numel() >= 2:
            assert not bool(last.all())
            seen["mixed"] += 1
    # which sizes carry what: 65 536, 65 537 and 70 001 have three blocks or more, 70 001 alone reaches past block 256
    assert seen == dict(kept=3, dropped=4, second_round=1, mixed=4), seen
    assert [forced(U)["last"][1] for U in SIZES] == [1, 255, 256, 1, 256, 1, 113]
    # the two realisations drop exactly the pattern's rows, the first through every one of the five tensors
    keep = keep_pattern(257)
    s, _ = scene_nonfinite(keep)
    per_tensor = torch.stack([t.reshape(257, -1).isfinite().all(1) for t in s.values()])
    assert torch.equal(per_tensor.all(0), keep) and not bool(per_tensor.all(1).any())
    s, threshold = scene_opacity(keep)
    assert torch.equal(torch.sigmoid(s["opacities"]) > threshold, keep) and all(bool(t.isfinite().all()) for t in s.values())


@pytest.mark.gpu
@pytest.mark.parametrize("realise", [scene_nonfinite, scene_opacity], ids=["nonfinite", "opacity"])
@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
def test_export_filter_lists_the_kept_rows_in_order(hip_lib, pattern, realise):
    from vist3a_amd import ops
    keep = keep_pattern(*pattern)
    s, threshold = realise(keep)
    s = {k: t.cuda() for k, t in s.items()}
    want = torch.nonzero(keep).flatten().to(torch.int32)
    runs = []
    for _ in range(2):
        rows, count = ops.splat_export_filter(s, quats_xyzw=False, opacity_threshold=threshold)
        n = int(count.item())
        runs.append((n, rows[:n].cpu()))       # rows past the count are not written
    print(f"[int_scan export U={keep.shape[0]}] count {runs[0][0]} want {want.shape[0]}")
    assert runs[0][0] == int(keep.sum())
    assert runs[0][1].dtype == torch.int32 and torch.equal(runs[0][1], want)
    assert runs[1][0] == runs[0][0] and torch.equal(runs[1][1], runs[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("U", SIZES)
def test_classify_offsets_are_the_exclusive_prefix_of_its_counts(hip_lib, U):
    from vist3a_amd import ops
    grad, count, p, _, _ = scene(U, 1)
    c = ops.densify_classify(torch.from_numpy(grad).cuda(), torch.from_numpy(count).cuda(), torch.from_numpy(p["scales"]).cuda(),
                             torch.from_numpy(p["opacities"]).cuda(), prune_big=True, **TH)
    fates, counts, offsets, totals = (c[k].cpu() for k in ("fates", "counts", "offsets", "totals"))
    if U >= 5:     # the scene's first five rows: keep, clone, split, split with oversized children, oversized keep
        assert set((fates & 3).tolist()) == {0, 1, 2} and bool((fates & 4).any()) and not bool((fates & 4).all())
    counts = counts.long()
    print(f"[int_scan classify U={U}] totals {totals.tolist()}")
    for s in range(3):
        assert torch.equal(offsets[s].long(), counts[s].cumsum(0) - counts[s]), s
        assert int(totals[s]) == int(counts[s].sum()), s
