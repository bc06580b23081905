"""The guard-band helper (tests/guard.py) checked against itself on CPU tensors: carve geometry and alignment, and a one-element
overrun in each of the three directions reported at the right coordinate."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))
import guard as G  # noqa: E402

DTYPES = [torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int32, torch.float8_e4m3fn]


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_all_ones_poisons_every_dtype(dtype):
    v = G.carve((3, 5), dtype, ld=8)
    if dtype.is_floating_point:
        assert v.float().isnan().all()
    else:
        assert (v == (255 if dtype == torch.uint8 else -1)).all()


@pytest.mark.parametrize("shape,dtype,ld,align,off", [
    ((7, 24), torch.bfloat16, 32, 256, 0),
    ((7, 24), torch.bfloat16, 32, 256, 16),      # the smallest alignment a `% 8 bf16 elements` ABI accepts
    ((1, 8), torch.float32, None, 64, 4),
    ((300, 5000), torch.float32, 5008, 256, 0),  # 256 rows x ld x 4 bytes > 1 MiB: the band follows the row pitch
    ((13,), torch.int32, None, 256, 0),
    ((2, 3, 4, 8), torch.bfloat16, None, 256, 0),
])
def test_carve_geometry_and_alignment(shape, dtype, ld, align, off):
    v = G.carve(shape, dtype, ld, align, off)
    g = v.guard
    isz = v.element_size()
    assert tuple(v.shape) == shape and v.dtype == dtype and v.stride(-1) == 1
    if len(shape) == 2:
        assert v.stride(0) == (ld or shape[1])
    else:
        assert v.is_contiguous()
    assert (v.data_ptr() - off) % align == 0 and v.data_ptr() == g.arena.buf.data_ptr() + g.start
    row_pitch = (v.stride(-2) if v.dim() >= 2 else shape[-1]) * isz
    want_band = max(256 * row_pitch, 1 << 20)
    assert g.band == want_band
    assert g.start >= want_band and g.arena.buf.numel() - (g.start + g.span) >= want_band
    last = sum((n - 1) * s for n, s in zip(v.shape, v.stride()))
    assert g.span == (last + 1) * isz
    assert bool((g.arena.buf == 0xFF).all())
    assert G.violations(v) == (0, [])                       # an untouched arena reports zero


def test_batched_strides_larger_than_the_problem():
    v = G.carve((3, 5, 16), torch.bfloat16, strides=(5 * 24 + 40, 24, 1))
    vals = torch.randn(3, 5, 16).to(torch.bfloat16)
    G.load(v, vals)
    assert G.unchanged(v, vals)
    flat = v.guard.arena.buf[v.guard.start:].view(torch.bfloat16)
    flat[1 * 160 + 5 * 24] = 1.0                            # "row 5" of batch item 1: between two problems
    n, where = G.violations(v)
    assert n == 2 and where[0] == ((160 + 120) // 24, (160 + 120) % 24)


def test_load_writes_the_valid_region_only_and_unchanged_sees_a_flipped_bit():
    v = G.carve((5, 24), torch.bfloat16, ld=40)
    vals = torch.randn(5, 24).to(torch.bfloat16)
    vals[2, 3] = float("nan")                               # bit comparison: a NaN the test itself loaded is not a change
    G.load(v, vals)
    assert G.violations(v) == (0, []) and G.unchanged(v, vals)
    v[4, 23] = -v[4, 23]
    assert not G.unchanged(v, vals) and G.violations(v)[0] == 0


def _elems(v):
    """the arena from the region's first element on, in the view's element type"""
    g = v.guard
    return g.arena.buf[g.start:].view(v.dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8], ids=["bf16", "f32", "u8"])
def test_one_element_overruns_are_reported_where_they_happen(dtype):
    M, N, ld = 5, 24, 40
    isz = torch.empty((), dtype=dtype).element_size()
    # one element past the last column (of row 2)
    v = G.carve((M, N), dtype, ld=ld)
    v.as_strided((M, N + 1), (ld, 1))[2, N] = 1
    n, where = G.violations(v)
    assert n == isz and where[0] == (2, N), (n, where)     # fp32 1.0 = 00 00 80 3f: every changed byte differs from 0xFF
    # one row past the last row (its first element)
    v = G.carve((M, N), dtype, ld=ld)
    v.as_strided((M + 1, N), (ld, 1))[M, 0] = 1
    n, where = G.violations(v)
    assert n == isz and where[0] == (M, 0), (n, where)
    # one byte before the region
    v = G.carve((M, N), dtype, ld=ld)
    v.guard.arena.buf[v.guard.start - 1] = 0
    n, where = G.violations(v)
    assert n == 1 and where == [(-1, ld - 1)], (n, where)
    # the same overruns with a tight row stride: past the last column IS the next row's first element, which is valid memory of the
    # view - only the last row's overrun leaves the region
    v = G.carve((M, N), dtype)
    _elems(v)[M * N] = 1
    assert G.violations(v)[1][0] == (M, 0)


def test_row_scatter_makes_skipped_rows_guard():
    v = G.carve((8, 16), torch.float32, ld=24)
    rows = torch.tensor([0, 1, 4, 5])
    v[rows] = 0.0
    assert G.violations(v, rows=rows) == (0, [])
    v[2, 7] = 0.0
    n, where = G.violations(v, rows=rows)
    assert n == 4 and where[0] == (2, 7)
    assert G.violations(v)[0] == 0                          # ... and valid again once the whole view is


def test_carve_rejects_what_it_cannot_guard():
    with pytest.raises(ValueError):
        G.carve((4, 8), torch.float32, ld=7)
    with pytest.raises(ValueError):
        G.carve((4, 8), torch.float32, offset_bytes=2)
    with pytest.raises(ValueError):
        G.violations(torch.zeros(4))
    with pytest.raises(ValueError):
        G.load(G.carve((4, 8), torch.float32), torch.zeros(4, 9))
