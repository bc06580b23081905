"""Guard-band helper: tensors carved out of all-0xFF arenas, so that a kernel that reads or writes outside the view it was given is
OBSERVED (a NaN in its result, a changed guard byte) inside memory the test owns instead of passing unnoticed.

All-ones is NaN in bf16 / fp32 / fp64 / e4m3fn, -1 in int32 and 255 in uint8: one pattern poisons inputs and marks outputs.

    a = carve((M, K), torch.bfloat16, ld=K + 8)        # view [M, K] with row stride K + 8, guard bands before and after
    load(a, values)                                    # writes the valid region only
    ... run the kernel ...
    n, where = violations(out)                         # bytes outside out's valid region that are no longer 0xFF, first few (row, col)
    ok = unchanged(a, values)                          # inputs: valid region bit-equal to what was loaded, and no violations

Works on CPU tensors too (tests/test_guard_host.py checks the helper against itself).  A plain module: no fixture, no conftest."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

POISON = 0xFF
MIN_BAND_BYTES = 1 << 20     # never less than 1 MiB per band
BAND_ROWS = 256              # ... nor than one row-block of the largest GEMM tile (256 rows x ld)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _itemsize(dtype: torch.dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


class Arena:
    """One 1-D uint8 tensor, every byte 0xFF."""

    def __init__(self, nbytes: int, device="cpu"):
        self.buf = torch.full((int(nbytes),), POISON, dtype=torch.uint8, device=device)


@dataclass
class Region:
    """Where a carved view lies in its arena (byte units unless noted)."""
    arena: Arena
    start: int                 # offset of element [0, ..., 0] in the arena
    shape: tuple               # logical shape (elements)
    strides: tuple             # element strides, last one 1
    itemsize: int
    band: int                  # guaranteed guard bytes before `start` and after the last valid byte

    @property
    def ld(self) -> int:
        """row stride in elements (coordinates of a violation are relative to rows of this length)"""
        return self.strides[-2] if len(self.shape) >= 2 else max(self.shape[-1] if self.shape else 1, 1)

    @property
    def span(self) -> int:
        """bytes from the first to one past the last valid byte"""
        return (sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + 1) * self.itemsize


def carve(shape, dtype: torch.dtype, ld: Optional[int] = None, align: int = 256, offset_bytes: int = 0, *, device="cpu",
          strides: Optional[Sequence[int]] = None) -> torch.Tensor:
    """A view of `shape` inside an arena of its own, a guard band before and one after it.
    ld: row stride (elements) of a 2-D view, default = cols.  strides: full element strides for batched / N-D layouts (last must be 1);
    default contiguous.  The data pointer is `align`-aligned plus `offset_bytes`.  The Region is attached as `view.guard`."""
    shape = tuple(int(n) for n in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    if not shape:
        shape = (1,)
    if min(shape) < 1:
        raise ValueError("carve: empty shapes have no region to guard")
    isz = _itemsize(dtype)
    if strides is None:
        strides, acc = [], 1
        for n in reversed(shape):
            strides.append(acc)
            acc *= n
        strides = tuple(reversed(strides))
        if ld is not None:
            if len(shape) != 2 or ld < shape[1]:
                raise ValueError("carve: ld applies to 2-D views and must be >= cols")
            strides = (int(ld), 1)
    else:
        strides = tuple(int(s) for s in strides)
        if ld is not None or len(strides) != len(shape) or strides[-1] != 1:
            raise ValueError("carve: strides must match the shape, end in 1 and exclude ld")
    if align < 1 or offset_bytes < 0 or offset_bytes % isz:
        raise ValueError("carve: offset_bytes must be a non-negative multiple of the element size")
    row = strides[-2] if len(shape) >= 2 else shape[-1]
    band = max(BAND_ROWS * row * isz, MIN_BAND_BYTES)
    span = (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * isz
    arena = Arena(band + align + offset_bytes + span + band, device)
    base = arena.buf.data_ptr()
    start = (base + band + align - 1) // align * align + offset_bytes - base
    flat = arena.buf[start:start + span].view(dtype)
    view = flat.as_strided(shape, strides)
    view.guard = Region(arena, start, shape, strides, isz, band)
    return view


def _region(view: torch.Tensor) -> Region:
    g = getattr(view, "guard", None)
    if g is None:
        raise ValueError("not a carved view (pass the tensor that carve() returned, not a slice of it)")
    return g


def bits(t: torch.Tensor) -> torch.Tensor:
    """the tensor's storage bits as integers of its element size (NaN-safe equality)"""
    return t.detach().view(_BITS[t.element_size()])


def load(view: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """Write `values` into the valid region only (the strided copy touches no padding)."""
    _region(view)
    if tuple(values.shape) != tuple(view.shape):
        raise ValueError(f"load: values {tuple(values.shape)} do not fit the view {tuple(view.shape)}")
    if values.dtype != view.dtype:
        if values.element_size() != view.element_size():
            raise ValueError("load: dtype mismatch")
        values = values.view(view.dtype)
    view.copy_(values)
    return view


def violations(view: torch.Tensor, rows: Optional[torch.Tensor] = None, limit: int = 8):
    """(count, first few (row, col)): the bytes of the arena OUTSIDE the valid region that are no longer 0xFF.
    rows (2-D views): only these rows belong to the valid region (a row scatter's skipped rows are guard).
    Coordinates are relative to the region in elements: row = floor(byte offset / row pitch), col = the element within that pitch -
    so column `cols` of row r is (r, cols), row `rows` is (rows, 0), the byte before the region is (-1, ld - 1)."""
    g = _region(view)
    buf = g.arena.buf
    bad = buf != POISON
    bshape = g.shape[:-1] + (g.shape[-1] * g.itemsize,)
    bstr = tuple(s * g.itemsize for s in g.strides[:-1]) + (1,)
    valid = bad[g.start:g.start + g.span].as_strided(bshape, bstr)
    if rows is None:
        valid.fill_(False)
    else:
        if len(g.shape) != 2:
            raise ValueError("violations: rows applies to 2-D views")
        valid[rows.to(device=buf.device, dtype=torch.long)] = False
    n = int(bad.sum().item())
    where = []
    if n:
        pitch = g.ld * g.itemsize
        for off in bad.nonzero()[:limit, 0].tolist():
            rel = off - g.start
            r = math.floor(rel / pitch)
            where.append((r, (rel - r * pitch) // g.itemsize))
    return n, where


def unchanged(view: torch.Tensor, values: torch.Tensor) -> bool:
    """Inputs: the valid region is still bit-equal to what was loaded and nothing around it was written."""
    if values.dtype != view.dtype:
        values = values.view(view.dtype)
    return bool(torch.equal(bits(view), bits(values.to(view.device)))) and violations(view)[0] == 0


def carve_like(values: torch.Tensor, ld: Optional[int] = None, align: int = 256, offset_bytes: int = 0,
               strides: Optional[Sequence[int]] = None) -> torch.Tensor:
    """carve + load on the device of `values`"""
    return load(carve(values.shape, values.dtype, ld, align, offset_bytes, device=values.device, strides=strides), values)
