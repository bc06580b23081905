"""What every wrapper module shares: the dtypes, the stream and pointer of a call, the per-call workspace, and the one
validator of "contiguous device tensor of dtype D and shape S"."""
import ctypes as C
from typing import Optional

import torch

from .. import lib as L

bf16 = torch.bfloat16
f32 = torch.float32


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _workspace(need: int, what: str, device):
    """The per-call workspace of a loss / metric entry point from the answer of its *_workspace_bytes query: a negative answer is the
    query's error code and raises as `what`.  -> (float64 tensor, its size in bytes): 8-byte aligned by its dtype, never empty, the
    size rounded up to a multiple of 8.  Not cached: the buffer lives as long as the call's tensors do."""
    need = int(need)
    if need < 0:
        L.check(need, what)
    ws = torch.empty(max((need + 7) // 8, 1), device=device, dtype=torch.float64)
    return ws, ws.numel() * 8


def _tensor(t, name: str, dtypes, shape=None, numel: Optional[int] = None) -> None:
    """ValueError unless `t` is a contiguous device tensor of dtype `dtypes` (one, or a tuple of them) with, where given, exactly
    `shape` (None in it = any size: (None,) * d asks for d dimensions) and `numel` elements.  `name` opens the message."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    if (t.dtype in dtypes and t.is_contiguous() and (numel is None or t.numel() == numel)
            and (shape is None or (t.dim() == len(shape) and all(w is None or w == g for w, g in zip(shape, t.shape))))):
        return
    want = " or ".join(str(d).replace("torch.", "") for d in dtypes) + " device tensor"
    if shape is not None:
        want += f" of shape [{','.join('*' if w is None else str(w) for w in shape)}]"
    if numel is not None:
        want += f" of {numel} elements"
    raise ValueError(f"{name} must be a contiguous {want}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _f32_dev(t, name: str, shape=None, numel: Optional[int] = None) -> None:
    _tensor(t, name, f32, shape, numel)


def _i32_dev(t, name: str, shape=None, numel: Optional[int] = None) -> None:
    _tensor(t, name, torch.int32, shape, numel)
