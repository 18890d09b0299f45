"""In-place row reorder of a KIVI cache (beam search): the slab lists of both layouts and the call of kivi_cache_reorder.

The reference reorders its 9-tuples with index_select (models/llama_kivi.py:951-957), a copy of the whole cache on every step.
Here beams of one request share every byte written before the fork point (rows are computed independently, DESIGN.md section
11), so a step only moves what was written after it: the K quantisation groups that hold a token >= from_token, the V tokens
from from_token on, the fp16 K residual, the V window and the range words.  Each store contributes slabs (include/kivi_hip.h,
kivi_reorder_slab) restricted to those bytes; moving a few bytes more than that (alignment) is harmless, it is what a whole-row
copy would write.
"""
from __future__ import annotations

import torch

from . import _lib
from . import slabs as _slabs


def _span(lo: int, hi: int, size: int):
    """Byte range [lo, hi) of a container of `size` bytes, widened to 16-byte (or 4-byte) boundaries inside the container."""
    al = 16 if size % 16 == 0 else 4
    if size % al:
        raise ValueError(f"a cache store row of {size} bytes is not word aligned")
    return lo // al * al, min(size, -(-hi // al) * al)


def slab(t: torch.Tensor, offset: int, levels, run: int):
    """A slab of tensor `t`: byte `offset` from its data pointer, levels [(count, byte stride)] (at most three), `run` bytes."""
    levels = list(levels) + [(1, 0)] * (3 - len(levels))
    return (t.data_ptr() + offset, t.stride(0) * t.element_size(), levels, run)


def check_idx(idx: torch.Tensor, B: int, group: int, device, check_values: bool = True) -> torch.Tensor:
    """Validate a reorder index (raises ValueError) and return it as a contiguous int32 / int64 device tensor."""
    if not torch.is_tensor(idx):
        idx = torch.as_tensor(idx, device=device)
    if idx.dim() != 1 or idx.shape[0] != B:
        raise ValueError(f"reorder index must have shape ({B},), got {tuple(idx.shape)}")
    if idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"reorder index must be int32 or int64, got {idx.dtype}")
    if group < 1 or B % group or group > _lib.REORDER_MAX_GROUP:
        raise ValueError(f"group={group}: it must divide the batch ({B}) and be at most {_lib.REORDER_MAX_GROUP}")
    idx = idx.to(device).contiguous()
    if check_values:
        own = torch.arange(B, device=device) // group
        if not bool(((idx >= 0) & (idx < B) & (idx.div(group, rounding_mode="floor") == own)).all()):
            raise ValueError(f"reorder index out of range: every idx[b] must lie in b's group of {group} rows")
    return idx


def run(slabs, B: int, group: int, idx: torch.Tensor) -> None:
    """One kivi_cache_reorder call per KIVI_REORDER_MAX_SLABS slabs (they are disjoint, so the calls are independent)."""
    for arr in _slabs.arrays(slabs):
        _lib.check(_lib.load().kivi_cache_reorder(arr, len(arr), B, group, _lib.ptr(idx), idx.element_size(), _lib.stream_ptr(idx)),
                   "kivi_cache_reorder")


def moved_bytes(slabs, rows: int) -> int:
    """Bytes read + written when `rows` rows move (the algorithmic traffic of a reorder)."""
    return 2 * rows * sum(map(_slabs.row_bytes, slabs))
