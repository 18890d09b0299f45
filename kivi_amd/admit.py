"""Admission of new requests into rows of a living KIVI cache (continuous batching): the admit slabs and the
call of kivi_cache_admit.

A layer cache has ONE length for all its rows, so a prompt admitted at length L is the prompt left-padded to L and run as an
ordinary prompt pass of its own (pads are masked cache tokens); what is left to do is to put the rows of that
temporary cache into chosen rows of the living one without touching any other row, buffer address or length.  Source and
destination are different allocations, their capacities (hence strides) may differ and their fp16 V windows sit at different
offsets, so a slab (include/kivi_hip.h, kivi_admit_slab) names both sides; each layout lists them in `_admit_slabs(src)`.

Admission at an offset: the prompt pass runs at a SHORT length and its packed stores land `offset` tokens
further up in the rows, the blocks below zeroed -- `check_offset`, and `admit_store`, the call of kivi_mf_store_admit for one packed
store of the matrix-pipe layout; each layout's part is `_admit_offset`.
"""
from __future__ import annotations

import torch

from . import _lib
from . import slabs as _slabs


def slab(dst: torch.Tensor, dst_off: int, src: torch.Tensor, src_off: int, levels, run: int):
    """An admit slab from tensor `src` (byte `src_off` from its data pointer) to tensor `dst` (byte `dst_off`): levels
    [(count, destination byte stride, source byte stride)] (at most three), `run` bytes.
    -> (dst base, dst row stride, [dst strides], src base, src row stride, [src strides], [counts], run)."""
    levels = list(levels) + [(1, 0, 0)] * (3 - len(levels))
    return (dst.data_ptr() + dst_off, dst.stride(0) * dst.element_size(), [d for _, d, _ in levels],
            src.data_ptr() + src_off, src.stride(0) * src.element_size(), [s for _, _, s in levels],
            [n for n, _, _ in levels], run)


def rows_tensor(rows) -> torch.Tensor:
    """The destination rows as a 1-D int32 / int64 tensor (where they are): ValueError for anything else."""
    if not torch.is_tensor(rows):
        try:
            rows = torch.as_tensor(list(rows))
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"rows must be a 1-D int32 or int64 tensor or a sequence of row indices, got {rows!r}") from None
        if rows.numel() == 0:
            rows = rows.long()
    if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"rows must be a 1-D int32 or int64 tensor or a sequence of row indices, got {tuple(rows.shape)} {rows.dtype}")
    return rows


def check_rows(rows, n: int, B: int, device, check_values: bool = True) -> torch.Tensor:
    """Validate the destination rows of an admission (raises ValueError) and return them as a contiguous int32 / int64 tensor on
    `device`: `n` distinct rows in [0, B).  `check_values=False` skips the look at the values (a device read): the kernel leaves a
    source row whose index lies outside [0, B) unused."""
    rows = rows_tensor(rows)
    if rows.shape[0] != n:
        raise ValueError(f"{rows.shape[0]} rows were named for {n} rows to admit")
    if not 1 <= n <= B:
        raise ValueError(f"{n} rows cannot be admitted into a cache of {B} rows")
    rows = rows.to(device).contiguous()
    if check_values:
        if not bool(((rows >= 0) & (rows < B)).all()):
            raise ValueError(f"rows out of range: every row must lie in [0, {B}), got {rows.tolist()}")
        if torch.unique(rows).numel() != n:
            raise ValueError(f"duplicate rows: {rows.tolist()} (every destination row takes one source row)")
    return rows


live = _slabs.live


def run(slabs, rows: torch.Tensor, B: int) -> None:
    """One kivi_cache_admit call per KIVI_REORDER_MAX_SLABS slabs (their destinations are disjoint, so the calls are independent)."""
    for arr in _slabs.arrays(slabs):
        _lib.check(_lib.load().kivi_cache_admit(arr, len(arr), rows.shape[0], _lib.ptr(rows), rows.element_size(), B,
                                                _lib.stream_ptr(rows)), "kivi_cache_admit")


def moved_bytes(slabs, rows: int) -> int:
    """Bytes read + written when `rows` rows are admitted (the algorithmic traffic of an admission)."""
    return 2 * rows * sum(map(_slabs.row_bytes, slabs))


# ---------------------------------------------------------------------- admission at an offset
BLOCK_TOKENS = 32


def check_offset(offset, quant: int, L: int, R: int, what: str = "admit_") -> int:
    """ValueError unless `offset` is an int >= 0, a multiple of `quant` (rebase_quantum) that leaves a source of at least R tokens
    below the living length L (nothing runs on a device)."""
    if isinstance(offset, bool) or not isinstance(offset, int):
        raise ValueError(f"{what}: offset has to be an int (tokens of masked zero blocks in front of the admitted prompt), got {offset!r}")
    if offset < 0:
        raise ValueError(f"{what}: offset={offset} is negative")
    if offset % quant:
        raise ValueError(f"{what}: offset={offset} is not a multiple of the rebase quantum {quant} (lcm of residual_length and the "
                         f"32-token block: anything else would re-quantise K groups)")
    if offset and L - offset < R:
        raise ValueError(f"{what}: offset={offset} leaves {L - offset} of the living caches' {L} tokens for the prompt pass, below "
                         f"residual_length = {R} (the fp16 residual and window stay where they are)")
    return offset


def admit_store(dst: torch.Tensor, src: torch.Tensor, rows: torch.Tensor, bits: int, is_k: bool, n_blocks: int,
                shift_blocks: int) -> None:
    """Blocks [0, n_blocks) of every row i of `src` (a store of kivi_amd.quant.mfma.alloc_store) -> blocks [shift_blocks, shift_blocks +
    n_blocks) of row rows[i] of `dst`, blocks [0, shift_blocks) of those rows zeroed, their range words replaced by the source's
    (kivi_mf_store_admit, one launch).  `rows`: a 1-D int32 / int64 tensor on the stores' device, read there."""
    from .quant import mfma
    room = dst.shape[2] * mfma.SB_TOKENS // BLOCK_TOKENS
    if not (0 <= shift_blocks and 0 <= n_blocks <= src.shape[2] * mfma.SB_TOKENS // BLOCK_TOKENS and n_blocks + shift_blocks <= room):
        raise ValueError(f"admit_store: shift_blocks={shift_blocks}, n_blocks={n_blocks}: the source holds "
                         f"{src.shape[2] * mfma.SB_TOKENS // BLOCK_TOKENS} blocks, the destination {room}")
    if rows.shape[0] > src.shape[0] or src.shape[1] != dst.shape[1]:
        raise ValueError(f"admit_store: {rows.shape[0]} rows of a source of shape {tuple(src.shape)} into {tuple(dst.shape)}")
    if n_blocks == 0 and shift_blocks == 0:
        return
    _lib.require_gpu(dst, "dst")
    _lib.require_gpu(src, "src")
    _lib.check(_lib.load().kivi_mf_store_admit(*mfma._st(dst, bits), *mfma._st(src, bits), bits, int(is_k), rows.shape[0], _lib.ptr(rows),
                                               rows.element_size(), dst.shape[0], dst.shape[1], n_blocks, shift_blocks,
                                               _lib.stream_ptr(dst)), "kivi_mf_store_admit")


def store_moved_bytes(store: torch.Tensor, rows: int, n_blocks: int, shift_blocks: int) -> int:
    """Bytes read + written by admit_store for `rows` rows (the algorithmic traffic: every source block read, every destination
    block written, the zeroed lead included; the range words are not counted)."""
    block = (store.shape[3] - 2048) // 16 * 4 + 2 * 256
    return rows * store.shape[1] * block * (2 * n_blocks + shift_blocks)
