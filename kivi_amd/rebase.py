"""Rebase of a living KIVI cache: the first `drop` tokens of every row leave the cache, in place.

A layer cache has ONE length for all its rows and that length only grows; a batch that has served many short requests
(continuous batching) carries a length far beyond its live prompts, and every step and every admission pays
for the pads.  When the first `drop` tokens of EVERY row are pads (or belong to requests that are done), they can go: RoPE positions
come from the 2D mask, so dropping masked tokens changes no position.  A drop by a multiple of the QUANTUM, lcm(residual_length, 32),
keeps every K group (aligned to multiples of residual_length, quantised per channel over 32 tokens) and every 32-token block of the
matrix-pipe stores whole: codes, scales and zero points keep their bits, only the block they sit in changes.  The fp16 K residual
and the fp16 V window hold the newest tokens and stay where they are.

Here: the quantum, the check of a drop, and the launch of kivi_mf_store_shift for one packed store of the matrix-pipe layout; each
layout's part is `_rebase_buffers` next to its `_admit_slabs` (cache.py, cache_mf.py), the method is KiviCacheBase.rebase_.
"""
from __future__ import annotations

import math

import torch

from . import _lib

BLOCK_TOKENS = 32


def quantum(residual_length: int) -> int:
    """lcm(residual_length, 32): the drops that move whole K flushes and whole 32-token blocks."""
    return residual_length * BLOCK_TOKENS // math.gcd(residual_length, BLOCK_TOKENS)


def check_drop(drop, quant: int, limit: int, what: str = "rebase_") -> int:
    """ValueError unless `drop` is an int in [0, limit] and a multiple of `quant` (nothing runs on a device)."""
    if isinstance(drop, bool) or not isinstance(drop, int):
        raise ValueError(f"{what}: drop has to be an int (tokens to drop from the front of every row), got {drop!r}")
    if drop < 0:
        raise ValueError(f"{what}: drop={drop} is negative (0 .. rebase_limit = {limit})")
    if drop % quant:
        raise ValueError(f"{what}: drop={drop} is not a multiple of the rebase quantum {quant} (lcm of residual_length and the "
                         f"32-token block: anything else would re-quantise K groups)")
    if drop > limit:
        raise ValueError(f"{what}: drop={drop} lies above rebase_limit = {limit} (min of the packed K and V lengths: the fp16 "
                         f"residual and window stay where they are)")
    return drop


def shift_store(store: torch.Tensor, bits: int, is_k: bool, n_blocks: int, shift_blocks: int) -> None:
    """Blocks [shift_blocks, n_blocks) of a store of kivi_amd.quant.mfma.alloc_store -> blocks [0, n_blocks - shift_blocks), in
    place, the vacated blocks zeroed, the range words recomputed from the scales kept (kivi_mf_store_shift, one launch; the words
    are zeroed on the same stream first, as the entry point asks)."""
    from .quant import mfma
    if not 0 <= shift_blocks <= n_blocks <= store.shape[2] * mfma.SB_TOKENS // BLOCK_TOKENS:
        raise ValueError(f"shift_store: shift_blocks={shift_blocks}, n_blocks={n_blocks}, the store holds "
                         f"{store.shape[2] * mfma.SB_TOKENS // BLOCK_TOKENS} blocks")
    if shift_blocks == 0 or n_blocks == 0:
        return
    _lib.require_gpu(store, "store")
    st = mfma._st(store, bits)
    mfma.range_flags(store).zero_()
    _lib.check(_lib.load().kivi_mf_store_shift(*st, bits, int(is_k), store.shape[0], store.shape[1], n_blocks, shift_blocks,
                                               _lib.stream_ptr(store)), "kivi_mf_store_shift")


def moved_bytes(store: torch.Tensor, bits: int, n_blocks: int, shift_blocks: int) -> int:
    """Bytes read + written by shift_store (the algorithmic traffic: every kept block once each way, the vacated blocks written)."""
    block = (store.shape[3] - 2048) // 16 * 4 + 2 * 256
    return store.shape[0] * store.shape[1] * block * (2 * (n_blocks - shift_blocks) + min(shift_blocks, n_blocks))
