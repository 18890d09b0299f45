"""Checkpoint and exact rollback of a KIVI cache: the checkpoint objects and the call of kivi_cache_snapshot.

A decode or extend step at length F writes the packed K from k_quant_len on, the packed V from v_quant_len on, the fp16 K
residual, the fp16 V window, the range words and the six lengths -- nothing before the packed lengths.  So a checkpoint is the six
lengths, the fusion flags of the hook-state layout and ONE gather launch of what a step overwrites in place (the live residual
rows, the window, the range words: KiviCacheBase._checkpoint_slabs) into a buffer of its own; a restore is one scatter launch of
those bytes into the buffers as they are then, and the lengths.  Packed bytes beyond the restored lengths are dead: nothing reads
them, and the flushes that reach them again overwrite them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch

from . import _lib
from . import slabs as _slabs

LENGTHS = ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len")
FLAGS = ("_attend_unfusable", "_softmax_unfusable", "_fused_unsupported")


def row_bytes(slabs) -> int:
    """Bytes the slabs of one row take in a snapshot buffer (every slab starts on a 16-byte boundary)."""
    return sum(-(-_slabs.row_bytes(s) // 16) * 16 for s in slabs)


def run(slabs, B: int, buf: torch.Tensor, direction: int) -> None:
    """One kivi_cache_snapshot launch: gather the slabs of every row into `buf` (B, row bytes) uint8 (direction 0) or scatter them
    back (1)."""
    arrs = _slabs.arrays(slabs)
    assert len(arrs) <= 1
    for arr in arrs:
        _lib.check(_lib.load().kivi_cache_snapshot(arr, len(arr), B, _lib.ptr(buf), buf.stride(0), direction, _lib.stream_ptr(buf)),
                   "kivi_cache_snapshot")


@dataclass
class KiviCheckpoint:
    """What KiviCacheBase.checkpoint() returns: host copies of the six lengths and the fusion flags, and a buffer of its own with the
    bytes a step overwrites in place.  It holds no view into the cache and stays valid when the cache grows (reserve)."""
    geometry: tuple              # layout class, B, nh_kv, D, bits, group, residual: what restore_ compares
    owner: object                # token of the cache that issued it
    serial: int                  # the cache's count of checkpoints when this one was taken (restore_: staleness)
    state: Tuple[int, ...]       # LENGTHS
    flags: Tuple[bool, ...]      # FLAGS
    buf: torch.Tensor            # (B, row bytes) uint8

    @property
    def kv_seq_len(self) -> int:
        return self.state[5]

    def nbytes(self) -> int:
        """Device bytes this checkpoint holds."""
        return self.buf.numel()


@dataclass
class KiviModelCheckpoint:
    """LlamaForCausalLM_KIVI.checkpoint(): one KiviCheckpoint per layer and the kv length they were taken at."""
    layers: List[KiviCheckpoint]
    kv_seq_len: int

    def nbytes(self) -> int:
        return sum(c.nbytes() for c in self.layers)
