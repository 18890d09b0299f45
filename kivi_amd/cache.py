"""Per-layer KIVI KV-cache state: the reference's 9-tuple, held in pre-allocated, in-place-appended buffers.

Reference contract (models/llama_kivi.py:454-455, read back at :315-322):
    (K_code_T, K_full, K_scale_T, K_mn_T, V_code, V_full, V_scale, V_mn, kv_seq_len)
      K_code_T (B, nh_kv, D, Tq/fpi) int32     K_scale_T, K_mn_T (B, nh_kv, D, Tq/g) fp16
      K_full   (B, nh_kv, 0..R-1, D) fp16 or None
      V_code   (B, nh_kv, Tv, D/fpi) int32     V_scale, V_mn (B, nh_kv, Tv, D/g) fp16
      V_full   (B, nh_kv, <=R, D) fp16
The reference grows every member with torch.cat -- packed V + scale + mn are re-copied EVERY step
(llama_kivi.py:393-395), packed K every R steps (:350-352).  Here a decode step moves only the new token(s):

  * V (per token) is stored exactly in the reference layout with spare rows at the end; appending a token
    writes one row and the 9-tuple members are plain views.
  * K (per channel) cannot be appended in the reference layout without striding every channel row by the
    capacity, which costs ~35 % of HBM efficiency on MI355X (profiles/).  It is stored in PAGES of
    `page_tokens` tokens, each page a contiguous (D, page_tokens/fpi) block = the reference layout of that token
    range; the fused GEMV reads pages directly (kivi_gemv_k_paged).  The reference-layout K members of the
    9-tuple are materialised (one copy) only if somebody actually indexes them.

Cache policy (llama_kivi.py:343-356, 386-399, 425-452):
  K: residual grows; when it holds exactly R tokens all R are quantised at once (per channel, groups of g tokens).
  V: sliding fp16 window of R tokens; when it holds R+1 the OLDEST token is quantised (per token, groups of g channels).
"""
from __future__ import annotations

import copy
import ctypes
import math
import warnings
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib, _tuning, admit, checkpoint, rebase, reorder
from ._lib import KiviUnsupported, check_mask_size, mask_arg, out_arg, unit_rows
from .quant import fused, matmul, new_pack

PAGE_TOKENS = 2048   # = the tile of the default qK^T kernels (64 lanes x 2 words x 16 codes; 4-bit: 4 words x 8)


class KiviCacheTuple(tuple):
    """The reference's 9-tuple.  `t[-1]` / `t[8]` (running kv length, what HF's generate loop reads,
    llama_kivi.py:698, :916) is free; tensor members are built from the live cache on first access."""

    def __new__(cls, layer: "KiviLayerCache"):
        t = super().__new__(cls, (None,) * 8 + (layer.kv_seq_len,))
        t.layer = layer
        t._items = None
        return t

    def _materialise(self):
        if self._items is None:
            n = tuple.__getitem__(self, 8)
            if self.layer.kv_seq_len != n:
                raise RuntimeError(f"stale KIVI cache tuple: issued at kv length {n}, the in-place cache is now at "
                                   f"{self.layer.kv_seq_len}; index the members before the next decode step (or clone the cache)")
            self._items = self.layer._tuple_members() + (n,)
        return self._items

    def __getitem__(self, i):
        if isinstance(i, int) and i in (8, -1):
            return tuple.__getitem__(self, 8)
        return self._materialise()[i]

    def __iter__(self):
        return iter(self._materialise())


@dataclass
class KiviConfig:
    k_bits: int = 2
    v_bits: int = 2
    group_size: int = 32
    residual_length: int = 32

    def __post_init__(self):
        assert self.k_bits in (2, 4) and self.v_bits in (2, 4), "the fused GEMV supports 2 and 4 bits (matmul.py:215)"
        assert self.residual_length % self.group_size == 0  # llama_kivi.py:344


_FUSION_ENV = _tuning.knob("KIVI_DECODE_FUSION")   # tuning sessions: "attend" (2 launches), "softmax" (3), "separate" (4)


def _fusion_level() -> int:
    """How much of the decode step goes into the sV launch: 2 = everything after the packed qK^T (kivi_decode_attend),
    1 = softmax + output, 0 = output only (softmax as its own launch).  Level 2 covers every tuned shape: for short
    MHA rows the block that owns a row does the row's softmax before it starts streaming; for grouped queries / long
    rows the library splits rows over blocks and adds a row-statistics launch (kivi_gemv_v.hip, v_run)."""
    if _FUSION_ENV:
        return {"attend": 2, "softmax": 1, "separate": 0}[_FUSION_ENV]
    return 2


_HOOK = None


def _hook():
    """kivi_amd.attention (which imports this module): KIVI_NATIVE_STEP lives there as `_NATIVE_STEP`, and tests switch it between
    two steps, so it is read at every step."""
    global _HOOK
    if _HOOK is None:
        from . import attention
        _HOOK = attention
    return _HOOK


class KiviPerformanceWarning(UserWarning):
    """A decode step left the fused kernels for a slower composition (results unchanged)."""


class KiviCacheBase:
    """What the two layouts of a layer's cache (KiviLayerCache here, KiviLayerCacheMF in cache_mf.py) share: the geometry, the six
    lengths of the state machine, the scratch of a decode step, and everything that follows from them alone.  A layout adds its
    buffers (`_BUFFERS`, `reserve`, `_own_buffers`, `_reorder_slabs`, `_checkpoint_slabs`, `_admit_slabs`, `_admit_offset`, `_rebase_buffers`, `prefill`), the readers of the reference layout
    (`k_quant_reference_layout`, `v_quant_views`, `v_res_view`) and its steps (`decode_step`, `extend`)."""

    def __init__(self, cfg: KiviConfig, batch: int, num_kv_heads: int, head_dim: int, max_len: int, dtype):
        assert dtype == torch.float16, "the reference extension is fp16 only (gemv_cuda.cu:526-529)"
        self.cfg = cfg
        R = cfg.residual_length
        self.B, self.nh_kv, self.D = batch, num_kv_heads, head_dim
        self.cap = ((max_len + R - 1) // R) * R
        self.k_quant_len = 0   # tokens in the packed K prefix (multiple of R)
        self.k_res_len = 0     # tokens in the fp16 K residual (< R between steps)
        self.v_quant_len = 0   # tokens in the packed V prefix
        self.v_res_start = 0
        self.v_res_len = 0     # tokens in the fp16 V window (<= R between steps)
        self.kv_seq_len = 0
        self._native = None    # (descriptor, int64[6] state array, key, entry point, scratch) of the layout's one-call step
        self._scores = self._probs = None     # (B, nh, 1, pitch) fp16 scratch rows of the multi-launch forms (hook-state layout)
        # fusion levels this cache has left for good (hook-state layout: KiviLayerCache._drop_fusion)
        self._attend_unfusable = self._softmax_unfusable = self._fused_unsupported = False
        self._forget_checkpoints()

    def _invalidate(self) -> None:
        """Forget the native descriptor and the scratch rows: they point into / are sized for buffers that have just been replaced."""
        self._native = self._scores = self._probs = None

    # ------------------------------------------------------------------ the six lengths <-> the int64[6] state array of the library
    def _store_state(self, state) -> None:
        state[0], state[1], state[2], state[3], state[4], state[5] = (
            self.k_quant_len, self.k_res_len, self.v_quant_len, self.v_res_start, self.v_res_len, self.kv_seq_len)

    def _load_state(self, state) -> None:
        self.k_quant_len, self.k_res_len, self.v_quant_len, self.v_res_start, self.v_res_len, self.kv_seq_len = (
            state[0], state[1], state[2], state[3], state[4], state[5])

    # ------------------------------------------------------------------ capacity, copies
    def ensure_room(self, tokens: int = 1) -> None:
        """Make room for `tokens` more tokens, doubling the capacity when it runs out (amortised O(1) copies)."""
        need = self.kv_seq_len + tokens
        if need > self.cap:
            self.reserve(max(need, 2 * self.cap))

    def clone(self):
        """Independent copy of the cache (what holding on to an old reference tuple gives for free): use it to continue one
        prefix twice (beam / contrastive / assisted decoding)."""
        other = copy.copy(self)
        other._own_buffers(None)
        other._invalidate()
        other._forget_checkpoints()
        return other

    def index_select(self, idx):
        """A new cache of len(idx) rows, row i a bit-identical copy of row idx[i] (whole rows): the fork of B requests into
        B * num_beams beams."""
        idx = torch.as_tensor(idx, device=self.k_res.device).long().flatten()
        if idx.numel() == 0 or not bool(((idx >= 0) & (idx < self.B)).all()):
            raise ValueError(f"index_select: indices must lie in [0, {self.B})")
        other = copy.copy(self)
        other.B = idx.numel()
        other._own_buffers(idx)
        other._invalidate()
        other._forget_checkpoints()
        return other

    # ------------------------------------------------------------------ beam search
    def reorder_(self, idx, group: Optional[int] = None, from_token: int = 0, check: bool = True):
        """row[b] <- row[idx[b]] in place (one kivi_cache_reorder launch): `idx` (B,) int32 / int64, idx[b] in b's group of `group`
        consecutive rows (default: B, an arbitrary reorder).  Only what was written from token `from_token` on moves -- rows of a
        group must be identical before it (beams forked at that length); 0 moves the rows up to the lengths in use.  Buffers,
        lengths and the native descriptors stay valid.  `check=False` skips the host-side check of the index values (a device
        read): the kernel leaves a row whose index lies outside its group as it is."""
        group = self.B if group is None else int(group)
        if not 0 <= int(from_token) <= self.kv_seq_len:
            raise ValueError(f"from_token={from_token} lies beyond the cache length {self.kv_seq_len}")
        idx = reorder.check_idx(idx, self.B, group, self.k_res.device, check)
        reorder.run(self._reorder_slabs(int(from_token)), self.B, group, idx)
        self._void_checkpoints()          # rows have changed places: no rollback across a reorder
        return self

    # ------------------------------------------------------------------ continuous batching
    def _admit_geometry(self) -> tuple:
        """What source and destination of an admission have to share: everything but the batch size, the capacity and where the V
        window stands."""
        return tuple(x for i, x in enumerate(self._geometry()) if i != 1)

    def check_admit(self, src, n: int, offset: int = 0) -> None:
        """Raise ValueError when `src` cannot be admitted into `n` rows of this cache at token `offset` (nothing runs on a device)."""
        if src is self:
            raise ValueError("admit_: the source is the destination cache itself")
        if not isinstance(src, KiviCacheBase) or src._admit_geometry() != self._admit_geometry():
            theirs = src._admit_geometry() if isinstance(src, KiviCacheBase) else type(src).__name__
            raise ValueError(f"admit_: the source is of another class or geometry: {theirs}, this cache is {self._admit_geometry()}")
        admit.check_offset(offset, self.rebase_quantum, self.kv_seq_len, self.cfg.residual_length)
        for name in ("kv_seq_len", "k_quant_len", "k_res_len", "v_quant_len", "v_res_len"):
            if not offset:
                if getattr(src, name) != getattr(self, name):
                    raise ValueError(f"admit_: {name} differs: the source is at {getattr(src, name)}, this cache at {getattr(self, name)} "
                                     f"(a prompt is admitted left-padded to the living cache's length)")
                continue
            want = getattr(self, name) - (0 if name.endswith("res_len") else offset)
            if getattr(src, name) != want:
                raise ValueError(f"admit_: {name} does not fit offset={offset}: the source is at {getattr(src, name)}, this cache at "
                                 f"{getattr(self, name)}, so the source has to be at {want} (a prompt pass over kv_seq_len - offset tokens)")
        if src.B != n:
            raise ValueError(f"admit_: the source holds {src.B} rows, {n} rows were named")
        mine = {getattr(self, b).untyped_storage().data_ptr() for b in self._BUFFERS}
        if any(getattr(src, b).untyped_storage().data_ptr() in mine for b in src._BUFFERS):
            raise ValueError("admit_: the source shares a buffer with this cache (admit from a cache of its own, e.g. a clone)")

    def admit_(self, rows, src, check: bool = True, offset: int = 0):
        """Row rows[i] of this cache <- row i of `src`, in place (kivi_cache_admit): a new request takes over the row of a finished
        one.  `src`: a cache of the same class and geometry -- batch size, capacity and v_res_start may differ -- of len(rows) rows at
        the same six lengths (a prompt pass over the prompts left-padded to this cache's length), sharing no buffer with this one.
        `rows`: distinct rows in [0, B), a 1-D int32 / int64 tensor or a sequence; `check=False` skips the host-side check of their
        values (a device read; the kernel leaves a source row with an index outside [0, B) unused).  What moves (`_admit_slabs`): the
        packed K and V up to their lengths, the range words (replaced), the fp16 K residual, the live fp16 window tokens from the
        source's window positions to this cache's.  Lengths, data pointers, the native descriptor, the scratch rows and the fusion
        flags stay: captured graphs remain valid.  Checkpoints issued so far become stale, as after a reorder.  ValueError before
        anything runs on a device for another class or geometry, a length that differs, a row count that does not fit, bad rows,
        `src is self` or a shared buffer.
        `offset` > 0: `src` is `offset` tokens SHORTER -- a prompt pass over kv_seq_len - offset >= residual_length
        tokens, its packed lengths `offset` below this cache's, the fp16 residual and window lengths the same -- and lands in tokens
        [offset, kv_seq_len) of the rows; tokens [0, offset) of the packed K and V become zero blocks, which the caller masks (the rows'
        2D mask starts with `offset` zeros).  `offset` is a multiple of `rebase_quantum`, so every K group, block, code, scale and
        zero point keeps its bits: the rows are what rebase_(offset) turns back into `src` (`_admit_offset`)."""
        rows = admit.rows_tensor(rows)
        self.check_admit(src, rows.shape[0], offset)
        rows = admit.check_rows(rows, rows.shape[0], self.B, self.k_res.device, check)
        if offset:
            self._admit_offset(rows, src, offset)
        else:
            admit.run(self._admit_slabs(src), rows, self.B)
        self._void_checkpoints()          # a row holds another request now: no rollback across an admission
        return self

    # ------------------------------------------------------------------ rebase
    @property
    def rebase_quantum(self) -> int:
        """The drops rebase_ takes are multiples of this: lcm(residual_length, 32)."""
        return rebase.quantum(self.cfg.residual_length)

    @property
    def rebase_limit(self) -> int:
        """The largest drop rebase_ takes now: only packed tokens leave, and K and V lose the same ones."""
        return min(self.k_quant_len, self.v_quant_len)

    def check_rebase(self, drop) -> None:
        """Raise ValueError when rebase_(drop) would refuse (nothing runs on a device)."""
        rebase.check_drop(drop, self.rebase_quantum, self.rebase_limit)

    def rebase_(self, drop: int):
        """The first `drop` tokens of every row leave the cache, in place: token t becomes token t - drop.  For rows whose first
        `drop` tokens are masked (leading pads) every later step computes what it would have computed over a
        cache built from the kept tokens alone, and the cache IS that cache: 9-tuple members and range words are bit-identical to
        it.  `drop`: a multiple of `rebase_quantum`, at most `rebase_limit`.  k_quant_len, v_quant_len and kv_seq_len fall by `drop`;
        the fp16 K residual, the fp16 V window and their lengths (v_res_start too) are untouched; capacity, data pointers and the
        fusion flags stay, the native descriptor's state array is brought in line.  Checkpoints issued so far become stale, as
        after a reorder; tuples issued before are stale: take as_tuple() again.  `drop == 0` does nothing and voids nothing.
        ValueError before anything runs on a device for a drop that is not an int, is negative, is not a multiple of the quantum
        or lies above the limit."""
        self.check_rebase(drop)
        if drop == 0:
            return self
        self._rebase_buffers(drop)
        self.k_quant_len -= drop
        self.v_quant_len -= drop
        self.kv_seq_len -= drop
        if self._native is not None:
            self._store_state(self._native[1])
        self._void_checkpoints()          # the packed stores no longer hold what a checkpoint continues
        return self

    # ------------------------------------------------------------------ checkpoint / rollback
    def _forget_checkpoints(self) -> None:
        """A cache of its own (new, cloned, index_selected): no checkpoint issued so far belongs to it."""
        self._ck_owner = object()
        self._ck_serial = 0      # checkpoints issued so far
        self._ck_lows = []       # [(serial at the time, length)]: restores (and, with length -1, reorders / prompt passes) that made
                                 # checkpoints stale -- only the entries no later one covers, so lengths rise with the serials

    def _void_checkpoints(self) -> None:
        """Every checkpoint issued so far becomes stale (reorder_, a new prompt pass)."""
        self._ck_lows = [(self._ck_serial, -1)]

    def _geometry(self) -> tuple:
        c = self.cfg
        return (type(self).__name__, self.B, self.nh_kv, self.D, getattr(self, "nh", None), c.k_bits, c.v_bits, c.group_size,
                c.residual_length)

    def checkpoint(self) -> "checkpoint.KiviCheckpoint":
        """The state to come back to with restore_(): the six lengths, the fusion flags and, through ONE kivi_cache_snapshot launch
        into a buffer the checkpoint owns, the bytes later steps overwrite in place (`_checkpoint_slabs`: the live fp16 K residual,
        the fp16 V window, the range words).  The packed stores are not copied: steps only write them from the packed lengths on.
        Any number of checkpoints may be outstanding; they hold no view into the cache and survive reserve()."""
        slabs = self._checkpoint_slabs()
        buf = torch.empty((self.B, checkpoint.row_bytes(slabs)), dtype=torch.uint8, device=self.k_res.device)
        checkpoint.run(slabs, self.B, buf, 0)
        self._ck_serial += 1
        return checkpoint.KiviCheckpoint(self._geometry(), self._ck_owner, self._ck_serial,
                                         tuple(int(getattr(self, n)) for n in checkpoint.LENGTHS),
                                         tuple(bool(getattr(self, n)) for n in checkpoint.FLAGS), buf)

    def check_restore(self, ck) -> None:
        """Raise ValueError when restore_(ck) would not give back the state `ck` was taken at (nothing runs on a device)."""
        if not isinstance(ck, checkpoint.KiviCheckpoint):
            raise ValueError(f"restore_ takes a KiviCheckpoint (KiviCacheBase.checkpoint()), got {type(ck).__name__}")
        if ck.geometry != self._geometry():
            raise ValueError(f"the checkpoint comes from another geometry or layout: {ck.geometry}, this cache is {self._geometry()}")
        if ck.owner is not self._ck_owner:
            raise ValueError("the checkpoint comes from another cache (a clone or index_select starts without checkpoints)")
        # a voided checkpoint is stale whatever the lengths (a rebase shortens the cache: "beyond" would name the symptom)
        for voided in (True, False):
            for serial, low in self._ck_lows:
                if serial >= ck.serial and low < ck.kv_seq_len and (low < 0) == voided:
                    what = "reordered, admitted into, rebased or prefilled again" if low < 0 else f"restored to kv length {low}"
                    raise ValueError(f"stale checkpoint: taken at kv length {ck.kv_seq_len}, the cache has since been {what}, so the "
                                     f"packed stores beyond that point no longer hold what the checkpoint continues")
            if voided and ck.kv_seq_len > self.kv_seq_len:
                raise ValueError(f"the checkpoint was taken at kv length {ck.kv_seq_len}, beyond the cache's {self.kv_seq_len}")

    def restore_(self, ck):
        """Back to the state checkpoint() saw, exactly (the 9-tuple, the range words and every later step are bit-identical to a
        cache that never went further): one scatter launch into the buffers as they are now, then the lengths and flags.  Nothing
        is reallocated or shrunk; the native descriptors and captured graphs stay valid.  Tuples issued before are stale: take
        as_tuple() again.  ValueError (before anything runs on a device) for a checkpoint of another geometry, layout or cache, one
        beyond the current length, or a stale one: the cache has since been restored below it, reordered or prefilled again."""
        self.check_restore(ck)
        checkpoint.run(self._checkpoint_slabs(dict(zip(checkpoint.LENGTHS, ck.state))), self.B, ck.buf, 1)
        for n, v in zip(checkpoint.LENGTHS + checkpoint.FLAGS, ck.state + ck.flags):
            setattr(self, n, v)
        self._ck_lows = [(s, low) for s, low in self._ck_lows if low < ck.kv_seq_len] + [(self._ck_serial, ck.kv_seq_len)]
        return self

    # ------------------------------------------------------------------ the 9-tuple
    def k_res_view(self) -> Optional[torch.Tensor]:
        return self.k_res[:, :, : self.k_res_len] if self.k_res_len else None

    def _tuple_members(self):
        kc, ks, km = self.k_quant_reference_layout()
        vc, vs, vm = self.v_quant_views()
        return (kc, self.k_res_view(), ks, km, vc, self.v_res_view(), vs, vm)

    def as_tuple(self) -> KiviCacheTuple:
        return KiviCacheTuple(self)

    def nbytes(self) -> int:
        """Resident cache bytes = what the reference's 9-tuple tensors would hold for the same state."""
        c = self.cfg
        per_k = self.D * self.k_quant_len * c.k_bits // 8 + 2 * self.D * (self.k_quant_len // c.group_size) * 2
        per_v = self.v_quant_len * self.D * c.v_bits // 8 + 2 * self.v_quant_len * (self.D // c.group_size) * 2
        res = (self.k_res_len + self.v_res_len) * self.D * 2
        return self.B * self.nh_kv * (per_k + per_v + res)

    def _adopt_residuals(self, past) -> None:
        """The fp16 members and the lengths of a plain reference 9-tuple (the packed members: the layout's from_tuple)."""
        kfull, vfull = past[1], past[5]
        if kfull is not None:
            self.k_res_len = kfull.shape[2]
            self.k_res[:, :, : self.k_res_len].copy_(kfull)
        self.v_res_len = vfull.shape[2]
        self.v_res[:, :, : self.v_res_len].copy_(vfull)
        self.kv_seq_len = int(past[8])


class KiviLayerCache(KiviCacheBase):
    """One layer's quantised KV cache with capacity `max_len` tokens, appended in place."""

    def __init__(self, cfg: KiviConfig, batch: int, num_kv_heads: int, head_dim: int, max_len: int,
                 device, dtype=torch.float16, page_tokens: int = None):
        super().__init__(cfg, batch, num_kv_heads, head_dim, max_len, dtype)
        R, g = cfg.residual_length, cfg.group_size
        assert head_dim % g == 0 and head_dim % (32 // cfg.v_bits) == 0
        if page_tokens is None:
            # a K flush of R tokens must not straddle pages AND a page is whole tiles of the default qK^T kernels: the smallest common
            # multiple (R = 32 / 64 / 128: 2048; R = 96 or 192: 6144 -- the reference accepts any multiple of the group size, llama_kivi.py:344)
            page_tokens = PAGE_TOKENS * R // math.gcd(PAGE_TOKENS, R)
        assert page_tokens % R == 0 and page_tokens % g == 0, "a K flush of R tokens must not straddle pages"
        self.page_tokens = page_tokens
        self.n_pages = (self.cap + page_tokens - 1) // page_tokens
        kf, vf = 32 // cfg.k_bits, 32 // cfg.v_bits
        dev = device
        # logical shape (B, nh_kv, P, D, page/fpi); in MEMORY the page index is outside the head index, so the pages in
        # use form one dense region and the spare capacity sits behind it (with the head index outside, every head's
        # unused pages would punch 64 KiB holes into the streamed range)
        self.k_code = self._paged((batch, num_kv_heads, self.n_pages, head_dim, page_tokens // kf), torch.int32, dev)
        self.k_scale = self._paged((batch, num_kv_heads, self.n_pages, head_dim, page_tokens // g), dtype, dev)
        self.k_mn = self._paged((batch, num_kv_heads, self.n_pages, head_dim, page_tokens // g), dtype, dev)
        self.k_res = torch.empty((batch, num_kv_heads, R, head_dim), dtype=dtype, device=dev)
        self.v_code = torch.empty((batch, num_kv_heads, self.cap, head_dim // vf), dtype=torch.int32, device=dev)
        self.v_scale = torch.empty((batch, num_kv_heads, self.cap, head_dim // g), dtype=dtype, device=dev)
        self.v_mn = torch.empty_like(self.v_scale)
        # fp16 V window: R (+1 transient) live tokens inside a 2R+1 buffer, compacted every R steps
        self.v_res = torch.empty((batch, num_kv_heads, 2 * R + 1, head_dim), dtype=dtype, device=dev)

    _BUFFERS = ("k_code", "k_scale", "k_mn", "k_res", "v_code", "v_scale", "v_mn", "v_res")

    def _admit_geometry(self) -> tuple:
        return super()._admit_geometry() + (self.page_tokens,)

    @staticmethod
    def _paged(shape, dtype, device) -> torch.Tensor:
        B, h, P, D, W = shape
        if _tuning.flag("KIVI_K_HEAD_MAJOR"):   # tuning sessions: the plain (B, nh_kv, P, ...) memory order
            return torch.empty(shape, dtype=dtype, device=device)
        return torch.empty((B, P, h, D, W), dtype=dtype, device=device).permute(0, 2, 1, 3, 4)

    # ------------------------------------------------------------------ capacity
    def reserve(self, max_len: int) -> None:
        """Grow the capacity to at least `max_len` tokens (the reference's torch.cat-grown tuple has no limit,
        llama_kivi.py:350-352, :393-395): new page / row buffers, the live contents copied once.  Scratch buffers and the
        cached native descriptor of the attention hook are dropped and rebuilt on the next step."""
        R = self.cfg.residual_length
        cap = ((max_len + R - 1) // R) * R
        if cap <= self.cap:
            return
        n_pages = (cap + self.page_tokens - 1) // self.page_tokens

        def grown(x, dim, n):
            shape = list(x.shape)
            shape[dim] = n
            y = torch.empty(shape, dtype=x.dtype, device=x.device)
            y.narrow(dim, 0, x.shape[dim]).copy_(x)
            return y
        if n_pages > self.n_pages:
            def grown_pages(x):
                y = self._paged((x.shape[0], x.shape[1], n_pages, x.shape[3], x.shape[4]), x.dtype, x.device)
                y[:, :, : x.shape[2]].copy_(x)
                return y
            self.k_code, self.k_scale, self.k_mn = (grown_pages(x) for x in (self.k_code, self.k_scale, self.k_mn))
            self.n_pages = n_pages
        self.v_code, self.v_scale, self.v_mn = (grown(x, 2, cap) for x in (self.v_code, self.v_scale, self.v_mn))
        self.cap = cap
        self._invalidate()

    def _own_buffers(self, idx) -> None:
        """Replace the buffers (still those of the cache this one was copied from) by copies of their own: whole, or rows `idx`."""
        for name in ("k_code", "k_scale", "k_mn"):
            src = getattr(self, name)
            dst = self._paged((self.B,) + tuple(src.shape[1:]), src.dtype, src.device)
            setattr(self, name, dst.copy_(src if idx is None else src.index_select(0, idx)))
        for name in ("k_res", "v_code", "v_scale", "v_mn", "v_res"):
            src = getattr(self, name)
            setattr(self, name, src.clone() if idx is None else src.index_select(0, idx))

    def _reorder_slabs(self, from_token: int):
        from .reorder import _span, slab
        g, P, kf, h = self.cfg.group_size, self.page_tokens, 32 // self.cfg.k_bits, self.nh_kv
        out = []
        a, kq = from_token // g * g, self.k_quant_len           # the first K group that holds a token >= from_token
        for p in range(a // P, (kq + P - 1) // P) if a < kq else ():
            lo, hi = max(a, p * P) - p * P, min(kq, (p + 1) * P) - p * P
            for x, per in ((self.k_code, kf), (self.k_scale, g), (self.k_mn, g)):
                es = x.element_size()
                b0, b1 = _span(lo // per * es, -(-hi // per) * es, x.shape[4] * es)
                out.append(slab(x, p * x.stride(2) * es + b0, [(h, x.stride(1) * es), (self.D, x.stride(3) * es)], b1 - b0))
        if self.k_res_len:
            out.append(slab(self.k_res, 0, [(h, self.k_res.stride(1) * 2)], self.k_res_len * self.D * 2))
        if from_token < self.v_quant_len:
            for x in (self.v_code, self.v_scale, self.v_mn):
                es, rowb = x.element_size(), x.shape[3] * x.element_size()
                b0, b1 = _span(from_token * rowb, self.v_quant_len * rowb, x.shape[2] * rowb)
                out.append(slab(x, b0, [(h, x.stride(1) * es)], b1 - b0))
        if self.v_res_len:
            rowb = self.D * 2
            b0, b1 = _span(self.v_res_start * rowb, (self.v_res_start + self.v_res_len) * rowb, self.v_res.shape[2] * rowb)
            out.append(slab(self.v_res, b0, [(h, self.v_res.stride(1) * 2)], b1 - b0))
        return out

    def _admit_slabs(self, src: "KiviLayerCache"):
        """Everything in use of a row of `src` (same geometry and lengths; its own capacity and window start) -> this cache's buffers:
        the K pages up to k_quant_len (whole pages as one slab with the page index as a level, each side with its own page stride;
        then the partly filled page), the fp16 K residual, the V triple up to v_quant_len, the window from the source's
        [v_res_start, + v_res_len) to this cache's."""
        from .reorder import _span
        g, P, kf, h, D = self.cfg.group_size, self.page_tokens, 32 // self.cfg.k_bits, self.nh_kv, self.D
        out = []
        full, part = divmod(self.k_quant_len, P)
        for x, y, per in ((self.k_code, src.k_code, kf), (self.k_scale, src.k_scale, g), (self.k_mn, src.k_mn, g)):
            es = x.element_size()
            inner = [(h, x.stride(1) * es, y.stride(1) * es), (D, x.stride(3) * es, y.stride(3) * es)]
            if full:
                out.append(admit.slab(x, 0, y, 0, [(full, x.stride(2) * es, y.stride(2) * es)] + inner, x.shape[4] * es))
            if part:
                b0, b1 = _span(0, -(-part // per) * es, x.shape[4] * es)
                out.append(admit.slab(x, full * x.stride(2) * es, y, full * y.stride(2) * es, inner, b1 - b0))
        rowb = D * 2
        if self.k_res_len:
            out.append(admit.slab(self.k_res, 0, src.k_res, 0, [(h, self.k_res.stride(1) * 2, src.k_res.stride(1) * 2)],
                                  self.k_res_len * rowb))
        if self.v_quant_len:
            for x, y in ((self.v_code, src.v_code), (self.v_scale, src.v_scale), (self.v_mn, src.v_mn)):
                es, tokb = x.element_size(), x.shape[3] * x.element_size()
                b0, b1 = _span(0, self.v_quant_len * tokb, min(x.shape[2], y.shape[2]) * tokb)
                out.append(admit.slab(x, 0, y, 0, [(h, x.stride(1) * es, y.stride(1) * es)], b1 - b0))
        if self.v_res_len:
            out.append(admit.slab(self.v_res, self.v_res_start * rowb, src.v_res, src.v_res_start * rowb,
                                  [(h, self.v_res.stride(1) * 2, src.v_res.stride(1) * 2)], self.v_res_len * rowb))
        return out

    def _admit_offset(self, rows: torch.Tensor, src: "KiviLayerCache", offset: int) -> None:
        """Admission at token `offset` (the UNTUNED path, as _rebase_buffers: torch ops on the tensors' device --
        an offset of 32 tokens is 2 bytes of fp16 K scales, below the 4-byte units of kivi_cache_admit).  The source's packed K in
        the reference layout behind `offset` tokens of zeros, written page by page (the shift crosses pages); the V triple behind
        `offset` zero rows; the fp16 K residual; the window from the source's [v_res_start, + v_res_len) to this cache's.  `rows`
        is only used on the device: an index outside [0, B) leaves its source row unused (it is redirected to the first good row
        WITH that row's source, a second write of the same bytes; with no good row, to row 0 with row 0's own bytes)."""
        kf, g, P = 32 // self.cfg.k_bits, self.cfg.group_size, self.page_tokens
        rows = rows.long()
        ok = (rows >= 0) & (rows < self.B)
        pick = torch.where(ok, torch.arange(rows.shape[0], device=rows.device), ok.int().argmax())     # the source row of every entry
        ok = ok.index_select(0, pick)
        tgt = torch.where(ok, rows.index_select(0, pick), torch.zeros_like(rows))

        def put(dst, val):                         # dst (B, ...) view <- val (n, ...) at the rows
            val = val.index_select(0, pick)
            dst.index_copy_(0, tgt, torch.where(ok.view(-1, *[1] * (val.dim() - 1)), val, dst.index_select(0, tgt)))

        def lead(x, dim, n):                       # n zeros in front of x along dim
            shape = list(x.shape)
            shape[dim] = n
            return torch.cat([x.new_zeros(shape), x], dim)
        kq = self.k_quant_len
        for x, y, per in zip((self.k_code, self.k_scale, self.k_mn), src.k_quant_reference_layout(), (kf, g, g)):
            y = lead(y, 3, offset // per)
            for p in range((kq + P - 1) // P):
                n = min(P, kq - p * P)
                put(x[:, :, p, :, : n // per], y[..., p * P // per: (p * P + n) // per])
        if self.k_res_len:
            put(self.k_res[:, :, : self.k_res_len], src.k_res[:, :, : self.k_res_len])
        for x, y in zip((self.v_code, self.v_scale, self.v_mn), (src.v_code, src.v_scale, src.v_mn)):
            put(x[:, :, : self.v_quant_len], lead(y[:, :, : src.v_quant_len], 2, offset))
        if self.v_res_len:
            put(self.v_res[:, :, self.v_res_start: self.v_res_start + self.v_res_len],
                src.v_res[:, :, src.v_res_start: src.v_res_start + self.v_res_len])

    def _rebase_buffers(self, drop: int) -> None:
        """The packed K and V from token `drop` on -> token 0, into the same buffers (the UNTUNED path, as extend: torch ops on the
        GPU).  Source and destination overlap, so the part that moves is cloned first: K through the reference layout (the pages
        gathered, sliced on whole words -- `drop` is a multiple of 32 tokens -- and written back page by page), the V triple row
        by row.  What lies beyond the new lengths is not touched: nothing reads it."""
        kf, g = 32 // self.cfg.k_bits, self.cfg.group_size
        if self.k_quant_len > drop:
            kc, ks, km = self.k_quant_reference_layout()
            self._write_k_pages(kc[..., drop // kf:].clone(), ks[..., drop // g:].clone(), km[..., drop // g:].clone())
        if self.v_quant_len > drop:
            for x in (self.v_code, self.v_scale, self.v_mn):
                x[:, :, : self.v_quant_len - drop].copy_(x[:, :, drop: self.v_quant_len].clone())

    def _write_k_pages(self, kc: torch.Tensor, ks: torch.Tensor, km: torch.Tensor) -> None:
        """Packed K in the reference layout (B, nh_kv, D, T / ...) -> the pages, from token 0."""
        kf, g, P = 32 // self.cfg.k_bits, self.cfg.group_size, self.page_tokens
        T = kc.shape[-1] * kf
        for p in range((T + P - 1) // P):
            n = min(P, T - p * P)
            self.k_code[:, :, p, :, : n // kf].copy_(kc[..., p * P // kf: (p * P + n) // kf])
            self.k_scale[:, :, p, :, : n // g].copy_(ks[..., p * P // g: (p * P + n) // g])
            self.k_mn[:, :, p, :, : n // g].copy_(km[..., p * P // g: (p * P + n) // g])

    def _checkpoint_slabs(self, state=None):
        """What steps overwrite in place, at the lengths `state` (default: the current ones): the live rows of the fp16 K residual and
        of the fp16 V window.  (This layout has no range words.)"""
        from .reorder import slab
        kl, vs, vl = (self.k_res_len, self.v_res_start, self.v_res_len) if state is None else \
            (state["k_res_len"], state["v_res_start"], state["v_res_len"])
        h, rowb = self.nh_kv, self.D * 2
        out = []
        if kl:
            out.append(slab(self.k_res, 0, [(h, self.k_res.stride(1) * 2)], kl * rowb))
        if vl:
            out.append(slab(self.v_res, vs * rowb, [(h, self.v_res.stride(1) * 2)], vl * rowb))
        return out

    # ------------------------------------------------------------------ the 9-tuple
    def k_quant_reference_layout(self):
        """(K_code_T, K_scale_T, K_mn_T) in the reference layout (B, nh_kv, D, Tq/...): gathers the pages (a copy)."""
        if self.k_quant_len == 0:
            return None, None, None
        kf, g = 32 // self.cfg.k_bits, self.cfg.group_size
        npg = (self.k_quant_len + self.page_tokens - 1) // self.page_tokens
        B, h, D = self.B, self.nh_kv, self.D

        def gather(x, per_tok):
            y = x[:, :, :npg].permute(0, 1, 3, 2, 4).reshape(B, h, D, -1)
            return y[..., : self.k_quant_len // per_tok].contiguous()
        return gather(self.k_code, kf), gather(self.k_scale, g), gather(self.k_mn, g)

    def v_quant_views(self):
        if self.v_quant_len == 0:
            return None, None, None
        n = self.v_quant_len
        return self.v_code[:, :, :n], self.v_scale[:, :, :n], self.v_mn[:, :, :n]

    def v_res_view(self) -> torch.Tensor:
        return self.v_res[:, :, self.v_res_start: self.v_res_start + self.v_res_len]

    def allocated_bytes(self) -> int:
        return sum(x.numel() * x.element_size() for x in (self.k_code, self.k_scale, self.k_mn, self.k_res, self.v_code,
                                                          self.v_scale, self.v_mn, self.v_res))

    # ------------------------------------------------------------------ K pages
    def _k_page(self, p: int):
        return self.k_code[:, :, p], self.k_scale[:, :, p], self.k_mn[:, :, p]

    def _quantise_k(self, key_states: torch.Tensor, t0: int) -> None:
        """Quantise tokens key_states (B, nh_kv, n, D), n % g == 0, into the packed prefix starting at token t0."""
        P, g = self.page_tokens, self.cfg.group_size
        n = key_states.shape[2]
        done = 0
        while done < n:
            p, off = divmod(t0 + done, P)
            take = min(n - done, P - off)
            new_pack.quantize_and_pack_k_tmajor(key_states[:, :, done: done + take], g, self.cfg.k_bits,
                                                out=self._k_page(p), token_offset=off)
            done += take

    # ------------------------------------------------------------------ prefill (llama_kivi.py:425-452)
    def prefill(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        """key/value_states (B, nh_kv, T, D) fp16 (any strides with a contiguous last dim)."""
        cfg = self.cfg
        R, g = cfg.residual_length, cfg.group_size
        T = key_states.shape[2]
        self.reserve(T)
        self._void_checkpoints()
        nq = (T // R) * R                      # quantised K prefix, fp16 remainder T % R
        if nq:
            self._quantise_k(key_states[:, :, :nq], 0)
        self.k_quant_len = nq
        self.k_res_len = T - nq
        if self.k_res_len:
            self.k_res[:, :, : self.k_res_len].copy_(key_states[:, :, nq:])
        nv = max(T - R, 0)                     # quantised V prefix, last min(T, R) tokens stay fp16
        if nv:
            code, scale, mn = new_pack.triton_quantize_and_pack_along_last_dim(value_states[:, :, :nv].contiguous(), g,
                                                                                cfg.v_bits)
            self.v_code[:, :, :nv].copy_(code)
            self.v_scale[:, :, :nv].copy_(scale)
            self.v_mn[:, :, :nv].copy_(mn)
        self.v_quant_len = nv
        self.v_res_start = 0
        self.v_res_len = T - nv
        self.v_res[:, :, : self.v_res_len].copy_(value_states[:, :, nv:])
        self.kv_seq_len = T

    # ------------------------------------------------------------------ decode-step mutations
    def append_k(self, key_states: torch.Tensor) -> None:
        """llama_kivi.py:333-336: K residual += the new token (B, nh_kv, 1, D)."""
        assert key_states.shape[2] == 1
        assert self.k_quant_len + self.k_res_len + 1 <= self.cap, "cache capacity exceeded"
        self.k_res[:, :, self.k_res_len: self.k_res_len + 1].copy_(key_states)
        self.k_res_len += 1

    def maybe_flush_k(self) -> None:
        """llama_kivi.py:343-356: when the residual holds exactly R tokens, quantise all of them in place."""
        R = self.cfg.residual_length
        if self.k_res_len == R:
            self._quantise_k(self.k_res, self.k_quant_len)
            self.k_quant_len += R
            self.k_res_len = 0

    def compact_v_window(self) -> None:
        """Move the live window rows to the front of the 2R+1 buffer (once every ~R steps)."""
        live = self.v_res[:, :, self.v_res_start: self.v_res_start + self.v_res_len].clone()
        self.v_res[:, :, : self.v_res_len].copy_(live)
        self.v_res_start = 0

    def append_v(self, value_states: torch.Tensor) -> None:
        """llama_kivi.py:377: V window += the new token."""
        assert value_states.shape[2] == 1
        R = self.cfg.residual_length
        if self.v_res_start + self.v_res_len + 1 > self.v_res.shape[2]:
            self.compact_v_window()
        pos = self.v_res_start + self.v_res_len
        self.v_res[:, :, pos: pos + 1].copy_(value_states)
        self.v_res_len += 1
        assert self.v_res_len <= R + 1

    def maybe_flush_v(self) -> None:
        """llama_kivi.py:386-399: when the window holds R+1 tokens, quantise the oldest one in place."""
        R, g = self.cfg.residual_length, self.cfg.group_size
        if self.v_res_len > R:
            assert self.v_res_len == R + 1 and self.v_quant_len + 1 <= self.cap
            oldest = self.v_res[:, :, self.v_res_start: self.v_res_start + 1]
            code, scale, mn = new_pack.triton_quantize_and_pack_along_last_dim(oldest.contiguous(), g, self.cfg.v_bits)
            n = self.v_quant_len
            self.v_code[:, :, n: n + 1].copy_(code)
            self.v_scale[:, :, n: n + 1].copy_(scale)
            self.v_mn[:, :, n: n + 1].copy_(mn)
            self.v_quant_len += 1
            self.v_res_start += 1
            self.v_res_len -= 1

    # ------------------------------------------------------------------ decode step (llama_kivi.py:314-399)
    def decode_step(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
                    attention_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    fused_kernels: bool = True, lead: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`lead` is accepted and ignored: this layout's kernels have no skip, the mask alone serves them.
        One new token: query (B, nh, 1, D), key / value (B, nh_kv, 1, D), RoPE applied -> (B, nh, 1, D) fp16 (`out` when the
        one-call step ran, a new tensor otherwise).  The most fused form the shape has a kernel for: one library call, the fused
        launches with the bookkeeping in Python, or -- also with `fused_kernels=False` -- the reference's op sequence composed
        from the fused GEMVs and torch ops."""
        cfg = self.cfg
        B, nh, q_len, D = query_states.shape
        assert q_len == 1, "decode branch: one new token (the reference kernel is q_len == 1 only)"
        if fused_kernels and not self._fused_unsupported:
            if _hook()._NATIVE_STEP and _fusion_level() == 2 and not self._attend_unfusable:
                try:
                    return self._decode_native(query_states, key_states, value_states, attention_mask, out)
                except KiviUnsupported as e:         # the Python path below picks the next fusion level
                    self._drop_fusion("_attend_unfusable", "the one-call layer step (kivi_decode_layer) is not available", str(e))
            try:
                return self._decode_fused(query_states, key_states, value_states, attention_mask)
            except KiviUnsupported as e:          # shape without a tuned kernel: compose the unfused ops from now on
                self._drop_fusion("_fused_unsupported", "no fused decode kernel covers the shape: composing the reference's op sequence "
                                  "from the fused GEMVs and torch ops", str(e))
        nh_kv = self.nh_kv
        rep = nh // nh_kv
        kv_seq_len = self.kv_seq_len + 1                                     # llama_kivi.py:307-309
        g = cfg.group_size

        # ---- scores over [quantised K prefix | fp16 K residual]  (:323-341)
        Tq = self.k_quant_len
        scores = self._row_buffer("_scores", nh)[..., :kv_seq_len]
        if Tq:   # :324, reading the K pages in place and writing straight into the scores buffer (scratch: may still raise)
            matmul.gemv_k_paged(g, query_states, self.k_code, self.k_scale, self.k_mn, Tq, cfg.k_bits, out=scores[..., :Tq])
        self.append_k(key_states)                                            # :333-336
        k_full = self.k_res_view()                                           # (B, nh_kv, L, D)
        att_qkfull = torch.matmul(query_states.reshape(B, nh_kv, rep, D), k_full.transpose(2, 3))  # :337 (repeat_kv folded)
        scores[..., Tq:].copy_(att_qkfull.view(B, nh, 1, -1))
        attn_weights = scores / math.sqrt(D)                                  # :339, fp16 division like the reference
        self.maybe_flush_k()                                                  # :343-356

        if attn_weights.size() != (B, nh, 1, kv_seq_len):
            raise ValueError(f"Attention weights should be of size {(B, nh, 1, kv_seq_len)}, but is {attn_weights.size()}")
        if attention_mask is not None:                                        # :364-372
            check_mask_size(attention_mask, (B, 1, 1, kv_seq_len))
            attn_weights = attn_weights + attention_mask
            attn_weights = torch.max(attn_weights, torch.tensor(torch.finfo(attn_weights.dtype).min, device=attn_weights.device))
        attn_weights = F.softmax(attn_weights, dim=-1, dtype=torch.float32).to(query_states.dtype)   # :375

        attn_output = self._composed_output(attn_weights, value_states, nh)   # :377-399
        self.kv_seq_len = kv_seq_len
        return attn_output

    def _drop_fusion(self, attr: str, what: str, why: str = "") -> None:
        """Mark this cache as unable to use one fusion level and say so ONCE per layer and level: a shape without a tuned kernel
        otherwise runs the slower composition forever without a word."""
        if getattr(self, attr):
            return
        setattr(self, attr, True)
        if _FUSION_ENV:          # a tuning session asked for the lower level
            return
        c = self.cfg
        warnings.warn(f"kivi_amd: {what} for this cache (k_bits={c.k_bits} v_bits={c.v_bits} group={c.group_size} "
                      f"residual={c.residual_length} head_dim={self.D} kv_heads={self.nh_kv}){': ' + why if why else ''} -- the step "
                      f"runs as more, slower launches from now on; results are unchanged", KiviPerformanceWarning, stacklevel=4)

    def _row_buffer(self, name: str, nh: int) -> torch.Tensor:
        """(B, nh, 1, pitch) per-layer fp16 scratch row buffer (`_scores` / `_probs`), pitch = a multiple of 8 halves >= capacity + 1
        (16-byte stores of the fused GEMV)."""
        pitch = ((self.cap + 1 + 7) // 8) * 8
        buf = getattr(self, name)
        if buf is None or buf.shape[1] != nh:
            buf = torch.empty((self.B, nh, 1, pitch), dtype=torch.float16, device=self.k_code.device)
            setattr(self, name, buf)
        return buf

    def _native_desc(self, nh: int):
        """The kivi_layer_desc of this layer (built once: buffers and strides never change), its state array."""
        cached = self._native
        if cached is not None and cached[2] == nh:
            return cached
        cfg = self.cfg
        scores = self._row_buffer("_scores", nh)
        ws = fused._workspace(self.k_code.device, self.B * nh, self.D)
        kc, ks, kr, vc, vs, vr = self.k_code, self.k_scale, self.k_res, self.v_code, self.v_scale, self.v_res
        d = _lib.LayerDesc(
            B=self.B, nh_kv=self.nh_kv, D=self.D, k_bits=cfg.k_bits, v_bits=cfg.v_bits, group_size=cfg.group_size,
            residual_length=cfg.residual_length, inv_scale=1.0 / math.sqrt(self.D),
            cap=self.cap, page_tokens=self.page_tokens, v_window_rows=vr.shape[2], s_pitch=scores.shape[3],
            k_code=kc.data_ptr(), kc_sb=kc.stride(0), kc_sh=kc.stride(1), kc_sp=kc.stride(2), kc_sr=kc.stride(3),
            k_scale=ks.data_ptr(), k_mn=self.k_mn.data_ptr(), ks_sb=ks.stride(0), ks_sh=ks.stride(1), ks_sp=ks.stride(2),
            ks_sr=ks.stride(3),
            k_res=kr.data_ptr(), kr_sb=kr.stride(0), kr_sh=kr.stride(1), kr_st=kr.stride(2),
            v_code=vc.data_ptr(), vc_sb=vc.stride(0), vc_sh=vc.stride(1), vc_sr=vc.stride(2),
            v_scale=vs.data_ptr(), v_mn=self.v_mn.data_ptr(), vs_sb=vs.stride(0), vs_sh=vs.stride(1), vs_sr=vs.stride(2),
            v_res=vr.data_ptr(), vr_sb=vr.stride(0), vr_sh=vr.stride(1), vr_st=vr.stride(2),
            scores=scores.data_ptr(), s_sb=scores.stride(0), s_sh=scores.stride(1),
            workspace=ws.data_ptr(), workspace_bytes=ws.numel() * ws.element_size())
        state = (ctypes.c_int64 * 6)()
        self._native = (d, state, nh, _lib.load().kivi_decode_layer, ws)   # ws: keeps the shared workspace alive
        return self._native

    def _decode_native(self, query_states, key_states, value_states, attention_mask, out=None) -> torch.Tensor:
        """The whole step (both launches + cache bookkeeping + K flush) through ONE library call (kivi_decode_layer):
        the host side of a layer step drops from ~40 us of Python to one ctypes call.  Same launches, same results as
        _decode_fused; raises KiviUnsupported (state untouched) when no tuned kernel covers the shape."""
        B, nh, _, D = query_states.shape
        d, state, _, fn, _ = self._native_desc(nh)
        q, k, v = unit_rows(query_states), unit_rows(key_states), unit_rows(value_states)
        mask_ptr, mask_sb = mask_arg(attention_mask, B, self.kv_seq_len + 1)
        self._store_state(state)
        out = out_arg(out, (B, nh, 1, D), q.device)
        hook = matmul.launch_hook
        if hook is not None and self.k_quant_len:   # bench.py: bracket the qK^T dispatch (the first launch of the call)
            hook("pre", "k", dict(B=B, nh=nh, nh_kv=self.nh_kv, K=D, N=self.k_quant_len, bits=self.cfg.k_bits,
                                  group_size=self.cfg.group_size, v_bits=self.cfg.v_bits, Tv=self.v_quant_len,
                                  k_res=self.k_res_len + 1, v_res=self.v_res_len + 1))
        rc = fn(ctypes.byref(d), state, q.data_ptr(), q.stride(0), q.stride(1), nh, k.data_ptr(), k.stride(0), k.stride(1),
                v.data_ptr(), v.stride(0), v.stride(1), mask_ptr, mask_sb, out.data_ptr(), out.stride(0), out.stride(1),
                torch.cuda.current_stream(q.device).cuda_stream)
        # the library writes `state` after every phase it has enqueued (a refused step leaves it untouched apart from a
        # completed window compaction), so the lengths are read back whether or not the call succeeded
        self._load_state(state)
        if rc:
            _lib.check(rc, "kivi_decode_layer")
        return out

    def _decode_fused(self, query_states, key_states, value_states, attention_mask) -> torch.Tensor:
        """The decode step in two launches (three when only the separate softmax fits; +1 when the K residual fills up): same arithmetic and roundings as the
        composed path of decode_step.  Raises KiviUnsupported when no tuned kernel covers the shape."""
        cfg = self.cfg
        B, nh, _, D = query_states.shape
        kv_seq_len = self.kv_seq_len + 1
        scores = self._row_buffer("_scores", nh)
        probs = self._row_buffer("_probs", nh)
        if attention_mask is not None:
            check_mask_size(attention_mask, (B, 1, 1, kv_seq_len))
        assert self.k_quant_len + self.k_res_len + 1 <= self.cap, "cache capacity exceeded"
        if self.v_res_start + self.v_res_len + 1 > self.v_res.shape[2]:     # make room in the window buffer
            self.compact_v_window()
        out = torch.empty((B, nh, 1, D), dtype=torch.float16, device=query_states.device)
        inv = 1.0 / math.sqrt(D)
        flushed = None
        level = _fusion_level()
        if level < 2:
            self._drop_fusion("_attend_unfusable", "fusion level lowered")
        if level < 1:
            self._drop_fusion("_softmax_unfusable", "fusion level lowered")
        if not self._attend_unfusable:
            # two launches: packed qK^T GEMV (:324), then residual scores + K append + softmax + output + V append/flush
            # only the launches that may be refused sit inside the try (they write scratch rows until the attend launch
            # runs); the bookkeeping follows once they have been enqueued
            try:
                if self.k_quant_len:
                    matmul.gemv_k_paged(cfg.group_size, query_states, self.k_code, self.k_scale, self.k_mn, self.k_quant_len,
                                        cfg.k_bits, out=scores[..., : self.k_quant_len])
                flushed = fused.decode_attend(self, query_states, key_states, value_states, scores, out, inv, attention_mask)
            except KiviUnsupported as e:             # e.g. rows too long for the LDS: use the three-launch form below
                self._drop_fusion("_attend_unfusable", "the fused attend launch (residual scores + softmax + output in one launch) is not available", str(e))
            else:
                self.k_res_len += 1
                self.maybe_flush_k()                                          # :343-356
        if flushed is None:
            fused.decode_scores(self, query_states, key_states, scores)      # :323-337 (+ the K append of :333-336)
            self.k_res_len += 1                      # committed: the launch above appended the key
            self.maybe_flush_k()                                              # :343-356
            if not self._softmax_unfusable:
                try:   # scale + mask + softmax (:339, :364-375) inside the sV launch (:377-399)
                    flushed = fused.decode_output(self, scores, value_states, out, softmax_inv_scale=inv, mask=attention_mask)
                except KiviUnsupported as e:         # keep the softmax as its own launch
                    self._drop_fusion("_softmax_unfusable", "the softmax cannot be folded into the sV launch", str(e))
        if flushed is None:
            fused.softmax_scaled(scores, probs, kv_seq_len, inv, attention_mask)
            try:
                flushed = fused.decode_output(self, probs, value_states, out)
            except KiviUnsupported:   # no tuned sV kernel for this head_dim / group: compose the output part
                out = self._composed_output(probs[..., :kv_seq_len], value_states, nh)
                self.kv_seq_len = kv_seq_len
                return out
        self.v_res_len += 1
        if flushed:
            self.v_quant_len += 1
            self.v_res_start += 1
            self.v_res_len -= 1
        self.kv_seq_len = kv_seq_len
        return out

    def _composed_output(self, attn_weights: torch.Tensor, value_states: torch.Tensor, nh: int) -> torch.Tensor:
        """Output over [quantised V prefix | fp16 V window], one launch per reference op (llama_kivi.py:377-399)."""
        cfg = self.cfg
        B, nh_kv, D = self.B, self.nh_kv, self.D
        rep = nh // nh_kv
        self.append_v(value_states)
        Tv, Lv = self.v_quant_len, self.v_res_len
        v_full = self.v_res_view()
        w_full = attn_weights[..., Tv:].reshape(B, nh_kv, rep, Lv)
        if Tv == 0:
            attn_output = torch.matmul(w_full, v_full).view(B, nh, 1, D)     # :380
        else:
            vc, vs, vm = self.v_quant_views()
            attn_output = matmul.cuda_bmm_fA_qB_outer(cfg.group_size, attn_weights[..., :Tv], vc, vs, vm, cfg.v_bits)   # :382
            attn_output += torch.matmul(w_full, v_full).view(B, nh, 1, D)    # :384
        self.maybe_flush_v()                                                  # :386-399
        return attn_output

    # ------------------------------------------------------------------ multi-token extend (untuned)
    def extend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
               attention_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Q >= 1 new tokens over this cache: the contract of KiviLayerCacheMF.extend (chunk row i attends to the cache as it stands
        plus chunk tokens 0..i; per row the rounding sequence of one decode step) for the shapes the matrix pipe does not cover.
        The UNTUNED path: composed from torch ops on the GPU (fp32 dequantisation of the packed prefix, fp32 matmuls rounded to
        fp16 where the hook rounds), then the cache bookkeeping of Q decode steps through append / flush, one token at a time."""
        cfg = self.cfg
        B, nh, Q, D = query_states.shape
        assert B == self.B and D == self.D and Q >= 1 and nh % self.nh_kv == 0
        assert self.kv_seq_len > 0, "extend needs a cache: run the prompt pass first"
        self.ensure_room(Q)
        ratio, P0 = nh // self.nh_kv, self.kv_seq_len
        total = P0 + Q

        def heads(x):
            return x if ratio == 1 else x.repeat_interleave(ratio, dim=1)

        def deq(code, scale, mn, bits):            # groups along the last dim, fp32 scale * code + zero
            fpi = 32 // bits
            sh = torch.arange(fpi, device=code.device, dtype=torch.int32) * bits
            c = ((code.unsqueeze(-1) >> sh) & (2 ** bits - 1)).reshape(*code.shape[:-1], code.shape[-1] * fpi).float()
            g = cfg.group_size
            lead, T = c.shape[:-1], c.shape[-1]
            return (c.view(*lead, T // g, g) * scale.float().unsqueeze(-1) + mn.float().unsqueeze(-1)).view(*lead, T)

        qf = query_states.float()
        parts = []
        kc, ks, km = self.k_quant_reference_layout()
        if kc is not None:
            parts.append(torch.matmul(qf, heads(deq(kc, ks, km, cfg.k_bits))).half())                 # (B, nh, Q, Tq)
        kfull = torch.cat([x for x in (self.k_res_view(), key_states) if x is not None], 2)
        parts.append(torch.matmul(qf, heads(kfull).float().transpose(2, 3)).half())
        w = torch.cat(parts, -1) / math.sqrt(D)
        if attention_mask is not None:
            check_mask_size(attention_mask, (B, 1, Q, total))
            w = w + attention_mask
            w = torch.max(w, torch.tensor(torch.finfo(w.dtype).min, device=w.device, dtype=w.dtype))
        causal = torch.ones((Q, Q), dtype=torch.bool, device=w.device).triu(1)
        w = w.float()
        w[..., P0:] = w[..., P0:].masked_fill(causal, float("-inf"))
        p = torch.softmax(w, dim=-1).half()
        vfull = torch.cat([self.v_res_view(), value_states], 2)
        Tv = self.v_quant_len
        res = torch.matmul(p[..., Tv:].float(), heads(vfull).float()).half()
        if Tv:
            vc, vs, vm = self.v_quant_views()
            res = torch.matmul(p[..., :Tv].float(), heads(deq(vc, vs, vm, cfg.v_bits))).half() + res
        for i in range(Q):                         # llama_kivi.py:333-356, :377-399 per token
            self.append_k(key_states[:, :, i: i + 1])
            self.maybe_flush_k()
            self.append_v(value_states[:, :, i: i + 1])
            self.maybe_flush_v()
            self.kv_seq_len += 1
        if out is not None:
            out.copy_(res)
            return out
        return res

    # ------------------------------------------------------------------ import of a plain reference tuple
    @classmethod
    def from_tuple(cls, cfg: KiviConfig, past, max_len: int) -> "KiviLayerCache":
        """Adopt a plain 9-tuple produced elsewhere (copies it into the in-place buffers once)."""
        kc, kfull, ks, km, vc, vfull, vs, vm, kv_len = past
        ref = vfull if vfull is not None else kfull
        B, nh_kv, _, D = ref.shape
        self = cls(cfg, B, nh_kv, D, max_len, ref.device, ref.dtype)
        if kc is not None:
            self.k_quant_len = kc.shape[-1] * (32 // cfg.k_bits)
            self._write_k_pages(kc, ks, km)
        if vc is not None:
            self.v_quant_len = vc.shape[2]
            self.v_code[:, :, : self.v_quant_len].copy_(vc)
            self.v_scale[:, :, : self.v_quant_len].copy_(vs)
            self.v_mn[:, :, : self.v_quant_len].copy_(vm)
        self._adopt_residuals(past)
        return self
