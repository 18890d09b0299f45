"""Per-layer KIVI cache in the matrix-pipe layout (kivi_amd/csrc/kivi_mfma_layout.h): grouped-query models (round 2) and
multi-head models (round 3).

Same state machine and the same bits as KiviLayerCache (cache.py; reference contract models/llama_kivi.py:454-455, read
back at :315-322; Mistral: models/mistral_kivi.py:381-385, :441-445): the 9-tuple members are reproduced bit for bit by
the relayout kernels.  What differs is where the packed codes live: super-blocks of 512 tokens whose words are B operands
of v_mfma_f32_16x16x32_f16, so that the nh / nh_kv query heads of a kv head share every code on the matrix pipe instead of
costing one FMA each (the shared-unpack VALU kernels run at ~0.35 of the HBM roofline for nh / nh_kv = 4).

A decode step is ONE library call (kivi_mf_decode_layer: lengths, the launches, the K flush through kivi_kt_pack every R
steps).  Launches: rows whose scores fit the LDS (nh = nh_kv: 16 super-blocks + the residual, nh / nh_kv = 4: 18) and enough of them
-> one (mf_row_kernel / mf_row4_kernel; longer grouped-query rows: one launch of slices); otherwise two (packed qK^T + residual scores + K append + softmax statistics, then
softmax-on-the-fly + packed sV + fp16 window + V append / quantise).  Every store carries range flags (quant/mfma.py) that
keep the fp16 operands of the matrix pipe finite for any finite scale.

Round 4: also 4-bit K / V for nh / nh_kv = 4 (the reference's published Mistral-7B + KIVI-4 shape, docs/long_bench.md:35-53): the same
state machine and calls over 10240-word super-blocks (kivi_mfma_layout.h, "KT4 / VT4").  Round 6: 4-bit K / V of multi-head models
(Llama-2-7B / LongChat-7B-32K + KIVI-4, docs/long_bench.md:5-26) too.
"""
from __future__ import annotations

import ctypes
import functools
import math

import torch

from . import _lib, _tuning, admit, rebase
from ._lib import check_mask_size, lead_arg, mask_arg, out_arg, rows16
from .cache import KiviCacheBase, KiviConfig, KiviLayerCache
from .quant import matmul, mfma, new_pack

SB = mfma.SB_TOKENS
_SCRATCH = {}   # (device, stream) -> dict(scores, stats, ws): shared by the layers that decode on that stream (launches are
                # stream-ordered; two streams must not share score rows or arrival counters)
_WS_COUNTER_BYTES = 65536


def supported(cfg: KiviConfig, head_dim: int, num_heads: int, num_kv_heads: int) -> bool:
    if _tuning.flag("KIVI_NO_MFMA_LAYOUT"):     # tuning sessions: keep every model on the hook-state layout
        return False
    if num_heads == num_kv_heads and _tuning.flag("KIVI_NO_MFMA_MHA"):   # tuning sessions (A/B): multi-head models on the hook-state layout
        return False
    return num_heads % num_kv_heads == 0 and mfma.supported(cfg.k_bits, cfg.v_bits, cfg.group_size, head_dim,
                                                            cfg.residual_length, num_heads // num_kv_heads) \
        and cfg.residual_length <= 128


def padded_heads(cfg: KiviConfig, head_dim: int, num_heads: int, num_kv_heads: int):
    """The query-head count a model that `supported` turns away can run this layout with, or None: every kv head's nh / nh_kv query
    heads padded to the next ratio the layout serves (mfma.padded_ratio) by zero heads.  The caller pads q
    (kivi_qk_rope) and cuts the pad heads' outputs off."""
    if num_heads % num_kv_heads or supported(cfg, head_dim, num_heads, num_kv_heads):
        return None
    rp = mfma.padded_ratio(cfg.k_bits, cfg.v_bits, num_heads // num_kv_heads)
    if rp is None or not supported(cfg, head_dim, num_kv_heads * rp, num_kv_heads):
        return None
    return num_kv_heads * rp


def _scratch(device, B: int, nh: int, nh_kv: int, pitch: int, nseg: int, slices: int):
    stream = torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0
    d = _SCRATCH.setdefault((str(device), stream), {})
    sc = d.get("scores")
    if sc is None or sc.shape[0] < B or sc.shape[1] < nh or sc.shape[3] < pitch:
        shape = (B, nh, 1, pitch) if sc is None else (max(B, sc.shape[0]), max(nh, sc.shape[1]), 1, max(pitch, sc.shape[3]))
        sc = torch.empty(shape, dtype=torch.float16, device=device)      # every dimension grows monotonically
        d["scores"] = sc
    st = d.get("stats")
    need = B * nh * nseg * 2
    if st is None or st.numel() < need:
        st = torch.empty(need, dtype=torch.float32, device=device)
        d["stats"] = st
    ws = d.get("ws")
    need = _WS_COUNTER_BYTES + B * nh_kv * 2 * (max(slices, 1) + 1) * (nh // nh_kv) * 128 * 4   # + 1: the window block's slot
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.uint8, device=device)   # arrival counters start at zero; the kernel resets them
        d["ws"] = ws
    return sc, st, ws


@functools.lru_cache(maxsize=256)
def _store_pieces(W: int, j0: int, j1: int, is_k: bool):
    """The pieces in use of a packed store of W-word super-blocks from block j0 to block j1, blocks of 32 tokens, 16 to a super-block
    (kivi_mfma_layout.h), as (first super-block, super-blocks, byte offset in the super-block, inner levels [(count, byte
    stride)] below the head level, run bytes).  Whole super-blocks come as one run with their count (otherwise the count is 0); of
    a partial one: the codes of block j at words [j BW, (j + 1) BW); the V scales / zero points of block j at halves j * 128 of
    their regions; the K scales / zero points of group j at halves (j >> 3) * 1024 + (c, kb) * 64 + (j & 7) * 8 (16 pieces of
    16 bytes per block).  Cached: a decoding cache asks for the same walk until it crosses a block."""
    S0, BW = (W - 2048) * 4, (W - 2048) // 16 * 4              # byte offset of the scale region, bytes of codes per block
    out, s = [], j0 // 16
    while s * 16 < j1 and j0 < j1:
        lo, hi = max(j0, 16 * s) - 16 * s, min(j1, 16 * s + 16) - 16 * s
        if lo == 0 and hi == 16:
            n = j1 // 16 - s
            out.append((s, n, 0, (), W * 4))
            s += n
            continue
        out.append((s, 0, lo * BW, (), (hi - lo) * BW))
        if is_k:
            for half in (0, 1):
                glo, ghi = max(lo, 8 * half), min(hi, 8 * half + 8)
                if glo < ghi:
                    out.append((s, 0, S0 + (half * 1024 + (glo & 7) * 8) * 2, ((2, 4096), (16, 128)), (ghi - glo) * 16))
        else:
            out.append((s, 0, S0 + lo * 256, ((2, 4096),), (hi - lo) * 256))
        s += 1
    return tuple(out)


class KiviLayerCacheMF(KiviCacheBase):
    """One layer's quantised KV cache (capacity `max_len` tokens, appended in place): 2-bit with nh / nh_kv in {1, 4, 8}, 4-bit with
    nh / nh_kv in {1, 4} (multi-head 4-bit: round 6)."""

    layout = "mfma"

    def __init__(self, cfg: KiviConfig, batch: int, num_kv_heads: int, head_dim: int, max_len: int, device,
                 dtype=torch.float16, num_heads: int = None):
        assert num_heads is not None and supported(cfg, head_dim, num_heads, num_kv_heads), \
            "matrix-pipe layout: group 32, head_dim 128, residual_length <= 128; 2-bit with nh / nh_kv in {1, 4, 8} or 4-bit with nh / nh_kv in {1, 4}"
        super().__init__(cfg, batch, num_kv_heads, head_dim, max_len, dtype)
        R = cfg.residual_length
        self.nh = num_heads
        self.n_sb = (self.cap + SB - 1) // SB
        self.kt = mfma.alloc_store(batch, num_kv_heads, self.n_sb, device, cfg.k_bits)
        self.vt = mfma.alloc_store(batch, num_kv_heads, self.n_sb, device, cfg.v_bits)
        self.k_res = torch.empty((batch, num_kv_heads, R, head_dim), dtype=dtype, device=device)
        # fp16 value window: a RING of R + 1 rows (row of window token t = (v_res_start + t) mod rows): nothing is ever compacted
        self.ring = True
        self.v_res = torch.empty((batch, num_kv_heads, R + 1, head_dim), dtype=dtype, device=device)
        self.flags = 0            # _lib.GQA_FORCE_SPLIT / GQA_FORCE_ROW (tests, tuning)

    _BUFFERS = ("kt", "vt", "k_res", "v_res")

    # ------------------------------------------------------------------ capacity
    def reserve(self, max_len: int) -> None:
        R = self.cfg.residual_length
        cap = ((max_len + R - 1) // R) * R
        if cap <= self.cap:
            return
        n_sb = (cap + SB - 1) // SB
        if n_sb > self.n_sb:
            for name in ("kt", "vt"):
                old = getattr(self, name)
                new = mfma.alloc_store(self.B, self.nh_kv, n_sb, old.device, self.cfg.k_bits)
                mfma.copy_store(new, old)                      # super-blocks in use + the store's range flags
                setattr(self, name, new)
            self.n_sb = n_sb
        self.cap = cap
        self._invalidate()

    def _own_buffers(self, idx) -> None:
        """Replace the buffers (still those of the cache this one was copied from) by copies of their own: whole, or rows `idx`
        (range words included)."""
        for name in ("kt", "vt"):
            src = getattr(self, name)
            dst = mfma.alloc_store(self.B, self.nh_kv, self.n_sb, src.device, self.cfg.k_bits)
            if idx is None:
                mfma.copy_store(dst, src)
            else:
                dst.copy_(src.index_select(0, idx))
                mfma.range_flags(dst).copy_(mfma.range_flags(src).index_select(0, idx))
            setattr(self, name, dst)
        for name in ("k_res", "v_res"):
            src = getattr(self, name)
            setattr(self, name, src.clone() if idx is None else src.index_select(0, idx))

    # ------------------------------------------------------------------ beam search
    def _reorder_slabs(self, from_token: int):
        """The blocks of both stores from from_token's on (K groups / V tokens), the range words, the fp16 K residual up to its
        length, the whole fp16 V ring."""
        from .reorder import slab
        h, W = self.nh_kv, mfma.sb_words(self.cfg.k_bits)
        out = []
        for st, n_tok, is_k in ((self.kt, self.k_quant_len, True), (self.vt, self.v_quant_len, False)):
            ss, sh = st.stride(2) * 4, st.stride(1) * 4
            for s, n, off, inner, run in _store_pieces(W, from_token // 32, -(-n_tok // 32), is_k):
                out.append(slab(st, s * ss + off, [(n, ss)] * (n > 0) + [(h, sh), *inner], run))
            out.append(slab(mfma.range_flags(st), 0, [], h * 4))
        if self.k_res_len:
            out.append(slab(self.k_res, 0, [(h, self.k_res.stride(1) * 2)], self.k_res_len * self.D * 2))
        out.append(slab(self.v_res, 0, [(h, self.v_res.stride(1) * 2)], self.v_res.shape[2] * self.D * 2))
        return out

    # ------------------------------------------------------------------ continuous batching
    def _admit_slabs(self, src: "KiviLayerCacheMF"):
        """Everything in use of a row of `src` (same geometry and lengths; its own super-block count and ring phase) -> this cache's
        buffers.  The stores move as the pieces of _reorder_slabs(0), every super-block and head stride taken from each side's own
        store (a partly filled V block arrives with the source's clean tail); the range words are replaced; the fp16 K residual up
        to its length; the live window tokens rotated from the source's ring phase to this cache's in at most three contiguous
        segments (token t: source row (s_src + t) mod rows -> row (s_dst + t) mod rows).  The ring row that holds no live token is
        not written."""
        h, W = self.nh_kv, mfma.sb_words(self.cfg.k_bits)
        out = []
        for st, sy, n_tok, is_k in ((self.kt, src.kt, self.k_quant_len, True), (self.vt, src.vt, self.v_quant_len, False)):
            heads = (h, st.stride(1) * 4, sy.stride(1) * 4)
            dss, sss = st.stride(2) * 4, sy.stride(2) * 4
            for s, n, off, inner, run in _store_pieces(W, 0, -(-n_tok // 32), is_k):
                out.append(admit.slab(st, s * dss + off, sy, s * sss + off,
                                      [(n, dss, sss)] * (n > 0) + [heads] + [(c, b, b) for c, b in inner], run))
            out.append(admit.slab(mfma.range_flags(st), 0, mfma.range_flags(sy), 0, [], h * 4))
        return out + self._admit_fp16_slabs(src)

    def _admit_fp16_slabs(self, src: "KiviLayerCacheMF"):
        """The fp16 part of an admission (the same at any offset: these tokens are the newest): the K residual up to its length, the
        live window tokens rotated from the source's ring phase to this cache's."""
        h, rowb, out = self.nh_kv, self.D * 2, []
        if self.k_res_len:
            out.append(admit.slab(self.k_res, 0, src.k_res, 0, [(h, self.k_res.stride(1) * 2, src.k_res.stride(1) * 2)],
                                  self.k_res_len * rowb))
        rows, t = self.v_res.shape[2], 0
        ring = [(h, self.v_res.stride(1) * 2, src.v_res.stride(1) * 2)]
        while t < self.v_res_len:                                # a segment ends where either side wraps (or the window does)
            d, s = (self.v_res_start + t) % rows, (src.v_res_start + t) % rows
            n = min(self.v_res_len - t, rows - d, rows - s)
            out.append(admit.slab(self.v_res, d * rowb, src.v_res, s * rowb, ring, n * rowb))
            t += n
        return out

    def _admit_offset(self, rows: torch.Tensor, src: "KiviLayerCacheMF", offset: int) -> None:
        """Admission at token `offset`: one kivi_mf_store_admit per store -- the source's blocks in use land
        `offset` / 32 blocks further up, the blocks under the offset are zeroed, the range words replaced -- then the fp16 K residual
        and the ring-rotated window through kivi_cache_admit, as at offset 0."""
        for st, sy, n_tok, is_k, bits in ((self.kt, src.kt, src.k_quant_len, True, self.cfg.k_bits),
                                          (self.vt, src.vt, src.v_quant_len, False, self.cfg.v_bits)):
            admit.admit_store(st, sy, rows, bits, is_k, -(-n_tok // 32), offset // 32)
        admit.run(self._admit_fp16_slabs(src), rows, self.B)

    # ------------------------------------------------------------------ rebase
    def _rebase_buffers(self, drop: int) -> None:
        """Both stores `drop` / 32 blocks towards token 0, in place: one kivi_mf_store_shift per store over the blocks in use (K
        groups; V tokens, a partly filled last block whole), the vacated blocks zeroed, the range words recomputed from the
        scales kept."""
        for st, n_tok, is_k, bits in ((self.kt, self.k_quant_len, True, self.cfg.k_bits), (self.vt, self.v_quant_len, False, self.cfg.v_bits)):
            rebase.shift_store(st, bits, is_k, -(-n_tok // 32), drop // 32)

    def _checkpoint_slabs(self, state=None):
        """What steps overwrite in place: the fp16 K residual up to its length (`state`: the lengths to use, default the current ones),
        the whole fp16 V ring, the range words of both stores."""
        from .reorder import slab
        kl = self.k_res_len if state is None else state["k_res_len"]
        h = self.nh_kv
        out = []
        if kl:
            out.append(slab(self.k_res, 0, [(h, self.k_res.stride(1) * 2)], kl * self.D * 2))
        out.append(slab(self.v_res, 0, [(h, self.v_res.stride(1) * 2)], self.v_res.shape[2] * self.D * 2))
        for st in (self.kt, self.vt):
            out.append(slab(mfma.range_flags(st), 0, [], h * 4))
        return out

    # ------------------------------------------------------------------ the 9-tuple
    def k_quant_reference_layout(self):
        if self.k_quant_len == 0:
            return None, None, None
        return mfma.kt_to_ref(self.kt, self.k_quant_len, self.D, self.cfg.group_size, self.cfg.k_bits)

    def v_quant_views(self):
        if self.v_quant_len == 0:
            return None, None, None
        return mfma.vt_to_ref(self.vt, self.v_quant_len, self.D, self.cfg.group_size, self.cfg.v_bits)

    def v_res_view(self):
        s, n, rows = self.v_res_start, self.v_res_len, self.v_res.shape[2]
        if s + n <= rows:
            return self.v_res[:, :, s: s + n]
        return torch.cat([self.v_res[:, :, s:], self.v_res[:, :, : s + n - rows]], dim=2)      # the ring wraps (9-tuple reads only)

    def allocated_bytes(self) -> int:
        return sum(x.numel() * x.element_size() for x in (self.kt, self.vt, self.k_res, self.v_res))

    # ------------------------------------------------------------------ prefill (llama_kivi.py:425-452)
    def prefill(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        cfg = self.cfg
        R, g = cfg.residual_length, cfg.group_size
        T = key_states.shape[2]
        self.reserve(T)
        self._void_checkpoints()
        if self.kv_seq_len:        # reuse of the object: the V slots are filled token by token later, start from clean storage
            for st in (self.kt, self.vt):
                st.zero_()
                mfma.range_flags(st).zero_()
        nq = (T // R) * R
        if nq:
            mfma.kt_pack(key_states[:, :, :nq], self.kt, 0, g, cfg.k_bits)
        self.k_quant_len = nq
        self.k_res_len = T - nq
        if self.k_res_len:
            self.k_res[:, :, : self.k_res_len].copy_(key_states[:, :, nq:])
        nv = max(T - R, 0)
        if nv:
            vq = value_states[:, :, :nv]
            if vq.stride(3) == 1 and vq.data_ptr() % 16 == 0 and all(st % 8 == 0 for st in vq.stride()[:3]):
                mfma.vt_pack(vq, self.vt, g, cfg.v_bits)           # one pass, straight into the layout
            else:                                                   # odd strides: through the hook-state tensors
                code, scale, mn = new_pack.triton_quantize_and_pack_along_last_dim(vq.contiguous(), g, cfg.v_bits)
                mfma.vt_from_ref(self.vt, code, scale, mn, g, cfg.v_bits)
        self.v_quant_len = nv
        self.v_res_start = 0
        self.v_res_len = T - nv
        self.v_res[:, :, : self.v_res_len].copy_(value_states[:, :, nv:])
        self.kv_seq_len = T

    @classmethod
    def from_tuple(cls, cfg: KiviConfig, past, max_len: int, num_heads: int) -> "KiviLayerCacheMF":
        kc, kfull, ks, km, vc, vfull, vs, vm, kv_len = past
        ref = vfull if vfull is not None else kfull
        B, nh_kv, _, D = ref.shape
        self = cls(cfg, B, nh_kv, D, max_len, ref.device, ref.dtype, num_heads=num_heads)
        if kc is not None:
            self.k_quant_len = kc.shape[-1] * (32 // cfg.k_bits)
            mfma.kt_from_ref(self.kt, kc.contiguous(), ks.contiguous(), km.contiguous(), cfg.group_size, cfg.k_bits)
        if vc is not None:
            self.v_quant_len = vc.shape[2]
            mfma.vt_from_ref(self.vt, vc.contiguous(), vs.contiguous(), vm.contiguous(), cfg.group_size, cfg.v_bits)
        self._adopt_residuals(past)
        return self

    # ------------------------------------------------------------------ decode step (llama_kivi.py:314-399)
    def _desc(self, nh: int, device):
        """kivi_mf_layer_desc of this cache (rebuilt when the stores were reallocated or the stream changed)."""
        stream = torch.cuda.current_stream(device).cuda_stream
        nat = self._native
        if nat is not None and nat[2] == (nh, stream):
            return nat
        pitch = ((self.n_sb * SB + self.cfg.residual_length + 1 + 7) // 8) * 8     # the longest row of any step the stores can hold
        scores, stats, ws = _scratch(device, self.B, nh, self.nh_kv, pitch, self.n_sb + 4, self.n_sb)
        kt, vt, kr, vr = self.kt, self.vt, self.k_res, self.v_res
        d = _lib.MfLayerDesc(
            B=self.B, nh_kv=self.nh_kv, D=self.D, bits=self.cfg.k_bits, group_size=self.cfg.group_size,
            residual_length=self.cfg.residual_length, inv_scale=1.0 / math.sqrt(self.D),
            cap=self.n_sb * SB, v_window_rows=vr.shape[2], s_pitch=scores.shape[3],
            kt=kt.data_ptr(), kt_sb=kt.stride(0), kt_sh=kt.stride(1), kt_ss=kt.stride(2),
            vt=vt.data_ptr(), vt_sb=vt.stride(0), vt_sh=vt.stride(1), vt_ss=vt.stride(2),
            k_res=kr.data_ptr(), kr_sb=kr.stride(0), kr_sh=kr.stride(1), kr_st=kr.stride(2),
            v_res=vr.data_ptr(), vr_sb=vr.stride(0), vr_sh=vr.stride(1), vr_st=vr.stride(2),
            scores=scores.data_ptr(), s_sb=scores.stride(0), s_sh=scores.stride(1),
            stats=stats.data_ptr(), stats_bytes=stats.numel() * 4,
            workspace=ws.data_ptr(), workspace_bytes=ws.numel(), flags=self._flags(),
            kt_range=mfma.range_flags(kt).data_ptr(), vt_range=mfma.range_flags(vt).data_ptr())
        state = (ctypes.c_int64 * 6)()
        self._native = (d, state, (nh, stream), _lib.load().kivi_mf_decode_layer, (scores, stats, ws))
        return self._native

    def _flags(self) -> int:
        return self.flags | (_lib.GQA_WINDOW_RING if self.ring else 0)

    def decode_step(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
                    attention_mask: torch.Tensor = None, out: torch.Tensor = None, fused_kernels: bool = True,
                    lead: torch.Tensor = None) -> torch.Tensor:
        """One new token in ONE library call (kivi_mf_decode_layer); `fused_kernels` is the other layout's switch (this one has no
        composed form).  `lead`: (B,) int32 on the device, the leading keys of every row that `attention_mask`
        masks -- the step goes through kivi_mf_decode_layer_lead, whose block-per-row forms skip them."""
        B, nh, _, D = query_states.shape
        assert nh == self.nh and B == self.B and D == self.D
        q, k, v = rows16(query_states), rows16(key_states), rows16(value_states)
        mask_ptr, mask_sb = mask_arg(attention_mask, B, self.kv_seq_len + 1)
        out = out_arg(out, (B, nh, 1, D), q.device)
        d, state, key, fn, _ = self._desc(nh, q.device)     # key = (nh, stream handle the descriptor was built for = the current one)
        d.flags = self._flags()
        self._store_state(state)
        hook = matmul.launch_hook
        if hook is not None and self.k_quant_len:
            hook("pre", "k", dict(B=B, nh=nh, nh_kv=self.nh_kv, K=D, N=self.k_quant_len, bits=self.cfg.k_bits,
                                  group_size=self.cfg.group_size, v_bits=self.cfg.v_bits, Tv=self.v_quant_len,
                                  k_res=self.k_res_len + 1, v_res=self.v_res_len + 1))
        args = (ctypes.byref(d), state, q.data_ptr(), q.stride(0), q.stride(1), nh, k.data_ptr(), k.stride(0), k.stride(1),
                v.data_ptr(), v.stride(0), v.stride(1), mask_ptr, mask_sb, out.data_ptr(), out.stride(0), out.stride(1))
        if lead is None:
            rc = fn(*args, key[1])
        else:
            rc = _lib.load().kivi_mf_decode_layer_lead(*args, lead_arg(lead, B), key[1])
        # the library writes `state` after every phase it has enqueued: read the lengths back whether or not the call succeeded
        self._load_state(state)
        if rc:
            _lib.check(rc, "kivi_mf_decode_layer")
        return out

    # ------------------------------------------------------------------ multi-token extend
    def extend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
               attention_mask: torch.Tensor = None, out: torch.Tensor = None, scores_dump: torch.Tensor = None) -> torch.Tensor:
        """Q >= 1 new tokens in ONE library call (kivi_mf_extend_layer): q (B, nh, Q, D), k / v (B, nh_kv, Q, D), RoPE applied.
        Chunk row i attends to the cache as it stands plus chunk tokens 0..i; `attention_mask`: optional additive
        (B, 1, Q, kv_seq_len + Q) fp16 (a view with dim-2 stride 0 -- a padding row expanded over the chunk -- is read as it is,
        without being built).  The cache afterwards is bit-identical to Q decode steps.  Returns (B, nh, Q, D) fp16.
        `scores_dump` (tests): a (B, nh, Q, >= kv_seq_len + Q) fp16 buffer with unit inner stride that receives the rows the
        softmax consumes (KIVI_GQA_DUMP_SCORES; keys a row does not see are left as they were)."""
        B, nh, Q, D = query_states.shape
        assert nh == self.nh and B == self.B and D == self.D and Q >= 1
        assert key_states.shape == value_states.shape == (B, self.nh_kv, Q, D)
        assert self.kv_seq_len > 0, "extend needs a cache: run the prompt pass first"
        self.ensure_room(Q)
        q, k, v = rows16(query_states), rows16(key_states), rows16(value_states)
        total = self.kv_seq_len + Q
        mask_ptr, mask_sb, mask_sq = None, 0, 0
        if attention_mask is not None:
            check_mask_size(attention_mask, (B, 1, Q, total))
            assert attention_mask.dtype == torch.float16
            if attention_mask.stride(2) == 0:    # one key row per batch row, expanded over the chunk: passed as mask_sq = 0
                if attention_mask.stride(3) != 1 or attention_mask.stride(0) < total:
                    row = torch.empty((B, 1, 1, total), dtype=torch.float16, device=q.device)
                    attention_mask = row.copy_(attention_mask[:, :, :1]).expand(B, 1, Q, total)
            elif attention_mask.stride(3) != 1 or attention_mask.stride(0) < Q * attention_mask.stride(2):
                attention_mask = attention_mask.contiguous()
            mask_ptr, mask_sb, mask_sq = attention_mask.data_ptr(), attention_mask.stride(0), attention_mask.stride(2)
        out = out_arg(out, (B, nh, Q, D), q.device)
        d, state, key, _, _ = self._desc(nh, q.device)
        d.flags = self._flags() & ~_lib.GQA_DUMP_SCORES     # the decode steps' dump flag: their scratch rows cannot hold Q rows
        if scores_dump is not None:              # a copy of the descriptor: the decode steps keep their scratch rows
            sd = scores_dump
            assert sd.dtype == torch.float16 and sd.dim() == 4 and sd.shape[:3] == (B, nh, Q) and sd.shape[3] >= total
            assert sd.stride(3) == 1 and sd.is_cuda
            d = _lib.MfLayerDesc.from_buffer_copy(d)
            d.flags |= _lib.GQA_DUMP_SCORES
            d.scores, d.s_sb, d.s_sh, d.s_pitch = sd.data_ptr(), sd.stride(0), sd.stride(1), sd.stride(2)
        self._store_state(state)
        rc = _lib.load().kivi_mf_extend_layer(ctypes.byref(d), state, Q, q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), nh,
                                              k.data_ptr(), k.stride(0), k.stride(1), k.stride(2), v.data_ptr(), v.stride(0),
                                              v.stride(1), v.stride(2), mask_ptr, mask_sb, mask_sq, out.data_ptr(), out.stride(0),
                                              out.stride(1), out.stride(2), key[1])
        _lib.check(rc, "kivi_mf_extend_layer")
        self._load_state(state)
        return out

    # ------------------------------------------------------------------ device-resident lengths (hipGraph capture; kivi_amd/graph.py)
    def host_step(self) -> "_lib.MfStep":
        """The six lengths of the NEXT decode step as a kivi_mf_step (include/kivi_hip.h)."""
        R = self.cfg.residual_length
        return _lib.MfStep(Tq=self.k_quant_len, Tv=self.v_quant_len, k_res_len=self.k_res_len, v_res_len=self.v_res_len,
                           v_win_start=self.v_res_start, v_flush=int(self.v_res_len + 1 > R))

    def apply_step(self, hs: "_lib.MfStep") -> None:
        """Take the lengths a driver advanced (kivi_mf_step_advance / the K flush) back into this cache."""
        self.k_quant_len, self.k_res_len, self.v_quant_len = int(hs.Tq), int(hs.k_res_len), int(hs.Tv)
        self.v_res_start, self.v_res_len = int(hs.v_win_start), int(hs.v_res_len)
        self.kv_seq_len = self.k_quant_len + self.k_res_len

    def decode_step_dyn(self, query_states, key_states, value_states, hs: "_lib.MfStep", dev_step: torch.Tensor, out: torch.Tensor,
                        attention_mask: torch.Tensor = None, lead: torch.Tensor = None) -> torch.Tensor:
        """The attend phase of one step with the lengths read from `dev_step` on the device (kivi_mf_decode_layer_dyn; with `lead`, a
        static (B,) int32 buffer the caller rewrites in place, kivi_mf_decode_layer_dyn_lead): what a hipGraph captures.  No bookkeeping happens here -- the caller advances `hs` (kivi_mf_step_advance), flushes K when due
        (flush_k) and applies the lengths (apply_step); buffers must be static across replays."""
        B, nh, _, D = query_states.shape
        assert nh == self.nh and B == self.B and D == self.D
        for t in (query_states, key_states, value_states):
            assert t.stride(3) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0, "static 16-byte rows"
        # the mask: a static (B, 1, 1, pitch >= capacity) buffer the caller refills every step
        mask_ptr, mask_sb = mask_arg(attention_mask, B, self.kv_seq_len + 1, wider=True)
        out = out_arg(out, (B, nh, 1, D), query_states.device)
        d, _, key, _, _ = self._desc(nh, query_states.device)
        d.flags = self._flags()
        q, k, v = query_states, key_states, value_states
        args = (ctypes.byref(d), ctypes.byref(hs), dev_step.data_ptr(), q.data_ptr(), q.stride(0), q.stride(1), nh, k.data_ptr(), k.stride(0),
                k.stride(1), v.data_ptr(), v.stride(0), v.stride(1), mask_ptr, mask_sb, out.data_ptr(), out.stride(0), out.stride(1))
        if lead is None:
            rc = _lib.load().kivi_mf_decode_layer_dyn(*args, key[1])
        else:
            rc = _lib.load().kivi_mf_decode_layer_dyn_lead(*args, lead_arg(lead, B), key[1])
        _lib.check(rc, "kivi_mf_decode_layer_dyn")
        return out

    def flush_k(self) -> None:
        """The K flush of llama_kivi.py:343-356 for a full residual: R tokens quantised per channel into the layout at token Tq."""
        R = self.cfg.residual_length
        assert self.k_res_len == R
        mfma.kt_pack(self.k_res, self.kt, self.k_quant_len, self.cfg.group_size, self.cfg.k_bits)
        self.k_quant_len += R
        self.k_res_len = 0


def make_layer_cache(cfg: KiviConfig, batch: int, num_kv_heads: int, head_dim: int, max_len: int, device,
                     dtype=torch.float16, num_heads: int = None):
    """The cache class for a model shape: the matrix-pipe layout for grouped queries it covers, the hook-state layout
    (KiviLayerCache) otherwise."""
    if num_heads is not None and supported(cfg, head_dim, num_heads, num_kv_heads):
        return KiviLayerCacheMF(cfg, batch, num_kv_heads, head_dim, max_len, device, dtype, num_heads=num_heads)
    return KiviLayerCache(cfg, batch, num_kv_heads, head_dim, max_len, device, dtype)
