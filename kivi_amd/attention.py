"""The KIVI attention hook: decode / prefill cache logic of the reference's
LlamaFlashAttention_KIVI.forward (models/llama_kivi.py:265-466) on the HIP kernels.

Same arithmetic sequence as the reference decode branch (:314-399):
  scores  = cat([ fused qK^T over packed K , q @ K_residual^T ]) / sqrt(D)      (fp16)
  weights = softmax(scores, fp32) -> fp16
  out     = fused sV over packed V  +  weights[..., -L:] @ V_residual           (fp16)
with the cache policy of cache.py.  What changed is data movement only: the fused GEMVs read the
hook-state layout directly and write into a scores buffer (no torch.cat, no transposed copies), and
the cache is appended in place.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, _tuning
from . import generation as _generation
from . import prefill as _prefill
from . import qkrope as _qkrope
from .cache import KiviCacheTuple, KiviConfig, KiviLayerCache, KiviPerformanceWarning  # noqa: F401
from .cache_mf import KiviLayerCacheMF, make_layer_cache, padded_heads as _padded_heads, supported as _mf_supported
from .wquant import make_linear

__all__ = ["kivi_attention_decode", "kivi_attention_prefill", "LlamaAttention_KIVI", "LlamaFlashAttention_KIVI",
           "MistralAttention_KIVI", "MistralFlashAttention_KIVI", "QwenAttention_KIVI",
           "KiviConfig", "KiviLayerCache", "KiviLayerCacheMF", "make_layer_cache"]


_NATIVE_STEP = _tuning.knob("KIVI_NATIVE_STEP", "1") != "0"   # tuning sessions: 0 = the Python bookkeeping path (read by KiviLayerCache.decode_step)


def kivi_attention_decode(query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
                          layer: KiviLayerCache, attention_mask: Optional[torch.Tensor] = None,
                          fused_kernels: bool = True, out: Optional[torch.Tensor] = None,
                          lead: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decode step for one layer.  query (B, nh, 1, D), key/value (B, nh_kv, 1, D), RoPE already applied.
    Mutates `layer` in place and returns attn_output (B, nh, 1, D) fp16 (before the o_proj transpose).
    `fused_kernels=False` forces the reference-style composition (one launch per reference op).
    `out`: optional preallocated (B, nh, 1, D) fp16 result buffer (static buffers of graph-captured callers).
    `lead`: (B,) int32 on the device -- the caller's promise that `attention_mask` masks keys [0, lead[b]) of
    row b (and not the new token).  The one-launch row kernels of the matrix-pipe layout then skip the packed K and V under it; every
    other form and the hook-state layout ignore it.  None: the call as it always was."""
    layer.ensure_room(1)     # the reference's tuple grows without bound; the in-place cache doubles when it is full
    if lead is None:
        res = layer.decode_step(query_states, key_states, value_states, attention_mask, out, fused_kernels)
    else:
        res = layer.decode_step(query_states, key_states, value_states, attention_mask, out, fused_kernels, lead=lead)
    if out is not None and res is not out:
        out.copy_(res)
        return out
    return res


def kivi_attention_extend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, layer, attention_mask: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Q >= 1 new tokens for one layer that already holds a cache (multi-turn continuation, a prompt fed in pieces, a block of
    draft tokens).  q (B, nh, Q, D), k / v (B, nh_kv, Q, D) fp16, RoPE applied.  Chunk row i sits at position P0 + i
    (P0 = layer.kv_seq_len before the call) and attends to the whole cache as it stood plus chunk tokens 0..i (causal, always);
    `attention_mask`: optional additive (B, 1, Q, P0 + Q) fp16 mask on top (a padding row expanded over the chunk -- dim-2 stride 0 --
    is read without being built).  Mutates `layer` in place -- afterwards it is
    bit-identical to Q decode steps fed the same keys and values -- and returns (B, nh, Q, D) fp16."""
    return layer.extend(q, k, v, attention_mask, out)


def kivi_attention_prefill(query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
                           layer: KiviLayerCache, attention_mask: Optional[torch.Tensor] = None, lead: Optional[torch.Tensor] = None,
                           kernel: bool = False) -> torch.Tensor:
    """Prompt pass (:401-452): attention over fp16 q/k/v, then split K/V into the quantised prefix and the fp16 residual.

    `attention_mask` None: causal -- the flash class, whose mask argument is hard-wired to None (:420-423).  Given
    (additive, (bsz, 1, q_len, kv_len), causal structure included, as HF builds it): the eager class's
    `attn_weights + attention_mask` (:228-237), e.g. for left-padded batches; a wrong shape raises like the reference.

    `kernel=False`: torch SDPA over K / V repeated per query head.  `kernel=True`: kivi_prefill_attention --
    causal, grouped queries mapped inside the kernel, `lead` (B,) int32 leading pads per row (a query attends to the keys from its
    row's lead on, the pads' own outputs are exact zeros) -- on GPU fp16 tensors of head_dim 128 with nh / nh_kv in {1, 2, 4, 8}, the
    torch restatement of the same contract otherwise (kivi_amd/prefill.py).  The kernel knows causal + lead only: an
    `attention_mask` given together with `kernel=True` takes the masked SDPA path unchanged.  `layer.prefill` sees the same
    tensors in every form."""
    if kernel and attention_mask is None:
        attn_output = _prefill.attention(query_states, key_states, value_states, lead)
        layer.prefill(key_states, value_states)
        return attn_output
    if lead is not None:
        raise ValueError("kivi_attention_prefill: `lead` belongs to kernel=True without an attention_mask")
    B, nh, T, D = query_states.shape
    rep = nh // layer.nh_kv
    k, v = key_states, value_states
    if rep > 1:
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    if attention_mask is None:
        attn_output = F.scaled_dot_product_attention(query_states, k, v, is_causal=True)
    else:
        if tuple(attention_mask.shape) != (B, 1, T, key_states.shape[-2]):
            raise ValueError(f"Attention mask should be of size {(B, 1, T, key_states.shape[-2])}, but is "
                             f"{tuple(attention_mask.shape)}")
        attn_output = F.scaled_dot_product_attention(query_states, k, v, attn_mask=attention_mask.to(query_states.dtype))
    layer.prefill(key_states, value_states)
    return attn_output


# --------------------------------------------------------------------------- module hook

def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def _rope_inv_freq(config, head_dim: int, theta: float) -> torch.Tensor:
    """Rotary frequencies incl. config.json's rope_scaling (the reference delegates RoPE to HF's rotary_emb,
    llama_kivi.py:52, which honours it): default, "linear" and Llama-3.1's "llama3" are implemented; anything else
    raises instead of decoding with silently wrong positions."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    rs = getattr(config, "rope_scaling", None)
    if not rs:
        return inv_freq
    rs = dict(rs) if not isinstance(rs, dict) else rs
    kind = rs.get("rope_type", rs.get("type", "default"))
    if kind == "default":
        return inv_freq
    if kind == "linear":
        return inv_freq / float(rs["factor"])
    if kind == "llama3":
        factor, lo, hi = float(rs["factor"]), float(rs["low_freq_factor"]), float(rs["high_freq_factor"])
        old = float(rs["original_max_position_embeddings"])
        wavelen = 2 * math.pi / inv_freq
        scaled = torch.where(wavelen > old / lo, inv_freq / factor, inv_freq)
        smooth = (old / wavelen - lo) / (hi - lo)
        medium = (wavelen >= old / hi) & (wavelen <= old / lo)
        return torch.where(medium, (1 - smooth) * scaled / factor + smooth * scaled, scaled)
    raise NotImplementedError(f"rope_scaling type {kind!r} is not implemented (default / linear / llama3 are)")


def rope_cos_sin(inv_freq: torch.Tensor, positions, dtype=None):
    """(cos, sin) of the rotary embedding, shape positions.shape + (head_dim,): `positions` an integer tensor, or a Python int (one
    position for every row).  fp32 arithmetic as HF's rotary_emb does it; `dtype`: the cast of the result (None: left to the
    copy_ into the caller's buffer)."""
    if torch.is_tensor(positions):
        positions = positions[..., None].float()
    freqs = positions * inv_freq.float()
    emb = torch.cat((freqs, freqs), dim=-1)
    cos, sin = emb.cos(), emb.sin()
    return (cos, sin) if dtype is None else (cos.to(dtype), sin.to(dtype))


_ROPE_CACHE = {}   # (device, dtype, head_dim, theta, rope_scaling, past_len, q_len) -> (cos, sin) of the current step


class LlamaAttention_KIVI(nn.Module):
    """Self-contained Llama attention block with the KIVI cache hook (reference: LlamaFlashAttention_KIVI,
    models/llama_kivi.py:264-466; constructor fields :22-61).

    `config` needs hidden_size, num_attention_heads, num_key_value_heads, max_position_embeddings, rope_theta and
    the four KIVI fields the reference monkey-patches onto the HF config (README.md:72-75): k_bits, v_bits,
    group_size, residual_length.  forward() keeps the reference signature and returns
    (attn_output, None, past_key_value) with past_key_value the 9-tuple of :454-455.
    """

    # the eager class adds `attention_mask` to the prompt pass's scores (:228-237); the flash subclass does not (:420-423).
    # config.kivi_prefill_kernel (off by default): the prompt pass runs kivi_prefill_attention, and a left-padded one arrives as a
    # PromptLead in place of the mask -- every class then serves it
    _prefill_uses_mask = True

    def __init__(self, config, layer_idx: Optional[int] = None):
        super().__init__()
        self.config = config
        self.layer_idx = layer_idx
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = getattr(config, "head_dim", None) or self.hidden_size // self.num_heads
        self.num_key_value_heads = getattr(config, "num_key_value_heads", self.num_heads)
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.max_position_embeddings = getattr(config, "max_position_embeddings", 4096)
        self.rope_theta = getattr(config, "rope_theta", 10000.0)
        self.kivi = KiviConfig(config.k_bits, config.v_bits, config.group_size, config.residual_length)
        self.prefill_kernel = bool(getattr(config, "kivi_prefill_kernel", False))
        self.k_bits, self.v_bits = config.k_bits, config.v_bits
        self.group_size, self.residual_length = config.group_size, config.residual_length
        if self.head_dim * self.num_heads != self.hidden_size and getattr(config, "head_dim", None) is None:
            raise ValueError("hidden_size must be divisible by num_heads")
        bias = getattr(config, "attention_bias", False)
        # nn.Linear, with config.kivi_weight_bits == 4 the 4-bit QuantLinear, with config.kivi_fp8_weights the
        # Fp8Linear (section 35), which a checkpoint's `modules_to_not_convert` may keep dense by the module's dotted name
        self.q_proj = make_linear(config, self.hidden_size, self.num_heads * self.head_dim, bias=bias, name=self._proj_name("q_proj"))
        self.k_proj = make_linear(config, self.hidden_size, self.num_key_value_heads * self.head_dim, bias=bias,
                                  name=self._proj_name("k_proj"))
        self.v_proj = make_linear(config, self.hidden_size, self.num_key_value_heads * self.head_dim, bias=bias,
                                  name=self._proj_name("v_proj"))
        self.o_proj = make_linear(config, self.num_heads * self.head_dim, self.hidden_size, bias=bias, name=self._proj_name("o_proj"))
        self.register_buffer("inv_freq", _rope_inv_freq(config, self.head_dim, self.rope_theta), persistent=False)
        # config.kivi_qk_kernel (off by default): q / k are prepared by one kivi_qk_rope launch, and a query-group
        # ratio the matrix-pipe layout does not serve runs on it padded: `cache_heads` query heads, nh_kv * the padded ratio
        self.qk_kernel = bool(getattr(config, "kivi_qk_kernel", False))
        self.cache_heads = self.num_heads
        if self.qk_kernel:
            self.cache_heads = _padded_heads(self.kivi, self.head_dim, self.num_heads, self.num_key_value_heads) or self.num_heads
        self.q_norm = self.k_norm = None            # the per-head RMSNorm of q and k before RoPE (QwenAttention_KIVI)

    def _proj_name(self, leaf: str) -> Optional[str]:
        """The projection's dotted name in the model (a checkpoint's names), or None for a block built outside a model."""
        return None if self.layer_idx is None else f"model.layers.{self.layer_idx}.self_attn.{leaf}"

    def _rope(self, q, k, position_ids):
        cos, sin = (x[:, None] for x in rope_cos_sin(self.inv_freq, position_ids, q.dtype))   # (B, 1, T, D)
        return q * cos + _rotate_half(q) * sin, k * cos + _rotate_half(k) * sin

    def _step_cos_sin(self, device, dtype, past_len: int, q_len: int):
        """cos / sin (1, 1, q_len, D) of consecutive positions from past_len on: the same for every layer of a step, so kept."""
        key = (device, dtype, self.head_dim, self.rope_theta, repr(getattr(self.config, "rope_scaling", None)), past_len, q_len)
        cs = _ROPE_CACHE.get(key)
        if cs is None:
            pos = torch.arange(past_len, past_len + q_len, device=device)[None]
            cs = tuple(x[:, None] for x in rope_cos_sin(self.inv_freq, pos, dtype))
            _ROPE_CACHE.clear()
            _ROPE_CACHE[key] = cs
        return cs

    def _prepared_qkv(self, hidden_states, position_ids, past_len: int, heads: int):
        """q, k, v of config.kivi_qk_kernel and of the classes with a head norm: head norm, RoPE and the
        head-major placement in one kivi_qk_rope launch, the query groups padded to `heads` query heads in all -- or, with the
        option off or outside what the kernel serves, the torch chain of the same formula (which cannot pad)."""
        bsz, q_len, _ = hidden_states.size()
        q_in = self.q_proj(hidden_states).view(bsz, q_len, self.num_heads, self.head_dim)
        k_in = self.k_proj(hidden_states).view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        v = self.v_proj(hidden_states).view(bsz, q_len, self.num_key_value_heads, self.head_dim).transpose(1, 2)
        if position_ids is None:
            cos, sin = (x[:, 0] for x in self._step_cos_sin(hidden_states.device, q_in.dtype, past_len, q_len))
        else:
            cos, sin = rope_cos_sin(self.inv_freq, position_ids, q_in.dtype)                    # (B, T, D)
        return self.prepare_qk(q_in, k_in, cos, sin, heads) + (v,)

    def prepare_qk(self, q_in, k_in, cos, sin, heads: int, q_out=None, k_out=None):
        """q_in (B, Q, nh, D), k_in (B, Q, nh_kv, D), cos / sin (1 or B, Q, D) -> q (B, heads, Q, D), k (B, nh_kv, Q, D), in
        `q_out` / `k_out` when given (the static buffers of a captured step)."""
        qw, kw, eps = (None, None, 0.0) if self.q_norm is None else (self.q_norm.weight, self.k_norm.weight, self.q_norm.eps)
        if self.qk_kernel and _qkrope.usable(q_in, self.head_dim):
            return _qkrope.qk_rope(q_in, k_in, cos, sin, heads // self.num_key_value_heads, qw, kw, eps, q_out, k_out)
        if heads != self.num_heads:
            raise _lib.KiviHipError("padded query groups need kivi_qk_rope: fp16 tensors on the GPU")
        q, k = _qkrope.qk_rope_torch(q_in, k_in, cos, sin, qw, kw, eps)
        return (q, k) if q_out is None else (q_out.copy_(q), k_out.copy_(k))

    def inv_freq_exact(self, device) -> torch.Tensor:
        """The rotary frequencies in fp32 whatever the module was cast to (`inv_freq` is a buffer: .bfloat16() rounds it to 8 bits):
        what the boundary's fp32 tables are made from."""
        t = self.__dict__.get("_inv_freq_exact")
        if t is None or t.device != device:
            t = self.__dict__["_inv_freq_exact"] = _rope_inv_freq(self.config, self.head_dim, self.rope_theta).to(device)
        return t

    def _boundary_qkv(self, hidden_states, position_ids, past_len: int, heads: int):
        """q, k, v of a model whose hidden states are not fp16: fp16, by one kivi_qkv_rope_bf16 launch or the
        torch restatement of its contract, from fp32 cos / sin tables."""
        _lib.require_gpu(hidden_states, "hidden_states")    # (the cache behind the boundary has no CPU path)
        bsz, q_len, _ = hidden_states.size()
        q_in = self.q_proj(hidden_states).view(bsz, q_len, self.num_heads, self.head_dim)
        k_in = self.k_proj(hidden_states).view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        v_in = self.v_proj(hidden_states).view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        device = hidden_states.device
        if position_ids is None:
            key = (device, "exact", self.head_dim, self.rope_theta, repr(getattr(self.config, "rope_scaling", None)), past_len, q_len)
            cs = _ROPE_CACHE.get(key)
            if cs is None:
                pos = torch.arange(past_len, past_len + q_len, device=device)[None]
                cs = rope_cos_sin(self.inv_freq_exact(device), pos)
                _ROPE_CACHE.clear()
                _ROPE_CACHE[key] = cs
            cos, sin = cs
        else:
            cos, sin = rope_cos_sin(self.inv_freq_exact(device), position_ids)                  # (B, T, D) fp32
        return self.boundary_qkv(q_in, k_in, v_in, cos, sin, heads)

    def boundary_qkv(self, q_in, k_in, v_in, cos, sin, heads: int, q_out=None, k_out=None, v_out=None):
        """q_in (B, Q, nh, D), k_in / v_in (B, Q, nh_kv, D) bf16 (fp32: the torch path), cos / sin (1 or B, Q, D) fp32 -> fp16
        q (B, heads, Q, D), k, v (B, nh_kv, Q, D), in the `_out` buffers when given.  The kernel serves wherever it can, with
        config.kivi_qk_kernel or without; only that option pads the query groups."""
        qw, kw, eps = (None, None, 0.0) if self.q_norm is None else (self.q_norm.weight, self.k_norm.weight, self.q_norm.eps)
        if _qkrope.boundary_usable(q_in, self.head_dim):
            return _qkrope.qkv_rope_bf16(q_in, k_in, v_in, cos, sin, heads // self.num_key_value_heads, qw, kw, eps, q_out, k_out,
                                         v_out)
        q, k, v = _qkrope.qkv_rope_bf16_torch(q_in, k_in, v_in, cos, sin, qw, kw, eps)
        if heads != self.num_heads:                 # (an fp32 model over padded caches: the zero heads by a copy)
            q = _qkrope.pad_groups(q, self.num_key_value_heads, heads // self.num_key_value_heads)
        return (q, k, v) if q_out is None else (q_out.copy_(q), k_out.copy_(k), v_out.copy_(v))

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.LongTensor] = None, past_key_value=None, output_attentions: bool = False,
                use_cache: bool = False, **kwargs) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[tuple]]:
        bsz, q_len, _ = hidden_states.size()
        past_len = 0 if past_key_value is None else int(past_key_value[-1])
        # a bf16 model, or an fp32 one on the GPU (the dense reference of the tests): q, k, v cross into fp16 here, the output back
        # below.  (fp32 modules off the GPU keep the path they had: host-side tests drive it over stand-in caches.)
        boundary = hidden_states.dtype == torch.bfloat16 or (hidden_states.dtype != torch.float16 and hidden_states.is_cuda)
        if boundary:
            heads = self.num_heads
            if isinstance(past_key_value, KiviCacheTuple):
                heads = getattr(past_key_value.layer, "nh", self.num_heads)
            elif past_key_value is not None:
                heads = self.cache_heads
            q, k, v = self._boundary_qkv(hidden_states, position_ids, past_len, heads)
        elif self.qk_kernel or self.q_norm is not None:
            heads = self.num_heads                  # the prompt pass launches nothing over the cache with q: no pad heads
            if isinstance(past_key_value, KiviCacheTuple):      # over a cache: as many query heads as it was built for
                heads = getattr(past_key_value.layer, "nh", self.num_heads)
            elif past_key_value is not None:                    # a plain tuple: the cache made of it below
                heads = self.cache_heads
            q, k, v = self._prepared_qkv(hidden_states, position_ids, past_len, heads)
        else:
            q = self.q_proj(hidden_states).view(bsz, q_len, self.num_heads, self.head_dim).transpose(1, 2)
            k = self.k_proj(hidden_states).view(bsz, q_len, self.num_key_value_heads, self.head_dim).transpose(1, 2)
            v = self.v_proj(hidden_states).view(bsz, q_len, self.num_key_value_heads, self.head_dim).transpose(1, 2)
            if position_ids is None:   # consecutive positions: cos / sin are the same for every layer of this step
                cos, sin = self._step_cos_sin(hidden_states.device, q.dtype, past_len, q_len)
                q, k = q * cos + _rotate_half(q) * sin, k * cos + _rotate_half(k) * sin
            else:
                q, k = self._rope(q, k, position_ids)

        if past_key_value is not None:
            if isinstance(past_key_value, KiviCacheTuple):
                layer = past_key_value.layer
                if past_len != layer.kv_seq_len:
                    # the reference's tuple is an immutable snapshot; this one is a single-use handle on a cache that is
                    # appended in place -- replaying an older one would append twice and rotate at the wrong position
                    raise RuntimeError(
                        f"stale KIVI past_key_value: the tuple was issued at kv length {past_len}, its cache has since "
                        f"advanced to {layer.kv_seq_len}. In-place cache tuples are single-use; clone the cache "
                        f"(KiviLayerCache.clone()) to continue one prefix twice.")
            elif _mf_supported(self.kivi, self.head_dim, self.cache_heads, self.num_key_value_heads):
                layer = KiviLayerCacheMF.from_tuple(self.kivi, past_key_value, self._capacity(past_len + q_len), self.cache_heads)
            else:  # a plain reference-style tuple: adopt it once
                layer = KiviLayerCache.from_tuple(self.kivi, past_key_value, self._capacity(past_len + q_len))
            if isinstance(attention_mask, _generation.DecodeLead):   # config.kivi_decode_lead: the key row travels with its lead
                if q_len > 1:                                        # (an extend ignores the lead)
                    attn_output = kivi_attention_extend(q, k, v, layer, attention_mask.mask.expand(-1, -1, q_len, -1))
                else:
                    attn_output = kivi_attention_decode(q, k, v, layer, attention_mask.mask, lead=attention_mask.lead)
            elif q_len > 1:
                attn_output = kivi_attention_extend(q, k, v, layer, attention_mask)
            else:
                attn_output = kivi_attention_decode(q, k, v, layer, attention_mask)
        else:
            layer = make_layer_cache(self.kivi, bsz, self.num_key_value_heads, self.head_dim, self._capacity(q_len),
                                     hidden_states.device, q.dtype, num_heads=self.cache_heads)
            mask = attention_mask if self._prefill_uses_mask else None
            if isinstance(attention_mask, _prefill.PromptLead):
                attn_output = kivi_attention_prefill(q, k, v, layer, None, lead=attention_mask.lead, kernel=True)
            elif self.prefill_kernel:
                attn_output = kivi_attention_prefill(q, k, v, layer, mask, kernel=True)
            else:                                          # the option is off: the call as it always was
                attn_output = kivi_attention_prefill(q, k, v, layer, mask)
        past = layer.as_tuple() if use_cache else None                                     # :454-455
        if boundary:                                     # the way back: the one copy in front of o_proj casts too
            attn_output = _qkrope.unpad(attn_output, self.num_key_value_heads, self.num_key_value_groups, hidden_states.dtype)
        elif attn_output.shape[1] != self.num_heads:     # padded query groups: the pad heads' outputs stay behind
            attn_output = _qkrope.unpad(attn_output, self.num_key_value_heads, self.num_key_value_groups)
        else:
            attn_output = attn_output.transpose(1, 2).reshape(bsz, q_len, self.num_heads * self.head_dim)
        return self.o_proj(attn_output), None, past

    def _capacity(self, needed: int) -> int:
        """Initial cache capacity: the prompt plus one residual window (the cache doubles when it runs out, like the
        reference's torch.cat-grown tuple, so memory follows the sequence; the matrix-pipe stores round it up to whole
        512-token super-blocks).  `config.kivi_max_cache_len` is an opt-in reservation for callers that know their final
        length; max_position_embeddings is never used (a 128k-context config would otherwise pre-allocate GBs per sequence
        for a 1k-token run)."""
        reserve = getattr(self.config, "kivi_max_cache_len", None) or 0
        return max(needed + self.residual_length, reserve)


class LlamaFlashAttention_KIVI(LlamaAttention_KIVI):
    """Reference: LlamaFlashAttention_KIVI (models/llama_kivi.py:264-466): same cache logic as the eager class; its prompt
    pass is causal flash attention with the mask argument hard-wired to None (:420-423), so `attention_mask` only
    reaches the decode steps."""
    _prefill_uses_mask = False


class MistralAttention_KIVI(LlamaAttention_KIVI):
    """Reference: MistralAttention_KIVI / MistralFlashAttention_KIVI (models/mistral_kivi.py:69-534).  Against the Llama
    hook the reference differs in three places, all reproduced or made unnecessary here:
      * projections never carry a bias (:96-99) -- `attention_bias` of the config is ignored;
      * grouped queries reach the fused GEMV through `repeat_kv_quant` copies of codes / scale / mn (:58-67, :381-385,
        :441-445, a 4x cache-sized copy per call at Mistral-7B's ratio); the kernels here map the nh / nh_kv query heads
        of a kv head themselves (gemv_cuda.cu:361-365 semantics), same results, no copy;
      * `config.sliding_window` exists but is never applied to the quantised history (:356-367 is commented out):
        the whole prefix stays attended.  The field is kept on the module for callers that inspect it."""

    def __init__(self, config, layer_idx: Optional[int] = None):
        if getattr(config, "attention_bias", False):
            from types import SimpleNamespace
            config = SimpleNamespace(**{**vars(config), "attention_bias": False})
        super().__init__(config, layer_idx)
        self.sliding_window = getattr(config, "sliding_window", None)


class HeadRMSNorm(nn.Module):
    """HF's Qwen3RMSNorm over head_dim, applied to every head of q / k before RoPE.  With config.kivi_qk_kernel its weight and eps go
    to kivi_qk_rope; forward() is the torch path of the same formula."""

    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        return _qkrope.head_norm(x, self.weight, self.eps)


class QwenAttention_KIVI(LlamaAttention_KIVI):
    """The attention block of HF's Qwen2 / Qwen3 around the same cache hook.  Against the Llama block:
      * `o_proj` never carries a bias; q / k / v carry one when `config.attention_bias` says so (Qwen2ForCausalLM_KIVI sets it:
        HF's Qwen2 always biases the three);
      * `config.kivi_head_norm` (Qwen3): `q_norm` / `k_norm`, an RMSNorm over head_dim with a weight of its own on every head of
        q and of k, before RoPE;
      * a sliding window is refused: the quantised history has no window here."""

    def __init__(self, config, layer_idx: Optional[int] = None):
        if getattr(config, "use_sliding_window", False):
            raise ValueError("use_sliding_window=True: the quantised KV history has no sliding window; load the model with "
                             "use_sliding_window=false (full attention) or do not use this cache")
        super().__init__(config, layer_idx)
        self.o_proj = make_linear(config, self.num_heads * self.head_dim, self.hidden_size, bias=False, name=self._proj_name("o_proj"))
        if getattr(config, "kivi_head_norm", False):
            eps = getattr(config, "rms_norm_eps", 1e-6)
            self.q_norm, self.k_norm = HeadRMSNorm(self.head_dim, eps), HeadRMSNorm(self.head_dim, eps)


class MistralFlashAttention_KIVI(MistralAttention_KIVI):
    """Reference: MistralFlashAttention_KIVI (models/mistral_kivi.py:319-534): causal flash prompt pass, no mask."""
    _prefill_uses_mask = False
