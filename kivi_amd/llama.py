"""A Llama / Mistral-shaped decoder around the KIVI attention hook -- the callers' side of the hot path.

Counterpart of the reference's LlamaForCausalLM_KIVI / MistralForCausalLM_KIVI wrappers (models/llama_kivi.py:564-1000,
models/mistral_kivi.py:673-1100) reduced to what decoding needs: token embedding, pre-norm decoder blocks
(RMSNorm, LlamaAttention_KIVI, SwiGLU MLP), final norm, lm_head, and the public methods of generation, scoring and checkpoints.
Parameter names follow the Hugging Face checkpoints (model.embed_tokens, model.layers.N.self_attn.q_proj, ..., lm_head), so
`load_state_dict` / `from_pretrained` take an unmodified Llama-2 / Llama-3 / Mistral checkpoint directory -- what lies between
such a directory and the filled model (config.json, the checkpoint's spellings, 4-bit packing, completeness) is
kivi_amd/loading.py; here are the family table, make_config and the modules.  Everything outside the attention block is plain
torch (rocBLAS / hipBLASLt GEMMs).  The reference patches k_bits / v_bits / group_size / residual_length onto the HF config
(README.md:72-75); the same four fields are read here.
The public methods carry the API documentation and delegate: what a generate call is made of (padding, sampler, prompt pass, eager
step, decode loop) is kivi_amd/generation.py; beam search kivi_amd/beam.py; the graphed step and the calls over it kivi_amd/graph.py;
score / perplexity kivi_amd/scoring.py; the scheduler kivi_amd/serving.py (over admit_() and kivi_amd/admit.py).  DESIGN.md section 33.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import admit, graph, loading, lora, scoring, serving, wquant
from .attention import LlamaAttention_KIVI
from .beam import beam_search
from .generation import (PADS_LEFT, DecodeLead, EagerStepper, _PaddedBatch, decode_loop, leading_pads, left_pad,  # noqa: F401
                         padding_key_row, padding_position_ids, padding_prompt_mask, observe_prompts, bind_suppress,
                         pack_result, resolve_sampler)
from .moe import QuantExperts, SparseMoeBlock
from .prefill import left_padded
from .stopping import SYNC_EVERY, StopRows, resolve_stopping


_SHARED_EXPERT_FIELDS = ("shared_expert_intermediate_size", "n_shared_experts", "num_shared_experts")


def make_config(d: dict, k_bits: int = 2, v_bits: int = 2, group_size: int = 32, residual_length: int = 32,
                max_cache_len: Optional[int] = None, prefill_kernel: bool = False, decode_lead: bool = False,
                qk_kernel: bool = False, moe_kernel: bool = True, moe_kernel_max_tokens: Optional[int] = None,
                weight_bits: Optional[int] = None, weight_group: int = 128,
                weight_kernel_max_tokens: Optional[int] = None, expert_bits: Optional[int] = None,
                expert_group: int = 128, fp8_weights: bool = False, fp8_skip_modules=None,
                fp8_experts: bool = False) -> SimpleNamespace:
    """HF config.json fields (+ the four KIVI fields) -> the namespace the modules read.  `prefill_kernel`: the prompt pass's
    attention runs kivi_prefill_attention, and every attention class serves left-padded prompts.
    `decode_lead`: the decode steps of a padded batch hand the kernels every row's leading pads, and the row kernels skip the packed
    K and V under them.  `qk_kernel`: q and k are prepared by one kivi_qk_rope launch per layer, and a model
    whose nh / nh_kv the matrix-pipe layout does not serve runs on it with padded query groups.
    A sparse mixture-of-experts config (Mixtral: `num_local_experts`; Qwen3-MoE: `num_experts`) also carries
    num_experts, num_experts_per_tok, moe_intermediate_size (Mixtral's `intermediate_size`), norm_topk_prob (always true for
    Mixtral), decoder_sparse_step and mlp_only_layers; `moe_kernel`: its routed blocks run kivi_moe_route / kivi_moe_experts, for at
    most `moe_kernel_max_tokens` tokens outside a capture (None: kivi_amd.moe.KERNEL_MAX_TOKENS).  Shared experts are refused.
    `weight_bits`: None, or 4 for 4-bit attention projections and dense MLPs in groups of `weight_group` (64 or 128) input channels
    (kivi_amd/wquant.py): the kernel runs under capture and for at most `weight_kernel_max_tokens` tokens
    otherwise (None: kivi_amd.wquant.KERNEL_MAX_TOKENS); embeddings, lm_head and the experts of a sparse block keep the model dtype.
    `expert_bits`: None, or 4 for 4-bit experts in the sparse blocks, in groups of `expert_group` (64 or 128) along the reduction
    axis (kivi_amd.moe.QuantExperts): the block dequantises each hit expert and runs the loop; it has no
    capturable form, so the graphed decode paths raise on such a model.  Independent of `weight_bits`; a config without experts
    refuses it.
    `fp8_weights`: the attention projections and dense MLPs hold FP8 weights in the form of transformers' fine-grained FP8
    checkpoints -- e4m3fn bytes and one fp32 `weight_scale_inv` per [128, 128] block -- under 16-bit activations (kivi_amd/wfp8.py,
    DESIGN.md section 35); `weight_kernel_max_tokens` bounds its kernel as it does the 4-bit one (None:
    kivi_amd.wfp8.KERNEL_MAX_TOKENS).  `fp8_skip_modules`: a checkpoint's `modules_to_not_convert`, patterns of module names that
    stay dense.  Embeddings, lm_head and the experts of a sparse block keep the model dtype.  Together with `weight_bits=4` it
    raises: the two are formats of the same weights; together with `expert_bits=4` it raises as well.
    `fp8_experts`: the experts of the sparse blocks hold the same FP8 format (kivi_amd.moe.Fp8Experts) and run
    kivi_moe_experts_w8, which a captured decode step may hold; H and the experts' intermediate size must be multiples of 128.  Given
    alone or with `fp8_weights`; with `expert_bits=4` or `weight_bits=4` it raises, and a config without experts refuses it."""
    if weight_bits not in (None, 4):
        raise ValueError(f"weight_bits has to be None or 4, got {weight_bits!r}")
    if weight_bits is not None and weight_group not in wquant.GROUPS:
        raise ValueError(f"weight_group has to be one of {wquant.GROUPS}, got {weight_group!r}")
    if expert_bits not in (None, 4):
        raise ValueError(f"expert_bits has to be None or 4, got {expert_bits!r}")
    if expert_bits is not None and expert_group not in wquant.GROUPS:
        raise ValueError(f"expert_group has to be one of {wquant.GROUPS}, got {expert_group!r}")
    if fp8_weights and weight_bits is not None:
        raise ValueError("fp8_weights and weight_bits=4 are two formats of the same weights: choose one")
    if fp8_weights and expert_bits is not None:
        raise ValueError("fp8_weights together with expert_bits=4 is not served: save_quantized has no format that holds both")
    if fp8_experts and expert_bits is not None:
        raise ValueError("fp8_experts and expert_bits=4 are two formats of the same experts: choose one")
    if fp8_experts and weight_bits is not None:
        raise ValueError("fp8_experts together with weight_bits=4 is not served: save_quantized has no format that holds both")
    extra = {}
    if fp8_weights:                         # (absent otherwise: the default namespace is what it was)
        extra = dict(kivi_fp8_weights=True, kivi_fp8_skip=None if fp8_skip_modules is None else list(fp8_skip_modules),
                     kivi_weight_kernel_max_tokens=weight_kernel_max_tokens, kivi_hf_config=dict(d))
    if weight_bits is not None:             # (absent otherwise: the default namespace is what it was)
        extra = dict(kivi_weight_bits=weight_bits, kivi_weight_group=weight_group,
                     kivi_weight_kernel_max_tokens=weight_kernel_max_tokens, kivi_hf_config=dict(d))
    if expert_bits is not None:
        if not int(d.get("num_local_experts", d.get("num_experts", 0)) or 0):
            raise ValueError("expert_bits: the config has no experts (num_local_experts / num_experts)")
        extra.update(kivi_expert_bits=expert_bits, kivi_expert_group=expert_group, kivi_hf_config=dict(d))
    if fp8_experts:                         # (absent otherwise)
        if not int(d.get("num_local_experts", d.get("num_experts", 0)) or 0):
            raise ValueError("fp8_experts: the config has no experts (num_local_experts / num_experts)")
        extra.update(kivi_fp8_experts=True, kivi_hf_config=dict(d))
    hidden, heads = d["hidden_size"], d["num_attention_heads"]
    for field in _SHARED_EXPERT_FIELDS:
        if d.get(field):
            raise ValueError(f"config field `{field}` = {d[field]!r} asks for a shared expert, which the sparse block here does not "
                             f"have (Qwen2-MoE, DeepSeek): only routed experts are served")
    mixtral = "num_local_experts" in d or d.get("model_type") == "mixtral"
    num_experts = int(d.get("num_local_experts", d.get("num_experts", 0)) or 0)
    return SimpleNamespace(
        hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=d.get("num_key_value_heads", heads),
        num_hidden_layers=d["num_hidden_layers"], intermediate_size=d["intermediate_size"], vocab_size=d["vocab_size"],
        max_position_embeddings=d.get("max_position_embeddings", 4096), rope_theta=d.get("rope_theta", 10000.0),
        rms_norm_eps=d.get("rms_norm_eps", 1e-5), attention_bias=d.get("attention_bias", False),
        rope_scaling=d.get("rope_scaling"), head_dim=d.get("head_dim"), sliding_window=d.get("sliding_window"),
        tie_word_embeddings=d.get("tie_word_embeddings", False),
        k_bits=d.get("k_bits", k_bits), v_bits=d.get("v_bits", v_bits), group_size=d.get("group_size", group_size),
        residual_length=d.get("residual_length", residual_length),
        kivi_max_cache_len=max_cache_len,   # opt-in reservation; by default the cache starts prompt-sized and doubles
        kivi_prefill_kernel=bool(prefill_kernel), kivi_decode_lead=bool(decode_lead), kivi_qk_kernel=bool(qk_kernel),
        model_type=d.get("model_type"), use_sliding_window=bool(d.get("use_sliding_window", False)),
        num_experts=num_experts, num_experts_per_tok=int(d.get("num_experts_per_tok", 2 if mixtral else 8)),
        moe_intermediate_size=d["intermediate_size"] if mixtral else d.get("moe_intermediate_size", d["intermediate_size"]),
        norm_topk_prob=True if mixtral else bool(d.get("norm_topk_prob", False)),
        decoder_sparse_step=int(d.get("decoder_sparse_step", 1) or 1), mlp_only_layers=list(d.get("mlp_only_layers") or []),
        kivi_moe_kernel=bool(moe_kernel), kivi_moe_kernel_max_tokens=moe_kernel_max_tokens, **extra)


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        return F.rms_norm(x, (x.shape[-1],), self.weight, self.eps)


class MLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.gate_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, bias=False)
        self.up_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, bias=False)
        self.down_proj = nn.Linear(cfg.intermediate_size, cfg.hidden_size, bias=False)

    def forward(self, x):
        return self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))


def layer_is_sparse(cfg, layer_idx: int) -> bool:
    """HF's rule (Qwen3MoeDecoderLayer): a layer carries the routed block when the config has experts, the layer is not in
    `mlp_only_layers` and (layer_idx + 1) is a multiple of `decoder_sparse_step`; Mixtral has neither field: every layer is sparse."""
    return (getattr(cfg, "num_experts", 0) > 0 and layer_idx not in getattr(cfg, "mlp_only_layers", ())
            and (layer_idx + 1) % getattr(cfg, "decoder_sparse_step", 1) == 0)


def make_mlp(cfg, layer_idx: int) -> nn.Module:
    """The feed-forward block of a layer: the dense SwiGLU MLP, or the sparse block of kivi_amd/moe.py."""
    if not layer_is_sparse(cfg, layer_idx):
        # MLP(cfg), with cfg.kivi_weight_bits == 4 the 4-bit QuantMLP (section 30), with cfg.kivi_fp8_weights the Fp8MLP (section 35)
        return wquant.make_dense_mlp(cfg, MLP, name=f"model.layers.{layer_idx}.mlp")
    return SparseMoeBlock(cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts, cfg.num_experts_per_tok,
                          norm_topk=cfg.norm_topk_prob, round_weights=getattr(cfg, "kivi_moe_round_weights", False),
                          kernel=getattr(cfg, "kivi_moe_kernel", True),
                          kernel_max_tokens=getattr(cfg, "kivi_moe_kernel_max_tokens", None),
                          expert_bits=getattr(cfg, "kivi_expert_bits", None), expert_group=getattr(cfg, "kivi_expert_group", 128),
                          expert_fp8=bool(getattr(cfg, "kivi_fp8_experts", False)))


class DecoderLayer_KIVI(nn.Module):
    def __init__(self, cfg, layer_idx: int, attention_cls=LlamaAttention_KIVI):
        super().__init__()
        self.self_attn = attention_cls(cfg, layer_idx)
        self.mlp = make_mlp(cfg, layer_idx)     # the attribute stays `mlp` for either kind: DecodeGraphs calls layer.mlp
        self.input_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)

    def forward(self, x, past, attention_mask=None, position_ids=None):
        a, _, past = self.self_attn(self.input_layernorm(x), attention_mask=attention_mask, position_ids=position_ids,
                                    past_key_value=past, use_cache=True)
        x = x + a
        return x + self.mlp(self.post_attention_layernorm(x)), past


class _Body(nn.Module):
    def __init__(self, cfg, attention_cls):
        super().__init__()
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList([DecoderLayer_KIVI(cfg, i, attention_cls) for i in range(cfg.num_hidden_layers)])
        self.norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)


class LlamaForCausalLM_KIVI(nn.Module):
    """`past_key_values` is a list with one entry per layer: None before the prompt pass, afterwards the 9-tuple of
    models/llama_kivi.py:454-455 (here the lazy KiviCacheTuple over the in-place cache).

    Prompts of different lengths are left-padded (`left_pad`) and described by HF's 2D mask (1 = real token): `padding_mask`
    of forward(), `attention_mask` of generate() / generate_graphed() / decode_graphed().  Pads are ordinary cache tokens
    that every query masks; a mask without a pad takes the unmasked path unchanged."""

    _QK_KERNEL = False          # from_pretrained's default of `qk_kernel` for the class

    def __init__(self, config, attention_cls=LlamaAttention_KIVI):
        super().__init__()
        self.config = config
        self.model = _Body(config, attention_cls)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.graphs = None          # kivi_amd.graph.DecodeGraphs of the last graphed decode (prepare_graphs / release_graphs)
        self._stoppers = {}         # (rows, device, pad) -> the StopRows that generate_graphed binds its keyword stops to
        self._quant_experts = None  # whether a sparse block holds 4-bit experts (_refuse_capture)
        self.lora = None            # kivi_amd.lora.LoraSet of enable_lora() (a plain attribute: not a module, no state_dict entry)
        self._lora_bindings = {}    # (rows, device) -> the RowBinding the graphed calls rebind (their captured steps hold its buffer)
        if getattr(config, "tie_word_embeddings", False):
            self.lm_head.weight = self.model.embed_tokens.weight

    @torch.no_grad()
    def forward(self, input_ids: torch.LongTensor, past_key_values: Optional[List] = None, attention_mask=None,
                last_token_only: bool = True, padding_mask: Optional[torch.Tensor] = None, adapters=None):
        """logits (B, 1 or T, vocab), new past_key_values.  `attention_mask`: the reference's additive (B, 1, 1, kv_len)
        fp16 mask for decode steps (llama_kivi.py:364-372); with it the prompt pass is causal over equal-length prompts.
        `padding_mask`: HF's 2D mask (B, past + T) of 0 / 1 (1 = real token) over the history and `input_ids` -- positions
        and the additive masks of every pass are derived from it (not together with `attention_mask`).
        `adapters`: the LoRA slot of every row (enable_lora) -- None: the base model, or the binding an outer
        call has set; one slot for all rows; one int or None per row (None and -1: the base model); ValueError for anything else."""
        if adapters is not None:
            with lora.call_binding(self, adapters, input_ids.shape[0]):
                return self.forward(input_ids, past_key_values, attention_mask, last_token_only, padding_mask)
        if padding_mask is None:
            return self._forward(input_ids, past_key_values, attention_mask, None, last_token_only, False)
        if attention_mask is not None:
            raise ValueError("pass either the 4D additive attention_mask or the 2D padding_mask, not both")
        past_len = self._past_len(past_key_values)
        padded = self._padded(padding_mask, input_ids.shape[0], past_len + input_ids.shape[1], past_len)
        if not padded:
            return self._forward(input_ids, past_key_values, None, None, last_token_only, False)
        pb = _PaddedBatch(padding_mask, past_len, input_ids.shape[1], lead=padded == PADS_LEFT)
        mask = pb.mask
        if past_len and input_ids.shape[1] == 1 and getattr(self.config, "kivi_decode_lead", False):
            mask = DecodeLead(mask, leading_pads(padding_mask))     # a decode step: the key row travels with its lead (section 21)
        return self._forward(input_ids, past_key_values, mask, pb.position_ids, last_token_only, True)

    def _forward(self, input_ids, past_key_values, attention_mask, position_ids, last_token_only, mask_prompt):
        x, new = self._hidden(input_ids, past_key_values, attention_mask, position_ids, mask_prompt)
        if last_token_only:
            x = x[:, -1:]
        return self.lm_head(self.model.norm(x)), new

    def _hidden(self, input_ids, past_key_values, attention_mask, position_ids, mask_prompt):
        """The decoder blocks of a pass -> (hidden states (B, T, H) before the final norm, new past_key_values)."""
        pasts = past_key_values or [None] * len(self.model.layers)
        x = self.model.embed_tokens(input_ids)
        new = []
        for layer, past in zip(self.model.layers, pasts):
            x, p = layer(x, past, attention_mask if past is not None or mask_prompt else None, position_ids)
            new.append(p)
        return x, new

    @staticmethod
    def _past_len(past_key_values) -> int:
        return int(past_key_values[0][-1]) if past_key_values and past_key_values[0] is not None else 0

    def _padded(self, mask: torch.Tensor, B: int, length: int, past_len: int, has_pad: Optional[bool] = None,
                left: Optional[bool] = None):
        """Validate a 2D padding mask; true when it holds a pad (False: the caller takes the unmasked path, no mask is built).
        `has_pad`, `left`: what the caller already knows about the mask (spares the synchronisation).
        With config.kivi_prefill_kernel a padded prompt pass (no history) whose mask is left-padded -- zeros, then ones, in every row,
        looked at in the same synchronisation -- answers PADS_LEFT: the pass runs on the leading pad counts (_PaddedBatch(lead=True)),
        on every attention class.  Any other mask takes the masked path of the eager classes and is refused by the flash classes."""
        if mask.dim() != 2 or tuple(mask.shape) != (B, length):
            raise ValueError(f"the 2D attention / padding mask should be of size {(B, length)} (history + new tokens), "
                             f"but is {tuple(mask.shape)}")
        kernel = past_len == 0 and bool(getattr(self.config, "kivi_prefill_kernel", False))
        if kernel and (has_pad is None or left is None):
            full, left = torch.stack([(mask != 0).all(), left_padded(mask)]).tolist()
            has_pad = not full
        elif has_pad is None:
            has_pad = not bool((mask != 0).all())
        if not has_pad:
            return False
        if kernel and left:
            return PADS_LEFT
        if past_len == 0 and not all(layer.self_attn._prefill_uses_mask for layer in self.model.layers):
            name = type(self.model.layers[0].self_attn).__name__
            if kernel:
                raise ValueError(f"{name}: the mask is not left-padded (zeros, then ones, in every row). The prefill kernel serves "
                                 f"leading pads only, and the prompt pass of this attention class ignores every other mask "
                                 f"(llama_kivi.py:420-423); use the eager class")
            raise ValueError(f"{name}: the prompt pass of this attention class ignores "
                             f"masks (llama_kivi.py:420-423), so padded prompts cannot be run; use the eager class")
        return True

    @staticmethod
    def _reorder_cache(past_key_values, beam_idx: torch.Tensor):
        """The reference's hook for HF's beam search (models/llama_kivi.py:951-957): row b of every layer's cache <- row
        beam_idx[b], here IN PLACE (kivi_cache_reorder, whole rows) instead of an index_select copy of every member.  Returns
        fresh 9-tuples of the same caches (plain 9-tuples, which have no in-place cache, are index_selected as the reference does)."""
        out = []
        for p in past_key_values:
            layer = getattr(p, "layer", None)
            if layer is None:
                out.append(tuple(x.index_select(0, beam_idx.to(x.device)) if torch.is_tensor(x) else x for x in p))
            else:
                out.append(layer.reorder_(beam_idx).as_tuple())
        return tuple(out)

    # ------------------------------------------------------------------ checkpoint / rollback
    @staticmethod
    def _layer_caches(past_key_values, what: str):
        caches = [getattr(p, "layer", None) for p in past_key_values or ()]
        if not caches or any(c is None for c in caches):
            raise ValueError(f"{what} needs the tuples of an in-place cache (what forward() / generate() return), not plain 9-tuples")
        return caches

    @classmethod
    def checkpoint(cls, past_key_values) -> "KiviModelCheckpoint":
        """The state of every layer's cache to come back to with restore_(): one launch per layer, a few MB where the caches hold
        hundreds (KiviCacheBase.checkpoint).  `past_key_values`: the tuples of forward() / generate(); a tuple whose length is stale
        still names its cache."""
        from .checkpoint import KiviModelCheckpoint
        caches = cls._layer_caches(past_key_values, "checkpoint")
        return KiviModelCheckpoint([c.checkpoint() for c in caches], caches[0].kv_seq_len)

    @classmethod
    def restore_(cls, past_key_values, ck) -> List:
        """Every layer's cache back to the checkpoint, exactly and in place (KiviCacheBase.restore_); returns fresh tuples to
        continue from with forward(), generate(past_key_values=...) or decode_graphed().  ValueError before any cache is touched when
        one of them refuses the checkpoint (another model shape, a stale checkpoint)."""
        caches = cls._layer_caches(past_key_values, "restore_")
        if len(caches) != len(ck.layers):
            raise ValueError(f"the checkpoint holds {len(ck.layers)} layers, past_key_values {len(caches)}")
        for c, k in zip(caches, ck.layers):
            c.check_restore(k)
        return [c.restore_(k).as_tuple() for c, k in zip(caches, ck.layers)]

    # ------------------------------------------------------------------ continuous batching
    @torch.no_grad()
    def admit_(self, past_key_values, rows, input_ids: torch.LongTensor, attention_mask: torch.Tensor, offset: int = 0,
               adapters=None):
        """New requests take over rows of living caches: -> (prompt logits (n, 1, vocab), fresh tuples of the living caches).
        `past_key_values`: the tuples of forward() / generate() over caches of B rows at kv length L.  `input_ids` (n, L) and HF's 2D
        `attention_mask` (n, L): the n new prompts left-padded to exactly L (left_pad(..., length=L); a prompt of L tokens has no
        pad).  `rows`: n distinct rows in [0, B).  The prompts run as an ordinary prompt pass of n rows,
        forward(input_ids, padding_mask=attention_mask) -- the flash classes refuse padded prompts there as ever -- and every layer's
        temporary cache is put into the rows in place (KiviCacheBase.admit_): the other rows, every buffer address and the lengths
        stay, so captured decode graphs over the living caches remain valid; the temporary caches die with the call.  ValueError
        before any forward pass for plain 9-tuples, input_ids of another length than L, a mask of another shape, n > B, bad rows.
        `offset` > 0: `input_ids` and `attention_mask` are (n, L - offset) -- the prompts left-padded to the SHORT
        length -- and the prompt pass costs O(L - offset), not O(L).  Positions come from the mask, so they are those of the L-padded
        pass; the result lands in tokens [offset, L) of the rows, tokens [0, offset) become zero blocks.  The caller's 2D mask for
        the rows is cat(zeros(offset), attention_mask): the lead is masked like any pad.  `offset`: an int, a multiple of
        rebase_quantum(past_key_values), with L - offset >= residual_length; anything else is a ValueError before the forward pass.
        The admitted rows are NOT bit-identical to an admission at offset 0 (serving.py has the reasons).
        `adapters`: the LoRA slots of the n admitted prompts, as forward() takes them: the prompt pass runs under a binding of the
        admitted rows alone (the caller then set_row()s the living batch's binding)."""
        bound = lora.call_binding(self, adapters, input_ids.shape[0] if input_ids.dim() == 2 else 1)
        caches = self._layer_caches(past_key_values, "admit_")
        L, B = caches[0].kv_seq_len, caches[0].B
        if offset != 0 or not isinstance(offset, int) or isinstance(offset, bool):
            for c in caches:
                admit.check_offset(offset, c.rebase_quantum, c.kv_seq_len, c.cfg.residual_length)
            if input_ids.dim() != 2 or input_ids.shape[1] != L - offset:
                raise ValueError(f"admit_: input_ids must be (n, L - offset) with L = {L} the kv length of the living caches and offset = "
                                 f"{offset} (left-pad the prompts to {L - offset}), got {tuple(input_ids.shape)}")
        elif input_ids.dim() != 2 or input_ids.shape[1] != L:
            raise ValueError(f"admit_: input_ids must be (n, L) with L = {L}, the kv length of the living caches (left-pad the prompts "
                             f"to it), got {tuple(input_ids.shape)}")
        n = input_ids.shape[0]
        if attention_mask is None or attention_mask.dim() != 2 or tuple(attention_mask.shape) != (n, L - offset):
            raise ValueError(f"admit_: the 2D attention mask should be of size {(n, L - offset)}, but is "
                             f"{None if attention_mask is None else tuple(attention_mask.shape)}")
        if not 1 <= n <= B:
            raise ValueError(f"admit_: {n} prompts for living caches of {B} rows")
        rows = admit.check_rows(rows, n, B, caches[0].k_res.device)
        with bound:
            logits, fresh = self.forward(input_ids, padding_mask=attention_mask)
        for c, t in zip(caches, fresh):
            c.admit_(rows, t.layer, check=False, offset=offset)
        return logits, [c.as_tuple() for c in caches]

    def generate_continuous(self, prompts, max_new_tokens, batch_size: int, eos_token_id: Optional[int] = None,
                            pad_token_id: Optional[int] = 0, sampling=None, graphed: bool = False, compact: Optional[int] = None,
                            short_admissions: bool = False, return_logprobs: bool = False, top_logprobs: int = 0, stopping=None,
                            return_finish: bool = False, allowed_fn=None, adapters=None):
        """Continuous batching over a queue of requests (kivi_amd/serving.py: generate_continuous): a batch of `batch_size` rows whose
        finished rows are taken over by the waiting prompts.  -> the generated tokens of every request, in request order.
        `compact`: None, or the fewest leading tokens worth dropping from the living caches between two steps (rebase_).
        `short_admissions`: admit at an offset, the prompt pass over about the prompt's length instead of the caches' (DESIGN.md
        section 19; tokens may differ from the default).
        `return_logprobs` / `top_logprobs=k`: -> (tokens, logprobs[, top_ids, top_logprobs]), each a list with one tensor per request
        (DESIGN.md section 23).
        `eos_token_id`: an int or a list; `stopping`: None, one StopParams, or one per request (stop ids, stop sequences, a limit of
        its own); `return_finish`: the result gains a list of (reason, index) per request.
        Per-request constraints (logit_bias, allowed_token_ids, min_new_tokens) come with `sampling`; `allowed_fn`: None, one callable
        or one per request, asked before every pick for the ids or the bitmask the request may emit next.
        `adapters`: None, one LoRA slot for every request, or one int or None per request: an admission runs
        its prompt pass under the admitted requests' slots, the batch's binding takes them by set_row -- the captured step is
        replayed --, and a finished row goes back to -1."""
        if graphed:
            self._refuse_capture("generate_continuous(graphed=True)")
        return serving.generate_continuous(self, prompts, max_new_tokens, batch_size, eos_token_id, pad_token_id, sampling, graphed,
                                           compact, short_admissions, return_logprobs, top_logprobs, stopping, return_finish, allowed_fn,
                                           adapters)

    # ------------------------------------------------------------------ rebase
    @classmethod
    def rebase_quantum(cls, past_key_values) -> int:
        """The drops rebase_ takes are multiples of this (every layer's KiviCacheBase.rebase_quantum: lcm(residual_length, 32))."""
        return math.lcm(*(c.rebase_quantum for c in cls._layer_caches(past_key_values, "rebase_quantum")))

    @classmethod
    def rebase_limit(cls, past_key_values) -> int:
        """The largest drop rebase_ takes now (the smallest KiviCacheBase.rebase_limit of the layers)."""
        return min(c.rebase_limit for c in cls._layer_caches(past_key_values, "rebase_limit"))

    @classmethod
    def rebase_(cls, past_key_values, drop: int) -> List:
        """The first `drop` tokens of every row leave every layer's living cache, in place (KiviCacheBase.rebase_): what a batch
        whose rows all start with at least `drop` pads does to stop paying for them.  Returns fresh tuples of the same caches; go
        on with a 2D mask without its first `drop` columns (positions come from the mask: they do not change).  ValueError before
        any cache is touched for plain 9-tuples or a drop some layer refuses (not an int, negative, not a multiple of
        rebase_quantum, above rebase_limit)."""
        caches = cls._layer_caches(past_key_values, "rebase_")
        for c in caches:
            c.check_rebase(drop)
        return [c.rebase_(drop).as_tuple() for c in caches]

    # ------------------------------------------------------------------ scoring given tokens
    _HEAD_SLAB = 4096            # rows of hidden states per lm_head call of score(): logits exist for one slab at a time
    _score_plan = staticmethod(scoring.score_plan)      # the name callers of the model know the plan by

    def score(self, input_ids: torch.LongTensor, attention_mask: Optional[torch.Tensor] = None,
              past_key_values: Optional[List] = None, first_chunk: Optional[int] = None, chunk_size: Optional[int] = None,
              return_rank: bool = False, top_logprobs: int = 0, adapters=None):
        """Teacher-forced log-probabilities of given tokens: (logprobs (B, T - 1) fp32, valid (B, T - 1) bool, past_key_values)
        [, ranks (B, T - 1) int32 with `return_rank`: 0 where the token is the argmax of its distribution, -1 where not valid]
        [, top_ids (B, T - 1, k) int64, top_logprobs (B, T - 1, k) fp32 with `top_logprobs=k` in [1, min(vocab_size, 32)]: the k most
        likely tokens of every distribution, most likely first, ties by ascending id, from the same launch as the logprobs
        (kivi_token_top_logprobs); id -1 and value 0 where not valid].
        Entry i is log p(input_ids[:, i + 1] | tokens <= i) under the model's raw distribution (kivi_amd/scoring.py,
        kivi_token_logprob); the caches are advanced over all T tokens, in place when `past_key_values` is given.

        `first_chunk` / `chunk_size` decide what the score measures.  The first `first_chunk` tokens (default: all T) go through the
        prompt pass -- with `past_key_values` through the multi-token extend over the caches of the earlier turn -- and the rest in
        pieces of `chunk_size` tokens (default: one piece), each a q_len > 1 extend over the QUANTISED cache, or the decode step when
        chunk_size == 1.  The prompt pass attends in fp16 and quantises afterwards, as the reference does, so a one-pass score does
        not see the quantiser at all; a chunked score does, and score(first_chunk=P, chunk_size=1) is exactly the arithmetic of
        generate() after a P-token prompt.  To measure what k_bits / v_bits / group_size / residual_length cost a model, chunk.

        `attention_mask`: HF's 2D left-padding mask (B, past + T) over the history and `input_ids`; entries whose target or context
        token is a pad have valid == False and logprob 0.  Every piece runs the padded path of forward() on the mask's first
        past + (tokens so far) columns (pads are on the left, so every such slice holds them).  Token ids are validated against
        vocab_size, and the mask is looked at, once: one synchronisation per call.  T < 2, a chunk size < 1 or first_chunk outside
        [1, T] raise ValueError before any device work.  `adapters`: the LoRA slot of every row, as forward() takes them."""
        with lora.call_binding(self, adapters, input_ids.shape[0]):
            return scoring.score(self, input_ids, attention_mask, past_key_values, first_chunk, chunk_size, return_rank, top_logprobs)

    def perplexity(self, input_ids: torch.LongTensor, attention_mask: Optional[torch.Tensor] = None,
                   past_key_values: Optional[List] = None, first_chunk: Optional[int] = None, chunk_size: Optional[int] = None,
                   adapters=None):
        """exp(-sum of the valid log-probabilities / number of valid entries) of score() with the same arguments:
        (per row (B,), over all rows ()) float64 on the device, the sums taken in fp64.  A row without a valid entry gives NaN."""
        with lora.call_binding(self, adapters, input_ids.shape[0]):
            return scoring.perplexity(self, input_ids, attention_mask, past_key_values, first_chunk, chunk_size)

    @torch.no_grad()
    def generate(self, input_ids: torch.LongTensor, max_new_tokens: int, past_key_values: Optional[List] = None,
                 attention_mask: Optional[torch.Tensor] = None, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, num_return_sequences: int = 1, return_scores: bool = False, do_sample: bool = False,
                 temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, min_p: Optional[float] = None,
                 seed: Optional[int] = None, return_logprobs: bool = False, sampling=None, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, top_logprobs: int = 0, stop_token_ids=None,
                 stop_sequences=None, stopping=None, logit_bias=None, allowed_token_ids=None, min_new_tokens: int = 0,
                 adapters=None):
        """Greedy decoding (the recipe of the reference's mem_spd_test.py / example.py), or sampling with `do_sample=True`.
        With `past_key_values` (the caches of an earlier turn) `input_ids` is the new turn: it is extended onto the caches in one
        pass (kivi_attention_extend) and decoding continues from there; the caches are advanced in place.  `attention_mask`:
        HF's 2D mask (B, past + T) of left-padded prompts (1 = real token; with `past_key_values` it covers the history and the
        new turn).  A row that has produced `eos_token_id` emits `pad_token_id` from then on; the loop stops when every row has
        finished.

        `num_beams > 1`: HF's beam search (kivi_amd/beam.py; `length_penalty`, `early_stopping` True / False / "never",
        `num_return_sequences` as in transformers).  The prompt pass runs on the B requests, the caches are then forked to
        B * num_beams rows, and every step reorders them in place from the fork point on.  With
        `past_key_values` the caller's caches are forked and left UNCHANGED (the new turn runs on a copy).  Returns
        (B * num_return_sequences, T + generated) sequences, and their sequences_scores when `return_scores`.

        `do_sample=True`: transformers' sampling path with HF's parameters and defaults (`temperature`, `top_k`, `top_p`, `min_p`),
        drawn by the fused HIP sampler (kivi_amd/sampling.py).  `seed`: the Philox seed of the call (None: one
        drawn from torch's default CPU generator); token i of the call is draw i of every row.  Not with beams.

        `sampling=`: per-request sampling (kivi_amd/sampling.py) -- one SamplingParams for every request, a
        list of B of them (greedy requests, do_sample=False, among sampled ones), or a ready RowSampler, which is used as it is
        (its draw indices are not reset) and has to hold B * num_return_sequences rows.  Not together with `do_sample=True`, a
        non-default `temperature` / `top_k` / `top_p` / `min_p` / `seed`, or beams.  With it `num_return_sequences=n` draws n samples
        of every prompt after ONE prompt pass: the caches are forked to B * n rows (with `past_key_values`: a clone of them, the
        caller's stay unchanged), output row b * n + j uses request b's parameters and seed with Philox stream j, and the n first
        tokens of a request are drawn from the same row of prompt logits.  Returns (B * n, T + generated).

        `return_logprobs=True` (greedy and sampling): returns (sequences, logprobs (B, generated) fp32), the log-probability of each
        emitted token under the model's RAW distribution -- temperature 1 and unfiltered, what HF derives from `output_logits`, not
        from the processed `output_scores` -- one kivi_token_logprob call per step on the logits the step has anyway; the pads of a
        row that has finished get 0.  On live positions they are score(sequences, first_chunk=T, chunk_size=1)[0][:, T - 1:]: bit for
        bit from the second new token on (the same head call on the same states); the first new token is scored on the prompt
        pass, whose head runs here on the last position alone and in score() on all T positions -- the same arithmetic, in
        whatever kernel the GEMM library picks for each row count.
        With beams use `return_scores`.  `top_logprobs=k` (with `return_logprobs`; k in [1, min(vocab_size, 32)]): the result gains
        top_ids (B, generated, k) int64 and top_logprobs (B, generated, k) fp32, the k most likely tokens of every step's raw
        distribution, most likely first -- one kivi_token_top_logprobs launch per step in place of the kivi_token_logprob launch
        (DESIGN.md section 23); the pads of a finished row get id -1 and value 0.

        `repetition_penalty` (HF, vLLM: over prompt and output tokens), `presence_penalty`, `frequency_penalty` (OpenAI, vLLM: over
        output tokens): applied inside the fused sampler (kivi_sample_rows_pen), greedy rows included.
        Non-neutral values make the call's sampler a RowSampler of identical rows (Philox streams 0..B-1, the call's `seed`), which
        draws what `do_sample=True` would have drawn from the penalised logits; with `sampling=` the penalties are those of the
        SamplingParams and the three arguments stay neutral.  The call marks its `input_ids` as the prompts (pads of the 2D mask
        are not marked; `num_return_sequences` forks carry the marks).  Not with beams.  `return_logprobs` stays under the RAW
        distribution.  Two facts: the loop's trailing pick (decode_loop) counts one token more than the call returns; and with
        `past_key_values` only this call's `input_ids` are known as prompt -- the earlier turns count only when the caller passes
        the same RowSampler again (`sampling=`), whose table keeps them.

        Finish conditions beyond one eos id (kivi_amd/stopping.py): `eos_token_id` may be a list, whose ids
        join `stop_token_ids` (at most 16 in all); `stop_sequences`: at most 8 sequences of 1 to 16 token ids, matched against the
        tokens the row has produced in this call, never into the prompt; or `stopping=`: a StopParams, a list of B of them (per-request
        conditions and limits), or a ready StopRows of B * num_return_sequences rows, used as it is (its state is not reset) -- not
        together with the other three.  With any of them the rows are tracked on the device (one kivi_stop_rows launch per token; the
        step's one synchronisation is the read of its live count): a finished row emits `pad_token_id`, which is required, and the
        stop itself stays in the output, as `eos_token_id` does; a call whose rows have all finished -- by their `max_new_tokens` too
        -- ends without the pass after the last token.  Beam search keeps its own handling of ONE `eos_token_id` and refuses the
        rest.  The plain call with one int `eos_token_id` is what it was.

        `logit_bias` (a dict from token id to an additive bias, +-inf allowed; -inf bans the token), `allowed_token_ids` (the only
        ids the call may emit) and `min_new_tokens` (every row's eos ids and stop token ids are masked for its first so many
        tokens): applied inside the fused sampler (kivi_sample_rows_con), before the penalties and the
        temperature, greedy rows included.  They route like the penalties: non-neutral values make the call's sampler a RowSampler
        of identical rows; with `sampling=` they come from the SamplingParams (a list may constrain every request differently) and
        the three arguments stay neutral.  Not with beams.  `min_new_tokens` does not hold back stop SEQUENCES, which may still end
        a row early, and a caller's RowSampler is used as it is (bind its suppressed ids with `suppress=`).  `return_logprobs` /
        `top_logprobs` stay under the RAW distribution: a token the constraints forbid can appear among the top ids.

        `adapters`: the LoRA slot of every request (enable_lora): None, one slot for all, or one int or None
        per request (None and -1: the base model).  `num_beams` / `num_return_sequences` expand a request's slot over its rows, as
        they expand its sampling parameters."""
        fan = max(num_beams, num_return_sequences, 1) if isinstance(num_beams, int) and isinstance(num_return_sequences, int) else 1
        with lora.call_binding(self, adapters, input_ids.shape[0], fan):
            return self._generate(input_ids, max_new_tokens, past_key_values, attention_mask, eos_token_id, pad_token_id, num_beams,
                                  length_penalty, early_stopping, num_return_sequences, return_scores, do_sample, temperature, top_k,
                                  top_p, min_p, seed, return_logprobs, sampling, repetition_penalty, presence_penalty,
                                  frequency_penalty, top_logprobs, stop_token_ids, stop_sequences, stopping, logit_bias,
                                  allowed_token_ids, min_new_tokens)

    def _generate(self, input_ids, max_new_tokens, past_key_values, attention_mask, eos_token_id, pad_token_id, num_beams, length_penalty,
                  early_stopping, num_return_sequences, return_scores, do_sample, temperature, top_k, top_p, min_p, seed,
                  return_logprobs, sampling, repetition_penalty, presence_penalty, frequency_penalty, top_logprobs, stop_token_ids,
                  stop_sequences, stopping, logit_bias, allowed_token_ids, min_new_tokens):
        """generate() under the call's LoRA binding, argument for argument."""
        if return_logprobs and num_beams > 1:
            raise ValueError("return_logprobs is for greedy decoding and sampling; beam search (num_beams > 1) returns its "
                             "sequences_scores with return_scores=True")
        scoring.check_top_logprobs(top_logprobs, return_logprobs, num_beams, self.config.vocab_size)
        pick, fan = resolve_sampler(input_ids.device, input_ids.shape[0], num_return_sequences, num_beams, do_sample, temperature,
                                    top_k, top_p, min_p, seed, sampling, repetition_penalty, presence_penalty, frequency_penalty,
                                    self.config.vocab_size, logit_bias, allowed_token_ids, min_new_tokens)
        if eos_token_id is not None and pad_token_id is None:
            raise ValueError("eos_token_id needs a pad_token_id for the rows that have finished")
        if sampling is None and (num_beams < 1 or num_return_sequences < 1 or num_return_sequences > num_beams):
            raise ValueError(f"num_return_sequences ({num_return_sequences}) must lie in [1, num_beams ({num_beams})]")
        if return_scores and num_beams == 1:
            raise ValueError("return_scores: sequences_scores exist for beam search (num_beams > 1) only")
        stops = resolve_stopping(input_ids.shape[0], max_new_tokens, eos_token_id, pad_token_id, stop_token_ids, stop_sequences,
                                 stopping, num_beams, self.config.vocab_size, fan)
        bind_suppress(pick, sampling, stops, eos_token_id)
        stepper = EagerStepper(self, input_ids, past_key_values, attention_mask, max_new_tokens, max(num_beams, fan))
        observe_prompts(pick, input_ids, attention_mask, fan)
        if num_beams > 1:                       # (with beams resolve_stopping has answered None: one eos id, handled there)
            seqs, scores = beam_search(stepper.step, input_ids, stepper.logits, num_beams, max_new_tokens, eos_token_id,
                                       pad_token_id, length_penalty, early_stopping, num_return_sequences)
            return (seqs, scores) if return_scores else seqs
        if stops is None:                       # the loop's torch path: no finish condition, or one int eos id
            finish = dict(eos_token_id=eos_token_id, pad_token_id=pad_token_id)
        else:                                   # a tracker on the device: the caller's, or one for this call
            finish = dict(stopper=stops if isinstance(stops, StopRows) else StopRows(stops, input_ids.device, pad_token_id=pad_token_id))
        new, logprobs = decode_loop(stepper.logits, stepper.step, pick or (lambda lg: lg.argmax(-1)), max_new_tokens,
                                    want_logprobs=return_logprobs, top_k=top_logprobs, **finish)
        return pack_result(stepper.input_ids, new, logprobs)

    # ------------------------------------------------------------------ hipGraph decode (kivi_amd/graph.py: DecodeGraphs)
    def _refuse_capture(self, what: str) -> None:
        """Raise, before anything runs, where the model holds a sparse block with 4-bit experts: that block's dequantising loop
        synchronises, so no decode step of the model can be captured."""
        if self._quant_experts is None:                         # (asked on every graphed step: walk the module tree once)
            self._quant_experts = any(isinstance(m, QuantExperts) for m in self.modules())
        if self._quant_experts:
            raise ValueError(f"{what}: a model built with expert_bits=4 has no capturable decode step (its sparse blocks run the "
                             f"dequantising loop, which synchronises); use the eager form")

    def prepare_graphs(self, batch: int, device, whole: bool = False, padded: bool = False, sampler=None,
                       logprobs: Optional[int] = None, stopper=None) -> None:
        """Capture the decode graphs for this batch size now (otherwise on the first graphed step).  `logprobs`, `stopper`: as
        decode_graphed."""
        graph.prepare_graphs(self, batch, device, whole, padded, sampler, logprobs, stopper)

    def release_graphs(self) -> None:
        """Drop the static buffers and everything captured; the next graphed decode builds them again."""
        self.graphs = None
        self._stoppers.clear()

    def decode_graphed(self, tok: torch.LongTensor, past_key_values: List, position: int, steps: int,
                       attention_mask: Optional[torch.Tensor] = None, sampler=None, sampling=None,
                       logprobs: Optional[int] = None, stopper=None, sync_every: int = SYNC_EVERY, adapters=None):
        """`steps` decode steps from token `tok` (B, 1) at position `position` with the dense part replayed from
        hipGraphs; the caches in `past_key_values` are advanced in place.  Returns the (B, steps) tokens fed to the model
        (tok first); the token following them is left in the graph's token buffer (`self.graphs.tok`).
        `attention_mask`: HF's 2D mask (B, kv_len + 1) over the cached tokens and `tok` (1 = real token); with a pad in it
        every row takes its own position from the mask (`position` is not used) and the pads are masked in every step.
        `sampler`: a kivi_amd.sampling.Sampler that draws each next token (one draw per step, inside the graph); None: greedy.
        `sampling`: a kivi_amd.sampling.RowSampler of B rows in its place (per-row parameters; not together with `sampler`).  The
        graphs depend on its buffers only: set_row() between steps or calls replays what was captured.
        `logprobs`: None, or k in [0, min(vocab_size, 32)] -- every captured step also scores the token it produces under its raw
        logits and the call returns (tokens, logprobs (B, steps) fp32[, top_ids (B, steps, k) int64,
        top_logprobs (B, steps, k) fp32 for k > 0]): entry s is the score of the token step s PRODUCED (tokens[:, s + 1]; the last
        one is the token left in `self.graphs.tok`).  The host clones the static buffers after every step, as it clones `tok`.
        `stopper`: a kivi_amd.stopping.StopRows of B rows, which has already seen `tok`; every captured step
        runs it on the token it produces (one kivi_stop_rows launch after the draw): finished rows feed its pad.  Before step s, for
        every s that is a multiple of `sync_every`, the host reads the stopper's `n_live` -- the only synchronisation -- and leaves
        when it is 0, so fewer than `steps` columns may come back and at most sync_every - 1 steps run after the last row has
        finished.  `sync_every=None`: never read, all `steps` run.
        `adapters`: the LoRA slots of the B rows -- a list as forward() takes it, which binds the model's own
        binding for B rows in place, or a kivi_amd.lora.RowBinding of B rows, used as it is.  The captured step holds the two launches
        per target linear and reads the binding's buffer: its key() joins what the graphs are matched by, and another request mix
        (bind, set_row) replays the graphs that exist."""
        with lora.call_binding(self, adapters, tok.shape[0], kept=True):
            return graph.decode_graphed(self, tok, past_key_values, position, steps, attention_mask, sampler, sampling, logprobs,
                                        stopper, sync_every)

    def generate_graphed(self, input_ids: torch.LongTensor, max_new_tokens: int,
                         attention_mask: Optional[torch.Tensor] = None, num_beams: int = 1, do_sample: bool = False,
                         temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, min_p: Optional[float] = None,
                         seed: Optional[int] = None, sampling=None, repetition_penalty: float = 1.0,
                         presence_penalty: float = 0.0, frequency_penalty: float = 0.0, return_logprobs: bool = False,
                         top_logprobs: int = 0, eos_token_id=None, pad_token_id: Optional[int] = None, stop_token_ids=None,
                         stop_sequences=None, stopping=None, sync_every: Optional[int] = SYNC_EVERY, logit_bias=None,
                         allowed_token_ids=None, min_new_tokens: int = 0, adapters=None):
        """generate() with the dense part of every decode step replayed from hipGraphs (kivi_amd.graph.DecodeGraphs).
        `attention_mask`: HF's 2D (B, T) mask of left-padded prompts (1 = real token).  Greedy, or sampling with `do_sample=True`
        and the parameters of generate() (the draw inside the graph; the same tokens as generate() with the same seed).  Beams
        are refused (a graphed beam step is open; use generate()).  `sampling=`: per-request parameters as in
        generate() (a SamplingParams, a list of B, or a RowSampler of B rows); the graphs are keyed by the RowSampler's buffers.
        `repetition_penalty` / `presence_penalty` / `frequency_penalty`: as in generate(); the penalised draw and the count of its
        token are inside the captured step.
        `return_logprobs` / `top_logprobs=k`: the tuple generate() returns with the same arguments: the first
        new token is scored eagerly on the prompt logits, every later one inside the captured step that produces it.
        `eos_token_id` (an int or a list) / `stop_token_ids` / `stop_sequences` / `stopping=` with `pad_token_id`: the finish
        conditions of generate(), tracked by one kivi_stop_rows launch inside the captured step; the first
        token goes through the tracker by one eager call.  The result is exactly what generate() returns for the same arguments,
        the width included: the host reads the live count before every `sync_every`-th step (None: never) and leaves when it is 0;
        the at most sync_every - 1 steps that ran past that point are cut off -- the caches of a graphed call die with it, nothing
        else observes them -- and the scores of a finished row's pads are masked from the tracker's lengths (0, id -1).  With the
        keyword forms the model keeps one tracker per (B, device, pad) and rebinds its rows, so another call with other stops
        replays the graphs that exist; a StopRows passed as `stopping=` is used as it is and keys the graphs by its own buffers.
        `logit_bias` / `allowed_token_ids` / `min_new_tokens`: as in generate(); the constrained draw is
        inside the captured step, and so is the advance towards the end of the suppression.
        `adapters`: as in generate(); the prompt pass and the captured steps run under the model's own binding
        for B rows, rebound in place, so another request mix replays the graphs that exist."""
        with lora.call_binding(self, adapters, input_ids.shape[0], kept=True):
            return graph.generate_graphed(self, input_ids, max_new_tokens, attention_mask, num_beams, do_sample, temperature, top_k,
                                          top_p, min_p, seed, sampling, repetition_penalty, presence_penalty, frequency_penalty,
                                          return_logprobs, top_logprobs, eos_token_id, pad_token_id, stop_token_ids, stop_sequences,
                                          stopping, sync_every, logit_bias, allowed_token_ids, min_new_tokens)

    # ------------------------------------------------------------------ per-request LoRA adapters
    def enable_lora(self, max_adapters: int, max_rank: int, target_modules=("q_proj", "v_proj")) -> "lora.LoraSet":
        """Attach adapter tables of `max_adapters` slots and table rank `max_rank` (8, 16, 32 or 64) to the linears named
        `target_modules`, a subset of q_proj, k_proj, v_proj, o_proj, gate_proj, up_proj, down_proj -> the kivi_amd.lora.LoraSet
        (load / unload adapters there; `adapters=` of the entry points binds rows to its slots).  On Mixtral and Qwen3-MoE the
        attention projections and the dense MLP layers are served; a sparse block is never a target.  Forward hooks on the target
        linears do the work: the module tree, the parameter and buffer names, state_dict() and what save_quantized writes stay.
        Captured graphs are released."""
        if self.lora is not None:
            self.disable_lora()
        self.lora = lora.LoraSet(self, max_adapters, max_rank, target_modules).attach()
        self.release_graphs()
        return self.lora

    def disable_lora(self) -> None:
        """Undo enable_lora: the hooks and the tables go, captured graphs are released."""
        if self.lora is not None:
            self.lora.detach()
        self.lora = None
        self._lora_bindings.clear()
        self.release_graphs()

    @classmethod
    def from_pretrained(cls, path: str, device="cuda", dtype=torch.float16, **kivi):
        """`path`: a local HF checkpoint directory (config.json + *.safetensors).  `kivi`: k_bits, v_bits, group_size,
        residual_length, max_cache_len, prefill_kernel, decode_lead, qk_kernel (default: the class's, on for the Qwen classes),
        moe_kernel, moe_kernel_max_tokens, weight_bits, weight_group, weight_kernel_max_tokens, expert_bits, expert_group,
        fp8_weights, fp8_skip_modules (an FP8 checkpoint's `modules_to_not_convert` is added to a list given here), fp8_experts.
        Called on LlamaForCausalLM_KIVI, a config.json whose `model_type` is qwen2 / qwen3 / mixtral / qwen3_moe builds that
        family's class.  The class, the config and the empty model are made here; reading config.json and filling the model are
        kivi_amd/loading.py: the files are read one at a time, and a checkpoint that leaves any tensor of
        the model unfilled raises KeyError.  With `expert_bits=4` every expert matrix is quantised into its slab of the sparse
        block's QuantExperts as its file is read: no dense expert stack ever exists.  With `weight_bits=4` the attention
        projections and dense MLPs are built 4-bit up front and every `*_proj.weight` is quantised on the device as its file is
        read; a directory written by save_quantized is recognised by its layout tag.  The experts of a sparse checkpoint are
        taken under HF's per-expert names or the fused ones of transformers 5: each expert is copied into the stacked parameter in
        turn.
        A fine-grained FP8 checkpoint (config.json: `quantization_config.quant_method == "fp8"`, e4m3, weight_block_size [128, 128]
        or null, float scales) is served as it lies on disk: its `weight` bytes and `weight_scale_inv` go into
        Fp8Linear modules unchanged, `modules_to_not_convert` stay dense, and an FP8 weight whose module the kernels do not serve is
        dequantised in torch.  `activation_scheme: "dynamic"` is accepted and NOT applied: activations stay 16-bit, the more exact
        arithmetic.  "static", `input_scale` / `activation_scale` tensors, ue8m0 scales, another block size and -- without
        `fp8_experts=True` -- FP8 experts raise.
        With `fp8_weights=True` a 16-bit checkpoint is quantised to that format on the device as its files are read.
        With `fp8_experts=True` the FP8 expert tensors of such a checkpoint -- per expert or fused, from any
        file in any order -- go into the sparse blocks' Fp8Experts unchanged, and 16-bit expert weights are quantised into them."""
        d = loading.read_config(path, kivi)     # (a directory of save_quantized: its tags become keywords of make_config)
        if cls is LlamaForCausalLM_KIVI:
            cls = {"qwen2": Qwen2ForCausalLM_KIVI, "qwen3": Qwen3ForCausalLM_KIVI, "mixtral": MixtralForCausalLM_KIVI,
                   "qwen3_moe": Qwen3MoeForCausalLM_KIVI}.get(d.get("model_type"), cls)
        kivi.setdefault("qk_kernel", cls._QK_KERNEL)
        cfg = make_config(d, **kivi)
        if getattr(cfg, "kivi_expert_bits", None) is not None and dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"from_pretrained(expert_bits=4) serves dtype torch.float16 or torch.bfloat16, got {dtype}")
        with torch.device(device):
            prev = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                model = cls(cfg)
            finally:
                torch.set_default_dtype(prev)
        return loading.load_weights(model, path, device, dtype)

    def save_quantized(self, path: str) -> None:
        """Write a model built with `weight_bits=4` or `expert_bits=4` to the directory `path`: config.json -- the fields it was
        loaded with plus kivi_weight_bits / kivi_weight_group, kivi_expert_bits / kivi_expert_group (those that are set) and the
        layout tag kivi_weight_layout -- and model.safetensors with the 4-bit modules' `qweight` / `scales` / `mins` under their
        module names.  A model built with `fp8_weights` is written in transformers' format instead: `weight` as float8_e4m3fn and
        `weight_scale_inv` as float32 under the module names, and a `quantization_config` block (fp8, e4m3, dynamic, [128, 128],
        float scales, `modules_to_not_convert`: the linears that stayed dense) in place of the tags; so is one built with
        `fp8_experts`, its experts under the per-expert names (read back with `fp8_experts=True`).  from_pretrained reads either
        back without quantising anything."""
        loading.save_quantized(self, path)


class MistralForCausalLM_KIVI(LlamaForCausalLM_KIVI):
    """Counterpart of models/mistral_kivi.py:921 (MistralForCausalLM_KIVI): the same decoder around MistralAttention_KIVI
    (bias-free projections, grouped queries mapped inside the kernels, `sliding_window` carried but -- like the reference,
    mistral_kivi.py:356-367 -- never applied to the quantised history)."""

    def __init__(self, config, attention_cls=None):
        from .attention import MistralAttention_KIVI
        super().__init__(config, attention_cls or MistralAttention_KIVI)


class MixtralForCausalLM_KIVI(MistralForCausalLM_KIVI):
    """HF's MixtralForCausalLM: Mistral's attention block (32 / 8 heads) and, in every layer, the sparse block of kivi_amd/moe.py in
    place of the MLP: `num_local_experts` experts of `intermediate_size`, `num_experts_per_tok` per token,
    the weights of a token always normalised over its experts and kept in fp32."""

    def __init__(self, config, attention_cls=None):
        super().__init__(SimpleNamespace(**{**vars(config), "kivi_moe_round_weights": False, "norm_topk_prob": True}), attention_cls)


class Qwen2ForCausalLM_KIVI(LlamaForCausalLM_KIVI):
    """HF's Qwen2ForCausalLM (Qwen2 / Qwen2.5) around QwenAttention_KIVI: a bias on q_proj / k_proj / v_proj and none on o_proj,
    `config.head_dim` when given, tied embeddings as the Llama class has them.  Their query-group ratios (7, 5, 6) are not the
    matrix-pipe layout's: with `qk_kernel` -- the default of these classes in from_pretrained, and of a config without the field --
    the groups run padded to 8.  `use_sliding_window=True` raises."""

    _QK_KERNEL = True
    _HEAD_NORM = False

    def __init__(self, config, attention_cls=None):
        from .attention import QwenAttention_KIVI
        fields = {**vars(config), "kivi_head_norm": self._HEAD_NORM, "kivi_qk_kernel": getattr(config, "kivi_qk_kernel", True)}
        if not self._HEAD_NORM:
            fields["attention_bias"] = True         # HF's Qwen2 has no such field: q / k / v always carry a bias
        super().__init__(SimpleNamespace(**fields), attention_cls or QwenAttention_KIVI)


class Qwen3ForCausalLM_KIVI(Qwen2ForCausalLM_KIVI):
    """HF's Qwen3ForCausalLM: as Qwen2 with `attention_bias` read from the config (default: none) and `q_norm` / `k_norm`, an RMSNorm
    over head_dim on every head of q and k before RoPE (checkpoint names self_attn.q_norm.weight / self_attn.k_norm.weight)."""

    _HEAD_NORM = True


class Qwen3MoeForCausalLM_KIVI(Qwen3ForCausalLM_KIVI):
    """HF's Qwen3MoeForCausalLM: Qwen3's attention block (head norms, head_dim 128) and the sparse block of kivi_amd/moe.py in the
    layers HF's rule names (layer_is_sparse), the dense MLP of `intermediate_size` in the others.  The
    router's weights are rounded to the model dtype, as HF's Qwen3MoeTopKRouter casts them."""

    def __init__(self, config, attention_cls=None):
        super().__init__(SimpleNamespace(**{**vars(config), "kivi_moe_round_weights": True}), attention_cls)
