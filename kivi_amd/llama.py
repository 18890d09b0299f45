"""A Llama / Mistral-shaped decoder around the KIVI attention hook -- the callers' side of the hot path.

Counterpart of the reference's LlamaForCausalLM_KIVI / MistralForCausalLM_KIVI wrappers (models/llama_kivi.py:564-1000,
models/mistral_kivi.py:673-1100) reduced to what decoding needs: token embedding, pre-norm decoder blocks
(RMSNorm, LlamaAttention_KIVI, SwiGLU MLP), final norm, lm_head, generate (greedy, sampling, beam search).  Parameter names
follow the Hugging Face checkpoints (model.embed_tokens, model.layers.N.self_attn.q_proj, ..., lm_head), so `load_state_dict` /
`from_pretrained` take an unmodified Llama-2 / Llama-3 / Mistral checkpoint directory; everything outside the attention
block is plain torch (rocBLAS / hipBLASLt GEMMs).  The reference patches k_bits / v_bits / group_size /
residual_length onto the HF config (README.md:72-75); the same four fields are read here.
"""
from __future__ import annotations

import glob
import json
import os
from types import SimpleNamespace
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .attention import LlamaAttention_KIVI, rope_cos_sin


def make_config(d: dict, k_bits: int = 2, v_bits: int = 2, group_size: int = 32, residual_length: int = 32,
                max_cache_len: Optional[int] = None) -> SimpleNamespace:
    """HF config.json fields (+ the four KIVI fields) -> the namespace the modules read."""
    hidden, heads = d["hidden_size"], d["num_attention_heads"]
    return SimpleNamespace(
        hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=d.get("num_key_value_heads", heads),
        num_hidden_layers=d["num_hidden_layers"], intermediate_size=d["intermediate_size"], vocab_size=d["vocab_size"],
        max_position_embeddings=d.get("max_position_embeddings", 4096), rope_theta=d.get("rope_theta", 10000.0),
        rms_norm_eps=d.get("rms_norm_eps", 1e-5), attention_bias=d.get("attention_bias", False),
        rope_scaling=d.get("rope_scaling"), head_dim=d.get("head_dim"), sliding_window=d.get("sliding_window"),
        tie_word_embeddings=d.get("tie_word_embeddings", False),
        k_bits=d.get("k_bits", k_bits), v_bits=d.get("v_bits", v_bits), group_size=d.get("group_size", group_size),
        residual_length=d.get("residual_length", residual_length),
        kivi_max_cache_len=max_cache_len)   # opt-in reservation; by default the cache starts prompt-sized and doubles


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


class DecoderLayer_KIVI(nn.Module):
    def __init__(self, cfg, layer_idx: int, attention_cls=LlamaAttention_KIVI):
        super().__init__()
        self.self_attn = attention_cls(cfg, layer_idx)
        self.mlp = MLP(cfg)
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


_MIN16 = torch.finfo(torch.float16).min


def left_pad(seqs, pad_token_id: int = 0, device=None):
    """A list of token id sequences -> (ids (B, T), mask (B, T)) left-padded to the longest one (HF's tokenizer with
    padding_side="left"): mask is 1 on real tokens, 0 on the `pad_token_id` fillers."""
    seqs = [torch.as_tensor(s, dtype=torch.long).flatten() for s in seqs]
    T = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), T), pad_token_id, dtype=torch.long)
    mask = torch.zeros((len(seqs), T), dtype=torch.long)
    for i, s in enumerate(seqs):
        if len(s):
            ids[i, T - len(s):] = s
            mask[i, T - len(s):] = 1
    return ids.to(device), mask.to(device)


def padding_position_ids(mask: torch.Tensor, q_len: int) -> torch.LongTensor:
    """HF's prepare_inputs_for_generation: positions cumsum(mask) - 1, pads at 1; the last `q_len` columns."""
    m = mask.long()
    pos = m.cumsum(-1) - 1
    return pos.masked_fill_(m == 0, 1)[:, -q_len:]


def padding_key_row(mask: torch.Tensor, length: Optional[int] = None) -> torch.Tensor:
    """(B, 1, 1, length) additive fp16 key row of a 2D padding mask: 0 on real tokens, finfo(fp16).min on pads (columns past
    the mask: 0).  Decode steps read views of it; an extend reads it expanded over the chunk."""
    B, L = mask.shape
    row = torch.zeros((B, 1, 1, length or L), dtype=torch.float16, device=mask.device)
    row[..., :L].masked_fill_((mask == 0)[:, None, None, :], _MIN16)
    return row


def padding_prompt_mask(mask: torch.Tensor) -> torch.Tensor:
    """HF's 4D causal + padding additive mask of a prompt pass (_prepare_4d_causal_attention_mask): (B, 1, T, T) fp16."""
    B, T = mask.shape
    causal = torch.full((T, T), _MIN16, dtype=torch.float16, device=mask.device).triu(1)
    return causal[None, None].repeat(B, 1, 1, 1).masked_fill_((mask == 0)[:, None, None, :], _MIN16)


class _PaddedBatch:
    """What a left-padded batch adds to the passes of one call, derived once from HF's 2D mask (B, past_len + T): `mask` and
    `position_ids` of the pass over the T new tokens (the prompt's 4D causal + padding mask; with a history, the key row expanded
    over the chunk), then per decode step a view of the key row one column longer (new tokens are real) and the advancing
    position.  `beams`: the decode steps run on every row repeated that often (the prompt pass does not)."""

    def __init__(self, mask2d: torch.Tensor, past_len: int, T: int, max_new_tokens: int = 0, beams: int = 1):
        n = past_len + T
        row = padding_key_row(mask2d, n + max_new_tokens)
        self.mask = padding_prompt_mask(mask2d) if past_len == 0 else row[..., :n].expand(-1, -1, T, -1)
        self.position_ids = padding_position_ids(mask2d, T)
        if max_new_tokens:
            pos = mask2d.long().sum(-1, keepdim=True)                  # (B, 1): position of the next token
            if beams > 1:
                row, pos = row.repeat_interleave(beams, dim=0), pos.repeat_interleave(beams, dim=0)
            self._row, self._pos, self._len = row, pos, n

    def step(self):
        """(additive key row (B, 1, 1, kv length incl. the new token), position ids (B, 1)) of the next decode step."""
        self._len += 1
        pos = self._pos
        self._pos = pos + 1
        return self._row[..., : self._len], pos


class LlamaForCausalLM_KIVI(nn.Module):
    """`past_key_values` is a list with one entry per layer: None before the prompt pass, afterwards the 9-tuple of
    models/llama_kivi.py:454-455 (here the lazy KiviCacheTuple over the in-place cache).

    Prompts of different lengths are left-padded (`left_pad`) and described by HF's 2D mask (1 = real token): `padding_mask`
    of forward(), `attention_mask` of generate() / generate_graphed() / decode_graphed().  Pads are ordinary cache tokens
    that every query masks; a mask without a pad takes the unmasked path unchanged."""

    def __init__(self, config, attention_cls=LlamaAttention_KIVI):
        super().__init__()
        self.config = config
        self.model = _Body(config, attention_cls)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        if getattr(config, "tie_word_embeddings", False):
            self.lm_head.weight = self.model.embed_tokens.weight

    @torch.no_grad()
    def forward(self, input_ids: torch.LongTensor, past_key_values: Optional[List] = None, attention_mask=None,
                last_token_only: bool = True, padding_mask: Optional[torch.Tensor] = None):
        """logits (B, 1 or T, vocab), new past_key_values.  `attention_mask`: the reference's additive (B, 1, 1, kv_len)
        fp16 mask for decode steps (llama_kivi.py:364-372); with it the prompt pass is causal over equal-length prompts.
        `padding_mask`: HF's 2D mask (B, past + T) of 0 / 1 (1 = real token) over the history and `input_ids` -- positions
        and the additive masks of every pass are derived from it (not together with `attention_mask`)."""
        if padding_mask is None:
            return self._forward(input_ids, past_key_values, attention_mask, None, last_token_only, False)
        if attention_mask is not None:
            raise ValueError("pass either the 4D additive attention_mask or the 2D padding_mask, not both")
        past_len = self._past_len(past_key_values)
        if not self._padded(padding_mask, input_ids.shape[0], past_len + input_ids.shape[1], past_len):
            return self._forward(input_ids, past_key_values, None, None, last_token_only, False)
        pb = _PaddedBatch(padding_mask, past_len, input_ids.shape[1])
        return self._forward(input_ids, past_key_values, pb.mask, pb.position_ids, last_token_only, True)

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

    def _padded(self, mask: torch.Tensor, B: int, length: int, past_len: int, has_pad: Optional[bool] = None) -> bool:
        """Validate a 2D padding mask; True when it holds a pad (False: the caller takes the unmasked path, no mask is built).
        `has_pad`: what the caller already knows about the mask (spares the synchronisation)."""
        if mask.dim() != 2 or tuple(mask.shape) != (B, length):
            raise ValueError(f"the 2D attention / padding mask should be of size {(B, length)} (history + new tokens), "
                             f"but is {tuple(mask.shape)}")
        if has_pad is None:
            has_pad = not bool((mask != 0).all())
        if not has_pad:
            return False
        if past_len == 0 and not all(layer.self_attn._prefill_uses_mask for layer in self.model.layers):
            raise ValueError(f"{type(self.model.layers[0].self_attn).__name__}: the prompt pass of this attention class ignores "
                             f"masks (llama_kivi.py:420-423), so padded prompts cannot be run; use the eager class")
        return True

    def _prompt_pass(self, input_ids, past_key_values, attention_mask, max_new_tokens: int, beams: int = 1):
        """The pass over `input_ids` of a generate call -> (the _PaddedBatch of a mask with a pad in it, else None; logits; pasts)."""
        B, T = input_ids.shape
        past_len = self._past_len(past_key_values)
        if attention_mask is not None and self._padded(attention_mask, B, past_len + T, past_len):
            pb = _PaddedBatch(attention_mask, past_len, T, max_new_tokens, beams)
            return (pb,) + self._forward(input_ids, past_key_values, pb.mask, pb.position_ids, True, True)
        return (None,) + self.forward(input_ids, past_key_values)

    def _decode_pass(self, tok, pasts, pb):
        """One decode step of a generate call -> (logits, pasts)."""
        if pb is None:
            return self.forward(tok, pasts)
        return self._forward(tok, pasts, *pb.step(), True, True)

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

    # ------------------------------------------------------------------ scoring given tokens
    _HEAD_SLAB = 4096            # rows of hidden states per lm_head call of score(): logits exist for one slab at a time

    def _score_plan(self, input_ids, first_chunk, chunk_size):
        """The [a, b) token ranges of the passes of a score() call; ValueError for arguments that cannot be scored (no device work)."""
        if input_ids.dim() != 2 or input_ids.shape[1] < 2:
            raise ValueError(f"score needs input_ids (B, T) with T >= 2 (entry i scores token i + 1), got {tuple(input_ids.shape)}")
        T = input_ids.shape[1]
        first = T if first_chunk is None else first_chunk
        if isinstance(first, bool) or not isinstance(first, int) or not 1 <= first <= T:
            raise ValueError(f"first_chunk has to be an integer in [1, T = {T}], got {first_chunk!r}")
        step = max(T - first, 1) if chunk_size is None else chunk_size
        if isinstance(step, bool) or not isinstance(step, int) or step < 1:
            raise ValueError(f"chunk_size has to be a positive integer, got {chunk_size!r}")
        return [(0, first)] + [(a, min(a + step, T)) for a in range(first, T, step)]

    def _head_logprobs(self, x, targets, return_rank):
        """token_logprobs of `targets` (B, q) under lm_head(norm(x)), x (B, q, H): the head runs on slabs of at most _HEAD_SLAB rows
        (one slab: the very call forward() makes), so logits never exist for more rows than that."""
        from .scoring import token_logprobs
        h = self.model.norm(x)
        B, q = targets.shape
        if B * q <= self._HEAD_SLAB:
            res = token_logprobs(self.lm_head(h), targets, return_rank=return_rank)
            return res if return_rank else (res, None)
        h, t = h.reshape(B * q, -1), targets.reshape(-1)
        lp = torch.empty(B * q, dtype=torch.float32, device=x.device)
        rk = torch.empty(B * q, dtype=torch.int32, device=x.device) if return_rank else None
        for s in range(0, B * q, self._HEAD_SLAB):
            res = token_logprobs(self.lm_head(h[s: s + self._HEAD_SLAB]), t[s: s + self._HEAD_SLAB], return_rank=return_rank)
            if return_rank:
                lp[s: s + self._HEAD_SLAB], rk[s: s + self._HEAD_SLAB] = res
            else:
                lp[s: s + self._HEAD_SLAB] = res
        return lp.view(B, q), rk.view(B, q) if return_rank else None

    @torch.no_grad()
    def score(self, input_ids: torch.LongTensor, attention_mask: Optional[torch.Tensor] = None,
              past_key_values: Optional[List] = None, first_chunk: Optional[int] = None, chunk_size: Optional[int] = None,
              return_rank: bool = False):
        """Teacher-forced log-probabilities of given tokens: (logprobs (B, T - 1) fp32, valid (B, T - 1) bool, past_key_values)
        [, ranks (B, T - 1) int32 with `return_rank`: 0 where the token is the argmax of its distribution, -1 where not valid].
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
        [1, T] raise ValueError before any device work."""
        plan = self._score_plan(input_ids, first_chunk, chunk_size)
        B, T = input_ids.shape
        facts = list(torch.aminmax(input_ids))
        if attention_mask is not None:
            facts.append((attention_mask == 0).any().to(input_ids.device, torch.long))
        lo, hi, *has_pad = (int(v) for v in torch.stack(facts).tolist())
        if lo < 0 or hi >= self.config.vocab_size:
            raise ValueError(f"input_ids hold token ids in [{lo}, {hi}], outside the vocabulary [0, {self.config.vocab_size})")
        past_len = self._past_len(past_key_values)
        valid = torch.ones((B, T - 1), dtype=torch.bool, device=input_ids.device)
        padded = attention_mask is not None and self._padded(attention_mask, B, past_len + T, past_len, bool(has_pad[0]))
        if padded:
            real = attention_mask[:, past_len:] != 0
            valid = real[:, 1:] & real[:, :-1]
        targets = torch.full((B, T), -100, dtype=torch.long, device=input_ids.device)     # the last token has nothing to predict
        targets[:, :-1] = torch.where(valid, input_ids[:, 1:], targets[:, :-1])
        logprobs = torch.empty((B, T), dtype=torch.float32, device=input_ids.device)
        ranks = torch.empty((B, T), dtype=torch.int32, device=input_ids.device) if return_rank else None
        pasts = past_key_values
        for a, b in plan:
            if padded:
                pb = _PaddedBatch(attention_mask[:, : past_len + b], past_len + a, b - a)
                x, pasts = self._hidden(input_ids[:, a:b], pasts, pb.mask, pb.position_ids, True)
            else:
                x, pasts = self._hidden(input_ids[:, a:b], pasts, None, None, False)
            lp, rk = self._head_logprobs(x, targets[:, a:b], return_rank)
            logprobs[:, a:b] = lp
            if return_rank:
                ranks[:, a:b] = rk
        res = (logprobs[:, :-1], valid, pasts)
        return res + (ranks[:, :-1],) if return_rank else res

    @torch.no_grad()
    def perplexity(self, input_ids: torch.LongTensor, attention_mask: Optional[torch.Tensor] = None,
                   past_key_values: Optional[List] = None, first_chunk: Optional[int] = None, chunk_size: Optional[int] = None):
        """exp(-sum of the valid log-probabilities / number of valid entries) of score() with the same arguments:
        (per row (B,), over all rows ()) float64 on the device, the sums taken in fp64.  A row without a valid entry gives NaN."""
        lp, valid, _ = self.score(input_ids, attention_mask, past_key_values, first_chunk, chunk_size)
        s, n = lp.double().sum(-1), valid.sum(-1).double()              # invalid entries are exactly 0
        return torch.exp(-s / n), torch.exp(-s.sum() / n.sum())

    @torch.no_grad()
    def generate(self, input_ids: torch.LongTensor, max_new_tokens: int, past_key_values: Optional[List] = None,
                 attention_mask: Optional[torch.Tensor] = None, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, num_return_sequences: int = 1, return_scores: bool = False, do_sample: bool = False,
                 temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, min_p: Optional[float] = None,
                 seed: Optional[int] = None, return_logprobs: bool = False, sampling=None):
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
        With beams use `return_scores`."""
        if return_logprobs and num_beams > 1:
            raise ValueError("return_logprobs is for greedy decoding and sampling; beam search (num_beams > 1) returns its "
                             "sequences_scores with return_scores=True")
        B, fan = input_ids.shape[0], 1
        if sampling is not None:
            sampler = self._row_sampler(input_ids.device, sampling, B, num_return_sequences, num_beams, do_sample, temperature,
                                        top_k, top_p, min_p, seed)
            fan = num_return_sequences
        else:
            sampler = self._sampler(input_ids.device, do_sample, num_beams, temperature, top_k, top_p, min_p, seed)
        if eos_token_id is not None and pad_token_id is None:
            raise ValueError("eos_token_id needs a pad_token_id for the rows that have finished")
        if sampling is None and (num_beams < 1 or num_return_sequences < 1 or num_return_sequences > num_beams):
            raise ValueError(f"num_return_sequences ({num_return_sequences}) must lie in [1, num_beams ({num_beams})]")
        if num_beams > 1:
            return self._generate_beams(input_ids, max_new_tokens, past_key_values, attention_mask, eos_token_id, pad_token_id,
                                        num_beams, length_penalty, early_stopping, num_return_sequences, return_scores)
        if return_scores:
            raise ValueError("return_scores: sequences_scores exist for beam search (num_beams > 1) only")
        if fan > 1 and past_key_values is not None:        # the fork below runs on a copy: the caller's caches stay as they are
            past_key_values = [p.layer.clone().as_tuple() for p in past_key_values]
        pb, logits, pasts = self._prompt_pass(input_ids, past_key_values, attention_mask, max_new_tokens, fan)
        if fan > 1:             # n samples per prompt: one prompt pass, then every request's row repeated n times (as the beams are)
            rows = torch.arange(B, device=input_ids.device).repeat_interleave(fan)
            pasts = [p.layer.index_select(rows).as_tuple() for p in pasts]
            logits, input_ids = logits.index_select(0, rows), input_ids.index_select(0, rows)
            B *= fan
        out, lps = [input_ids], []
        if return_logprobs:
            from .scoring import token_logprobs
        pick = (lambda lg: lg.argmax(-1)) if sampler is None else sampler
        tok = pick(logits)
        live = None if eos_token_id is None else torch.ones((B, 1), dtype=torch.bool, device=tok.device)
        for _ in range(max_new_tokens):
            if live is not None:
                tok = torch.where(live, tok, torch.full_like(tok, pad_token_id))
            if return_logprobs:                            # a finished row scores nothing: its target is the ignore_index
                lps.append(token_logprobs(logits, tok if live is None else torch.where(live, tok, torch.full_like(tok, -100))))
            if live is not None:
                live = live & (tok != eos_token_id)
            out.append(tok)
            if live is not None and not bool(live.any()):
                break
            logits, pasts = self._decode_pass(tok, pasts, pb)
            tok = pick(logits)
        if return_logprobs:
            return torch.cat(out, dim=1), torch.cat(lps or [logits.new_empty((B, 0), dtype=torch.float32)], dim=1)
        return torch.cat(out, dim=1)

    @staticmethod
    def _sampler(device, do_sample, num_beams, temperature, top_k, top_p, min_p, seed):
        """The Sampler of a do_sample call (None when greedy); every argument is checked before anything runs on a device."""
        if not do_sample:
            return None
        if num_beams != 1:
            raise ValueError(f"beam sampling (do_sample=True with num_beams={num_beams}) is not supported")
        from .sampling import Sampler
        return Sampler(temperature, top_k, top_p, min_p, seed, device)

    @staticmethod
    def _row_sampler(device, sampling, B, n, num_beams, do_sample, temperature, top_k, top_p, min_p, seed):
        """The RowSampler of a `sampling=` call over B requests with n samples each (row b * n + j: request b, stream j); every
        argument is checked before anything runs on a device."""
        from .sampling import RowSampler, SamplingParams
        if do_sample or temperature != 1.0 or top_k != 50 or top_p != 1.0 or min_p is not None or seed is not None:
            raise ValueError("sampling= carries the parameters of every row: it cannot be combined with do_sample=True or with "
                             "temperature / top_k / top_p / min_p / seed arguments")
        if num_beams != 1:
            raise ValueError(f"sampling= with beam search (num_beams={num_beams}) is not supported")
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"num_return_sequences ({n!r}) must be a positive integer")
        if isinstance(sampling, RowSampler):
            if sampling.B != B * n:
                raise ValueError(f"the RowSampler holds {sampling.B} rows; {B} requests x {n} samples need {B * n}")
            return sampling
        if isinstance(sampling, SamplingParams):
            sampling = [sampling] * B
        elif not isinstance(sampling, (list, tuple)) or not all(isinstance(p, SamplingParams) for p in sampling):
            raise ValueError("sampling has to be a SamplingParams, a list of B of them, or a RowSampler")
        if len(sampling) != B:
            raise ValueError(f"{len(sampling)} SamplingParams for a batch of {B} requests")
        bound = [RowSampler._bind(p) for p in sampling]          # one seed per request, shared by its n streams
        return RowSampler([p for p in bound for _ in range(n)], device, [j for _ in bound for j in range(n)])

    def _generate_beams(self, input_ids, max_new_tokens, past_key_values, attention_mask, eos_token_id, pad_token_id, nb,
                        length_penalty, early_stopping, num_return_sequences, return_scores):
        from .beam import beam_search
        B, T = input_ids.shape
        past_len = self._past_len(past_key_values)
        if past_key_values is not None:              # the caller's caches stay as they are
            past_key_values = [p.layer.clone().as_tuple() for p in past_key_values]
        pb, logits, pasts = self._prompt_pass(input_ids, past_key_values, attention_mask, max_new_tokens, nb)
        # the fork: every request's rows repeated over its beams; rows of a group agree on every byte before `fork`
        fork = past_len + T
        caches = [p.layer.index_select(torch.arange(B, device=input_ids.device).repeat_interleave(nb)) for p in pasts]

        def step(tok, beam_idx):
            for c in caches:
                c.reorder_(beam_idx, group=nb, from_token=fork, check=False)
            logits, _ = self._decode_pass(tok, [c.as_tuple() for c in caches], pb)
            return logits[:, -1].float()

        seqs, scores = beam_search(step, input_ids, logits[:, -1].float(), nb, max_new_tokens, eos_token_id, pad_token_id,
                                   length_penalty, early_stopping, num_return_sequences)
        return (seqs, scores) if return_scores else seqs

    # ------------------------------------------------------------------ hipGraph decode
    # The dense part of a decode step is ~30 small launches per layer; in eager mode the host needs longer to enqueue
    # them than the GPU to run them.  Everything with static shapes is captured once per batch size into hipGraphs
    # (torch.cuda.CUDAGraph): per layer one graph from the block input to the rotated q / k / v, one from the attention
    # output to the block output, plus embedding and head; the KIVI step between them stays one eager
    # kivi_decode_layer call per layer (its lengths change every step).  Same kernels, same results as forward().
    # Round 4: when every layer's cache is in the matrix-pipe layout the attention launches read their lengths from device
    # memory (kivi_amd/graph.py), so the WHOLE step -- dense parts and attention of all layers -- is ONE graph (whole=True).
    # Padded batches (padded=True): cos / sin hold one position per row, and `mask` is a static additive (B, 1, 1, pitch) fp16
    # buffer, pitch >= the cache capacity, that the attention of every step reads (its new column is 0: new tokens are real).
    # Sampling (sampler=): the last layer's post() draws into g.tok with the sampler instead of argmax; the captured call holds the
    # sampler's parameters and state buffer, so the graphs are keyed by Sampler.key() and captured again for another sampler.
    # A RowSampler keeps its parameters in device memory: its key() is the row count and two buffer pointers, so new parameter
    # values in the same RowSampler (set_row, or another request mix) replay the graphs that exist.
    def _build_graphs(self, B: int, device, whole: bool = False, padded: bool = False, sampler=None):
        cfg = self.config
        nh, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        D, H = self.model.layers[0].self_attn.head_dim, cfg.hidden_size
        dt = self.lm_head.weight.dtype
        rows = B if padded else 1
        g = SimpleNamespace(B=B, tok=torch.zeros((B, 1), dtype=torch.long, device=device),
                            cos=torch.zeros((rows, 1, 1, D), dtype=dt, device=device),
                            sin=torch.zeros((rows, 1, 1, D), dtype=dt, device=device),
                            x=[torch.zeros((B, 1, H), dtype=dt, device=device) for _ in range(len(self.model.layers) + 1)],
                            attn=torch.zeros((B, nh, 1, D), dtype=dt, device=device), qkv=[], pre=[], post=[], whole=whole,
                            padded=padded, mask=None, pos=None, sampler=sampler,
                            sample_key=None if sampler is None else sampler.key(), warmup=False)

        def rot(t):
            return torch.cat((-t[..., D // 2:], t[..., : D // 2]), dim=-1)

        def pre(i):
            layer = self.model.layers[i]
            a = layer.self_attn
            if i == 0:
                g.x[0].copy_(self.model.embed_tokens(g.tok))
            h = layer.input_layernorm(g.x[i])
            q = a.q_proj(h).view(B, 1, nh, D).transpose(1, 2)
            k = a.k_proj(h).view(B, 1, nkv, D).transpose(1, 2)
            v = a.v_proj(h).view(B, 1, nkv, D).transpose(1, 2)
            g.qkv[i][0].copy_(q * g.cos + rot(q) * g.sin)
            g.qkv[i][1].copy_(k * g.cos + rot(k) * g.sin)
            g.qkv[i][2].copy_(v)

        def post(i):
            layer = self.model.layers[i]
            x = g.x[i] + layer.self_attn.o_proj(g.attn.transpose(1, 2).reshape(B, 1, nh * D))
            g.x[i + 1].copy_(x + layer.mlp(layer.post_attention_layernorm(x)))
            if i == len(self.model.layers) - 1:
                logits = self.lm_head(self.model.norm(g.x[i + 1]))
                if g.sampler is None or g.warmup:       # (the warm-up must not consume a draw)
                    g.tok.copy_(logits.argmax(-1))
                else:
                    g.sampler(logits, out=g.tok)

        for _ in self.model.layers:
            g.qkv.append((torch.zeros((B, nh, 1, D), dtype=dt, device=device),
                          torch.zeros((B, nkv, 1, D), dtype=dt, device=device),
                          torch.zeros((B, nkv, 1, D), dtype=dt, device=device)))
        g.pre_fn, g.post_fn = pre, post
        if whole:               # captured by kivi_amd.graph.GraphedDecode together with the attention launches
            return g
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        g.warmup = True
        with torch.cuda.stream(side):          # warm-up outside capture (library workspaces, autotuning)
            for i in range(len(self.model.layers)):
                pre(i)
                post(i)
        torch.cuda.current_stream(device).wait_stream(side)
        g.warmup = False
        from .graph import no_gc_in_capture
        pool = None
        with no_gc_in_capture():
            for i in range(len(self.model.layers)):
                for fn, dst in ((pre, g.pre), (post, g.post)):
                    cg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cg, pool=pool):
                        fn(i)
                    pool = pool or cg.pool()
                    dst.append(cg)
        g.tok.zero_()
        return g

    def prepare_graphs(self, batch: int, device, whole: bool = False, padded: bool = False, sampler=None) -> None:
        """Capture the decode graphs for this batch size now (otherwise on the first graphed step)."""
        g = getattr(self, "_graphs", None)
        key = None if sampler is None else sampler.key()
        if g is None or g.B != batch or g.whole != whole or g.padded != padded or g.sample_key != key:
            self._graphs = self._build_graphs(batch, device, whole, padded, sampler)

    @staticmethod
    def _mask_room(g, caches, whole: bool) -> bool:
        """Room for one more token in every cache and a mask buffer as wide as their capacity (the whole-step graph: the tokens
        the stores can hold, so that the buffer moves only when the stores do).  True when the buffer was reallocated."""
        from .cache_mf import SB
        for c in caches:
            c.ensure_room(1)
        need = caches[0].n_sb * SB if whole else ((caches[0].cap + 7) // 8) * 8
        if g.mask is not None and g.mask.shape[3] >= need:
            return False
        new = torch.zeros((g.B, 1, 1, need), dtype=torch.float16, device=g.tok.device)
        if g.mask is not None:
            new[..., : g.mask.shape[3]].copy_(g.mask)
        g.mask = new
        return True

    def _graph_inputs(self, g, caches, whole: bool, padded: bool, position: int) -> bool:
        """The inputs of one graphed step in their static buffers: cos / sin of the step's position (padded: of the per-row positions
        g.pos, which then advance, and room in the mask buffer -- True when that was reallocated)."""
        inv_freq = self.model.layers[0].self_attn.inv_freq
        cos, sin = rope_cos_sin(inv_freq, g.pos if padded else position)
        g.cos.copy_(cos.view(-1, 1, 1, cos.shape[-1]))
        g.sin.copy_(sin.view(-1, 1, 1, sin.shape[-1]))
        if not padded:
            return False
        g.pos += 1
        return self._mask_room(g, caches, whole)

    @torch.no_grad()
    def decode_graphed(self, tok: torch.LongTensor, past_key_values: List, position: int, steps: int,
                       attention_mask: Optional[torch.Tensor] = None, sampler=None, sampling=None) -> torch.LongTensor:
        """`steps` decode steps from token `tok` (B, 1) at position `position` with the dense part replayed from
        hipGraphs; the caches in `past_key_values` are advanced in place.  Returns the (B, steps) tokens fed to the model
        (tok first); the token following them is left in the graph's token buffer (`self._graphs.tok`).
        `attention_mask`: HF's 2D mask (B, kv_len + 1) over the cached tokens and `tok` (1 = real token); with a pad in it
        every row takes its own position from the mask (`position` is not used) and the pads are masked in every step.
        `sampler`: a kivi_amd.sampling.Sampler that draws each next token (one draw per step, inside the graph); None: greedy.
        `sampling`: a kivi_amd.sampling.RowSampler of B rows in its place (per-row parameters; not together with `sampler`).  The
        graphs depend on its buffers only: set_row() between steps or calls replays what was captured."""
        if sampling is not None:
            if sampler is not None:
                raise ValueError("pass either sampler= or sampling=, not both")
            if not callable(sampling) or not hasattr(sampling, "key"):
                raise ValueError("decode_graphed(sampling=) takes a RowSampler")
            if getattr(sampling, "B", tok.shape[0]) != tok.shape[0]:
                raise ValueError(f"the RowSampler holds {sampling.B} rows, the step has {tok.shape[0]}")
            sampler = sampling
        from .attention import kivi_attention_decode
        from .cache_mf import KiviLayerCacheMF
        caches = [p.layer for p in past_key_values]
        whole = all(isinstance(c, KiviLayerCacheMF) for c in caches)
        B, kv0 = tok.shape[0], caches[0].kv_seq_len
        padded = attention_mask is not None and self._padded(attention_mask, B, kv0 + 1, kv0)
        self.prepare_graphs(B, tok.device, whole, padded, sampler)
        g = self._graphs
        g.tok.copy_(tok)
        if padded:
            if self._mask_room(g, caches, whole):
                self._graphed = None             # a graph captured over the old buffer is stale
            g.mask.zero_()
            g.mask[..., : kv0 + 1].masked_fill_((attention_mask == 0)[:, None, None, :], _MIN16)
            g.pos = attention_mask.long().sum(-1) - 1                    # (B,): position of `tok`
        out = []
        if whole:
            from .graph import GraphedDecode, MfStepDriver
            # the driver and its captured graph live on the model, for the caches (held weakly: MfStepDriver.serves) and the static
            # buffers they were built for: a second decode_graphed call over the same caches replays the graph it already has instead
            # of paying an eager step and a 32-layer capture again (only a new geometry class or a reallocated buffer re-captures:
            # MfStepDriver.prepare).  Nothing here keeps a finished request's KV cache alive.
            st = getattr(self, "_graphed", None)
            if st is not None and st[0] is g and st[1].serves(caches):
                drv, gd = st[1], st[2]
                drv.resync()
            else:
                drv = MfStepDriver(caches)

                def body():
                    for i in range(len(self.model.layers)):
                        g.pre_fn(i)
                        drv.enqueue(i, *g.qkv[i], g.attn, g.mask)
                        g.post_fn(i)

                gd = GraphedDecode(drv, body)
                self._graphed = (g, drv, gd)
            for _ in range(steps):
                out.append(g.tok.clone())
                if self._graph_inputs(g, caches, whole, padded, position):     # the stores grew: so did the buffer, capture again
                    gd.graph, gd.warm = None, False
                gd.step()
                position += 1
            self._last_graph_stats = (gd.eager, gd.captures, gd.replays)
            return torch.cat(out, dim=1)
        for _ in range(steps):
            out.append(g.tok.clone())
            self._graph_inputs(g, caches, whole, padded, position)
            mask = g.mask[..., : caches[0].kv_seq_len + 1] if padded else None
            for i in range(len(self.model.layers)):
                g.pre[i].replay()
                q, k, v = g.qkv[i]
                kivi_attention_decode(q, k, v, caches[i], attention_mask=mask, out=g.attn)
                g.post[i].replay()
            position += 1
        return torch.cat(out, dim=1)

    @torch.no_grad()
    def generate_graphed(self, input_ids: torch.LongTensor, max_new_tokens: int,
                         attention_mask: Optional[torch.Tensor] = None, num_beams: int = 1, do_sample: bool = False,
                         temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, min_p: Optional[float] = None,
                         seed: Optional[int] = None, sampling=None) -> torch.LongTensor:
        """generate() with the dense part of every decode step replayed from hipGraphs (see _build_graphs).
        `attention_mask`: HF's 2D (B, T) mask of left-padded prompts (1 = real token).  Greedy, or sampling with `do_sample=True`
        and the parameters of generate() (the draw inside the graph; the same tokens as generate() with the same seed).  Beams
        are refused (a graphed beam step is open; use generate()).  `sampling=`: per-request parameters as in
        generate() (a SamplingParams, a list of B, or a RowSampler of B rows); the graphs are keyed by the RowSampler's buffers."""
        if sampling is not None:
            sampler = self._row_sampler(input_ids.device, sampling, input_ids.shape[0], 1, num_beams, do_sample, temperature,
                                        top_k, top_p, min_p, seed)
        else:
            if num_beams != 1 and not do_sample:
                raise ValueError(f"generate_graphed is greedy only (num_beams={num_beams}); use generate(num_beams=...)")
            sampler = self._sampler(input_ids.device, do_sample, num_beams, temperature, top_k, top_p, min_p, seed)
        logits, pasts = self.forward(input_ids, padding_mask=attention_mask)
        if attention_mask is not None:
            attention_mask = torch.cat([attention_mask, torch.ones_like(attention_mask[:, :1])], dim=1)
        tok = logits.argmax(-1) if sampler is None else sampler(logits)
        new = self.decode_graphed(tok, pasts, input_ids.shape[1], max_new_tokens, attention_mask, sampler)
        self._graphed = None        # the caches of this request die with it: so does the graph captured over them
        return torch.cat([input_ids, new], dim=1)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda", dtype=torch.float16, **kivi):
        """`path`: a local HF checkpoint directory (config.json + *.safetensors).  `kivi`: k_bits, v_bits, group_size,
        residual_length, max_cache_len."""
        from safetensors.torch import load_file
        cfg = make_config(json.load(open(os.path.join(path, "config.json"))), **kivi)
        with torch.device(device):
            prev = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                model = cls(cfg)
            finally:
                torch.set_default_dtype(prev)
        state = {}
        for f in sorted(glob.glob(os.path.join(path, "*.safetensors"))):
            state.update(load_file(f, device=str(device)))
        missing, unexpected = model.load_state_dict(state, strict=False)
        missing = [m for m in missing if "inv_freq" not in m and not (cfg.tie_word_embeddings and m == "lm_head.weight")]
        if missing:
            raise KeyError(f"checkpoint lacks {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        return model


class MistralForCausalLM_KIVI(LlamaForCausalLM_KIVI):
    """Counterpart of models/mistral_kivi.py:921 (MistralForCausalLM_KIVI): the same decoder around MistralAttention_KIVI
    (bias-free projections, grouped queries mapped inside the kernels, `sliding_window` carried but -- like the reference,
    mistral_kivi.py:356-367 -- never applied to the quantised history)."""

    def __init__(self, config, attention_cls=None):
        from .attention import MistralAttention_KIVI
        super().__init__(config, attention_cls or MistralAttention_KIVI)
