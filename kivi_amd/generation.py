"""What a generate call is made of, apart from the model: left padding, the sampler of the call, the prompt pass with its fork to
n rows per request, the eager decode step, and the ONE loop of greedy decoding and sampling over two callables, `step(tok) -> logits`
and `pick(logits) -> tok`.  Beam search (kivi_amd/beam.py) is fed the same EagerStepper; the graphed step: kivi_amd/graph.py."""
from __future__ import annotations

from typing import Callable, Optional

import torch

from .prefill import PromptLead

_MIN16 = torch.finfo(torch.float16).min
PADS_LEFT = 2     # what LlamaForCausalLM_KIVI._padded answers for a padded prompt pass that runs the prefill kernel (True otherwise)


def left_pad(seqs, pad_token_id: int = 0, device=None, length: Optional[int] = None):
    """A list of token id sequences -> (ids (B, T), mask (B, T)) left-padded to the longest one (HF's tokenizer with
    padding_side="left"): mask is 1 on real tokens, 0 on the `pad_token_id` fillers.  `length`: pad to T = length instead (an
    admission into living caches pads to their length); ValueError when a sequence is longer."""
    seqs = [torch.as_tensor(s, dtype=torch.long).flatten() for s in seqs]
    T = max(len(s) for s in seqs)
    if length is not None:
        if isinstance(length, bool) or not isinstance(length, int) or length < T:
            raise ValueError(f"length={length!r}: the longest sequence has {T} tokens, it cannot be left-padded to that")
        T = length
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


def leading_pads(mask2d: torch.Tensor) -> torch.Tensor:
    """(B,) int32 on the mask's device: the zeros at the front of every row of a 2D padding mask (0 for a row without pads) --
    derived on the device, never read on the host."""
    return ((mask2d != 0).cumsum(-1) == 0).sum(-1).to(torch.int32)


class DecodeLead:
    """What a padded decode step hands its attention modules in place of the additive key row with config.kivi_decode_lead (DESIGN.md
    section 21): the row itself, `mask` (B, 1, 1, kv length incl. the new token), and `lead` (B,) int32, the leading keys of every
    row that it masks.  The row kernels skip them; the mask is applied to everything they read all the same."""

    def __init__(self, mask: torch.Tensor, lead: torch.Tensor):
        self.mask, self.lead = mask, lead


def decode_key_row(mask2d: torch.Tensor, lead: bool = False):
    """The additive key row of a decode step over the 2D mask (B, kv length incl. the new token); `lead`: as a DecodeLead, the lead
    derived from the same mask -- so a mask an admission or a rebase has changed brings its own."""
    row = padding_key_row(mask2d)
    return DecodeLead(row, leading_pads(mask2d)) if lead else row


class _PaddedBatch:
    """What a left-padded batch adds to the passes of one call, derived once from HF's 2D mask (B, past_len + T): `mask` and
    `position_ids` of the pass over the T new tokens (the prompt's 4D causal + padding mask; with a history, the key row expanded
    over the chunk), then per decode step a view of the key row one column longer (new tokens are real) and the advancing
    position.  `beams`: the decode steps run on every row repeated that often (the prompt pass does not).  `lead`: the prompt pass
    (no history) runs the prefill kernel -- its `mask` is a PromptLead, the leading pads of every row, and no 4D mask is built.
    `decode_lead` (config.kivi_decode_lead): every decode step gets its key row as a DecodeLead, with the leading zeros of every
    row of the mask (repeated over beams like the row)."""

    def __init__(self, mask2d: torch.Tensor, past_len: int, T: int, max_new_tokens: int = 0, beams: int = 1, lead: bool = False,
                 decode_lead: bool = False):
        n = past_len + T
        row = padding_key_row(mask2d, n + max_new_tokens)
        if past_len == 0:
            self.mask = PromptLead(mask2d) if lead else padding_prompt_mask(mask2d)
        else:
            self.mask = row[..., :n].expand(-1, -1, T, -1)
        self.position_ids = padding_position_ids(mask2d, T)
        if max_new_tokens:
            pos = mask2d.long().sum(-1, keepdim=True)                  # (B, 1): position of the next token
            dl = leading_pads(mask2d) if decode_lead else None
            if beams > 1:
                row, pos = row.repeat_interleave(beams, dim=0), pos.repeat_interleave(beams, dim=0)
                dl = None if dl is None else dl.repeat_interleave(beams, dim=0)
            self._row, self._pos, self._len, self._lead = row, pos, n, dl

    def step(self):
        """(additive key row (B, 1, 1, kv length incl. the new token), position ids (B, 1)) of the next decode step."""
        self._len += 1
        pos = self._pos
        self._pos = pos + 1
        row = self._row[..., : self._len]
        return (row if self._lead is None else DecodeLead(row, self._lead)), pos


def resolve_sampler(device, B: int, num_return_sequences: int, num_beams: int, do_sample: bool, temperature, top_k, top_p, min_p,
                    seed, sampling, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                    vocab_size: Optional[int] = None, logit_bias=None, allowed_token_ids=None, min_new_tokens: int = 0):
    """The sampler of a generate / generate_graphed call -> (pick, fan): `pick(logits) -> tokens` is a Sampler (`do_sample=True`), a
    RowSampler (`sampling=`: B requests with `fan` = num_return_sequences samples each, row b * fan + j is request b with Philox
    stream j) or None (greedy); without `sampling=` fan is 1.  Every argument is checked before anything runs on a device.
    A non-neutral `repetition_penalty` / `presence_penalty` / `frequency_penalty` without `sampling=`: a
    RowSampler of B identical rows with streams 0..B-1 and the call's seed -- by the identity of kivi_sample_rows what the Sampler
    would have drawn from the penalised logits --, greedy rows when `do_sample=False`; not with beams.  With `sampling=` the penalties
    come from the SamplingParams, the three arguments have to be neutral.  `vocab_size`: the width of the history table of a
    RowSampler made here for penalised or constrained rows.
    `logit_bias` / `allowed_token_ids` / `min_new_tokens` route like the penalties: non-neutral values without
    `sampling=` make that RowSampler of identical rows, with constraint state; with `sampling=` they come from the SamplingParams and
    the three arguments stay neutral; not with beams.  The ids `min_new_tokens` suppresses are bound later, once the call's finish
    conditions are resolved (bind_suppress)."""
    from .sampling import NEUTRAL, UNCONSTRAINED, RowSampler, Sampler, SamplingParams, check_constraints, check_penalties
    check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
    penalised = (float(repetition_penalty), float(presence_penalty), float(frequency_penalty)) != NEUTRAL
    constrained = check_constraints(logit_bias, allowed_token_ids, min_new_tokens) != UNCONSTRAINED
    if sampling is None and (penalised or constrained):
        if num_beams != 1:
            raise ValueError(f"repetition / presence / frequency penalties, logit_bias, allowed_token_ids and min_new_tokens with beam "
                             f"search (num_beams={num_beams}) are not supported")
        p = RowSampler._bind(SamplingParams(bool(do_sample), temperature, top_k, top_p, min_p, seed, repetition_penalty=repetition_penalty,
                                            presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                                            logit_bias=logit_bias, allowed_token_ids=allowed_token_ids, min_new_tokens=min_new_tokens))
        return RowSampler([p] * B, device, list(range(B)), vocab_size=vocab_size), 1
    if sampling is None:
        if not do_sample:
            return None, 1
        if num_beams != 1:
            raise ValueError(f"beam sampling (do_sample=True with num_beams={num_beams}) is not supported")
        return Sampler(temperature, top_k, top_p, min_p, seed, device), 1
    n = num_return_sequences
    if do_sample or temperature != 1.0 or top_k != 50 or top_p != 1.0 or min_p is not None or seed is not None or penalised \
            or constrained:
        raise ValueError("sampling= carries the parameters of every row: it cannot be combined with do_sample=True or with "
                         "temperature / top_k / top_p / min_p / seed / repetition_penalty / presence_penalty / frequency_penalty / "
                         "logit_bias / allowed_token_ids / min_new_tokens arguments")
    if num_beams != 1:
        raise ValueError(f"sampling= with beam search (num_beams={num_beams}) is not supported")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"num_return_sequences ({n!r}) must be a positive integer")
    if isinstance(sampling, RowSampler):
        if sampling.B != B * n:
            raise ValueError(f"the RowSampler holds {sampling.B} rows; {B} requests x {n} samples need {B * n}")
        return sampling, n
    if isinstance(sampling, SamplingParams):
        sampling = [sampling] * B
    elif not isinstance(sampling, (list, tuple)) or not all(isinstance(p, SamplingParams) for p in sampling):
        raise ValueError("sampling has to be a SamplingParams, a list of B of them, or a RowSampler")
    if len(sampling) != B:
        raise ValueError(f"{len(sampling)} SamplingParams for a batch of {B} requests")
    bound = [RowSampler._bind(p) for p in sampling]          # one seed per request, shared by its n streams
    return RowSampler([p for p in bound for _ in range(n)], device, [j for _ in bound for j in range(n)],
                      vocab_size=vocab_size if any(p.penalised or p.constrained for p in bound) else None), n


def bind_suppress(pick, sampling, stops, eos_token_id) -> None:
    """A generate call hands the RowSampler it has made (not a caller's, which is used as it is) the ids that `min_new_tokens`
    suppresses: per row its eos ids and the stop token ids of its StopParams -- `stops`, resolve_stopping's result (None: the one int
    `eos_token_id` of the torch path, or nothing).  Stop sequences are not suppressed: they may still end a request early."""
    if pick is None or pick is sampling or getattr(pick, "_con", None) is None:
        return
    from .stopping import stop_ids
    if stops is None:
        ids = [stop_ids(eos_token_id, None)] * pick.B
    else:
        ids = [p.stop_token_ids for p in (stops if isinstance(stops, (list, tuple)) else stops.rows)]
    pick.bind_suppress(ids)


def observe_prompts(pick, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], fan: int = 1) -> None:
    """A generate call marks its `input_ids` (B, T) in the history table of its RowSampler, if it has one (any other `pick` knows no
    history): without the pads of HF's 2D mask (B, past + T), whose last T columns cover `input_ids`, and `fan` times per request,
    once for every forked row.  With `past_key_values` only this call's `input_ids` are known: the earlier turns stay marked only
    in a RowSampler that the caller passes again."""
    if getattr(pick, "seen", None) is None:
        return
    T = input_ids.shape[1]
    mask = None if attention_mask is None or attention_mask.dim() != 2 else attention_mask[:, attention_mask.shape[1] - T:]
    if fan > 1:
        input_ids = input_ids.repeat_interleave(fan, dim=0)
        mask = None if mask is None else mask.repeat_interleave(fan, dim=0)
    pick.observe_prompt(input_ids, attention_mask=mask)


class EagerStepper:
    """The eager passes of one generate call: the pass over `input_ids` here, then `step(tok) -> logits`, over caches (`pasts`,
    advanced in place) and the _PaddedBatch of a mask with a pad in it, which it owns.  `n` > 1 is the ONE fork of beams and of n
    samples per prompt: after the prompt pass on the B requests every request's row is repeated n times -- on a copy when the
    caches are the caller's (`past_key_values`), which stay byte for byte what they were.  `logits` (B * n, 1, vocab): the prompt
    pass's; `input_ids` (B * n, T).  Beams: `step(tok, beam_idx)`, the step callback of beam_search, calls `reorder_` first."""

    def __init__(self, model, input_ids, past_key_values, attention_mask, max_new_tokens: int, n: int = 1):
        B, T = input_ids.shape
        past_len = model._past_len(past_key_values)
        if n > 1 and past_key_values is not None:
            past_key_values = [p.layer.clone().as_tuple() for p in past_key_values]
        self.model, self.padded, self.group, self.fork = model, None, n, past_len + T
        padded = attention_mask is not None and model._padded(attention_mask, B, past_len + T, past_len)
        if padded:
            self.padded = _PaddedBatch(attention_mask, past_len, T, max_new_tokens, n, lead=padded == PADS_LEFT,
                                       decode_lead=bool(getattr(model.config, "kivi_decode_lead", False)))
            logits, pasts = model._forward(input_ids, past_key_values, self.padded.mask, self.padded.position_ids, True, True)
        else:
            logits, pasts = model.forward(input_ids, past_key_values)
        if n > 1:
            rows = torch.arange(B, device=input_ids.device).repeat_interleave(n)
            pasts = [p.layer.index_select(rows).as_tuple() for p in pasts]
            logits, input_ids = logits.index_select(0, rows), input_ids.index_select(0, rows)
        self.pasts, self.logits, self.input_ids = pasts, logits, input_ids

    def step(self, tok: torch.LongTensor, beam_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        if beam_idx is not None:
            self.reorder_(beam_idx)
        mask, position_ids = (None, None) if self.padded is None else self.padded.step()
        logits, self.pasts = self.model._forward(tok, self.pasts, mask, position_ids, True, True)
        return logits

    def reorder_(self, beam_idx: torch.Tensor) -> None:
        """Row b of every cache <- row beam_idx[b], in place and from the fork on (rows of a request agree on every byte before it)."""
        for p in self.pasts:
            p.layer.reorder_(beam_idx, group=self.group, from_token=self.fork, check=False)


def decode_loop(first_logits: torch.Tensor, step: Callable, pick: Callable, max_new_tokens: int,
                eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, want_logprobs: bool = False,
                top_k: int = 0, stopper=None):
    """Greedy decoding and sampling: every token is `pick` of the logits (B, 1, vocab) before it -- `first_logits`, then `step(tok)`.
    -> (tokens (B, generated) int64, their fp32 log-probabilities under the raw distribution or None).  A row that has produced
    `eos_token_id` emits `pad_token_id` from then on and scores target -100; the loop stops when every row has finished (the one
    synchronisation of a step, only with `eos_token_id`).  Otherwise the last token is still stepped and picked over: caches end
    max_new_tokens tokens on, a sampler max_new_tokens + 1 draws on.
    `top_k` > 0 (with want_logprobs): the second result is (logprobs, top_ids (B, generated, top_k) int64, top_logprobs (B, generated,
    top_k) fp32) -- the k most likely tokens of every step's raw distribution, from ONE kivi_token_top_logprobs launch per step in
    place of the kivi_token_logprob launch; a finished row's pads get id -1 and value 0.
    `stopper` (not with `eos_token_id`): a finish tracker in place of the torch `live` arithmetic -- an object
    with `reason` ((B,) integers, 0 = the row is live), `__call__(tok)` (takes the picked tokens (B, 1) in place: a live row's token
    is counted and may finish the row, a finished row's is overwritten with the pad) and `n_live` (one integer, the live rows after
    the call); kivi_amd.stopping.StopRows is one, on the device.  A row that was not live before its token scores target -100;
    `int(stopper.n_live)` is the step's one synchronisation, and the loop leaves when it is 0 -- a length limit is a finish like any
    other, so a call whose rows all end by their limits does NOT run the pass after the last token."""
    if stopper is not None and eos_token_id is not None:
        raise ValueError("decode_loop takes either eos_token_id or a stopper (whose stop ids include it), not both")
    from .scoring import picked_scores                 # here, not at the top: scoring imports this module (this breaks the cycle)
    k = (top_k or 0) if want_logprobs else None
    logits, out, cols = first_logits, [], ([], [], [])  # cols: logprob, top ids, top log-probabilities of every token
    tok = pick(logits)
    B = tok.shape[0]
    live = None if eos_token_id is None else torch.ones((B, 1), dtype=torch.bool, device=tok.device)
    for _ in range(max_new_tokens):
        if stopper is not None:
            live = (stopper.reason == 0).view(B, 1)    # before this token: a new tensor, the tracker's own state moves on below
            stopper(tok)
        elif live is not None:
            tok = torch.where(live, tok, torch.full_like(tok, pad_token_id))
        if k is not None:                              # a finished row scores nothing: its target is the ignore_index
            sc = picked_scores(logits, tok if live is None else torch.where(live, tok, torch.full_like(tok, -100)), k)
            if k and live is not None:                 # ... and its lists hold id -1, value 0
                sc = (sc[0], sc[1].masked_fill(~live.unsqueeze(-1), -1), sc[2].masked_fill(~live.unsqueeze(-1), 0.0))
            for col, v in zip(cols, sc):
                col.append(v)
        if stopper is None and live is not None:
            live = live & (tok != eos_token_id)
        out.append(tok)
        if stopper is not None:
            if int(stopper.n_live) == 0:
                break
        elif live is not None and not bool(live.any()):
            break
        logits = step(tok)
        tok = pick(logits)
    lps = None
    if k is not None:
        lps = torch.cat(cols[0], dim=1) if out else logits.new_empty((B, 0), dtype=torch.float32)
        if k:
            lps = (lps, torch.cat(cols[1], dim=1) if out else tok.new_empty((B, 0, k)),
                   torch.cat(cols[2], dim=1) if out else logits.new_empty((B, 0, k), dtype=torch.float32))
    return torch.cat(out, dim=1) if out else tok.new_empty((B, 0)), lps


def pack_result(input_ids: torch.Tensor, new: torch.Tensor, scores=()):
    """What a generate call returns: the prompts with the new tokens behind them, alone or as (sequences, logprobs[, top_ids,
    top_logprobs]) -- `scores`: those of the new tokens as a tuple, or as decode_loop gives them (None, or the logprobs alone)."""
    if not isinstance(scores, tuple):
        scores = () if scores is None else (scores,)
    seqs = torch.cat([input_ids, new], dim=1)
    return (seqs,) + scores if scores else seqs
