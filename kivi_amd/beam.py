"""Beam search over a step callback: the vectorised GenerationMixin._beam_search of Hugging Face transformers v5 and its helpers
(_get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic,
_beam_search_has_unfinished_sequences), with the same length_penalty / early_stopping semantics, the same beams_to_keep, the same
padding of finished sequences and the same sequences_scores.  Greedy search only (no sampling, no logits processors).

The model is reached through `step(tokens (B * nb, 1), beam_idx (B * nb,)) -> logits (B * nb, vocab) or (B * nb, 1, vocab)`:
reorder the caches by `beam_idx` (flat indices, beam b * nb + j of request b), then run one decode step.  The prompt pass is the
caller's: its logits come in as `first_logits`, in either shape.  transformers is not imported.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import torch


def _gather(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


def _flat(t: torch.Tensor) -> torch.Tensor:
    return t.reshape([t.shape[0] * t.shape[1]] + list(t.shape[2:]))


def beam_search(step: Callable, input_ids: torch.LongTensor, first_logits: torch.Tensor, num_beams: int, max_new_tokens: int,
                eos_token_id: Optional[Union[int, list]] = None, pad_token_id: Optional[int] = None, length_penalty: float = 1.0,
                early_stopping: Union[bool, str] = False, num_return_sequences: int = 1):
    """-> (sequences (B * num_return_sequences, T + generated) int64, sequences_scores (B * num_return_sequences,) fp32).
    `input_ids` (B, T): the prompts (not expanded); `first_logits`: the prompt pass's last-position logits, (B, vocab) or
    (B * num_beams, vocab)."""
    if num_return_sequences > num_beams:
        raise ValueError(f"num_return_sequences ({num_return_sequences}) must be <= num_beams ({num_beams})")
    if early_stopping not in (True, False, "never"):
        raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
    B, cur_len = input_ids.shape
    nb = num_beams
    dev = first_logits.device
    vocab = first_logits.shape[-1]
    eos = None if eos_token_id is None else torch.as_tensor(eos_token_id, device=dev).flatten()
    prompt_len = cur_len
    max_length = cur_len + max_new_tokens
    beams_to_keep = max(2, 1 + (0 if eos is None else eos.numel())) * nb
    top_num_beam_mask = torch.cat((torch.ones(nb, dtype=torch.bool), torch.zeros(beams_to_keep - nb, dtype=torch.bool))).to(dev)
    fill = (pad_token_id if pad_token_id else int(eos[0])) if eos is not None else -1      # HF: `pad or eos[0] if eos else -1`

    running_sequences = torch.full((B, nb, max_length), fill, dtype=torch.int64, device=dev)
    running_sequences[:, :, :cur_len] = input_ids.to(dev)[:, None, :]
    sequences = running_sequences.clone()
    running_beam_scores = torch.zeros((B, nb), dtype=torch.float, device=dev)
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((B, nb), -1e9, dtype=torch.float, device=dev)
    is_sent_finished = torch.zeros((B, nb), dtype=torch.bool, device=dev)
    unsatisfied = torch.ones((B, 1), dtype=torch.bool, device=dev)
    hits = torch.zeros((B, nb), dtype=torch.bool, device=dev)
    running_beam_indices = torch.full((B, nb, max_length - cur_len), -1, dtype=torch.int32, device=dev)
    beam_indices = running_beam_indices.clone()
    batch_offset = torch.arange(B, device=dev).view(-1, 1) * nb

    logits = first_logits.float()
    if logits.shape[0] == B and nb > 1:
        logits = logits.repeat_interleave(nb, dim=0)
    beam_idx = None
    while True:
        if beam_idx is not None:
            logits = step(_flat(running_sequences[:, :, cur_len - 1: cur_len]), beam_idx).float()
        log_probs = torch.log_softmax(logits, dim=-1).view(B, nb, vocab) + running_beam_scores[:, :, None]
        log_probs = log_probs.reshape(B, nb * vocab)

        # _get_top_k_continuations
        topk_log_probs, topk_indices = torch.topk(log_probs, k=beams_to_keep)
        topk_beam = topk_indices // vocab
        topk_running_beam_indices = _gather(running_beam_indices, topk_beam)
        topk_running_sequences = _gather(running_sequences, topk_beam)
        topk_running_sequences[:, :, cur_len] = topk_indices % vocab
        topk_running_beam_indices[:, :, cur_len - prompt_len] = (topk_beam + batch_offset).to(torch.int32)

        # stopping criteria of the candidates: max length, EOS
        last = topk_running_sequences[:, :, cur_len]
        hits = torch.full_like(last, cur_len + 1 >= max_length, dtype=torch.bool)
        if eos is not None:
            hits = hits | torch.isin(last, eos)

        # _get_running_beams_for_next_iteration
        topk_running_log_probs = topk_log_probs + hits.to(torch.float32) * -1.0e9
        nxt = torch.topk(topk_running_log_probs, k=nb)[1]
        running_sequences = _gather(topk_running_sequences, nxt)
        running_beam_scores = _gather(topk_running_log_probs, nxt)
        running_beam_indices = _gather(topk_running_beam_indices, nxt)

        # _update_finished_beams
        just_finished = hits & top_num_beam_mask[None, :]
        fin = topk_log_probs / ((cur_len + 1 - prompt_len) ** length_penalty)
        full = torch.all(is_sent_finished, dim=-1, keepdim=True) & (early_stopping is True)
        fin = fin + full.to(torch.float32) * -1.0e9
        fin = fin + (~unsatisfied).to(torch.float32) * -1.0e9
        fin = fin + (~just_finished) * -1.0e9
        merged_idx = torch.topk(torch.cat((beam_scores, fin), dim=1), k=nb)[1]
        sequences = _gather(torch.cat((sequences, topk_running_sequences), dim=1), merged_idx)
        beam_scores = _gather(torch.cat((beam_scores, fin), dim=1), merged_idx)
        beam_indices = _gather(torch.cat((beam_indices, topk_running_beam_indices), dim=1), merged_idx)
        is_sent_finished = _gather(torch.cat((is_sent_finished, just_finished), dim=1), merged_idx)

        beam_idx = _flat(running_beam_indices[..., cur_len - prompt_len])
        cur_len += 1

        # _check_early_stop_heuristic
        if early_stopping == "never" and length_penalty > 0.0:
            best_len = max_length - prompt_len
        else:
            best_len = cur_len - prompt_len
        best_running = running_beam_scores[:, :1] / (best_len ** length_penalty)
        worst_finished = torch.where(is_sent_finished, torch.min(beam_scores, dim=1, keepdim=True)[0], -1.0e9)
        unsatisfied = unsatisfied & torch.any(best_running > worst_finished, dim=-1, keepdim=True)

        # _beam_search_has_unfinished_sequences
        open_beam = not (bool(torch.all(is_sent_finished)) and early_stopping is True)
        if not (bool(torch.any(unsatisfied)) and open_beam and not bool(torch.all(hits))):
            break

    sequences = _flat(sequences[:, :num_return_sequences, :])
    beam_scores = _flat(beam_scores[:, :num_return_sequences])
    beam_indices = _flat(beam_indices[:, :num_return_sequences, :])
    generated = int(((beam_indices + 1).bool()).sum(dim=1).max())
    return sequences[:, : prompt_len + generated], beam_scores
