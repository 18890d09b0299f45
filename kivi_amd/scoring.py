"""Log-probabilities of given tokens with the fused HIP kernel kivi_token_logprob (log-softmax + gather).

`token_logprobs(logits, targets)` is what teacher-forced scoring, perplexity and the log-probabilities of generated tokens are made
of (LlamaForCausalLM_KIVI.score / perplexity / generate(return_logprobs=True)).  The contract per row, with t the row's target and
x_j = float(logit j): m = max x; S = sum_j floor(exp(x_j - m) * 2^40), an integer sum of the weights kivi_sample draws from, so the
same row gives the same bits on every run and in every memory layout; lse = m + log(S * 2^-40); logprob = x_t - lse; rank = the
number of j with x_j > x_t, or x_j == x_t and j < t (0 exactly when argmax of the row is t).  t == ignore_index: logprob 0, rank -1.

`top_logprobs(logits, k[, targets])` adds the k most likely tokens of each row with their log-probabilities, in the order the rank
counts in, from one launch of kivi_token_top_logprobs; with targets its target_logprob / lse / rank hold the
bits token_logprobs gives.

`picked_scores(logits, tokens, k)` chooses between the two for the tokens a decode loop has just picked (generation.decode_loop,
graph.generate_graphed, serving.generate_continuous); `score_into` is the same launch into the static buffers of a captured step.
`score(model, ...)` / `perplexity(model, ...)`: teacher-forced scoring over a model, behind the model's
methods of those names -- `score_plan` cuts the tokens into passes, `head_logprobs` runs the head on slabs of model._HEAD_SLAB rows.

`reference_token_logprobs` / `reference_top_logprobs` restate the contracts in fp64 on the CPU for tests and tools; the product
path never calls them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from .generation import PADS_LEFT, _PaddedBatch
from .prefill import left_padded


def _row_stride(logits: torch.Tensor):
    """The element stride between consecutive rows when the leading dimensions of (..., V) collapse to one, else None."""
    stride = None
    for size, st in zip(reversed(logits.shape[:-1]), reversed(logits.stride()[:-1])):
        if size == 1:
            continue
        if stride is None:
            stride, span = st, st * size
        elif st == span:
            span = st * size
        else:
            return None
    return logits.shape[-1] if stride is None else stride


def token_logprobs(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100, return_lse: bool = False,
                   return_rank: bool = False):
    """log p(targets) under softmax(logits): logits (..., V) fp16 / bf16 / fp32 on the GPU, targets int64 of the leading shape -> fp32 of
    the leading shape [, lse fp32] [, rank int32].  The last dimension must be contiguous; leading dimensions are taken by stride
    when they collapse to one row stride ((B, T, V)[:, a:b] with B == 1, padded-vocabulary buffers, (B, 1, V) views) and copied
    otherwise.  Targets outside [0, V) other than `ignore_index` give NaN (the kernel cannot raise): validate token ids first."""
    _lib.require_gpu(logits, "logits")
    _lib.require_gpu(targets, "targets")
    if logits.dim() < 1 or logits.dtype not in _lib.LOGITS_BITS:
        raise ValueError(f"logits must be (..., V) fp16 / bf16 / fp32, got {tuple(logits.shape)} {logits.dtype}")
    lead, V = logits.shape[:-1], logits.shape[-1]
    if targets.dtype != torch.int64 or targets.shape != lead or targets.device != logits.device:
        raise ValueError(f"targets must be int64 of shape {tuple(lead)} on {logits.device}, got {tuple(targets.shape)} {targets.dtype}")
    if logits.stride(-1) != 1 and V > 1:
        raise ValueError("the vocabulary (last) dimension of logits must be contiguous")
    N = targets.numel()
    out = torch.empty(lead, dtype=torch.float32, device=logits.device)
    lse = torch.empty(lead, dtype=torch.float32, device=logits.device) if return_lse else None
    rank = torch.empty(lead, dtype=torch.int32, device=logits.device) if return_rank else None
    if N:
        stride = _row_stride(logits)
        if stride is None or stride < V:
            logits, stride = logits.contiguous(), V
        targets = targets.contiguous()
        _lib.check(_lib.load().kivi_token_logprob(_lib.ptr(logits), _lib.LOGITS_BITS[logits.dtype], stride, N, V,
                                                  _lib.ptr(targets), 1, ignore_index, _lib.ptr(out),
                                                  None if lse is None else _lib.ptr(lse), None if rank is None else _lib.ptr(rank),
                                                  _lib.stream_ptr(logits)),
                   "kivi_token_logprob")
    res = (out,) + ((lse,) if return_lse else ()) + ((rank,) if return_rank else ())
    return res[0] if len(res) == 1 else res


TOP_LOGPROBS_MAX = 32                                 # KIVI_TOP_LOGPROBS_MAX of include/kivi_hip.h


class TopLogprobs(NamedTuple):
    ids: torch.Tensor                                 # int64 (..., k): the tokens of rank 0 .. k - 1
    logprobs: torch.Tensor                            # fp32 (..., k): their log-probabilities
    target_logprob: Optional[torch.Tensor]            # fp32 (...), with targets
    lse: Optional[torch.Tensor]                       # fp32 (...), with return_lse
    rank: Optional[torch.Tensor]                      # int32 (...), with return_rank


def check_top_k(k: int, V: int, what: str = "k") -> None:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(V, TOP_LOGPROBS_MAX):
        raise ValueError(f"{what}={k!r} must be an integer in [1, min(V, {TOP_LOGPROBS_MAX})] (V={V})")


def check_top_logprobs(k, return_logprobs: bool, num_beams: int, V: int) -> None:
    """The `top_logprobs=k` argument of a generate call (0: off): ValueError before any device work."""
    if isinstance(k, int) and not isinstance(k, bool) and k == 0:
        return
    if not return_logprobs:
        raise ValueError("top_logprobs needs return_logprobs=True")
    if num_beams != 1:
        raise ValueError(f"top_logprobs with beam search (num_beams={num_beams}) is not supported")
    check_top_k(k, V, "top_logprobs")


def top_logprobs(logits: torch.Tensor, k: int, targets: Optional[torch.Tensor] = None, ignore_index: int = -100,
                 return_lse: bool = False, return_rank: bool = False) -> TopLogprobs:
    """The k most likely tokens of every row of logits (..., V) with their log-probabilities, by kivi_token_top_logprobs (DESIGN.md
    section 23): rank i is the i-th token in the order "larger logit first, ties by ascending index".  With `targets` (int64 of the
    leading shape) the same launch also gives what token_logprobs gives, in the same bits.  Strides as in token_logprobs."""
    V = logits.shape[-1] if logits.dim() >= 1 else 0
    check_top_k(k, V)
    if return_rank and targets is None:
        raise ValueError("return_rank needs targets")
    _lib.require_gpu(logits, "logits")
    if targets is not None:
        _lib.require_gpu(targets, "targets")
    if logits.dtype not in _lib.LOGITS_BITS:
        raise ValueError(f"logits must be (..., V) fp16 / bf16 / fp32, got {tuple(logits.shape)} {logits.dtype}")
    lead = logits.shape[:-1]
    if targets is not None and (targets.dtype != torch.int64 or targets.shape != lead or targets.device != logits.device):
        raise ValueError(f"targets must be int64 of shape {tuple(lead)} on {logits.device}, got {tuple(targets.shape)} {targets.dtype}")
    if logits.stride(-1) != 1 and V > 1:
        raise ValueError("the vocabulary (last) dimension of logits must be contiguous")
    dev = logits.device
    ids = torch.empty(lead + (k,), dtype=torch.int64, device=dev)
    top = torch.empty(lead + (k,), dtype=torch.float32, device=dev)
    out = torch.empty(lead, dtype=torch.float32, device=dev) if targets is not None else None
    lse = torch.empty(lead, dtype=torch.float32, device=dev) if return_lse else None
    rank = torch.empty(lead, dtype=torch.int32, device=dev) if return_rank else None
    N = ids.numel() // k
    if N:
        stride = _row_stride(logits)
        if stride is None or stride < V:
            logits, stride = logits.contiguous(), V
        if targets is not None:
            targets = targets.contiguous()
        opt = lambda t: None if t is None else _lib.ptr(t)   # noqa: E731
        _lib.check(_lib.load().kivi_token_top_logprobs(_lib.ptr(logits), _lib.LOGITS_BITS[logits.dtype], stride, N, V, k,
                                                       opt(targets), 1, ignore_index, _lib.ptr(ids), _lib.ptr(top), k, opt(out),
                                                       opt(lse), opt(rank), _lib.stream_ptr(logits)),
                   "kivi_token_top_logprobs")
    return TopLogprobs(ids, top, out, lse, rank)


def score_into(logits: torch.Tensor, tokens: torch.Tensor, lp: torch.Tensor, top_ids: Optional[torch.Tensor] = None,
               top_lp: Optional[torch.Tensor] = None) -> None:
    """One launch into the caller's buffers, nothing allocated (a captured decode step, kivi_amd/graph.py): log p(tokens) under
    contiguous logits (B, 1, V) into lp (B, 1) fp32 by kivi_token_logprob, or, with top_ids / top_lp (B, 1, k), by
    kivi_token_top_logprobs together with the lists -- the bits token_logprobs / top_logprobs give."""
    B, V = tokens.numel(), logits.shape[-1]
    assert logits.is_contiguous() and tokens.is_contiguous() and lp.is_contiguous() and logits.numel() == B * V
    bits, lib = _lib.LOGITS_BITS[logits.dtype], _lib.load()
    if top_ids is None:
        _lib.check(lib.kivi_token_logprob(_lib.ptr(logits), bits, V, B, V, _lib.ptr(tokens), 1, -100, _lib.ptr(lp), None, None,
                                          _lib.stream_ptr(logits)), "kivi_token_logprob")
    else:
        k = top_ids.shape[-1]
        assert top_ids.is_contiguous() and top_lp.is_contiguous() and top_lp.shape[-1] == k
        _lib.check(lib.kivi_token_top_logprobs(_lib.ptr(logits), bits, V, B, V, k, _lib.ptr(tokens), 1, -100, _lib.ptr(top_ids),
                                               _lib.ptr(top_lp), k, _lib.ptr(lp), None, None, _lib.stream_ptr(logits)),
                   "kivi_token_top_logprobs")


def picked_scores(logits: torch.Tensor, tokens: torch.Tensor, k: Optional[int]) -> tuple:
    """The scores of the tokens just picked, `tokens` (B, 1), under the logits in hand (B, 1, V): () for k None (nothing is asked
    for), (logprob (B, 1),) for k == 0 from one kivi_token_logprob launch, (logprob, top_ids (B, 1, k), top_logprobs (B, 1, k)) for
    k > 0 from one kivi_token_top_logprobs launch.  A token of -100 (a row with nothing to score) gets logprob 0."""
    if k is None:
        return ()
    if not k:
        return (token_logprobs(logits, tokens),)
    res = top_logprobs(logits, k, tokens)
    return res.target_logprob, res.ids, res.logprobs


# ------------------------------------------------------------------ scoring a model's given tokens
def score_plan(input_ids: torch.Tensor, first_chunk: Optional[int], chunk_size: Optional[int]):
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


def head_logprobs(model, x, targets, return_rank, top_k: int = 0):
    """token_logprobs of `targets` (B, q) under lm_head(norm(x)), x (B, q, H): the head runs on slabs of at most model._HEAD_SLAB
    rows (one slab: the very call forward() makes), so logits never exist for more rows than that.  -> (logprobs, ranks or None,
    top ids or None, top log-probabilities or None); `top_k` > 0: one kivi_token_top_logprobs launch per slab in place of the
    kivi_token_logprob launch, with the lists (B, q, top_k) of every row."""
    def head(hs, ts):
        if top_k:
            r = top_logprobs(model.lm_head(hs), top_k, ts, return_rank=return_rank)
            return r.target_logprob, r.rank, r.ids, r.logprobs
        r = token_logprobs(model.lm_head(hs), ts, return_rank=return_rank)
        return (r + (None, None)) if return_rank else (r, None, None, None)

    h = model.model.norm(x)
    B, q = targets.shape
    slab = model._HEAD_SLAB
    if B * q <= slab:
        return head(h, targets)
    h, t = h.reshape(B * q, -1), targets.reshape(-1)
    slabs = [head(h[s:s + slab], t[s:s + slab]) for s in range(0, B * q, slab)]
    return tuple(None if p[0] is None else torch.cat(p).view((B, q) + p[0].shape[1:]) for p in zip(*slabs))


@torch.no_grad()
def score(model, input_ids, attention_mask, past_key_values, first_chunk, chunk_size, return_rank, top_k):
    """LlamaForCausalLM_KIVI.score (its docstring is the reference; `top_k` is its `top_logprobs`)."""
    plan = score_plan(input_ids, first_chunk, chunk_size)
    k, vocab = top_k, model.config.vocab_size
    if k != 0:
        check_top_k(k, vocab, "top_logprobs")
    B, T = input_ids.shape
    facts = list(torch.aminmax(input_ids))
    past_len = model._past_len(past_key_values)
    if attention_mask is not None:
        facts.append((attention_mask == 0).any().to(input_ids.device, torch.long))
        if past_len == 0 and getattr(model.config, "kivi_prefill_kernel", False):
            facts.append(left_padded(attention_mask).to(input_ids.device, torch.long))
    lo, hi, *has_pad = (int(v) for v in torch.stack(facts).tolist())        # the one synchronisation of the call
    if lo < 0 or hi >= vocab:
        raise ValueError(f"input_ids hold token ids in [{lo}, {hi}], outside the vocabulary [0, {vocab})")
    valid = torch.ones((B, T - 1), dtype=torch.bool, device=input_ids.device)
    padded = attention_mask is not None and model._padded(attention_mask, B, past_len + T, past_len, bool(has_pad[0]),
                                                          bool(has_pad[1]) if len(has_pad) > 1 else None)
    if padded:
        real = attention_mask[:, past_len:] != 0
        valid = real[:, 1:] & real[:, :-1]
    targets = torch.full((B, T), -100, dtype=torch.long, device=input_ids.device)     # the last token has nothing to predict
    targets[:, :-1] = torch.where(valid, input_ids[:, 1:], targets[:, :-1])
    pasts, passes = past_key_values, []
    for a, b in plan:
        if padded:
            pb = _PaddedBatch(attention_mask[:, : past_len + b], past_len + a, b - a, lead=padded == PADS_LEFT)
            x, pasts = model._hidden(input_ids[:, a:b], pasts, pb.mask, pb.position_ids, True)
        else:
            x, pasts = model._hidden(input_ids[:, a:b], pasts, None, None, False)
        passes.append(head_logprobs(model, x, targets[:, a:b], return_rank, k))
    lp, rk, ti, tl = (None if p[0] is None else torch.cat(p, dim=1)[:, :-1] for p in zip(*passes))
    res = (lp, valid, pasts) + ((rk,) if return_rank else ())
    if k:
        res += (ti.masked_fill(~valid.unsqueeze(-1), -1), tl.masked_fill(~valid.unsqueeze(-1), 0.0))
    return res


@torch.no_grad()
def perplexity(model, input_ids, attention_mask, past_key_values, first_chunk, chunk_size):
    """LlamaForCausalLM_KIVI.perplexity: exp(-mean valid log-probability) of model.score() with the same arguments, sums in fp64."""
    lp, valid, _ = model.score(input_ids, attention_mask, past_key_values, first_chunk, chunk_size)
    s, n = lp.double().sum(-1), valid.sum(-1).double()              # invalid entries are exactly 0
    return torch.exp(-s / n), torch.exp(-s.sum() / n.sum())


# ------------------------------------------------------------------ CPU restatement (tests, tools)
def reference_top_logprobs(logits: torch.Tensor, k: int):
    """fp64 CPU restatement of the lists of kivi_token_top_logprobs: (ids int64 (..., k), logprobs float64 (..., k)).  A stable
    descending sort keeps equal values (-0 == +0 among them) in ascending index."""
    x = logits.detach().cpu().double()
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[..., :k]
    return order, x.gather(-1, order) - torch.logsumexp(x, -1, keepdim=True)


def reference_token_logprobs(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100):
    """fp64 CPU restatement of kivi_token_logprob: (logprob, lse) float64 and rank int64 of the leading shape."""
    x = logits.detach().cpu().double()
    t = targets.detach().cpu().long()
    V = x.shape[-1]
    lse = torch.logsumexp(x, -1)
    ignored = t == ignore_index
    scored = ~ignored & (t >= 0) & (t < V)
    ts = torch.where(scored, t, torch.zeros_like(t)).unsqueeze(-1)
    xt = x.gather(-1, ts)
    lp = xt.squeeze(-1) - lse
    j = torch.arange(V).expand(x.shape)
    rank = ((x > xt) | ((x == xt) & (j < ts))).sum(-1)
    lp = torch.where(scored, lp, torch.full_like(lp, float("nan")))
    lp = torch.where(ignored, torch.zeros_like(lp), lp)
    return lp, lse, torch.where(scored, rank, torch.full_like(rank, -1))
