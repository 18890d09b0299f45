"""Log-probabilities of given tokens with the fused HIP kernel kivi_token_logprob (log-softmax + gather).

`token_logprobs(logits, targets)` is what teacher-forced scoring, perplexity and the log-probabilities of generated tokens are made
of (LlamaForCausalLM_KIVI.score / perplexity / generate(return_logprobs=True)).  The contract per row, with t the row's target and
x_j = float(logit j): m = max x; S = sum_j floor(exp(x_j - m) * 2^40), an integer sum of the weights kivi_sample draws from, so the
same row gives the same bits on every run and in every memory layout; lse = m + log(S * 2^-40); logprob = x_t - lse; rank = the
number of j with x_j > x_t, or x_j == x_t and j < t (0 exactly when argmax of the row is t).  t == ignore_index: logprob 0, rank -1.

`top_logprobs(logits, k[, targets])` adds the k most likely tokens of each row with their log-probabilities, in the order the rank
counts in, from one launch of kivi_token_top_logprobs; with targets its target_logprob / lse / rank hold the
bits token_logprobs gives.

`reference_token_logprobs` / `reference_top_logprobs` restate the contracts in fp64 on the CPU for tests and tools; the product
path never calls them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib


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
