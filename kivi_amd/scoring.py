"""Log-probabilities of given tokens with the fused HIP kernel kivi_token_logprob (log-softmax + gather).

`token_logprobs(logits, targets)` is what teacher-forced scoring, perplexity and the log-probabilities of generated tokens are made
of (LlamaForCausalLM_KIVI.score / perplexity / generate(return_logprobs=True)).  The contract per row, with t the row's target and
x_j = float(logit j): m = max x; S = sum_j floor(exp(x_j - m) * 2^40), an integer sum of the weights kivi_sample draws from, so the
same row gives the same bits on every run and in every memory layout; lse = m + log(S * 2^-40); logprob = x_t - lse; rank = the
number of j with x_j > x_t, or x_j == x_t and j < t (0 exactly when argmax of the row is t).  t == ignore_index: logprob 0, rank -1.

`reference_token_logprobs` restates the contract in fp64 on the CPU for tests and tools; the product path never calls it.
"""
from __future__ import annotations

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
    """log p(targets) under softmax(logits): logits (..., V) fp16 / fp32 on the GPU, targets int64 of the leading shape -> fp32 of
    the leading shape [, lse fp32] [, rank int32].  The last dimension must be contiguous; leading dimensions are taken by stride
    when they collapse to one row stride ((B, T, V)[:, a:b] with B == 1, padded-vocabulary buffers, (B, 1, V) views) and copied
    otherwise.  Targets outside [0, V) other than `ignore_index` give NaN (the kernel cannot raise): validate token ids first."""
    _lib.require_gpu(logits, "logits")
    _lib.require_gpu(targets, "targets")
    if logits.dim() < 1 or logits.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"logits must be (..., V) fp16 / fp32, got {tuple(logits.shape)} {logits.dtype}")
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
        _lib.check(_lib.load().kivi_token_logprob(_lib.ptr(logits), 16 if logits.dtype == torch.float16 else 32, stride, N, V,
                                                  _lib.ptr(targets), 1, ignore_index, _lib.ptr(out),
                                                  None if lse is None else _lib.ptr(lse), None if rank is None else _lib.ptr(rank),
                                                  _lib.stream_ptr(logits)),
                   "kivi_token_logprob")
    res = (out,) + ((lse,) if return_lse else ()) + ((rank,) if return_rank else ())
    return res[0] if len(res) == 1 else res


# ------------------------------------------------------------------ CPU restatement (tests, tools)
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
