"""The prompt pass's attention with leading pads: kivi_prefill_attention behind `attention()`, the torch
restatement of the same contract for what the kernel does not serve, and `PromptLead`, the small object that stands in for the
(B, 1, T, T) additive mask of a left-padded prompt pass on its way from the model to the attention modules.

The contract, for batch row b with lead[b] leading pads (0 without `lead`): a query i >= lead[b] attends to the keys [lead[b], i],
a query under the lead is a pad and its output is exactly zero.  Query head h reads kv head h // (nh // nh_kv)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib

RATIOS = (1, 2, 4, 8)        # nh / nh_kv of the kernel (include/kivi_hip.h)


class PromptLead:
    """What a left-padded prompt pass hands its attention modules in place of the additive mask: `lead` (B,) int32 on the mask's
    device, the number of leading pads of every row, T - mask.sum(-1) -- derived on the device, never read on the host."""

    def __init__(self, mask2d: torch.Tensor):
        self.lead = (mask2d.shape[1] - (mask2d != 0).sum(-1)).to(torch.int32)


def left_padded(mask2d: torch.Tensor) -> torch.Tensor:
    """0-dim bool tensor: every row of the 2D mask is zeros, then ones (no host synchronisation here)."""
    real = mask2d != 0
    return (real[:, 1:] | ~real[:, :-1]).all()


def _rows16(x: torch.Tensor) -> torch.Tensor:
    ok = x.stride(3) == 1 and x.data_ptr() % 16 == 0 and all(x.stride(d) % 8 == 0 for d in range(3))
    return x if ok else x.contiguous()


def kernel_serves(q: torch.Tensor, k: torch.Tensor) -> bool:
    return (q.is_cuda and q.dtype == torch.float16 and k.dtype == torch.float16 and q.shape[-1] == 128
            and q.shape[1] % k.shape[1] == 0 and q.shape[1] // k.shape[1] in RATIOS)


def attention_kernel(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, lead: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kivi_prefill_attention on GPU fp16 tensors: q (B, nh, T, 128), k / v (B, nh_kv, T, 128) with unit channel stride (transposed
    views of (B, T, heads, D) go in without a copy), `lead` (B,) int32 on the device or None.  -> (B, nh, T, 128) fp16, a transposed
    view of a new (B, T, nh, 128) buffer (the transpose before o_proj is then free), or `out` (any strides with unit channel stride,
    16-byte aligned rows)."""
    lib = _lib.load()
    for name, t in (("q", q), ("k", k), ("v", v)):
        _lib.require_gpu(t, name)
        if t.dtype != torch.float16 or t.dim() != 4:
            raise ValueError(f"prefill attention: {name} has to be a 4-D fp16 tensor, got {tuple(t.shape)} {t.dtype}")
    B, nh, T, D = q.shape
    nh_kv = k.shape[1]
    if k.shape != (B, nh_kv, T, D) or v.shape != k.shape:
        raise ValueError(f"prefill attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not belong together")
    if lead is not None:
        _lib.require_gpu(lead, "lead")
        if lead.dtype != torch.int32 or tuple(lead.shape) != (B,) or not lead.is_contiguous():
            raise ValueError(f"prefill attention: lead has to be a contiguous (B,) = ({B},) int32 tensor, got {tuple(lead.shape)} {lead.dtype}")
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    if out is None:
        out = torch.empty((B, T, nh, D), dtype=torch.float16, device=q.device).transpose(1, 2)
    elif out.shape != q.shape or out.dtype != torch.float16 or not out.is_cuda:
        raise ValueError(f"prefill attention: out has to be a GPU fp16 tensor of shape {tuple(q.shape)}")
    _lib.check(lib.kivi_prefill_attention(
        _lib.ptr(q), q.stride(0), q.stride(1), q.stride(2), _lib.ptr(k), k.stride(0), k.stride(1), k.stride(2),
        _lib.ptr(v), v.stride(0), v.stride(1), v.stride(2), _lib.ptr(out), out.stride(0), out.stride(1), out.stride(2),
        None if lead is None else _lib.ptr(lead), B, nh, nh_kv, T, D, 1.0 / math.sqrt(D) if scale is None else float(scale),
        _lib.stream_ptr(q)), "kivi_prefill_attention")
    return out


def attention_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, lead: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same contract in torch (CPU tensors, head dims and ratios the kernel does not serve): SDPA over the live key range of
    every row, the pad rows zeroed.  Without `lead` it is the causal call of the unpadded prompt pass."""
    B, nh, T, _ = q.shape
    rep = nh // k.shape[1]
    if rep > 1:
        k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    if lead is None:
        return F.scaled_dot_product_attention(q, k, v, is_causal=True)
    pos = torch.arange(T, device=q.device)
    lead = lead.to(q.device).clamp(0, T).long()[:, None]                          # (B, 1)
    live = pos[None] >= lead                                                      # (B, T): not a pad
    allowed = (pos[None, :, None] >= pos[None, None, :]) & live[:, None, :]       # (B, T query, T key): lead <= j <= i
    allowed |= torch.eye(T, dtype=torch.bool, device=q.device)[None] & ~live[:, :, None]   # a pad row sees itself: no empty softmax
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=allowed[:, None])
    return out * live[:, None, :, None].to(out.dtype)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, lead: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal grouped-query attention of a prompt over itself with `lead` leading pads per row: the kernel where it serves the
    tensors (GPU, fp16, head_dim 128, nh / nh_kv in RATIOS), the torch restatement otherwise."""
    return attention_kernel(q, k, v, lead) if kernel_serves(q, k) else attention_torch(q, k, v, lead)
