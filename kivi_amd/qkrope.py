"""q and k of a layer made ready for the attention: the per-head RMSNorm of Qwen3, the rotary embedding, and the
placement into (B, heads, Q, D) with every group of query heads padded to a ratio the matrix-pipe layout serves -- one launch of
kivi_qk_rope (kivi_amd/csrc/kivi_qkrope.hip) in place of the chain of torch elementwise launches, and the torch statement of the
same arithmetic for what the kernel does not cover (head_dim != 128, tensors off the GPU).

Further down: the way into the fp16 attention for a model whose dense layers run in bf16 -- one launch of
kivi_qkv_rope_bf16 takes bf16 q / k / v projections and fp32 cos / sin tables to fp16 q, k and v with a single rounding -- and
the torch statement of that contract."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

HEAD_DIM = 128      # the kernel's head size: the matrix-pipe layout's


def head_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """HF's Qwen3RMSNorm over the last dimension: fp32 mean of squares, the normalised values rounded to x's dtype, then the weight."""
    x32 = x.float()
    var = x32.pow(2).mean(-1, keepdim=True)
    return weight * (x32 * torch.rsqrt(var + eps)).to(x.dtype)


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def usable(x: torch.Tensor, head_dim: int) -> bool:
    """True where kivi_qk_rope serves: fp16 on the GPU at head size 128."""
    return x.is_cuda and x.dtype == torch.float16 and head_dim == HEAD_DIM


def qk_rope_torch(q_in: torch.Tensor, k_in: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                  q_weight: Optional[torch.Tensor] = None, k_weight: Optional[torch.Tensor] = None, eps: float = 0.0
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The torch path: q_in (B, Q, nh, D), k_in (B, Q, nh_kv, D), cos / sin (Bc, Q, D) -> q (B, nh, Q, D), k (B, nh_kv, Q, D) (views;
    no padding)."""
    if q_weight is not None:
        q_in, k_in = head_norm(q_in, q_weight, eps), head_norm(k_in, k_weight, eps)
    q, k = q_in.transpose(1, 2), k_in.transpose(1, 2)
    cos, sin = cos[:, None], sin[:, None]
    return q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin


def qk_rope(q_in: torch.Tensor, k_in: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, ratio_padded: Optional[int] = None,
            q_weight: Optional[torch.Tensor] = None, k_weight: Optional[torch.Tensor] = None, eps: float = 0.0,
            q_out: Optional[torch.Tensor] = None, k_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One kivi_qk_rope launch.  q_in (B, Q, nh, D), k_in (B, Q, nh_kv, D) fp16 with unit channel stride (views of the projections'
    outputs are read as they are); cos / sin (Bc, Q, D) fp16, Bc in {1, B}; `ratio_padded`: Rp >= nh / nh_kv (None: no padding).
    -> q (B, nh_kv * Rp, Q, D) with query head kv * R + r at kv * Rp + r and exact zeros in the pad heads, k (B, nh_kv, Q, D);
    `q_out` / `k_out`: contiguous buffers of those shapes to write into (the static buffers of a captured step)."""
    B, Q, nh, D = q_in.shape
    nh_kv = k_in.shape[2]
    for t, name in ((q_in, "q_in"), (k_in, "k_in"), (cos, "cos"), (sin, "sin")):
        _lib.require_gpu(t, name)
        if t.dtype != torch.float16 or t.stride(-1) != 1:
            raise ValueError(f"kivi_qk_rope: {name} must be fp16 with unit channel stride, got {t.dtype}, strides {t.stride()}")
    if tuple(k_in.shape) != (B, Q, nh_kv, D) or nh % nh_kv:
        raise ValueError(f"kivi_qk_rope: q_in {tuple(q_in.shape)} and k_in {tuple(k_in.shape)} do not go together")
    if cos.shape != sin.shape or cos.stride() != sin.stride() or cos.dim() != 3 or cos.shape[0] not in (1, B) \
            or tuple(cos.shape[1:]) != (Q, D):
        raise ValueError(f"kivi_qk_rope: cos / sin must be two (1 or {B}, {Q}, {D}) tables of one layout, got {tuple(cos.shape)}, "
                         f"{tuple(sin.shape)}")
    if (q_weight is None) != (k_weight is None):
        raise ValueError("kivi_qk_rope: the head norm takes both weights or none")
    for w in (q_weight, k_weight):
        if w is not None and not (w.is_cuda and w.dtype == torch.float16 and tuple(w.shape) == (D,) and w.is_contiguous()):
            raise ValueError(f"kivi_qk_rope: a head-norm weight is ({D},) fp16 on the GPU")
    rp = nh // nh_kv if ratio_padded is None else int(ratio_padded)
    shapes = ((B, nh_kv * rp, Q, D), (B, nh_kv, Q, D))
    outs = []
    for buf, shape in zip((q_out, k_out), shapes):
        if buf is None:
            buf = torch.empty(shape, dtype=torch.float16, device=q_in.device)
        elif tuple(buf.shape) != shape or buf.dtype != torch.float16 or not buf.is_contiguous() or not buf.is_cuda:
            raise ValueError(f"kivi_qk_rope: an output buffer must be contiguous fp16 {shape} on the GPU")
        outs.append(buf)
    rc = _lib.load().kivi_qk_rope(
        q_in.data_ptr(), q_in.stride(0), q_in.stride(1), q_in.stride(2), k_in.data_ptr(), k_in.stride(0), k_in.stride(1),
        k_in.stride(2), cos.data_ptr(), sin.data_ptr(), cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1),
        None if q_weight is None else q_weight.data_ptr(), None if k_weight is None else k_weight.data_ptr(), float(eps),
        outs[0].data_ptr(), outs[1].data_ptr(), B, Q, nh, nh_kv, rp, D, _lib.stream_ptr(q_in))
    _lib.check(rc, "kivi_qk_rope")
    return outs[0], outs[1]


def unpad(attn: torch.Tensor, num_kv_heads: int, ratio: int, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """(B, nh_kv * Rp, Q, D) attention output -> (B, Q, nh_kv * ratio * D), the pad heads cut off: a view until the reshape that feeds
    o_proj, which is the one copy the unpadded path makes there too.  `dtype`: that copy casts as well."""
    B, nhp, Q, D = attn.shape
    v = attn.view(B, num_kv_heads, nhp // num_kv_heads, Q, D)[:, :, :ratio].permute(0, 3, 1, 2, 4)
    if dtype is not None and dtype != attn.dtype:
        return v.to(dtype, memory_format=torch.contiguous_format).view(B, Q, num_kv_heads * ratio * D)
    return v.reshape(B, Q, num_kv_heads * ratio * D)


# ---------------------------------------------------------------------------------------------------------------------------------
# The boundary of a model whose dense layers are not fp16: bf16 (or fp32) projections in, fp16 q / k / v out.
F16_MAX = 65504.0


def round_once_f16(d: torch.Tensor) -> torch.Tensor:
    """fp64 -> fp16 with ONE rounding (to nearest even), a finite value that would become an infinity stored as +-65504, NaN kept.
    Through the fp32 value of the same sign that is truncated and carries a sticky last bit (round to odd), which rounds to the fp16
    the fp64 value rounds to -- torch's own fp64 -> fp16 cast may go through fp32 rounded to nearest, two roundings."""
    f = d.float()
    bits = f.view(torch.int32) - (f.double().abs() > d.abs()).int()         # towards zero: one step back where the cast rounded away
    f = bits.view(torch.float32)
    f = (bits | (f.double() != d).int()).view(torch.float32)                # sticky (a NaN compares unequal and stays a NaN)
    f = torch.where(torch.isfinite(d), f.clamp(-F16_MAX, F16_MAX), f)
    return f.half()


def qkv_rope_bf16_torch(q_in: torch.Tensor, k_in: torch.Tensor, v_in: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                        q_weight: Optional[torch.Tensor] = None, k_weight: Optional[torch.Tensor] = None, eps: float = 0.0
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The contract of kivi_qkv_rope_bf16 in torch, for what the kernel does not cover (tensors off the GPU, head_dim != 128, fp32
    models -- the dense reference of the tests): q_in (B, Q, nh, D), k_in / v_in (B, Q, nh_kv, D) bf16 or fp32, cos / sin (Bc, Q, D)
    -> q (B, nh, Q, D), k, v (B, nh_kv, Q, D) fp16 (no padding).  Every input is the exact number it holds; with weights
    y = (w * x) * (1 / sqrt(sum(x^2) / D + eps)), eps as fp32; out = y * cos + rot(y) * sin; each operation is one fp64 operation
    in the order written, and the result is rounded once (round_once_f16).  v is rounded the same way."""
    def prep(x, w):
        x = x.double()
        if w is not None:
            e = torch.tensor(float(eps), dtype=torch.float32).double().item()
            rs = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[-1] + e)
            x = (w.double() * x) * rs
        x = x.transpose(1, 2)
        return round_once_f16(x * cos.double()[:, None] + rotate_half(x) * sin.double()[:, None])
    if (q_weight is None) != (k_weight is None):
        raise ValueError("kivi_qkv_rope_bf16: the head norm takes both weights or none")
    return prep(q_in, q_weight), prep(k_in, k_weight), round_once_f16(v_in.double().transpose(1, 2))


def pad_groups(q: torch.Tensor, num_kv_heads: int, ratio_padded: int) -> torch.Tensor:
    """(B, nh_kv * R, Q, D) -> (B, nh_kv * Rp, Q, D), query head kv * R + r at kv * Rp + r and zeros in the pad heads: the layout
    the kernels write, by a copy, for the torch path."""
    B, nh, Q, D = q.shape
    out = q.new_zeros((B, num_kv_heads, ratio_padded, Q, D))
    out[:, :, : nh // num_kv_heads] = q.reshape(B, num_kv_heads, nh // num_kv_heads, Q, D)
    return out.view(B, num_kv_heads * ratio_padded, Q, D)


def boundary_usable(x: torch.Tensor, head_dim: int) -> bool:
    """True where kivi_qkv_rope_bf16 serves: bf16 on the GPU at head size 128."""
    return x.is_cuda and x.dtype == torch.bfloat16 and head_dim == HEAD_DIM


def qkv_rope_bf16(q_in: torch.Tensor, k_in: torch.Tensor, v_in: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                  ratio_padded: Optional[int] = None, q_weight: Optional[torch.Tensor] = None,
                  k_weight: Optional[torch.Tensor] = None, eps: float = 0.0, q_out: Optional[torch.Tensor] = None,
                  k_out: Optional[torch.Tensor] = None, v_out: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One kivi_qkv_rope_bf16 launch.  q_in (B, Q, nh, D), k_in / v_in (B, Q, nh_kv, D) bf16 with unit channel stride; cos / sin
    (Bc, Q, D) FP32, Bc in {1, B} (rope_cos_sin(..., dtype=None)); `ratio_padded` as in qk_rope; head-norm weights (D,) bf16.
    -> fp16 q (B, nh_kv * Rp, Q, D) with exact zeros in the pad heads, k and v (B, nh_kv, Q, D); `q_out` / `k_out` / `v_out`:
    contiguous buffers of those shapes to write into."""
    if q_in.dim() != 4:
        raise ValueError(f"kivi_qkv_rope_bf16: q_in must be (B, Q, nh, D), got {tuple(q_in.shape)}")
    B, Q, nh, D = q_in.shape
    nh_kv = k_in.shape[2] if k_in.dim() == 4 else 0
    for t, name, dt in ((q_in, "q_in", torch.bfloat16), (k_in, "k_in", torch.bfloat16), (v_in, "v_in", torch.bfloat16),
                        (cos, "cos", torch.float32), (sin, "sin", torch.float32)):
        if t.dtype != dt or t.stride(-1) != 1:
            raise ValueError(f"kivi_qkv_rope_bf16: {name} must be {dt} with unit channel stride, got {t.dtype}, strides {t.stride()}")
    if nh_kv < 1 or tuple(k_in.shape) != (B, Q, nh_kv, D) or tuple(v_in.shape) != (B, Q, nh_kv, D) or nh % nh_kv:
        raise ValueError(f"kivi_qkv_rope_bf16: q_in {tuple(q_in.shape)}, k_in {tuple(k_in.shape)} and v_in {tuple(v_in.shape)} do not "
                         f"go together")
    if cos.shape != sin.shape or cos.stride() != sin.stride() or cos.dim() != 3 or cos.shape[0] not in (1, B) \
            or tuple(cos.shape[1:]) != (Q, D):
        raise ValueError(f"kivi_qkv_rope_bf16: cos / sin must be two (1 or {B}, {Q}, {D}) tables of one layout, got "
                         f"{tuple(cos.shape)}, {tuple(sin.shape)}")
    if (q_weight is None) != (k_weight is None):
        raise ValueError("kivi_qkv_rope_bf16: the head norm takes both weights or none")
    for w in (q_weight, k_weight):
        if w is not None and not (w.dtype == torch.bfloat16 and tuple(w.shape) == (D,) and w.is_contiguous()):
            raise ValueError(f"kivi_qkv_rope_bf16: a head-norm weight is ({D},) bf16")
    rp = nh // nh_kv if ratio_padded is None else int(ratio_padded)
    for t, name in ((q_in, "q_in"), (k_in, "k_in"), (v_in, "v_in"), (cos, "cos"), (sin, "sin"), (q_weight, "q_weight"),
                    (k_weight, "k_weight")):
        if t is not None:
            _lib.require_gpu(t, name)
    shapes = ((B, nh_kv * rp, Q, D), (B, nh_kv, Q, D), (B, nh_kv, Q, D))
    outs = []
    for buf, shape in zip((q_out, k_out, v_out), shapes):
        if buf is None:
            buf = torch.empty(shape, dtype=torch.float16, device=q_in.device)
        elif tuple(buf.shape) != shape or buf.dtype != torch.float16 or not buf.is_contiguous() or not buf.is_cuda:
            raise ValueError(f"kivi_qkv_rope_bf16: an output buffer must be contiguous fp16 {shape} on the GPU")
        outs.append(buf)
    rc = _lib.load().kivi_qkv_rope_bf16(
        q_in.data_ptr(), q_in.stride(0), q_in.stride(1), q_in.stride(2), k_in.data_ptr(), k_in.stride(0), k_in.stride(1),
        k_in.stride(2), v_in.data_ptr(), v_in.stride(0), v_in.stride(1), v_in.stride(2), cos.data_ptr(), sin.data_ptr(),
        cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1), None if q_weight is None else q_weight.data_ptr(),
        None if k_weight is None else k_weight.data_ptr(), float(eps), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
        B, Q, nh, nh_kv, rp, D, _lib.stream_ptr(q_in))
    _lib.check(rc, "kivi_qkv_rope_bf16")
    return outs[0], outs[1], outs[2]
