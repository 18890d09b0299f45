"""Weight-only 4-bit dense layers: group-wise asymmetric along the input axis, G in {64, 128}.

The contract (include/kivi_hip.h): for a weight W (O, K) the codes, `scale` and `mn` are exactly what the reference's last-dim
quantiser gives for the fp16 image of W viewed as (1, 1, O, K) at 4 bits -- `quantize_ref` states it in torch --, the represented
weight is the real number code * scale + mn, and a linear is y[n, o] = sum_k x[n, k] * (code * scale + mn)[o, k] (+ bias[o]),
accumulated in fp32 and rounded once to x's dtype.  `pack` / `dequant` / `linear` / `gate_up` are the four HIP entries
(kivi_amd/csrc/kivi_w4.hip): launches only, so a captured decode step may hold them.  `to_ref` / `from_ref` convert between the
device layout ("WT4", kivi_amd/csrc/kivi_mfma_layout.h) and the reference's triple -- (O, K / 8) int32 with element 8 c + i of a row
in bits 4 i of word c, (O, K / G) fp16 scale and mn -- in torch, on any device: the importer's entry point for a quantisation made
elsewhere.  `QuantLinear` / `QuantMLP` are the modules `make_config(..., weight_bits=4)` puts in place of the attention projections
and of the dense MLP."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .lora import active_binding

LAYOUT = "WT4"                  # the tag save_quantized writes and from_pretrained recognises
GROUPS = (64, 128)
ROW_TILE, K_TILE, TILE_WORDS = 16, 128, 256         # kivi_amd/csrc/kivi_w4_plan.h
# Eager calls of more tokens than this dequantise into the shared scratch and run F.linear (rocBLAS); under stream capture the
# kernel always runs.  The largest N at which tools/w4_time.py measured the kernel ahead of dequant + F.linear on EVERY shape
# (profiles/w4_time.log, the line "crossover", MI355X): at 32 it is 1.4-2.7x ahead, at the next measured size, 64, the 4096 -> 1024
# projection is behind (0.85x) while the five larger shapes stay 1.3-1.6x ahead.
KERNEL_MAX_TOKENS = 32
_DTYPES = {torch.float16: 16, torch.bfloat16: _lib.LOGITS_BF16}
_NIBBLE = [(e >> 1) + 4 * (e & 1) for e in range(8)]  # element e of a word's 8 -> its 4-bit field in the WT4 word


def usable(out_features: int, in_features: int, group: int = 128) -> bool:
    """True for the shapes the kernels serve: O a multiple of 16, K a multiple of 128, G in {64, 128}."""
    return (group in GROUPS and out_features >= ROW_TILE and out_features % ROW_TILE == 0 and in_features >= K_TILE
            and in_features % K_TILE == 0)


def shapes(out_features: int, in_features: int, group: int):
    """Shapes of the three buffers: qweight int32, scales and mins int16 (fp16 bit patterns)."""
    if not usable(out_features, in_features, group):
        raise ValueError(f"4-bit weights need out_features a multiple of 16, in_features a multiple of 128 and a group of 64 or 128, got "
                         f"({out_features}, {in_features}), group {group}")
    s = out_features // ROW_TILE
    return (s, in_features // K_TILE, TILE_WORDS), (s, in_features // group, ROW_TILE), (s, in_features // group, ROW_TILE)


# ------------------------------------------------------------------------------------------------ the layout, in torch
def _move_nibbles(words: torch.Tensor, to_wt4: bool) -> torch.Tensor:
    u = words.to(torch.int64) & 0xFFFFFFFF
    out = torch.zeros_like(u)
    for e, p in enumerate(_NIBBLE):
        src, dst = (4 * e, 4 * p) if to_wt4 else (4 * p, 4 * e)
        out |= ((u >> src) & 15) << dst
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


def from_ref(code: torch.Tensor, scale: torch.Tensor, mn: torch.Tensor, group: int):
    """The reference's triple -- code (O, K / 8) int32, scale and mn (O, K / G) fp16 -> (qweight, scales, mins) in WT4."""
    O, K = code.shape[0], code.shape[1] * 8
    qs, ss, _ = shapes(O, K, group)
    if code.dtype != torch.int32 or tuple(scale.shape) != (O, K // group) or tuple(mn.shape) != (O, K // group) \
            or scale.dtype != torch.float16 or mn.dtype != torch.float16:
        raise ValueError("from_ref: code (O, K / 8) int32, scale and mn (O, K / G) fp16")
    # chunk c of row o = 16 * stripe + r: tile c // 16, j = (c % 16) // 4, kb = c % 4 -> word (r + 16 kb) * 4 + j of the tile
    w = _move_nibbles(code, True).view(O // 16, 16, K // 128, 4, 4)           # (stripe, r, tile, j, kb)
    qweight = w.permute(0, 2, 4, 1, 3).reshape(qs).contiguous()               # (stripe, tile, kb, r, j)
    def lay(t):
        return t.contiguous().view(torch.int16).view(O // 16, 16, K // group).permute(0, 2, 1).reshape(ss).contiguous()
    return qweight, lay(scale), lay(mn)


def to_ref(qweight: torch.Tensor, scales: torch.Tensor, mins: torch.Tensor):
    """(qweight, scales, mins) in WT4 -> the reference's triple (code (O, K / 8) int32, scale, mn (O, K / G) fp16)."""
    S, T, _ = qweight.shape
    O, K, ng = S * 16, T * 128, scales.shape[1]
    w = qweight.view(S, T, 4, 16, 4).permute(0, 3, 1, 4, 2).reshape(O, K // 8)   # (stripe, r, tile, j, kb)
    def lay(t):
        return t.view(S, ng, 16).permute(0, 2, 1).reshape(O, ng).contiguous().view(torch.float16)
    return _move_nibbles(w, False), lay(scales), lay(mins)


def quantize_ref(w: torch.Tensor, group: int):
    """The quantiser in torch, statement for statement the reference's (quant/new_pack.py:236-241) on the fp16 image of `w` (O, K),
    evaluated op by op in fp16 as its CUDA run does; a NaN quotient becomes code 0.  -> the reference's triple.  Any device."""
    O, K = w.shape
    h = w.to(torch.float16).reshape(O, K // group, group)
    mn, mx = h.min(dim=-1, keepdim=True).values, h.max(dim=-1, keepdim=True).values
    scale = (mx - mn) / 15
    q = ((h - mn) / scale).float()
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp_(0, 15).round_().to(torch.int64).reshape(O, K // 8, 8)
    code = torch.zeros((O, K // 8), dtype=torch.int64, device=w.device)
    for i in range(8):
        code |= q[:, :, i] << (4 * i)
    code = torch.where(code >= 2 ** 31, code - 2 ** 32, code).to(torch.int32)
    return code, scale.reshape(O, K // group), mn.reshape(O, K // group)


def dequant_torch(qweight: torch.Tensor, scales: torch.Tensor, mins: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """The dense weight of kivi_w4_dequant in torch: round_to_dtype(fma(code, scale, mn)) with the fused multiply-add in fp32 --
    evaluated in fp64, where the product (4 x 11 bits) and the sum are exact, and rounded to fp32 and to the dtype."""
    code, scale, mn = to_ref(qweight, scales, mins)
    O, ng = scale.shape
    K = code.shape[1] * 8
    u = code.to(torch.int64) & 0xFFFFFFFF
    q = torch.stack([(u >> (4 * i)) & 15 for i in range(8)], dim=-1).reshape(O, ng, K // ng).double()
    return (q * scale.double()[:, :, None] + mn.double()[:, :, None]).float().reshape(O, K).to(dtype)


# ------------------------------------------------------------------------------------------------ the four entries
def _check_x(x: torch.Tensor, K: int, what: str) -> torch.Tensor:
    _lib.require_gpu(x, "x")
    if x.dim() != 2 or x.shape[1] != K or x.shape[0] < 1 or x.dtype not in _DTYPES:
        raise ValueError(f"{what}: x must be (N >= 1, {K}) fp16 or bf16, got {tuple(x.shape)} {x.dtype}")
    if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        x = x.contiguous()
    return x


def pack(w: torch.Tensor, group: int = 128, name: str = "weight", out=None):
    """One kivi_w4_pack launch: w (O, K) fp16 or bf16 on the GPU -> (qweight, scales, mins).  A weight whose fp16 image holds an
    infinity is refused, by `name`.  `out`: three contiguous buffers of those shapes and dtypes on w's device to write into (views
    of a larger buffer: a stack of experts is packed slab by slab, kivi_amd/moe.py)."""
    _lib.require_gpu(w, name)
    if w.dim() != 2 or w.dtype not in _DTYPES:
        raise ValueError(f"{name}: a 2-D fp16 or bf16 weight is needed, got {tuple(w.shape)} {w.dtype}")
    O, K = w.shape
    qs, ss, ms = shapes(O, K, group)
    if bool(torch.isinf(w if w.dtype == torch.float16 else w.to(torch.float16)).any()):
        raise ValueError(f"{name}: the fp16 image of the weight holds an infinity; it cannot be quantised to 4 bits")
    if w.stride(1) != 1 or w.stride(0) % 8 or w.data_ptr() % 16:
        w = w.contiguous()
    if out is None:
        qweight = torch.empty(qs, dtype=torch.int32, device=w.device)
        scales = torch.empty(ss, dtype=torch.int16, device=w.device)
        mins = torch.empty(ms, dtype=torch.int16, device=w.device)
    else:
        qweight, scales, mins = out
        for t, shape, dt in ((qweight, qs, torch.int32), (scales, ss, torch.int16), (mins, ms, torch.int16)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != w.device:
                raise ValueError(f"{name}: out must be contiguous (qweight {qs} int32, scales {ss} int16, mins {ms} int16) on {w.device}")
    rc = _lib.load().kivi_w4_pack(w.data_ptr(), w.stride(0), _DTYPES[w.dtype], O, K, group, qweight.data_ptr(), scales.data_ptr(),
                                  mins.data_ptr(), _lib.stream_ptr(w))
    _lib.check(rc, "kivi_w4_pack")
    return qweight, scales, mins


def _dims(qweight, scales, mins):
    S, T, _ = qweight.shape
    O, K = S * ROW_TILE, T * K_TILE
    group = K // scales.shape[1]
    if (tuple(qweight.shape), tuple(scales.shape), tuple(mins.shape)) != shapes(O, K, group) or qweight.dtype != torch.int32 \
            or scales.dtype != torch.int16 or mins.dtype != torch.int16 \
            or not (qweight.is_contiguous() and scales.is_contiguous() and mins.is_contiguous()):
        raise ValueError("qweight (O / 16, K / 128, 256) int32, scales and mins (O / 16, K / G, 16) int16, contiguous")
    return O, K, group


def dequant(qweight, scales, mins, dtype=torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One kivi_w4_dequant launch -> the dense (O, K) weight in `dtype`; `out`: a contiguous buffer of that shape to write into."""
    _lib.require_gpu(qweight, "qweight")
    O, K, group = _dims(qweight, scales, mins)
    if out is None:
        out = torch.empty((O, K), dtype=dtype, device=qweight.device)
    elif tuple(out.shape) != (O, K) or out.dtype != dtype or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"dequant: out must be contiguous {dtype} {(O, K)} on the GPU")
    rc = _lib.load().kivi_w4_dequant(qweight.data_ptr(), scales.data_ptr(), mins.data_ptr(), O, K, group, _DTYPES[dtype], out.data_ptr(),
                                     out.stride(0), _lib.stream_ptr(qweight))
    _lib.check(rc, "kivi_w4_dequant")
    return out


def linear(x: torch.Tensor, qweight, scales, mins, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One kivi_w4_linear launch.  x (N, K) fp16 or bf16 (a view with a row stride is read as it is when its rows are 16-byte
    aligned) -> (N, O) in x's dtype."""
    O, K, group = _dims(qweight, scales, mins)
    x = _check_x(x, K, "kivi_w4_linear")
    if bias is not None and (bias.dtype != x.dtype or tuple(bias.shape) != (O,) or not bias.is_contiguous() or not bias.is_cuda):
        raise ValueError(f"kivi_w4_linear: bias must be ({O},) {x.dtype} on the GPU")
    y = torch.empty((x.shape[0], O), dtype=x.dtype, device=x.device)
    rc = _lib.load().kivi_w4_linear(x.data_ptr(), x.stride(0), _DTYPES[x.dtype], x.shape[0], O, K, group, qweight.data_ptr(),
                                    scales.data_ptr(), mins.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
                                    y.stride(0), _lib.stream_ptr(x))
    _lib.check(rc, "kivi_w4_linear")
    return y


def gate_up(x: torch.Tensor, gate, up) -> torch.Tensor:
    """One kivi_w4_gate_up launch: silu(x Wg~^T) * (x Wu~^T), rounded once.  gate, up: (qweight, scales, mins) of two weights of
    one shape (I, K) and one group."""
    I, K, group = _dims(*gate)
    if _dims(*up) != (I, K, group):
        raise ValueError("kivi_w4_gate_up: gate and up must share shape and group")
    x = _check_x(x, K, "kivi_w4_gate_up")
    y = torch.empty((x.shape[0], I), dtype=x.dtype, device=x.device)
    rc = _lib.load().kivi_w4_gate_up(x.data_ptr(), x.stride(0), _DTYPES[x.dtype], x.shape[0], I, K, group, *(t.data_ptr() for t in gate),
                                     *(t.data_ptr() for t in up), y.data_ptr(), y.stride(0), _lib.stream_ptr(x))
    _lib.check(rc, "kivi_w4_gate_up")
    return y


# ------------------------------------------------------------------------------------------------ modules
_SCRATCH = {}       # (device, dtype) -> the one buffer every QuantLinear dequantises into above kernel_max_tokens: the largest weight


def _scratch(device, dtype, rows: int, cols: int) -> torch.Tensor:
    buf = _SCRATCH.get((device, dtype))
    if buf is None or buf.numel() < rows * cols:
        buf = _SCRATCH[(device, dtype)] = torch.empty(rows * cols, dtype=dtype, device=device)
    return buf[: rows * cols].view(rows, cols)


class QuantLinear(nn.Module):
    """nn.Linear's place with a 4-bit weight: buffers `qweight`, `scales`, `mins` (the latter two int16 bit patterns of fp16 values,
    so that .half() / .bfloat16() / .to(dtype) cannot re-round them) and an optional `bias` parameter.  forward runs kivi_w4_linear
    under stream capture and for at most `kernel_max_tokens` tokens; above that it dequantises into the shared scratch and runs
    F.linear."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, group: int = 128,
                 kernel_max_tokens: Optional[int] = None):
        super().__init__()
        qs, ss, ms = shapes(out_features, in_features, group)
        self.in_features, self.out_features, self.group = in_features, out_features, group
        self.kernel_max_tokens = KERNEL_MAX_TOKENS if kernel_max_tokens is None else int(kernel_max_tokens)
        self.register_buffer("qweight", torch.zeros(qs, dtype=torch.int32))
        self.register_buffer("scales", torch.zeros(ss, dtype=torch.int16))
        self.register_buffer("mins", torch.zeros(ms, dtype=torch.int16))
        self.bias = nn.Parameter(torch.zeros(out_features)) if bias else None

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, group={self.group}"

    @property
    def triple(self):
        return self.qweight, self.scales, self.mins

    def pack_(self, weight: torch.Tensor, name: str = "weight") -> "QuantLinear":
        """Quantise `weight` (out_features, in_features) on its device into the module's buffers."""
        if tuple(weight.shape) != (self.out_features, self.in_features):
            raise ValueError(f"{name}: shape {tuple(weight.shape)} does not fit ({self.out_features}, {self.in_features})")
        for buf, t in zip(self.triple, pack(weight, self.group, name)):
            if buf.device != t.device:
                raise ValueError(f"{name}: the weight is on {t.device}, the module on {buf.device}")
            buf.copy_(t)
        return self

    @classmethod
    def from_linear(cls, linear: nn.Linear, group: int = 128, kernel_max_tokens: Optional[int] = None) -> "QuantLinear":
        """Pack an nn.Linear that lives on the GPU in fp16 or bf16."""
        w = linear.weight.data
        with torch.device(w.device):
            m = cls(linear.in_features, linear.out_features, linear.bias is not None, group, kernel_max_tokens)
        m.pack_(w)
        if linear.bias is not None:
            m.bias.data = linear.bias.data.clone()
        return m

    def dequant(self, dtype=torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return dequant(*self.triple, dtype=dtype, out=out)

    def uses_kernel(self, n_tokens: int) -> bool:
        return torch.cuda.is_current_stream_capturing() or n_tokens <= self.kernel_max_tokens

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _lib.require_gpu(x, "x")
        x2 = x.reshape(-1, self.in_features)
        if self.uses_kernel(x2.shape[0]):
            y = linear(x2, *self.triple, self.bias)
        else:
            y = F.linear(x2, self.dequant(x.dtype, _scratch(x.device, x.dtype, self.out_features, self.in_features)), self.bias)
        return y.view(*x.shape[:-1], self.out_features)


def swiglu_forward(mlp: nn.Module, x: torch.Tensor, fused_gate_up, down_linear) -> torch.Tensor:
    """The forward pass of a SwiGLU MLP over quantised linears `mlp.gate_proj / up_proj / down_proj` -- the one statement of the
    policy, whatever the weight format (QuantMLP here, Fp8MLP of kivi_amd/wfp8.py).  `fused_gate_up(x2)`: the format's gate_up launch
    over (N, K) rows; `down_linear(a)`: its linear launch over the down matrix, without the module's hooks."""
    _lib.require_gpu(x, "x")
    x2 = x.reshape(-1, x.shape[-1])
    if not mlp.down_proj.uses_kernel(x2.shape[0]):
        return mlp.down_proj(F.silu(mlp.gate_proj(x)) * mlp.up_proj(x))
    a = fused_gate_up(x2)
    bound = active_binding(mlp.gate_proj, mlp.up_proj)
    if bound is not None and x.dim() == 3:
        # A LoRA adapter on gate or up needs the two linears apart: the three-linear route, each linear
        # the format's linear launch and its hook.  The fused launch rounds silu(g) * u once, that route three times, so the rows of
        # the base model (slot -1) keep the fused value: their bytes stay those of a pass without adapters.
        adapted = (F.silu(mlp.gate_proj(x)) * mlp.up_proj(x)).view_as(a)
        rows = (bound.for_rows(x.shape[0]).slots >= 0).repeat_interleave(x.shape[1])
        a = torch.where(rows[:, None], adapted, a)
    if active_binding(mlp.down_proj) is not None and x.dim() == 3:
        return mlp.down_proj(a.view(*x.shape[:-1], -1))         # the same linear launch, then the module's hook
    return down_linear(a).view(x.shape)


class QuantMLP(nn.Module):
    """The dense SwiGLU MLP over 4-bit weights under the checkpoint's names gate_proj / up_proj / down_proj: one kivi_w4_gate_up
    launch and one kivi_w4_linear launch; above `kernel_max_tokens` outside a capture the three linears through the scratch."""

    def __init__(self, hidden: int, intermediate: int, group: int = 128, kernel_max_tokens: Optional[int] = None):
        super().__init__()
        self.gate_proj = QuantLinear(hidden, intermediate, False, group, kernel_max_tokens)
        self.up_proj = QuantLinear(hidden, intermediate, False, group, kernel_max_tokens)
        self.down_proj = QuantLinear(intermediate, hidden, False, group, kernel_max_tokens)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return swiglu_forward(self, x, lambda x2: gate_up(x2, self.gate_proj.triple, self.up_proj.triple),
                              lambda a: linear(a, *self.down_proj.triple))


# ------------------------------------------------------------------------------------------------ the factory the models use
def weight_bits_of(cfg) -> Optional[int]:
    bits = getattr(cfg, "kivi_weight_bits", None)
    if bits not in (None, 4):
        raise ValueError(f"weight_bits has to be None or 4, got {bits!r}")
    return bits


def fp8_weights_of(cfg) -> bool:
    fp8 = bool(getattr(cfg, "kivi_fp8_weights", False))
    if fp8 and weight_bits_of(cfg) is not None:
        raise ValueError("fp8_weights and weight_bits=4 are two formats of the same weights: choose one")
    return fp8


def _fp8_converts(cfg, *names) -> bool:
    """Whether the checkpoint's `modules_to_not_convert` (cfg.kivi_fp8_skip) leaves all of the dotted module names to FP8."""
    from .wfp8 import should_convert
    return all(should_convert(n, getattr(cfg, "kivi_fp8_skip", None)) for n in names)


def make_linear(cfg, in_features: int, out_features: int, bias: bool = False, name: Optional[str] = None) -> nn.Module:
    """nn.Linear; with `cfg.kivi_weight_bits == 4` and a shape the kernels serve a QuantLinear; with `cfg.kivi_fp8_weights`, a shape
    the FP8 kernels serve and a dotted module `name` the checkpoint's `modules_to_not_convert` does not hold, an Fp8Linear
    (kivi_amd/wfp8.py)."""
    max_tokens = getattr(cfg, "kivi_weight_kernel_max_tokens", None)
    if fp8_weights_of(cfg):
        from .wfp8 import Fp8Linear, usable as fp8_usable
        if fp8_usable(out_features, in_features) and _fp8_converts(cfg, name):
            return Fp8Linear(in_features, out_features, bias, max_tokens)
        return nn.Linear(in_features, out_features, bias=bias)
    group = getattr(cfg, "kivi_weight_group", 128)
    if weight_bits_of(cfg) is None or not usable(out_features, in_features, group):
        return nn.Linear(in_features, out_features, bias=bias)
    return QuantLinear(in_features, out_features, bias, group, max_tokens)


def make_dense_mlp(cfg, plain_cls, name: Optional[str] = None) -> nn.Module:
    """`plain_cls(cfg)`; with `cfg.kivi_weight_bits == 4` and sizes the kernels serve a QuantMLP; with `cfg.kivi_fp8_weights`, sizes
    the FP8 kernels serve and none of the three projections under the dotted module `name` in `modules_to_not_convert`, an Fp8MLP."""
    hidden, inter = cfg.hidden_size, cfg.intermediate_size
    max_tokens = getattr(cfg, "kivi_weight_kernel_max_tokens", None)
    if fp8_weights_of(cfg):
        from .wfp8 import Fp8MLP, usable as fp8_usable
        names = [None if name is None else f"{name}.{p}_proj" for p in ("gate", "up", "down")]
        if fp8_usable(inter, hidden) and fp8_usable(hidden, inter) and _fp8_converts(cfg, *names):
            return Fp8MLP(hidden, inter, max_tokens)
        return plain_cls(cfg)
    group = getattr(cfg, "kivi_weight_group", 128)
    if weight_bits_of(cfg) is None or not (usable(inter, hidden, group) and usable(hidden, inter, group)):
        return plain_cls(cfg)
    return QuantMLP(hidden, inter, group, max_tokens)
