"""FP8 weights under 16-bit activations, W8A16: the fine-grained FP8 checkpoint format of transformers
(`quant_method: "fp8"`) served as it lies on disk.

The contract (include/kivi_hip.h): for a linear (O, K) two buffers in the checkpoint's own form -- `weight` (O, K), one OCP e4m3fn
byte per element and no NaN byte, and `weight_scale_inv` (ceil(O / 128), K / 128) fp32, which despite its name is the factor one
multiplies by (transformers/integrations/finegrained_fp8.py).  The represented weight is the real number
e4m3(weight[o, k]) * weight_scale_inv[o // 128, k // 128]; a linear is y[n, o] = sum_k x[n, k] * W~[o, k] (+ bias[o]) with x in fp16
or bf16 and NOT quantised, accumulated in fp32 and rounded once to x's dtype.  `dequant` / `linear` / `gate_up` are the three HIP
entries (kivi_amd/csrc/kivi_w8.hip): launches only, so a captured decode step may hold them.  `quantize` is the load-time quantiser
of a 16-bit weight, in torch on the weight's device, statement for statement transformers' Fp8Quantize._quantize_one.  `Fp8Linear`
/ `Fp8MLP` are the modules `make_config(..., fp8_weights=True)` puts in place of the attention projections and of the dense MLP."""
from __future__ import annotations

import re
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, wquant

BLOCK = 128                     # the scale block is BLOCK x BLOCK: the only block size served
ROW_TILE, K_TILE = 16, 128      # kivi_amd/csrc/kivi_w8_plan.h
FP8_MAX = 448.0                 # torch.finfo(torch.float8_e4m3fn).max
# Eager calls of more tokens than this dequantise into the shared scratch and run F.linear (rocBLAS); under stream capture the
# kernel always runs.  Set as section 30 set its own: the largest N at which tools/w8_time.py measured the kernel ahead of dequant +
# F.linear on EVERY shape (profiles/w8_time.log, MI355X): "crossover: the kernel beats dequant + F.linear on every shape at N in
# [1, 8, 32]; the largest such N below the first N at which it loses on some shape: 32" -- at 32 it is 1.3-2.3x ahead, at the next
# measured size, 64, the 4096 -> 1024 projection is behind (0.80x) while the five larger shapes stay 1.1-1.6x ahead (DESIGN.md
# section 35).
KERNEL_MAX_TOKENS = 32
_DTYPES = {torch.float16: 16, torch.bfloat16: _lib.LOGITS_BF16}


def usable(out_features: int, in_features: int) -> bool:
    """True for the shapes the kernels serve: O a positive multiple of 16, K a positive multiple of 128."""
    return out_features >= ROW_TILE and out_features % ROW_TILE == 0 and in_features >= K_TILE and in_features % K_TILE == 0


def scale_shape(out_features: int, in_features: int):
    """Shape of the block grid of a weight (out_features, in_features): the last block-row and -column may be partial."""
    return (out_features + BLOCK - 1) // BLOCK, (in_features + BLOCK - 1) // BLOCK


def shapes(out_features: int, in_features: int):
    """Shapes of the two buffers: weight uint8, weight_scale_inv int32 (fp32 bit patterns)."""
    if not usable(out_features, in_features):
        raise ValueError(f"FP8 weights need out_features a multiple of 16 and in_features a multiple of 128, got "
                         f"({out_features}, {in_features})")
    return (out_features, in_features), scale_shape(out_features, in_features)


def should_convert(name: Optional[str], patterns: Optional[Sequence[str]]) -> bool:
    """transformers' rule for `modules_to_not_convert` (quantizers_utils.should_convert_module), restated: a module stays dense when
    a pattern, read as a regular expression, matches the beginning of its dotted name -- alone or followed by a dot -- or when the
    name ends with the pattern."""
    if not patterns or name is None:
        return True
    return not any(re.match(f"{key}\\.", name) or re.match(f"{key}", name) or name.endswith(key) for key in patterns)


# ------------------------------------------------------------------------------------------------ the format, in torch
def as_bytes(weight: torch.Tensor, name: str = "weight") -> torch.Tensor:
    """A float8_e4m3fn (or uint8) tensor -> its bytes; a NaN byte (0x7F, 0xFF) is refused, by `name`."""
    if weight.dtype == torch.float8_e4m3fn:
        weight = weight.view(torch.uint8)
    elif weight.dtype != torch.uint8:
        raise ValueError(f"{name}: float8_e4m3fn (or its bytes as uint8) is needed, got {weight.dtype}")
    if bool(((weight & 0x7F) == 0x7F).any()):
        raise ValueError(f"{name}: the FP8 weight holds a NaN byte (0x7F or 0xFF)")
    return weight


def as_scale(scale: torch.Tensor, out_features: int, in_features: int, name: str = "weight_scale_inv") -> torch.Tensor:
    """A checkpoint's scale tensor -> the fp32 block grid of the weight: a per-tensor scalar (one element) is expanded to it; a
    non-finite scale and any other shape are refused, by `name`."""
    grid = scale_shape(out_features, in_features)
    if scale.dtype != torch.float32:
        raise ValueError(f"{name}: fp32 scales are needed, got {scale.dtype} (ue8m0 scales are not served)")
    if not bool(torch.isfinite(scale).all()):
        raise ValueError(f"{name}: a scale is not finite")
    if scale.numel() == 1:
        return scale.reshape(1, 1).expand(grid).contiguous()
    if tuple(scale.shape) != grid:
        raise ValueError(f"{name}: shape {tuple(scale.shape)} does not fit the [128, 128] block grid {grid} of a weight "
                         f"({out_features}, {in_features})")
    return scale.contiguous()


def quantize(w: torch.Tensor, name: str = "weight"):
    """The load-time quantiser of a weight (O, K), K a multiple of 128, on w's device -> (bytes (O, K) uint8, scale_inv
    (ceil(O / 128), K / 128) fp32): transformers' Fp8Quantize._quantize_one statement for statement on the fp32 image of `w` -- per
    block s = 448 / max|w| (1 where the block is all zero), inv = 1 / s in fp32, codes clamp(w * s, -448, 448).to(float8_e4m3fn).
    The last block-row may be partial: its maximum runs over the rows that exist (it is padded with zeros, which change neither a
    maximum nor a code).  A weight that is not finite is refused, by `name`."""
    if w.dim() != 2 or w.shape[1] % BLOCK or not w.is_floating_point():
        raise ValueError(f"{name}: a 2-D floating-point weight with in_features a multiple of {BLOCK} is needed, got "
                         f"{tuple(w.shape)} {w.dtype}")
    O, K = w.shape
    R, C = scale_shape(O, K)
    v = w.detach().to(torch.float32)
    if not bool(torch.isfinite(v).all()):
        raise ValueError(f"{name}: the weight is not finite; it cannot be quantised to FP8")
    if R * BLOCK != O:
        v = torch.cat([v, v.new_zeros((R * BLOCK - O, K))])
    blocks = v.reshape(R, BLOCK, C, BLOCK)
    max_abs = blocks.abs().amax(dim=(-3, -1))
    safe = torch.where(max_abs > 0, max_abs, torch.ones_like(max_abs))
    scales = FP8_MAX / safe
    scales = torch.where(max_abs > 0, scales, torch.ones_like(scales))
    inv = (1.0 / scales).to(torch.float32)
    scaled = blocks * scales.unsqueeze(-1).unsqueeze(-3)
    codes = torch.clamp(scaled, min=-FP8_MAX, max=FP8_MAX).to(torch.float8_e4m3fn).reshape(R * BLOCK, K)[:O]
    return codes.contiguous().view(torch.uint8), inv.contiguous()


def expand_scale(scale: torch.Tensor, out_features: int, in_features: int) -> torch.Tensor:
    """The fp32 block grid -> one scale per element (out_features, in_features)."""
    return scale.repeat_interleave(BLOCK, 0)[:out_features].repeat_interleave(BLOCK, 1)[:, :in_features]


def dequant_torch(weight: torch.Tensor, scale: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """The dense weight of kivi_w8_dequant in torch, on any device and for any shape: (w8.float() * s).to(dtype) -- the fp32 image
    of the byte is exact, the product is rounded to fp32 and then to the dtype.  `scale`: the fp32 block grid."""
    O, K = weight.shape
    return (weight.view(torch.float8_e4m3fn).to(torch.float32) * expand_scale(scale, O, K)).to(dtype)


# ------------------------------------------------------------------------------------------------ the three entries
def _dims(weight: torch.Tensor, scale_bits: torch.Tensor):
    O, K = weight.shape
    if weight.dtype != torch.uint8 or scale_bits.dtype != torch.int32 or (tuple(weight.shape), tuple(scale_bits.shape)) != shapes(O, K) \
            or not (weight.is_contiguous() and scale_bits.is_contiguous()):
        raise ValueError("weight (O, K) uint8 and weight_scale_inv (ceil(O / 128), K / 128) int32 (fp32 bit patterns), contiguous")
    return O, K


def dequant(weight, scale_bits, dtype=torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One kivi_w8_dequant launch -> the dense (O, K) weight in `dtype`; `out`: a contiguous buffer of that shape to write into."""
    _lib.require_gpu(weight, "weight")
    O, K = _dims(weight, scale_bits)
    if dtype not in _DTYPES:
        raise ValueError(f"kivi_w8_dequant: dtype must be fp16 or bf16, got {dtype}")
    if out is None:
        out = torch.empty((O, K), dtype=dtype, device=weight.device)
    elif tuple(out.shape) != (O, K) or out.dtype != dtype or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"dequant: out must be contiguous {dtype} {(O, K)} on the GPU")
    rc = _lib.load().kivi_w8_dequant(weight.data_ptr(), scale_bits.data_ptr(), O, K, _DTYPES[dtype], out.data_ptr(), out.stride(0),
                                     _lib.stream_ptr(weight))
    _lib.check(rc, "kivi_w8_dequant")
    return out


def linear(x: torch.Tensor, weight, scale_bits, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One kivi_w8_linear launch.  x (N, K) fp16 or bf16 (a view with a row stride is read as it is when its rows are 16-byte
    aligned) -> (N, O) in x's dtype."""
    O, K = _dims(weight, scale_bits)
    x = wquant._check_x(x, K, "kivi_w8_linear")
    if bias is not None and (bias.dtype != x.dtype or tuple(bias.shape) != (O,) or not bias.is_contiguous() or not bias.is_cuda):
        raise ValueError(f"kivi_w8_linear: bias must be ({O},) {x.dtype} on the GPU")
    y = torch.empty((x.shape[0], O), dtype=x.dtype, device=x.device)
    rc = _lib.load().kivi_w8_linear(x.data_ptr(), x.stride(0), _DTYPES[x.dtype], x.shape[0], O, K, weight.data_ptr(),
                                    scale_bits.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(), y.stride(0),
                                    _lib.stream_ptr(x))
    _lib.check(rc, "kivi_w8_linear")
    return y


def gate_up(x: torch.Tensor, gate, up) -> torch.Tensor:
    """One kivi_w8_gate_up launch: silu(x Wg~^T) * (x Wu~^T), rounded once.  gate, up: (weight, weight_scale_inv) of two weights of
    one shape (I, K)."""
    I, K = _dims(*gate)
    if _dims(*up) != (I, K):
        raise ValueError("kivi_w8_gate_up: gate and up must share their shape")
    x = wquant._check_x(x, K, "kivi_w8_gate_up")
    y = torch.empty((x.shape[0], I), dtype=x.dtype, device=x.device)
    rc = _lib.load().kivi_w8_gate_up(x.data_ptr(), x.stride(0), _DTYPES[x.dtype], x.shape[0], I, K, *(t.data_ptr() for t in gate),
                                     *(t.data_ptr() for t in up), y.data_ptr(), y.stride(0), _lib.stream_ptr(x))
    _lib.check(rc, "kivi_w8_gate_up")
    return y


# ------------------------------------------------------------------------------------------------ modules
class Fp8Linear(nn.Module):
    """nn.Linear's place with an FP8 weight: buffers `weight` (uint8: the e4m3fn bytes) and `weight_scale_inv` (int32 bit patterns
    of the fp32 scales, so that .half() / .bfloat16() / .to(dtype) cannot re-round them -- the reason QuantLinear keeps int16) under
    the checkpoint's names, and an optional `bias` parameter.  forward runs kivi_w8_linear under stream capture and for at most
    `kernel_max_tokens` tokens; above that it dequantises into the scratch QuantLinear shares and runs F.linear."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, kernel_max_tokens: Optional[int] = None):
        super().__init__()
        ws, ss = shapes(out_features, in_features)
        self.in_features, self.out_features = in_features, out_features
        self.kernel_max_tokens = KERNEL_MAX_TOKENS if kernel_max_tokens is None else int(kernel_max_tokens)
        self.register_buffer("weight", torch.zeros(ws, dtype=torch.uint8))
        self.register_buffer("weight_scale_inv", torch.zeros(ss, dtype=torch.int32))
        self.bias = nn.Parameter(torch.zeros(out_features)) if bias else None

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, fp8=e4m3fn [128, 128]"

    @property
    def pair(self):
        return self.weight, self.weight_scale_inv

    @property
    def scale(self) -> torch.Tensor:
        """The fp32 block grid (a view of the buffer's bits)."""
        return self.weight_scale_inv.view(torch.float32)

    def load_(self, weight_fp8: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, name: str = "weight") -> "Fp8Linear":
        """Take a checkpoint's tensors as they are, either or both: `weight_fp8` (O, K) float8_e4m3fn is checked for NaN bytes and
        copied as bytes; `scale`, fp32, is checked to be finite and copied as bits, a per-tensor scalar expanded to the grid."""
        if weight_fp8 is not None:
            if tuple(weight_fp8.shape) != (self.out_features, self.in_features):
                raise ValueError(f"{name}: shape {tuple(weight_fp8.shape)} does not fit ({self.out_features}, {self.in_features})")
            self.weight.copy_(as_bytes(weight_fp8, name))
        if scale is not None:
            self.weight_scale_inv.copy_(as_scale(scale, self.out_features, self.in_features, name).view(torch.int32))
        return self

    def quantize_(self, weight16: torch.Tensor, name: str = "weight") -> "Fp8Linear":
        """Quantise `weight16` (out_features, in_features) on its device into the module's buffers (`quantize`)."""
        if tuple(weight16.shape) != (self.out_features, self.in_features):
            raise ValueError(f"{name}: shape {tuple(weight16.shape)} does not fit ({self.out_features}, {self.in_features})")
        codes, inv = quantize(weight16, name)
        if codes.device != self.weight.device:
            raise ValueError(f"{name}: the weight is on {codes.device}, the module on {self.weight.device}")
        self.weight.copy_(codes)
        self.weight_scale_inv.copy_(inv.view(torch.int32))
        return self

    def dequant(self, dtype=torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The dense weight in `dtype`: kivi_w8_dequant on the GPU, dequant_torch (the same bits) elsewhere."""
        if not self.weight.is_cuda:
            t = dequant_torch(self.weight, self.scale, dtype)
            return t if out is None else out.copy_(t)
        return dequant(*self.pair, dtype=dtype, out=out)

    def uses_kernel(self, n_tokens: int) -> bool:
        return torch.cuda.is_current_stream_capturing() or n_tokens <= self.kernel_max_tokens

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _lib.require_gpu(x, "x")
        x2 = x.reshape(-1, self.in_features)
        if self.uses_kernel(x2.shape[0]):
            y = linear(x2, *self.pair, self.bias)
        else:
            y = F.linear(x2, self.dequant(x.dtype, wquant._scratch(x.device, x.dtype, self.out_features, self.in_features)), self.bias)
        return y.view(*x.shape[:-1], self.out_features)


class Fp8MLP(nn.Module):
    """The dense SwiGLU MLP over FP8 weights under the checkpoint's names gate_proj / up_proj / down_proj: one kivi_w8_gate_up launch
    and one kivi_w8_linear launch; above `kernel_max_tokens` outside a capture the three linears through the scratch.  The policy --
    when the fused launches run, and what a LoRA binding changes -- is wquant.swiglu_forward, the statement QuantMLP runs."""

    def __init__(self, hidden: int, intermediate: int, kernel_max_tokens: Optional[int] = None):
        super().__init__()
        self.gate_proj = Fp8Linear(hidden, intermediate, False, kernel_max_tokens)
        self.up_proj = Fp8Linear(hidden, intermediate, False, kernel_max_tokens)
        self.down_proj = Fp8Linear(intermediate, hidden, False, kernel_max_tokens)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return wquant.swiglu_forward(self, x, lambda x2: gate_up(x2, self.gate_proj.pair, self.up_proj.pair),
                                     lambda a: linear(a, *self.down_proj.pair))
