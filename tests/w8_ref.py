"""CPU restatements for the FP8 weight tests; nothing here imports kivi_amd or transformers.

  E4M3                 byte -> value, built from the IEEE-style definition of OCP e4m3fn (1 sign, 4 exponent bits of bias 7, 3
                       mantissa bits, subnormals at exponent 0, no infinities, NaN at 0x7F / 0xFF), not from torch
  quantize_ref         transformers' Fp8Quantize._quantize_one restated on the CPU for a [128, 128] block grid whose last block-row
                       may be partial (its maximum runs over the rows that exist)
  represented          the contract's real weight, in fp64: E4M3[byte] * scale of the element's block
  should_convert_ref   transformers' should_convert_module, restated
  write_fp8_dir        a tiny FP8 checkpoint directory (config.json with the quantization_config block + *.safetensors)"""
import json
import os
import re

import torch

BLOCK = 128
FP8_MAX = 448.0
NAN_BYTES = (0x7F, 0xFF)


def _e4m3(b: int) -> float:
    sign, e, m = -1.0 if b & 0x80 else 1.0, (b >> 3) & 15, b & 7
    if e == 15 and m == 7:
        return float("nan")
    if e == 0:
        return sign * m / 8.0 * 2.0 ** -6
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


E4M3 = torch.tensor([_e4m3(b) for b in range(256)], dtype=torch.float64)
FINITE_BYTES = torch.tensor([b for b in range(256) if b not in NAN_BYTES], dtype=torch.uint8)       # the 254 codes of a weight


def grid(O: int, K: int):
    return (O + BLOCK - 1) // BLOCK, (K + BLOCK - 1) // BLOCK


def expand(scale: torch.Tensor, O: int, K: int) -> torch.Tensor:
    return scale.repeat_interleave(BLOCK, 0)[:O].repeat_interleave(BLOCK, 1)[:, :K]


def quantize_ref(w: torch.Tensor):
    """-> (bytes (O, K) uint8, scale_inv (ceil(O / 128), K / 128) fp32) of a weight (O, K), K a multiple of 128, on the CPU."""
    O, K = w.shape
    R, C = grid(O, K)
    v = torch.zeros((R * BLOCK, K), dtype=torch.float32)
    v[:O] = w.detach().cpu().to(torch.float32)
    value = v.reshape(R, BLOCK, C, BLOCK)
    max_abs = value.abs().amax(dim=(-3, -1))
    safe_max_abs = torch.where(max_abs > 0, max_abs, torch.ones_like(max_abs))
    scales = FP8_MAX / safe_max_abs
    scales = torch.where(max_abs > 0, scales, torch.ones_like(scales))
    inv_scales = (1.0 / scales).to(torch.float32)
    scaled = value * scales.unsqueeze(-1).unsqueeze(-3)
    quantized = torch.clamp(scaled, min=-FP8_MAX, max=FP8_MAX).to(torch.float8_e4m3fn).reshape(R * BLOCK, K)[:O]
    return quantized.contiguous().view(torch.uint8), inv_scales


def represented(weight_u8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The real weight of the contract in fp64 (exact: 4 significant bits times 24)."""
    O, K = weight_u8.shape
    return E4M3[weight_u8.cpu().long()] * expand(scale.cpu().double(), O, K)


def should_convert_ref(full_name, patterns) -> bool:
    if patterns is None:
        return True
    return not any(re.match(f"{key}\\.", full_name) or re.match(f"{key}", full_name) or full_name.endswith(key) for key in patterns)


def random_bytes(shape, seed: int) -> torch.Tensor:
    """Bytes uniform over the 254 finite codes."""
    g = torch.Generator().manual_seed(seed)
    return FINITE_BYTES[torch.randint(0, 254, shape, generator=g)]


def block_scales(O: int, K: int, seed: int) -> torch.Tensor:
    """2^-6 * u with u distinct per block in [0.5, 2): a wrong block index moves an output by order one."""
    R, C = grid(O, K)
    n = R * C
    u = 0.5 + 1.5 * (torch.randperm(n, generator=torch.Generator().manual_seed(seed)).double() + 0.25) / n
    return (u * 2.0 ** -6).float().reshape(R, C)


QUANT_CONFIG = dict(quant_method="fp8", fmt="e4m3", activation_scheme="dynamic", weight_block_size=[128, 128], scale_fmt="float")


def write_fp8_dir(path: str, config: dict, tensors: dict, quant: dict = None, files=None) -> None:
    """config.json = `config` + quantization_config (`quant`: overrides / additions to QUANT_CONFIG; a value of ... drops the key),
    and the tensors in model.safetensors -- or, with `files` = [[names], [names], ...], one file per list, in that order."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    q = dict(QUANT_CONFIG)
    q.update(quant or {})
    q = {k: v for k, v in q.items() if v is not ...}
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(config, quantization_config=q), fh)
    if files is None:
        save_file({k: v.contiguous() for k, v in tensors.items()}, os.path.join(path, "model.safetensors"))
        return
    assert sorted(n for f in files for n in f) == sorted(tensors)
    for i, names in enumerate(files):
        save_file({k: tensors[k].contiguous() for k in names}, os.path.join(path, f"model-{i + 1:05d}-of-{len(files):05d}.safetensors"))


def fp8_state(state: dict, keep_dense=()) -> dict:
    """A 16-bit state_dict -> the FP8 checkpoint of it: every `*_proj.weight` outside experts whose shape the format blocks evenly
    along K (and whose name is not in `keep_dense`) becomes float8_e4m3fn bytes plus `weight_scale_inv`."""
    out = {}
    for k, v in state.items():
        if k.endswith("_proj.weight") and ".experts." not in k and v.dim() == 2 and v.shape[1] % BLOCK == 0 and k not in keep_dense:
            codes, inv = quantize_ref(v)
            out[k] = codes.view(torch.float8_e4m3fn)
            out[k[: -len("weight")] + "weight_scale_inv"] = inv
        else:
            out[k] = v.detach().cpu()
    return out
