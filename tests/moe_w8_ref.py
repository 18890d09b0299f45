"""The contract of the FP8 expert block (kivi_moe_experts_w8, kivi_amd/moe.py) restated in fp64, shared by
tests/test_moe_w8_cpu.py and tests/test_moe_w8_gpu.py; nothing here imports kivi_amd.  The represented weight of every expert is
w8_ref.represented -- E4M3[byte] * scale of the element's [128, 128] block, exact in fp64 --, the block over those weights is
moe_ref.experts_ref: nothing is rounded.  Also the inputs of the GPU tests: bytes uniform over the 254 finite codes, block scales
distinct per block, scaled so that the intermediate and the output stay far inside fp16."""
import torch

import moe_ref
import w8_ref

BLOCK = 128


def represented_stacks(gate_up_u8, gate_up_scale, down_u8, down_scale):
    """The four buffers (bytes uint8, scales fp32; stacked over E) -> the real weights gate_up (E, 2 I, H), down (E, H, I) in fp64.
    The stacked (2 I, H) matrix of an expert is one matrix of the format: I is a multiple of 128."""
    E = down_u8.shape[0]
    gu = torch.stack([w8_ref.represented(gate_up_u8[e], gate_up_scale[e]) for e in range(E)])
    dn = torch.stack([w8_ref.represented(down_u8[e], down_scale[e]) for e in range(E)])
    return gu, dn


def experts_w8_ref(x, idx, w, gate_up_u8, gate_up_scale, down_u8, down_scale):
    """-> (out (N, H) fp64 on the CPU, the largest |silu(g) * u| of any pair): moe_ref.experts_ref's statement over the represented
    weights, those of one hit expert at a time (at E = 128 the fp64 stacks would be most of a gigabyte)."""
    x64, w64, idx = x.double().cpu(), w.double().cpu(), idx.cpu()
    I = down_u8.shape[2]
    out, a_max = torch.zeros_like(x64), 0.0
    for e in idx.unique().tolist():
        tok, slot = torch.where(idx == e)
        gu = x64[tok] @ w8_ref.represented(gate_up_u8[e], gate_up_scale[e]).T
        g, u = gu[:, :I], gu[:, I:]
        a = g * torch.sigmoid(g) * u
        a_max = max(a_max, float(a.abs().max()))
        out.index_add_(0, tok, (a @ w8_ref.represented(down_u8[e], down_scale[e]).T) * w64[tok, slot, None])
    return out, a_max


# Block scales are w8_ref.block_scales (2^-6 * u, u distinct per block in [0.5, 2)) times this factor.  With x ~ N(0, 1) and bytes
# uniform over the finite codes, the fp64 reference over the GPU tests' shapes, plans and seeds gives a worst intermediate
# |silu(g) * u| of 46 and a worst output of 13.3 (H = 640, I = 384, E = 8, every token to one expert), output rms 0.11 .. 1.7: far
# below 65504 / 16 = 4094 and far above fp16's subnormals.  tests/test_moe_w8_cpu.py asserts the bound on the largest case.
SCALE_FACTOR = 2.0 ** -5


def random_experts(E: int, H: int, I: int, seed: int):
    """The four buffers of E experts on the CPU: bytes uniform over the 254 finite codes, scales distinct per block of every expert
    (w8_ref.block_scales per expert matrix, seeded apart) times SCALE_FACTOR."""
    gu = w8_ref.random_bytes((E, 2 * I, H), seed)
    dn = w8_ref.random_bytes((E, H, I), seed + 1)
    gus = torch.stack([w8_ref.block_scales(2 * I, H, seed * 1000 + e) for e in range(E)]) * SCALE_FACTOR
    dns = torch.stack([w8_ref.block_scales(H, I, seed * 1000 + 500 + e) for e in range(E)]) * SCALE_FACTOR
    return gu, gus.float(), dn, dns.float()
