"""The contract of the 4-bit weight entries (include/kivi_hip.h) in fp64, and the inputs of their tests.

  represented    W~[o, k] = code * scale + mn as a real number, from the reference's triple (code (O, K / 8) int32 with element
                 8 c + i of a row in bits 4 i of word c; scale, mn (O, K / G) fp16)
  linear_ref     y[n, o] = sum_k x[n, k] W~[o, k] (+ bias[o]) in fp64;  gate_up_ref: silu(g) * u of two such products
  word_bit       where the device layout keeps element (o, k): restated here independently of kivi_amd/wquant.py
  oracle_triple  the reference's last-dim quantiser (oracle.kivi_oracle) on the fp16 image of W viewed as (1, 1, O, K)
  weights        normal / one outlier per group / a constant group / a group whose range is one fp16-subnormal ulp"""
import torch


def codes_of(code: torch.Tensor) -> torch.Tensor:
    """(O, K / 8) int32 -> (O, K) int64 codes."""
    u = code.to(torch.int64) & 0xFFFFFFFF
    return torch.stack([(u >> (4 * i)) & 15 for i in range(8)], dim=-1).reshape(code.shape[0], -1)


def represented(code, scale, mn, group: int) -> torch.Tensor:
    q = codes_of(code).double()
    O, K = q.shape
    s = scale.double().repeat_interleave(group, dim=1)
    z = mn.double().repeat_interleave(group, dim=1)
    assert s.shape == (O, K)
    return q * s + z


def linear_ref(x, wt, bias=None) -> torch.Tensor:
    y = x.double().cpu() @ wt.double().cpu().T
    return y if bias is None else y + bias.double().cpu()


def gate_up_ref(x, wg, wu) -> torch.Tensor:
    g, u = linear_ref(x, wg), linear_ref(x, wu)
    return g / (1.0 + torch.exp(-g)) * u


def word_bit(o: int, k: int, K: int):
    """(index of the int32 word in the flat code buffer, bit of the 4-bit field) of element (o, k) of a weight (O, K)."""
    tile = (o // 16) * (K // 128) + k // 128
    kk = k % 128
    lane = (o % 16) + 16 * ((kk // 8) % 4)
    return tile * 256 + lane * 4 + kk // 32, 4 * ((k % 8) // 2) + 16 * (k % 2)


def sm_half(o: int, g: int, K: int, group: int) -> int:
    """index of the half of (row o, group g) in the flat scale / mn buffers"""
    return ((o // 16) * (K // group) + g) * 16 + o % 16


def oracle_triple(w: torch.Tensor, group: int):
    from oracle import kivi_oracle
    O, K = w.shape
    code, scale, mn = kivi_oracle.quantize_and_pack_along_last_dim(w.detach().cpu().to(torch.float16).view(1, 1, O, K).contiguous(),
                                                                   group, 4)
    return code.view(O, K // 8), scale.view(O, K // group), mn.view(O, K // group)


def weights(kind: str, O: int, K: int, group: int, dtype, seed: int) -> torch.Tensor:
    """(O, K) in `dtype` on the CPU."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((O, K), generator=g) * 0.05
    if kind == "outlier":                       # one value per group far outside the rest
        w = w.view(O, K // group, group)
        pos = torch.randint(0, group, (O, K // group, 1), generator=g)
        w.scatter_(2, pos, torch.full((O, K // group, 1), 3.0) * (torch.randint(0, 2, (O, K // group, 1), generator=g) * 2.0 - 1.0))
        w = w.view(O, K)
    elif kind == "constant":                    # group 0 of every odd row constant (scale 0, every code 0), row 0's at zero
        w[1::2, :group] = 0.37
        w[0, :group] = 0.0
    elif kind == "ulp":                         # group 0 of every row: two neighbouring fp16 subnormals (scale rounds to 0)
        bits = torch.randint(3, 60, (O, 1), generator=g) + torch.randint(0, 2, (O, group), generator=g)
        bits[:, 0] = bits[:, 1:].min(dim=1).values          # both values present wherever the draw gave both
        tiny = bits.to(torch.int16).view(torch.float16).float()
        w[:, :group] = tiny * (torch.randint(0, 2, (O, 1), generator=g) * 2.0 - 1.0)
    elif kind != "normal":
        raise ValueError(kind)
    return w.to(dtype)
