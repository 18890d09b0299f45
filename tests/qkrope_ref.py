"""The references of the kivi_qk_rope tests (tests/test_qkrope_gpu.py, tests/test_qkrope_ref_cpu.py): the torch expression of the
rotation, the fp64 evaluation of the head norm's rounding sequence, the two conditions a result is held to against it, and the
inputs of the norm tests."""
import numpy as np
import torch

D = 128
EPS = 1e-6


def rot(x):
    return torch.cat((-x[..., D // 2:], x[..., : D // 2]), dim=-1)


def rope_torch(q_in, k_in, cos, sin):
    """What the attention modules have always computed, on fp16 tensors: (B, Q, h, D) -> (B, h, Q, D)."""
    q, k = q_in.transpose(1, 2), k_in.transpose(1, 2)
    cos, sin = cos[:, None], sin[:, None]
    return q * cos + rot(q) * sin, k * cos + rot(k) * sin


def place(q, R, Rp):
    """(B, nh_kv * R, Q, D) -> (B, nh_kv * Rp, Q, D): head kv * R + r at kv * Rp + r, zeros in the pad heads."""
    B, nh, Q, _ = q.shape
    out = torch.zeros((B, nh // R, Rp, Q, D), dtype=q.dtype, device=q.device)
    out[:, :, :R] = q.reshape(B, nh // R, R, Q, D)
    return out.view(B, nh // R * Rp, Q, D)


def h16(x64: torch.Tensor) -> torch.Tensor:
    """fp64 -> fp16 in ONE rounding to nearest even (numpy converts directly; torch goes through fp32, a second rounding)."""
    return torch.from_numpy(x64.detach().cpu().numpy().astype(np.float16))


def norm64(x: torch.Tensor, w: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """HF's Qwen3RMSNorm as a rounding sequence over exact values: normalise, round to fp16, multiply by the weight, round.  eps is
    the fp32 number HF adds to its fp32 variance."""
    x64 = x.detach().cpu().double()
    var = x64.pow(2).mean(-1, keepdim=True)
    n = h16(x64 * (var + float(np.float32(eps))).rsqrt())
    return h16(w.detach().cpu().double() * n.double())


def rope64(q_in, k_in, cos, sin):
    """rope_torch with every product and sum exact in fp64 and rounded to fp16 once (fp16 inputs, on the CPU)."""
    def one(x):
        x = x.transpose(1, 2).double()
        c, s = cos[:, None].double(), sin[:, None].double()
        return h16(h16(x * c).double() + h16(rot(x) * s).double())
    return one(q_in.cpu()), one(k_in.cpu())


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Number of fp16 values between two finite fp16 tensors (0: the same value; +0 and -0 count as one)."""
    def key(t):
        i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def within_norm_bars(got: torch.Tensor, ref: torch.Tensor):
    """The two conditions of the head-norm tests -> (ok, worst ulp distance, share of elements not bit-equal): every element within
    1 fp16 ulp of the fp64 sequence, at most 1 % not bit-equal (an fp32 evaluation a few 2^-24 off the fp64 one changes an fp16
    rounding only within that distance of a tie: about 1e-3 of elements)."""
    d = ulp_distance(got, ref)
    worst, off = int(d.max()), float((d != 0).float().mean())
    return worst <= 1 and off <= 0.01, worst, off


def norm_inputs(seed: int, B: int = 2, Q: int = 4, nh: int = 5, nh_kv: int = 1):
    """q_in (B, Q, nh, D), k_in (B, Q, nh_kv, D) fp16 and two weights: token 0 plain randn, token 1 thirty times that, token 2 a
    thousandth (eps then matters), token 3 randn with one outlier channel per head."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([1.0, 30.0, 1e-3, 1.0])[:Q].view(1, Q, 1, 1)
    out = []
    for h in (nh, nh_kv):
        x = torch.randn((B, Q, h, D), generator=g) * scale
        if Q > 3:
            ch = torch.randint(0, D, (B, h), generator=g)
            x[:, 3].scatter_(-1, ch[..., None], 200.0)
        out.append(x.half())
    ws = [(1.0 + 0.3 * torch.randn(D, generator=g)).half() for _ in range(2)]
    return out[0], out[1], ws[0], ws[1]


def tables(seed: int, Bc: int, Q: int):
    """cos / sin (Bc, Q, D) fp16 of random positions below 4096, as rope_cos_sin builds them (theta 10000)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, 4096, (Bc, Q), generator=g)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    freqs = pos[..., None].float() * inv_freq
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().half(), emb.sin().half()
