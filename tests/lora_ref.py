"""The contract of kivi_amd/lora.py restated in fp64 on the stored values, and the bound the tests hold the
kernels and apply_torch to.  For token n of row b = n // Q with s = slots[b] >= 0

    y64[n, o] = y[n, o] + scale[s] * sum_j B[s, o, j] * sum_k A[s, j, k] * x[n, k]

and for every element

    |y' - y64| <= u |y64| + gamma_(K + R + 3) * scale * sum_j |B_oj| sum_k |A_jk| |x_k| + 2^-24 |y|

with u = 2^-11 (fp16) / 2^-8 (bf16), the rounding of the result, and gamma_n = n 2^-24 / (1 - n 2^-24), the standard bound of an
fp32 dot product of n terms (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1): the K products and sums of t, the
R of d, the multiplication by scale, the addition to y and one spare.  Nothing here is fitted to the code under test."""
import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def gamma(n: int) -> float:
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)


def statement64(y, x, A, B, scale, slots):
    """y, x (Bt, Q, .), A (S, R, K), B (S, O, R), scale (S,) on any device; slots: a list of Bt ints.  -> (y64, magnitude), fp64 on
    the CPU: the exact result and scale * sum_j |B| sum_k |A| |x| of every element (0 on rows whose slot is outside [0, S))."""
    y64, x64 = y.detach().double().cpu().clone(), x.detach().double().cpu()
    A64, B64, sc = A.detach().double().cpu(), B.detach().double().cpu(), scale.detach().double().cpu()
    mag = torch.zeros_like(y64)
    for b, s in enumerate(slots):
        if 0 <= s < A64.shape[0]:
            y64[b] += sc[s] * (x64[b] @ A64[s].t()) @ B64[s].t()
            mag[b] = sc[s].abs() * (x64[b].abs() @ A64[s].abs().t()) @ B64[s].abs().t()
    return y64, mag


def bound(y0, y64, mag, K: int, R: int, dtype):
    """The bound above, per element, fp64."""
    return U[dtype] * y64.abs() + gamma(K + R + 3) * mag + 2.0 ** -24 * y0.detach().double().cpu().abs()


def worst_ratio(got, y0, y64, mag, K: int, R: int, dtype, factor: float = 1.0):
    """max over elements of |got - y64| / (factor * bound); elements whose bound is 0 have to be exact (ratio 0 or inf)."""
    err = (got.detach().double().cpu() - y64).abs()
    b = factor * bound(y0, y64, mag, K, R, dtype)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ratio.max().item()


def tables(S: int, R: int, K: int, O: int, ranks, dtype, device, seed: int, std: float = 0.05):
    """Tables as a LoraSet holds them: slot s carries a rank ranks[s] adapter ~ N(0, std) in rows / columns [0, r), zeros behind."""
    g = torch.Generator().manual_seed(seed)
    A, B = torch.zeros((S, R, K)), torch.zeros((S, O, R))
    for s, r in enumerate(ranks):
        A[s, :r] = torch.randn((r, K), generator=g) * std
        B[s, :, :r] = torch.randn((O, r), generator=g) * std
    scale = torch.tensor([2.0 / max(r, 1) ** 0.5 if r else 0.0 for r in ranks], dtype=torch.float32)
    return (A.to(dtype).to(device), B.to(dtype).to(device), scale.to(device),
            torch.tensor(list(ranks), dtype=torch.int32, device=device))


def make_adapter(model, r: int, alpha: float, seed: int, targets, std: float = 0.05, dtype=torch.float32, rslora: bool = False):
    """A LoraAdapter ~ N(0, std) of rank r on every linear of `model` named in `targets` (PEFT's layout: A (r, in), B (out, r))."""
    from kivi_amd.lora import LoraAdapter
    g = torch.Generator().manual_seed(seed)
    t = {}
    for name, m in model.named_modules():
        if name.rsplit(".", 1)[-1] in targets and hasattr(m, "in_features") and ".experts." not in name:
            t[name] = ((torch.randn((r, m.in_features), generator=g) * std).to(dtype),
                       (torch.randn((m.out_features, r), generator=g) * std).to(dtype))
    return LoraAdapter(t, r, alpha, rslora, targets)
