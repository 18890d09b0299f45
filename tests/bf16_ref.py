"""The references of the bf16 tests, shared by tests/test_bf16_cpu.py, tests/test_bf16_boundary_gpu.py and
tests/test_bf16_model_gpu.py.  Everything but `on_gpu` and `models` stays on the CPU.

`exact` is the contract of kivi_qkv_rope_bf16 evaluated in numpy fp64 and rounded ONCE to fp16 by an explicit round to odd
(`once`), not by a library cast of fp64 to fp16.  `models` builds one tiny model of tests/tiny_qk_models.py in several dtypes from
weights that are the same numbers in all of them (`shared_weights`)."""
import numpy as np
import torch

EPS = 1e-6
D = 128
F16_MAX = 65504.0


def once(d: np.ndarray) -> np.ndarray:
    """fp64 -> fp16, one rounding to nearest even: through the fp32 value truncated towards zero with a sticky last bit.  A finite
    value that would round to an infinity becomes +-65504; NaN stays NaN."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = d.astype(np.float32)                                        # to nearest: one step back where it went away from zero
        away = np.abs(f.astype(np.float64)) > np.abs(d)
        f = np.where(away, np.nextafter(f, np.float32(0.0)), f).astype(np.float32)
        bits = f.view(np.uint32) | (f.astype(np.float64) != d).astype(np.uint32)
        f = bits.view(np.float32)
        f = np.where(np.isfinite(d), np.clip(f, -F16_MAX, F16_MAX), f).astype(np.float32)
        return f.astype(np.float16)


def _np64(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().double().numpy()


def rot(y: np.ndarray) -> np.ndarray:
    h = y.shape[-1] // 2
    return np.concatenate((-y[..., h:], y[..., :h]), axis=-1)


def exact(q_in, k_in, v_in, cos, sin, q_w=None, k_w=None, eps: float = 0.0, ratio_padded=None):
    """q_in (B, Q, nh, D), k_in / v_in (B, Q, nh_kv, D) bf16 or fp32 tensors, cos / sin (Bc, Q, D) fp32 -> fp16 tensors
    q (B, nh_kv * Rp, Q, D) with zero pad heads, k, v (B, nh_kv, Q, D): the formula of include/kivi_hip.h in fp64, one rounding."""
    c, s = _np64(cos)[:, :, None, :], _np64(sin)[:, :, None, :]
    e = float(np.float32(eps))                                          # the entry takes eps as fp32

    def side(x, w):
        x = _np64(x)
        if w is not None:
            rs = 1.0 / np.sqrt((x * x).sum(-1, keepdims=True) / x.shape[-1] + e)
            x = (_np64(w) * x) * rs
        return once(x * c + rot(x) * s).transpose(0, 2, 1, 3)
    q, k, v = side(q_in, q_w), side(k_in, k_w), once(_np64(v_in)).transpose(0, 2, 1, 3)
    B, nh, Q, _ = q.shape
    nkv = k.shape[1]
    R = nh // nkv
    rp = R if ratio_padded is None else ratio_padded
    if rp != R:
        qp = np.zeros((B, nkv, rp, Q, q.shape[-1]), dtype=np.float16)
        qp[:, :, :R] = q.reshape(B, nkv, R, Q, -1)
        q = qp.reshape(B, nkv * rp, Q, -1)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (q, k, v))


def tables(positions: torch.Tensor, head_dim: int = D):
    """fp32 cos / sin (Bc, Q, D) of integer positions (Bc, Q), as rope_cos_sin(inv_freq, positions) leaves them (theta 10000)."""
    from kivi_amd.attention import rope_cos_sin
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    return rope_cos_sin(inv_freq, positions)


def inputs(seed: int, B: int, Q: int, nkv: int, R: int, dtype=torch.bfloat16, fused: bool = False, head_dim: int = D):
    """q_in, k_in, v_in in `dtype`, values in the hundreds at most (what a q / k / v projection carries); `fused`: three views into
    one (B, Q, (nh + 2 nh_kv) * D) buffer, the strides of a fused projection.  And head-norm weights around 1."""
    g = torch.Generator().manual_seed(seed)
    nh = nkv * R
    buf = (torch.randn((B, Q, (nh + 2 * nkv) * head_dim), generator=g) * 8).to(dtype)
    buf[0, 0, :4] = torch.tensor([300.0, -250.0, 0.0, 2.0 ** -20]).to(dtype)
    q, k, v = buf.split([nh * head_dim, nkv * head_dim, nkv * head_dim], dim=-1)
    q, k, v = q.unflatten(-1, (nh, head_dim)), k.unflatten(-1, (nkv, head_dim)), v.unflatten(-1, (nkv, head_dim))
    if not fused:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    qw, kw = ((1.0 + 0.2 * torch.randn(head_dim, generator=g)).to(dtype) for _ in range(2))
    return q, k, v, qw, kw


def on_gpu(*tensors):
    """The tensors on the device with the strides they have here: views keep their places in one copy of their common base."""
    bases, out = {}, []
    for t in tensors:
        if t._base is None:
            out.append(t.cuda())
        else:
            base = bases.setdefault(id(t._base), t._base.cuda())
            out.append(torch.as_strided(base, t.shape, t.stride(), t.storage_offset()))
    return out


# ------------------------------------------------------------------ the tiny models in several dtypes
def shared_weights(state: dict) -> dict:
    """Every floating-point tensor rounded to bf16, magnitudes under 2^-14 (fp16's smallest normal) zeroed: what is left is exactly
    representable in bf16, fp16 and fp32 alike."""
    out = {}
    for name, t in state.items():
        if t.is_floating_point():
            t = t.detach().float().bfloat16()
            t = torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
        out[name] = t
    return out


def same_numbers(state: dict) -> bool:
    """True when every tensor of shared_weights() reads the same in bf16, fp16 and fp32."""
    for t in state.values():
        if t.is_floating_point():
            f = t.float()
            if t.dtype != torch.bfloat16 or not torch.equal(f.half().float(), f) or not torch.equal(f.bfloat16().float(), f) \
                    or not torch.isfinite(f).all():
                return False
    return True


def models(cls, ratio: int, seed: int, dtypes, head_dim: int = D, **kw):
    """One tiny model of tests/tiny_qk_models.py per dtype of `dtypes`, on the GPU, all holding shared_weights() of build()'s draw."""
    import tiny_qk_models as M
    from kivi_amd.llama import make_config

    def cfg():
        if head_dim == D:
            return M.config(ratio, **kw)
        d = dict(hidden_size=256, num_attention_heads=2 * ratio, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=512,
                 vocab_size=M.VOCAB, head_dim=head_dim, rms_norm_eps=1e-6)
        return make_config(d, k_bits=2, v_bits=2, group_size=32, residual_length=32, **kw)
    if head_dim == D:
        base = M.build(cls, ratio, seed, **kw)
    else:                                                               # (build() has no head size: its draw, written out)
        torch.manual_seed(seed)
        base = cls(cfg()).half().cuda()
        for name, p in base.named_parameters():
            if p.dim() > 1:
                p.data.normal_(0.0, 0.05)
            elif name.endswith("bias"):
                p.data.normal_(0.0, 0.1)
            elif "q_norm" in name or "k_norm" in name:
                p.data.normal_(1.0, 0.2)
    state = shared_weights(base.state_dict())
    assert same_numbers(state)
    out = []
    for dt in dtypes:
        m = cls(cfg()).to(dt)
        missing, unexpected = m.load_state_dict(state, strict=False)
        assert not missing and not unexpected
        out.append(m.cuda().eval())
    return out
