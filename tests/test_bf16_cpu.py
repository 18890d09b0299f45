"""CPU: the bf16 boundary and the bf16 logits value without a device.

* qkv_rope_bf16_torch, the torch statement of kivi_qkv_rope_bf16's contract, bit-equal to the fp64 evaluation of tests/bf16_ref.py
  (numpy, an explicit round to odd; no library cast of fp64 to fp16) for bf16 and fp32 inputs, with and without the head norm; the
  reference's own rounding cross-checked against numpy's direct fp64 -> fp16 conversion.
* Saturation at +-65504, NaN kept.
* The argument checks of qkv_rope_bf16, all before a device is asked for.
* The C entries: KIVI_LOGITS_BF16 of the header is what the binding passes, and an unknown logits_bits is KIVI_EINVAL in all six.
* The weight rule the model tests rely on: tests/tiny_qk_models.build's weights, rounded to bf16 with magnitudes under 2^-14 zeroed,
  are the same numbers in bf16, fp16 and fp32.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bf16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int16)


def test_the_references_rounding_is_one_rounding():
    g = np.random.default_rng(3)
    h = np.float16(g.standard_normal(50000))
    tie = h.astype(np.float64) + np.sign(h.astype(np.float64)) * np.spacing(np.abs(h)).astype(np.float64) / 2
    d = np.concatenate([g.standard_normal(200000) * 10.0 ** g.integers(-9, 5, 200000),
                        # halfway between fp16 neighbours, and what an fp32 detour rounds the wrong way: a tie plus a 2^-40th of itself
                        tie, tie * (1 + 2.0 ** -40), tie * (1 - 2.0 ** -40),
                        [0.0, -0.0, 65504.0, 65519.99, -65519.99, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -50), 6e-8]])
    with np.errstate(over="ignore"):
        direct = d.astype(np.float16)                     # numpy converts fp64 to fp16 from the fp64 bits, correctly rounded
    assert np.array_equal(R.once(d).view(np.uint16), direct.view(np.uint16))
    two = d.astype(np.float32).astype(np.float16)         # (the double rounding the contract rules out does differ on this set)
    assert not np.array_equal(two.view(np.uint16), direct.view(np.uint16))
    sat = R.once(np.array([1e6, -1e6, 65520.0, -65520.0, 1e300, np.inf, -np.inf, np.nan]))
    assert sat[:7].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, np.inf, -np.inf] and np.isnan(sat[7])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "headnorm"])
@pytest.mark.parametrize("ratio", [1, 4])
def test_torch_restatement_equals_the_fp64_evaluation(ratio, norm, dtype):
    from kivi_amd.qkrope import qkv_rope_bf16_torch
    B, Q, nkv = 2, 5, 2
    q, k, v, qw, kw = R.inputs(10 * ratio + norm, B, Q, nkv, ratio, dtype)
    pos = torch.tensor([[0, 1, 77, 4095, 100000], [3, 99999, 65536, 12345, 31]])
    for positions in (pos, pos[:1]):
        cos, sin = R.tables(positions)
        assert cos.dtype == torch.float32 and tuple(cos.shape) == (positions.shape[0], Q, R.D)
        w = (qw, kw, R.EPS) if norm else (None, None, 0.0)
        got = qkv_rope_bf16_torch(q, k, v, cos, sin, *w)
        want = R.exact(q, k, v, cos, sin, *w)
        for name, x, y in zip("qkv", got, want):
            assert x.dtype == torch.float16 and x.shape == y.shape, name
            assert torch.equal(_bits(x), _bits(y)), (name, int((_bits(x) != _bits(y)).sum()))
        assert torch.equal(_bits(got[2]), _bits(v.transpose(1, 2).to(torch.float16)))   # in range: torch's own cast of v
    # (the padded layout of the reference: the heads of a group first, zero heads behind them)
    qp = R.exact(q, k, v, cos, sin, *w, ratio_padded=ratio + 3)[0].view(B, nkv, ratio + 3, Q, R.D)
    assert torch.equal(_bits(qp[:, :, :ratio].reshape(B, nkv * ratio, Q, R.D)), _bits(want[0])) and not qp[:, :, ratio:].any()


def test_saturation_and_nan():
    from kivi_amd.qkrope import qkv_rope_bf16_torch
    q, k, v, qw, kw = R.inputs(5, 1, 2, 1, 1)
    q[0, 0, 0, :4] = torch.tensor([1e6, -1e6, float("nan"), 7e4]).bfloat16()
    q[0, 0, 0, 64:68] = 0.0
    k[0, 1, 0, :2] = torch.tensor([-1e6, float("nan")]).bfloat16()
    k[0, 1, 0, 64:66] = 0.0
    v[0, 0, 0, :4] = torch.tensor([1e6, -1e6, float("nan"), 65504.0]).bfloat16()
    cos, sin = torch.ones(1, 2, R.D), torch.zeros(1, 2, R.D)
    for got in (qkv_rope_bf16_torch(q, k, v, cos, sin), R.exact(q, k, v, cos, sin)):
        gq, gk, gv = got
        assert gq[0, 0, 0, :2].tolist() == [65504.0, -65504.0] and gq[0, 0, 0, 2].isnan() and gq[0, 0, 0, 3].item() == 65504.0
        assert gk[0, 0, 1, 0].item() == -65504.0 and gk[0, 0, 1, 1].isnan()
        assert gv[0, 0, 0, :2].tolist() == [65504.0, -65504.0] and gv[0, 0, 0, 2].isnan() and gv[0, 0, 0, 3].item() == 65504.0
        assert torch.isfinite(gq[0, :, 1]).all() and torch.isfinite(gk[0, :, 0]).all()


def test_argument_checks_come_before_any_device_work():
    """On the CPU a call that reached the device check raises KiviHipError (no CPU path): a ValueError shows the check came first."""
    from kivi_amd._lib import KiviHipError
    from kivi_amd.qkrope import qkv_rope_bf16
    q, k, v, qw, kw = R.inputs(6, 2, 3, 2, 4)
    cos, sin = R.tables(torch.arange(3)[None])
    bad = [
        dict(q_in=q.half()), dict(k_in=k.half()), dict(v_in=v.float()),                       # an fp16 / fp32 input
        dict(cos=cos.bfloat16(), sin=sin.bfloat16()), dict(cos=cos.half(), sin=sin.half()),   # a 16-bit table
        dict(k_in=k[:, :, :1].expand(-1, -1, 3, -1)), dict(v_in=v[:, :2]), dict(q_in=q[0]),   # shapes that do not go together
        dict(cos=cos[:, :2], sin=sin[:, :2]), dict(cos=cos.expand(3, -1, -1), sin=sin.expand(3, -1, -1)), dict(sin=sin[0]),
        dict(q_in=q.transpose(2, 3).contiguous().transpose(2, 3)),                            # a channel stride of nh
        dict(cos=cos.transpose(1, 2).contiguous().transpose(1, 2)),                               # ... and of Q in a table
        dict(q_weight=qw), dict(q_weight=qw.half(), k_weight=kw.half()), dict(q_weight=qw[:64], k_weight=kw[:64]),
    ]
    for kw_ in bad:
        args = dict(q_in=q, k_in=k, v_in=v, cos=cos, sin=sin)
        args.update(kw_)
        with pytest.raises(ValueError):
            qkv_rope_bf16(**args)
    with pytest.raises(KiviHipError):                     # every check passed: the device is asked for, and there is none here
        qkv_rope_bf16(q, k, v, cos, sin, 4, qw, kw, R.EPS)


def test_header_value_binding_and_unknown_logits_bits(lib):
    from kivi_amd import _lib
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    value = int(re.search(r"#define KIVI_LOGITS_BF16 (0x[0-9A-Fa-f]+)", src).group(1), 16)
    assert value == _lib.LOGITS_BF16 == _lib.LOGITS_BITS[torch.bfloat16] and value not in (8, 16, 32, 64)
    assert _lib.LOGITS_BITS[torch.float16] == 16 and _lib.LOGITS_BITS[torch.float32] == 32
    assert lib.kivi_abi_version() == 3 and re.search(r"#define KIVI_ABI_VERSION 3\b", src)
    res, args = _lib.SIGNATURES["kivi_qkv_rope_bf16"]
    decl = re.search(r"\bint\s+kivi_qkv_rope_bf16\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    assert hasattr(lib, "kivi_qkv_rope_bf16") and res is ctypes.c_int32 and len(args) == len(decl.split(",")) == 29
    p = ctypes.c_void_p
    a, b, c, d, e, f, g = (p(0x10000 * i) for i in range(1, 8))          # plausible, aligned, never dereferenced

    def calls(bits):
        return {
            "kivi_sample": lib.kivi_sample(a, bits, 320, 2, 320, 1.0, 0, 1.0, 0.0, b, c, 1, None),
            "kivi_sample_rows": lib.kivi_sample_rows(a, bits, 320, 2, 320, b, c, d, 1, None),
            "kivi_sample_rows_pen": lib.kivi_sample_rows_pen(a, bits, 320, 2, 320, b, c, d, e, 320, f, 1, None),
            "kivi_sample_rows_con": lib.kivi_sample_rows_con(a, bits, 320, 2, 320, b, c, d, e, 320, f, g, 12, None, 0, p(0x90000), 1,
                                                             None),
            "kivi_token_logprob": lib.kivi_token_logprob(a, bits, 320, 4, 320, b, 1, -100, c, None, None, None),
            "kivi_token_top_logprobs": lib.kivi_token_top_logprobs(a, bits, 320, 4, 320, 5, b, 1, -100, c, d, 5, e, None, None, None),
        }
    for bits in (0, 8, 17, 64, value + 1, value - 16, -value, 0x100):
        for name, rc in calls(bits).items():
            assert rc == -1, (name, bits)                                # KIVI_EINVAL, nothing enqueued
    assert lib.kivi_token_top_logprobs(a, 12, 320, 4, 320, 5, b, 1, -100, c, d, 5, e, None, None, None) == -1
    assert b"logits_bits=12" in lib.kivi_last_error() and b"KIVI_LOGITS_BF16" in lib.kivi_last_error()
    # the bf16 value is taken as 2-byte elements: an odd address is KIVI_EALIGN, as for fp16
    assert lib.kivi_token_logprob(p(0x10001), value, 320, 4, 320, b, 1, -100, c, None, None, None) == -2
    assert lib.kivi_sample_rows(p(0x10001), value, 320, 2, 320, b, c, d, 1, None) == -2
    # and the boundary entry's own refusals
    def rope(D=128, nh=8, nkv=2, Rp=4, cos=d, q=a, eps=1e-6, q_sb=1024):
        return lib.kivi_qkv_rope_bf16(q, q_sb, 1024, 128, b, 256, 256, 128, c, 256, 256, 128, cos, e, 0, 128, None, None, eps, f, g,
                                      p(0x90000), 2, 1, nh, nkv, Rp, D, None)
    for kw_ in (dict(D=64), dict(nh=7), dict(Rp=3), dict(Rp=65), dict(cos=None), dict(q=None), dict(eps=-1.0), dict(q_sb=-1)):
        assert rope(**kw_) == -1, kw_
        assert b"kivi_qkv_rope_bf16" in lib.kivi_last_error()
    assert rope(q=p(0x10001)) == -2 and rope(cos=p(0x40002)) == -2


def test_the_tiny_models_weights_are_the_same_numbers_in_three_formats(monkeypatch):
    import tiny_qk_models as M
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, Qwen3ForCausalLM_KIVI
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)        # build() without a device
    for cls, ratio, seed in ((LlamaForCausalLM_KIVI, 4, 31), (Qwen2ForCausalLM_KIVI, 7, 48), (Qwen3ForCausalLM_KIVI, 5, 46)):
        model = M.build(cls, ratio, seed)
        raw = model.state_dict()
        state = R.shared_weights(raw)
        assert R.same_numbers(state) and set(state) == set(raw)
        for name, t in state.items():
            f = t.float()
            assert (f == 0).float().mean().item() < 0.01, name                      # the rule zeroes a fraction of a percent
            for dt in (torch.float16, torch.bfloat16, torch.float32):
                m = torch.nn.Parameter(torch.empty_like(f, dtype=dt), requires_grad=False)
                m.data.copy_(t)                                                     # what load_state_dict does
                assert torch.equal(m.data.double(), f.double()), (name, dt)
        assert any("q_norm" in n for n in state) == (cls is Qwen3ForCausalLM_KIVI)
    tiny = R.shared_weights({"w": torch.tensor([2.0 ** -15 * 1.25, -(2.0 ** -20), 2.0 ** -14, 0.3], dtype=torch.float16)})["w"]
    assert tiny.tolist() == [0.0, 0.0, 2.0 ** -14, float(torch.tensor(0.3).bfloat16())]
