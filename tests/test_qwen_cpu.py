"""No GPU: the Qwen2 / Qwen3 model classes -- where their biases and head norms sit, that a state dict under
HF's parameter names loads completely, the class from_pretrained picks, and the refusal of a sliding window."""
import json

import pytest
import torch

from kivi_amd.attention import QwenAttention_KIVI
from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, Qwen3ForCausalLM_KIVI, make_config
from kivi_amd.qkrope import head_norm


def _d(ratio, **kw):
    return dict(hidden_size=256, num_attention_heads=2 * ratio, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=512,
                vocab_size=64, head_dim=128, rms_norm_eps=1e-6, **kw)


def _hf_names(ratio, bias, norms, tied=False):
    """The parameter names and shapes of HF's Qwen2ForCausalLM / Qwen3ForCausalLM for the tiny config, written out."""
    nh, H, D, I, V = 2 * ratio, 256, 128, 512, 64
    out = {"model.embed_tokens.weight": (V, H), "model.norm.weight": (H,)}
    if not tied:
        out["lm_head.weight"] = (V, H)
    for i in range(2):
        p = f"model.layers.{i}."
        out.update({p + "self_attn.q_proj.weight": (nh * D, H), p + "self_attn.k_proj.weight": (2 * D, H),
                    p + "self_attn.v_proj.weight": (2 * D, H), p + "self_attn.o_proj.weight": (H, nh * D),
                    p + "mlp.gate_proj.weight": (I, H), p + "mlp.up_proj.weight": (I, H), p + "mlp.down_proj.weight": (H, I),
                    p + "input_layernorm.weight": (H,), p + "post_attention_layernorm.weight": (H,)})
        if bias:
            out.update({p + "self_attn.q_proj.bias": (nh * D,), p + "self_attn.k_proj.bias": (2 * D,), p + "self_attn.v_proj.bias": (2 * D,)})
        if norms:
            out.update({p + "self_attn.q_norm.weight": (D,), p + "self_attn.k_norm.weight": (D,)})
    return out


def test_qwen2_builds_with_qkv_bias_only():
    m = Qwen2ForCausalLM_KIVI(make_config(_d(7, model_type="qwen2")))
    for layer in m.model.layers:
        a = layer.self_attn
        assert isinstance(a, QwenAttention_KIVI)
        assert a.q_proj.bias is not None and a.k_proj.bias is not None and a.v_proj.bias is not None and a.o_proj.bias is None
        assert a.q_norm is None and a.k_norm is None
        assert a.head_dim == 128 and a.q_proj.out_features == 14 * 128 and a.o_proj.in_features == 14 * 128


def test_qwen3_builds_with_head_norms():
    m = Qwen3ForCausalLM_KIVI(make_config(_d(5, model_type="qwen3")))
    for layer in m.model.layers:
        a = layer.self_attn
        assert a.q_proj.bias is None and a.o_proj.bias is None              # Qwen3: attention_bias defaults to none
        assert tuple(a.q_norm.weight.shape) == tuple(a.k_norm.weight.shape) == (128,) and a.q_norm.eps == 1e-6
        assert a.q_norm.weight is not a.k_norm.weight
    b = Qwen3ForCausalLM_KIVI(make_config(_d(5, model_type="qwen3", attention_bias=True))).model.layers[0].self_attn
    assert b.q_proj.bias is not None and b.o_proj.bias is None


@pytest.mark.parametrize("cls,ratio,bias,norms", [(Qwen2ForCausalLM_KIVI, 7, True, False), (Qwen3ForCausalLM_KIVI, 5, False, True)])
def test_hf_state_dict_loads_completely(cls, ratio, bias, norms):
    m = cls(make_config(_d(ratio)))
    g = torch.Generator().manual_seed(1)
    state = {k: torch.randn(s, generator=g) for k, s in _hf_names(ratio, bias, norms).items()}
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    assert torch.equal(m.model.layers[1].self_attn.k_proj.weight, state["model.layers.1.self_attn.k_proj.weight"])
    if norms:
        assert torch.equal(m.model.layers[1].self_attn.k_norm.weight, state["model.layers.1.self_attn.k_norm.weight"])


def test_tied_embeddings_as_the_llama_class():
    m = Qwen2ForCausalLM_KIVI(make_config(_d(6, tie_word_embeddings=True)))
    assert m.lm_head.weight is m.model.embed_tokens.weight
    state = {k: torch.zeros(s) for k, s in _hf_names(6, True, False, tied=True).items()}
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and set(missing) <= {"lm_head.weight"}


@pytest.mark.parametrize("cls", [Qwen2ForCausalLM_KIVI, Qwen3ForCausalLM_KIVI])
def test_sliding_window_is_refused(cls):
    with pytest.raises(ValueError, match="sliding window"):
        cls(make_config(_d(7, use_sliding_window=True, sliding_window=4096)))
    cls(make_config(_d(7, use_sliding_window=False, sliding_window=4096)))      # the field alone, unused: as Mistral's


def test_qk_kernel_defaults():
    """Off wherever make_config built the config without it; on for the Qwen classes through from_pretrained and for a config that
    does not carry the field; off for Llama either way."""
    assert not Qwen2ForCausalLM_KIVI(make_config(_d(7))).model.layers[0].self_attn.qk_kernel
    on = Qwen2ForCausalLM_KIVI(make_config(_d(7), qk_kernel=True)).model.layers[0].self_attn
    assert on.qk_kernel and on.cache_heads == 16
    cfg = make_config(_d(5))
    del cfg.kivi_qk_kernel
    assert Qwen3ForCausalLM_KIVI(cfg).model.layers[0].self_attn.qk_kernel
    assert not LlamaForCausalLM_KIVI(cfg).model.layers[0].self_attn.qk_kernel
    assert Qwen2ForCausalLM_KIVI._QK_KERNEL and Qwen3ForCausalLM_KIVI._QK_KERNEL and not LlamaForCausalLM_KIVI._QK_KERNEL


@pytest.mark.parametrize("model_type,cls,ratio,bias,norms", [("qwen2", Qwen2ForCausalLM_KIVI, 7, True, False),
                                                             ("qwen3", Qwen3ForCausalLM_KIVI, 5, False, True),
                                                             ("llama", LlamaForCausalLM_KIVI, 4, False, False)])
def test_from_pretrained_picks_the_class(tmp_path, model_type, cls, ratio, bias, norms):
    st = pytest.importorskip("safetensors.torch")
    g = torch.Generator().manual_seed(2)
    state = {k: torch.randn(s, generator=g).half() for k, s in _hf_names(ratio, bias, norms).items()}
    st.save_file(state, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(_d(ratio, model_type=model_type)))
    m = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu")
    assert type(m) is cls
    a = m.model.layers[0].self_attn
    assert a.qk_kernel == (model_type != "llama")
    assert torch.equal(a.q_proj.weight, state["model.layers.0.self_attn.q_proj.weight"])
    if norms:
        assert torch.equal(a.q_norm.weight, state["model.layers.0.self_attn.q_norm.weight"])
    off = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu", qk_kernel=False)
    assert not off.model.layers[0].self_attn.qk_kernel
    with pytest.raises(KeyError):                               # a checkpoint that lacks a parameter is not loaded quietly
        state.pop("model.layers.1.self_attn.k_proj.weight")
        st.save_file(state, str(tmp_path / "model.safetensors"))
        LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu")


def test_head_norm_is_hf_qwen3_rmsnorm():
    """The torch path of the head norm, against the formula of HF's Qwen3RMSNorm written out, on fp16 inputs."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((2, 5, 3, 128), generator=g) * 3).half()
    w = (1 + 0.1 * torch.randn(128, generator=g)).half()
    h = x.to(torch.float32)
    variance = h.pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + 1e-6)
    assert torch.equal(head_norm(x, w, 1e-6), w * h.to(torch.float16))
