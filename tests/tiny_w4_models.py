"""The tiny models of tests/test_w4_model_gpu.py, shaped as tests/tiny_qk_models.py / tests/tiny_moe_models.py: 2 layers, vocab 64,
hidden 256, head_dim 128, 2 kv heads, intermediate 512 (every reduction length a multiple of 128), group 32, residual 32.
  llama     8 / 2 heads (ratio 4), no biases
  qwen2     14 / 2 heads (ratio 7, run padded to 8), a bias on q / k / v
  mixtral   8 / 2 heads, 8 experts of intermediate 128, 2 per token: with weight_bits=4 only its attention is quantised"""
import torch

VOCAB = 64
FAMILIES = {
    "llama": dict(model_type="llama", num_attention_heads=8, intermediate_size=512),
    "qwen2": dict(model_type="qwen2", num_attention_heads=14, intermediate_size=512),
    "mixtral": dict(model_type="mixtral", num_attention_heads=8, num_local_experts=8, num_experts_per_tok=2, intermediate_size=128),
}


def config_dict(family: str) -> dict:
    return dict(hidden_size=256, num_key_value_heads=2, num_hidden_layers=2, vocab_size=VOCAB, head_dim=128, rms_norm_eps=1e-6,
                **FAMILIES[family])


def classes():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, MixtralForCausalLM_KIVI, Qwen2ForCausalLM_KIVI
    return {"llama": LlamaForCausalLM_KIVI, "qwen2": Qwen2ForCausalLM_KIVI, "mixtral": MixtralForCausalLM_KIVI}


def config(family: str, **kw):
    from kivi_amd.llama import make_config
    kw.setdefault("qk_kernel", family == "qwen2")
    return make_config(config_dict(family), k_bits=2, v_bits=2, group_size=32, residual_length=32, **kw)


def build_dense(family: str, seed: int, dtype=torch.float16):
    """The family's model with dense weights on the GPU: matrices ~ N(0, 0.05), router rows ~ N(0, 0.3), biases ~ N(0, 0.1); every
    value exactly representable in bf16 and fp16 alike."""
    torch.manual_seed(seed)
    model = classes()[family](config(family))
    for name, p in model.named_parameters():
        if name.endswith("mlp.gate.weight"):
            p.data.normal_(0.0, 0.3)
        elif p.dim() > 1:
            p.data.normal_(0.0, 0.05)
        elif name.endswith("bias"):
            p.data.normal_(0.0, 0.1)
        t = p.data.bfloat16()
        p.data.copy_(torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t).float())
    return model.to(dtype).cuda().eval()


def quantised(family: str, dense, group: int = 128, **kw):
    """The 4-bit model of `dense`: the same class built with weight_bits=4, every QuantLinear packed from the dense model's
    nn.Linear by QuantLinear.from_linear's route (pack_), everything else copied."""
    from kivi_amd.wquant import QuantLinear
    dtype = next(dense.parameters()).dtype
    model = classes()[family](config(family, weight_bits=4, weight_group=group, **kw)).to(dtype).cuda().eval()
    src = dict(dense.named_modules())
    rest = dict(dense.state_dict())
    for name, m in model.named_modules():
        if isinstance(m, QuantLinear):
            m.pack_(src[name].weight.data, name + ".weight")
            rest.pop(name + ".weight")
    missing, unexpected = model.load_state_dict(rest, strict=False)
    assert not unexpected and all(k.rsplit(".", 1)[1] in ("qweight", "scales", "mins") for k in missing), (missing, unexpected)
    return model


def fake_quant_twin(family: str, model):
    """The same class with nn.Linears holding the 4-bit model's dequantised weights."""
    from kivi_amd.wquant import QuantLinear
    dtype = next(model.parameters()).dtype
    other = classes()[family](config(family)).to(dtype).cuda().eval()
    state = {k: v for k, v in model.state_dict().items() if k.rsplit(".", 1)[1] not in ("qweight", "scales", "mins")}
    for name, m in model.named_modules():
        if isinstance(m, QuantLinear):
            state[name + ".weight"] = m.dequant(dtype)
    missing, unexpected = other.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return other


def prompts(seed: int, B: int, T: int):
    return torch.randint(1, VOCAB, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()
