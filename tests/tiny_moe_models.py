"""The tiny sparse models of tests/test_moe_gpu.py, shaped as tests/tiny_qk_models.py: 2 layers, vocab 64, hidden 256, head_dim 128,
2 kv heads, group 32, residual 32.
  mixtral     8 experts, 2 per token, intermediate 128, 8 / 2 heads (ratio 4), every layer sparse
  qwen3_moe   16 experts, 4 per token, moe_intermediate 96, 16 / 2 heads (ratio 8), head norms, layer 0 dense (mlp_only_layers) with
              intermediate 512, norm_topk_prob on"""
import torch

VOCAB = 64
FAMILIES = {
    "mixtral": dict(model_type="mixtral", num_attention_heads=8, num_local_experts=8, num_experts_per_tok=2, intermediate_size=128),
    "qwen3_moe": dict(model_type="qwen3_moe", num_attention_heads=16, num_experts=16, num_experts_per_tok=4, moe_intermediate_size=96,
                      intermediate_size=512, mlp_only_layers=[0], decoder_sparse_step=1, norm_topk_prob=True),
}


def config_dict(family: str) -> dict:
    return dict(hidden_size=256, num_key_value_heads=2, num_hidden_layers=2, vocab_size=VOCAB, head_dim=128, rms_norm_eps=1e-6,
                **FAMILIES[family])


def classes():
    from kivi_amd.llama import MixtralForCausalLM_KIVI, Qwen3MoeForCausalLM_KIVI
    return {"mixtral": MixtralForCausalLM_KIVI, "qwen3_moe": Qwen3MoeForCausalLM_KIVI}


def config(family: str, **kw):
    from kivi_amd.llama import make_config
    kw.setdefault("qk_kernel", family == "qwen3_moe")
    return make_config(config_dict(family), k_bits=2, v_bits=2, group_size=32, residual_length=32, **kw)


def build(family: str, seed: int, dtype=torch.float16, **kw):
    """A model of the family on the GPU: matrices and expert stacks ~ N(0, 0.05), router rows ~ N(0, 0.3) (so that the routing
    weights differ), head-norm weights around 1; every value exactly representable in bf16 and fp16 alike."""
    torch.manual_seed(seed)
    model = classes()[family](config(family, **kw))
    for name, p in model.named_parameters():
        if name.endswith("mlp.gate.weight"):
            p.data.normal_(0.0, 0.3)
        elif p.dim() > 1:
            p.data.normal_(0.0, 0.05)
        elif "q_norm" in name or "k_norm" in name:
            p.data.normal_(1.0, 0.2)
        t = p.data.bfloat16()
        p.data.copy_(torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t).float())
    return model.to(dtype).cuda().eval()


def twin(family: str, model, **kw):
    """The same weights under another configuration (moe_kernel off: the torch loop)."""
    other = classes()[family](config(family, **kw)).to(next(model.parameters()).dtype).cuda().eval()
    missing, unexpected = other.load_state_dict(model.state_dict(), strict=False)
    assert not missing and not unexpected
    return other


def prompts(seed: int, B: int, T: int):
    return torch.randint(1, VOCAB, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()
