"""The tiny sparse models of tests/test_moe_w4_model_gpu.py: those of tests/tiny_moe_models.py with hidden and expert intermediate
multiples of 128 -- 2 layers, vocab 64, hidden 256, head_dim 128, 2 kv heads, group 32, residual 32.
  mixtral     8 experts, 2 per token, intermediate 128, 8 / 2 heads, every layer sparse
  qwen3_moe   16 experts, 4 per token, moe_intermediate 128, 16 / 2 heads, head norms, layer 0 dense (intermediate 512)"""
import torch

VOCAB = 64
FAMILIES = {
    "mixtral": dict(model_type="mixtral", num_attention_heads=8, num_local_experts=8, num_experts_per_tok=2, intermediate_size=128),
    "qwen3_moe": dict(model_type="qwen3_moe", num_attention_heads=16, num_experts=16, num_experts_per_tok=4, moe_intermediate_size=128,
                      intermediate_size=512, mlp_only_layers=[0], decoder_sparse_step=1, norm_topk_prob=True),
}
_PACKED = ("qweight", "scales", "mins")


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


def build_dense(family: str, seed: int, dtype=torch.float16):
    """The family's dense model on the GPU: matrices and expert stacks ~ N(0, 0.05), router rows ~ N(0, 0.3), head-norm weights
    around 1; every value exactly representable in bf16 and fp16 alike."""
    torch.manual_seed(seed)
    model = classes()[family](config(family))
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


def quantised(family: str, dense, group: int = 128, weight_bits=None, **kw):
    """The model of `dense` with 4-bit experts (and with `weight_bits=4` 4-bit dense layers): every QuantExperts is
    QuantExperts.from_dense of the dense model's stacks, every QuantLinear packed from its nn.Linear, everything else copied."""
    from kivi_amd.moe import QuantExperts
    from kivi_amd.wquant import QuantLinear
    dtype = next(dense.parameters()).dtype
    model = classes()[family](config(family, expert_bits=4, expert_group=group, weight_bits=weight_bits, weight_group=group, **kw))
    model = model.to(dtype).cuda().eval()
    src = dict(dense.named_modules())
    rest = dict(dense.state_dict())
    for name, m in model.named_modules():
        if isinstance(m, QuantExperts):
            m.load_state_dict(QuantExperts.from_dense(src[name].gate_up_proj.data, src[name].down_proj.data, group).state_dict())
            rest.pop(name + ".gate_up_proj")
            rest.pop(name + ".down_proj")
        elif isinstance(m, QuantLinear):
            m.pack_(src[name].weight.data, name + ".weight")
            rest.pop(name + ".weight")
    missing, unexpected = model.load_state_dict(rest, strict=False)
    assert not unexpected and all(k.rsplit(".", 1)[1] in _PACKED for k in missing), (missing, unexpected)
    return model


def fake_quant_twin(family: str, model):
    """The same class with dense experts (and nn.Linears) holding the 4-bit model's dequantised weights, its sparse blocks on the
    torch loop (moe_kernel off): the same arithmetic as the 4-bit model's, from dense stacks."""
    from kivi_amd.moe import QuantExperts
    from kivi_amd.wquant import QuantLinear
    dtype = next(model.parameters()).dtype
    other = classes()[family](config(family, moe_kernel=False)).to(dtype).cuda().eval()
    state = {k: v for k, v in model.state_dict().items() if k.rsplit(".", 1)[1] not in _PACKED}
    for name, m in model.named_modules():
        if isinstance(m, QuantExperts):
            both = [m.dequant_expert(e, dtype) for e in range(m.num_experts)]
            state[name + ".gate_up_proj"] = torch.stack([b[0] for b in both])
            state[name + ".down_proj"] = torch.stack([b[1] for b in both])
        elif isinstance(m, QuantLinear):
            state[name + ".weight"] = m.dequant(dtype)
    missing, unexpected = other.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return other


def hf_names(state: dict, family: str) -> dict:
    """A dense state dict with the sparse blocks under HF's per-expert checkpoint names (Mixtral: block_sparse_moe, w1 / w3 / w2)."""
    out = {}
    for name, t in state.items():
        if ".mlp.experts." in name:
            prefix = name[: name.index(".mlp.experts.")]
            mid = ".block_sparse_moe.experts." if family == "mixtral" else ".mlp.experts."
            gname, uname, dname = ("w1", "w3", "w2") if family == "mixtral" else ("gate_proj", "up_proj", "down_proj")
            for e in range(t.shape[0]):
                if name.endswith("gate_up_proj"):
                    inter = t.shape[1] // 2
                    out[f"{prefix}{mid}{e}.{gname}.weight"] = t[e, :inter].contiguous()
                    out[f"{prefix}{mid}{e}.{uname}.weight"] = t[e, inter:].contiguous()
                else:
                    out[f"{prefix}{mid}{e}.{dname}.weight"] = t[e].contiguous()
        elif name.endswith(".mlp.gate.weight") and family == "mixtral":
            out[name.replace(".mlp.", ".block_sparse_moe.")] = t
        else:
            out[name] = t
    return out


def prompts(seed: int, B: int, T: int):
    return torch.randint(1, VOCAB, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()
