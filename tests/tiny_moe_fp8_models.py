"""The tiny sparse models of tests/test_moe_w8_model_gpu.py and tests/test_moe_w8_cpu.py: tests/tiny_moe_models.py's two families with
an expert intermediate size the FP8 block scales serve (a multiple of 128).  2 layers, vocab 64, hidden 256, head_dim 128, 2 kv heads.
  mixtral     8 experts, 2 per token, intermediate 128, every layer sparse
  qwen3_moe   16 experts, 4 per token, moe_intermediate 128, head norms, layer 0 dense (mlp_only_layers) with intermediate 512"""
import torch

import tiny_moe_models as M

VOCAB = M.VOCAB
FAMILIES = {"mixtral": dict(M.FAMILIES["mixtral"]), "qwen3_moe": dict(M.FAMILIES["qwen3_moe"], moe_intermediate_size=128)}
classes, prompts = M.classes, M.prompts


def config_dict(family: str) -> dict:
    return dict(hidden_size=256, num_key_value_heads=2, num_hidden_layers=2, vocab_size=VOCAB, head_dim=128, rms_norm_eps=1e-6,
                **FAMILIES[family])


def config(family: str, **kw):
    from kivi_amd.llama import make_config
    kw.setdefault("qk_kernel", family == "qwen3_moe")
    return make_config(config_dict(family), k_bits=2, v_bits=2, group_size=32, residual_length=32, **kw)


def dense_state(family: str, seed: int, dtype=torch.float16) -> dict:
    """The state_dict, on the CPU, of a dense 16-bit model of the family: matrices and expert stacks ~ N(0, 0.05), router rows ~
    N(0, 0.3), head-norm weights around 1 (tiny_moe_models.build's statement), every value representable in bf16 and fp16 alike."""
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
    return {k: v.detach().to(dtype).contiguous() for k, v in model.state_dict().items() if not k.endswith("inv_freq")}


def hf_names(state: dict, family: str) -> dict:
    """A state dict with the sparse blocks under HF's per-expert checkpoint names: Mixtral's `block_sparse_moe.experts.{e}.w1 / w3 /
    w2`, Qwen3-MoE's `mlp.experts.{e}.gate_proj / up_proj / down_proj`."""
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
