"""The tiny random-weight models of tests/test_group_pad_gpu.py and tests/test_qwen_gpu.py: 2 layers, vocab 64, hidden 256, explicit
head_dim 128, 2 kv heads, group 32, residual 32."""
import torch

VOCAB = 64


def config(ratio: int, bits: int = 2, **kw):
    from kivi_amd.llama import make_config
    d = dict(hidden_size=256, num_attention_heads=2 * ratio, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=512,
             vocab_size=VOCAB, head_dim=128, rms_norm_eps=1e-6)
    return make_config(d, k_bits=bits, v_bits=bits, group_size=32, residual_length=32, **kw)


def build(cls, ratio: int, seed: int, bits: int = 2, **kw):
    """A model of `cls` on the GPU in fp16: matrices ~ N(0, 0.05), biases and head-norm weights drawn too (so that they matter)."""
    torch.manual_seed(seed)
    model = cls(config(ratio, bits, **kw)).half().cuda().eval()
    for name, p in model.named_parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.05)
        elif name.endswith("bias"):
            p.data.normal_(0.0, 0.1)
        elif "q_norm" in name or "k_norm" in name:
            p.data.normal_(1.0, 0.2)
    return model


def twin(cls, model, ratio: int, bits: int = 2, **kw):
    """The same weights under another configuration (qk_kernel off: the hook-state layout and the torch chain)."""
    other = cls(config(ratio, bits, **kw)).half().cuda().eval()
    missing, unexpected = other.load_state_dict(model.state_dict(), strict=False)
    assert not missing and not unexpected
    return other


def prompts(seed: int, B: int, T: int):
    return torch.randint(1, VOCAB, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()
