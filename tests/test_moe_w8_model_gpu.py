"""GPU: sparse models with FP8 experts through the public interface.  tests/tiny_moe_fp8_models.py: the
Mixtral-like and the Qwen3-MoE-like model with an expert intermediate size of 128, fp16 and one bf16 case; `fp8_experts` alone and
together with `fp8_weights`.

Tree      every sparse block holds an Fp8Experts; its bytes are 0.5 of the fp16 experts' plus the scales.
Loading   from_pretrained of a written FP8 directory (save_quantized) and of the 16-bit directory with fp8_experts=True give the same
          buffers, those of the CPU restatement's quantiser.
Logits    per pass against the fake-quant twin -- dense experts (and linears) holding `dequant` of the same bytes, on the fp16
          expert kernels -- under shared routing (tests/test_w8_model_gpu.py's _SharedRouting), at that test's bars: 1e-2 of the
          rms in fp16, 5e-2 in bf16, over a 140-token prompt pass and 24 steps.  The tokens whose own routing differed are printed.
          As in that test the prompt pass of both models runs the torch loop (`moe_kernel_max_tokens=64`, the dense block's
          default, below the 140 tokens), the steps the kernels: the two then decode from the SAME 2-bit KV cache.  With the FP8
          block's own default (256) the prompt pass takes the kernel, its hidden states differ from the twin's loop by 0.0026 of
          the rms, and the 2-bit cache quantised from them is no continuous function of them: the first step was then 0.0131
          apart in the Mixtral-like fp16 model (measured on an MI355X) -- a property of comparing two caches, not of the kernel,
          whose own error the steps and tests/test_moe_w8_gpu.py hold.
Decoding  generate equals generate_graphed token for token from a whole-step capture; generate_continuous, eager and graphed,
          equals the restated policy of tests/test_admit_gpu.py."""
import functools
import json

import pytest
import torch

import tiny_moe_fp8_models as T
import w8_ref as R
from test_w8_model_gpu import _SharedRouting, _forced_logits

pytestmark = pytest.mark.gpu
T0, STEPS = 70, 24
CASES = [("mixtral", torch.float16, False), ("qwen3_moe", torch.float16, False), ("mixtral", torch.bfloat16, False),
         ("qwen3_moe", torch.float16, True)]
IDS = ["mixtral-fp16", "qwen3_moe-fp16", "mixtral-bf16", "qwen3_moe-fp16-fp8_weights"]


@functools.lru_cache(maxsize=None)
def _state(family, dtype):
    return T.dense_state(family, 50 + len(family), dtype)


@functools.lru_cache(maxsize=None)
def _model(family, dtype, both, max_tokens=None):
    """The model with FP8 experts (`both`: FP8 linears too), filled from the dense 16-bit state through the loader's quantising
    route.  `max_tokens`: moe_kernel_max_tokens (None: the FP8 block's default)."""
    from kivi_amd.loading import CheckpointLoader
    cfg = T.config(family, fp8_experts=True, fp8_weights=both, moe_kernel_max_tokens=max_tokens)
    model = T.classes()[family](cfg).to(dtype).cuda().eval()
    loader = CheckpointLoader(model, dtype)
    loader.take({k: v.cuda() for k, v in _state(family, dtype).items()})
    loader.finish()
    assert not loader.unexpected
    return model


def _twin(family, model):
    """The dense model of the same class whose experts and linears hold `dequant` of the FP8 model's bytes."""
    from kivi_amd.moe import Fp8Experts
    from kivi_amd.wfp8 import Fp8Linear
    dtype = next(model.parameters()).dtype
    other = T.classes()[family](T.config(family)).to(dtype).cuda().eval()
    mods = dict(model.named_modules())
    quant = {n for n, m in mods.items() if isinstance(m, (Fp8Experts, Fp8Linear))}
    state = {k: v for k, v in model.state_dict().items() if k.rsplit(".", 1)[0] not in quant}
    for n in quant:
        if isinstance(mods[n], Fp8Experts):
            state[n + ".gate_up_proj"], state[n + ".down_proj"] = mods[n].dequant(dtype)
        else:
            state[n + ".weight"] = mods[n].dequant(dtype)
    missing, unexpected = other.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return other


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("family,dtype,both", CASES, ids=IDS)
def test_module_tree_and_bytes(family, dtype, both):
    from kivi_amd.moe import Fp8Experts, SparseMoeBlock
    from kivi_amd.wfp8 import Fp8Linear
    model = _model(family, dtype, both)
    blocks = [layer.mlp for layer in model.model.layers if isinstance(layer.mlp, SparseMoeBlock)]
    assert len(blocks) == (2 if family == "mixtral" else 1)
    assert any(isinstance(m, Fp8Linear) for m in model.modules()) == both
    state = _state(family, dtype)
    for i, layer in enumerate(model.model.layers):
        if not isinstance(layer.mlp, SparseMoeBlock):
            continue
        ex = layer.mlp.experts
        assert isinstance(ex, Fp8Experts) and layer.mlp.expert_fp8 and layer.mlp.kernel and not list(ex.parameters())
        E, H, I = ex.num_experts, ex.hidden, ex.intermediate
        codes = sum(b.numel() * b.element_size() for n, b in ex.named_buffers() if not n.endswith("_scale_inv"))
        scales = sum(b.numel() * b.element_size() for n, b in ex.named_buffers() if n.endswith("_scale_inv"))
        fp16_bytes = 2 * 3 * E * H * I
        assert codes == fp16_bytes // 2 and scales == 4 * 3 * E * (H // 128) * (I // 128)
        assert all(b.is_cuda for b in ex.buffers()) and layer.mlp.gate.weight.dtype == dtype
        for name, stack in (("gate_up_proj", ex.gate_up_proj), ("down_proj", ex.down_proj)):       # the CPU restatement's bytes
            dense = state[f"model.layers.{i}.mlp.experts.{name}"]
            for e in (0, E - 1):
                q = [R.quantize_ref(m)[0] for m in ((dense[e],) if name == "down_proj" else (dense[e, :I], dense[e, I:]))]
                assert torch.equal(stack[e].cpu(), torch.cat(q)), (i, name, e)


@pytest.mark.parametrize("family,dtype,both", CASES, ids=IDS)
def test_from_pretrained_of_both_directories_gives_the_same_buffers(family, dtype, both, tmp_path):
    import safetensors.torch as st
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    want = _model(family, dtype, both)
    src = tmp_path / "dense"
    src.mkdir()
    st.save_file(T.hf_names(_state(family, dtype), family), str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps(T.config_dict(family)))
    from16 = LlamaForCausalLM_KIVI.from_pretrained(str(src), dtype=dtype, residual_length=32, fp8_experts=True, fp8_weights=both)
    assert type(from16) is T.classes()[family]
    _same_state(from16, want)
    dst = tmp_path / "fp8"
    from16.save_quantized(str(dst))
    saved = st.load_file(str(dst / "model.safetensors"))
    assert saved["model.layers.1.mlp.experts.3.up_proj.weight"].dtype == torch.float8_e4m3fn
    assert saved["model.layers.1.mlp.experts.3.up_proj.weight_scale_inv"].dtype == torch.float32
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(dst), dtype=dtype, residual_length=32, fp8_experts=True)
    assert type(loaded) is T.classes()[family]
    _same_state(loaded, want)


@pytest.mark.parametrize("family,dtype,both", CASES, ids=IDS)
def test_logits_against_the_fake_quant_twin(family, dtype, both, monkeypatch):
    from kivi_amd.moe import KERNEL_MAX_TOKENS, SparseMoeBlock
    model = _model(family, dtype, both, KERNEL_MAX_TOKENS)         # the prompt pass on the loop in both models: one KV cache
    twin = _twin(family, model)
    for m in (model, twin):
        assert all(b.kernel and b.kernel_max_tokens == KERNEL_MAX_TOKENS < 2 * T0 for b in m.modules() if isinstance(b, SparseMoeBlock))
    assert not any(k.endswith("_scale_inv") for k in twin.state_dict())
    ids = T.prompts(4, 2, T0)
    forced = torch.randint(1, T.VOCAB, (STEPS, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    shared = _SharedRouting(monkeypatch)
    b = _forced_logits(twin, ids, forced)
    shared.second_model()
    a = _forced_logits(model, ids, forced)
    assert len(shared.choices) == (2 if family == "mixtral" else 1) * len(a) and shared.replay == []
    bar = 1e-2 if dtype == torch.float16 else 5e-2
    worst = 0.0
    for s, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all() and x.dtype == y.dtype
        rms = y.float().pow(2).mean().sqrt().item()
        d = (x.float() - y.float()).abs().max().item() / rms
        worst = max(worst, d)
        print(f"pass {s}: {d:.3g}")
        assert d <= bar, (s, d)
    print(f"{family} {dtype} fp8_weights={both}: worst |FP8 experts - fake-quant twin| / rms over the prompt pass and {STEPS} steps = "
          f"{worst:.3g} (bar {bar}); tokens whose own routing differed from the twin's: {shared.differ}")


@pytest.mark.parametrize("family,dtype,both", CASES, ids=IDS)
def test_generate_graphed_and_continuous(family, dtype, both):
    import test_admit_gpu as AD
    model = _model(family, dtype, both)
    ids = T.prompts(3, 2, T0)
    eager = model.generate(ids, STEPS)
    graphed = model.generate_graphed(ids, STEPS)
    assert torch.equal(eager, graphed)
    eager_steps, captures, replays = model.graphs.stats
    assert model.graphs.whole and captures >= 1 and replays >= STEPS - 2 * captures - 4, model.graphs.stats
    assert eager.shape == (2, T0 + STEPS) and int(eager.min()) >= 0 and int(eager.max()) < T.VOCAB
    model.release_graphs()
    g = torch.Generator().manual_seed(9)
    lens, limits = [21, 5, 33, 47, 12], [4, 30, 9, 12, 6]
    prompts = [torch.randint(1, T.VOCAB, (n,), generator=g).tolist() for n in lens]
    want, landed = AD._restate(model, prompts, limits, 3)
    out = model.generate_continuous(prompts, limits, 3)
    assert [o.tolist() for o in out] == want and len(landed) > 3
    out = model.generate_continuous(prompts, limits, 3, graphed=True)
    assert [o.tolist() for o in out] == want
    model.release_graphs()
