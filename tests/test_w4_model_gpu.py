"""GPU: models with 4-bit weights through the public interface.  tests/tiny_w4_models.py: a Llama-like in
fp16 and bf16, a Qwen2-like with biases and a padded query-group ratio, the Mixtral-like with only its attention quantised.

Loading   from_pretrained(weight_bits=4) from a safetensors checkpoint written by the test equals QuantLinear packing of the dense
          model, buffer for buffer; save_quantized then from_pretrained round-trips bit-identically and re-quantises nothing; an
          unknown layout tag raises.
Logits    per step against the fake-quant twin -- the same class with nn.Linears holding dequant() --: 1e-2 of the rms in fp16,
          5e-2 in bf16, the bars DESIGN.md section 29 uses for kernels against the torch statement.  The prompt pass (140 tokens)
          runs the dequantise + F.linear path, the steps the kernels.
Decoding  generate equals generate_graphed token for token from a whole-step capture; generate_continuous, eager and graphed, equals
          the restated policy of tests/test_admit_gpu.py.  These run with the kernel at every N (weight_kernel_max_tokens above any
          pass): a token's bits then do not depend on how the requests are batched, which is what the equalities need.
Memory    the buffers of every quantised module take O K / 2 + 4 O K / G bytes, and no dense `weight` remains on them."""
import functools
import json

import pytest
import torch

import tiny_w4_models as M

pytestmark = pytest.mark.gpu
T0, STEPS = 70, 24
CASES = [("llama", torch.float16, 128), ("llama", torch.bfloat16, 64), ("qwen2", torch.float16, 64), ("mixtral", torch.float16, 128)]
IDS = ["llama-fp16-g128", "llama-bf16-g64", "qwen2-fp16-g64", "mixtral-fp16-g128"]
ALWAYS = 1 << 20


@functools.lru_cache(maxsize=None)
def _dense(family, dtype):
    return M.build_dense(family, 40 + len(family), dtype)


@functools.lru_cache(maxsize=None)
def _model(family, dtype, group, kernel_max_tokens=None):
    return M.quantised(family, _dense(family, dtype), group, weight_kernel_max_tokens=kernel_max_tokens)


def _quant_modules(model):
    from kivi_amd.wquant import QuantLinear
    return {n: m for n, m in model.named_modules() if isinstance(m, QuantLinear)}


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("family,dtype,group", CASES, ids=IDS)
def test_module_tree_and_bytes(family, dtype, group):
    from kivi_amd import wquant
    from kivi_amd.moe import SparseMoeBlock
    model = _model(family, dtype, group)
    mods = _quant_modules(model)
    per_layer = 4 if family == "mixtral" else 7
    assert len(mods) == 2 * per_layer
    for layer in model.model.layers:
        assert type(layer.mlp) is (SparseMoeBlock if family == "mixtral" else wquant.QuantMLP)
        assert type(layer.self_attn.q_proj) is wquant.QuantLinear and (layer.self_attn.q_proj.bias is not None) == (family == "qwen2")
        assert layer.self_attn.o_proj.bias is None
    for name, m in mods.items():
        O, K = m.out_features, m.in_features
        got = sum(b.numel() * b.element_size() for b in m.buffers())
        assert got == O * K // 2 + 4 * O * K // group == wquant._lib.load().kivi_w4_bytes(O, K, group), name
        assert not hasattr(m, "weight") and all(b.is_cuda for b in m.buffers())
        assert not any(p.dim() > 1 for p in m.parameters())
    assert model.lm_head.weight.dtype == dtype and model.model.embed_tokens.weight.dtype == dtype
    if family == "mixtral":
        assert model.model.layers[0].mlp.experts.gate_up_proj.dtype == dtype


@pytest.mark.parametrize("family,dtype,group", CASES[:3], ids=IDS[:3])
def test_from_pretrained_packs_as_its_files_arrive_and_save_quantized_round_trips(family, dtype, group, tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd import wquant
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    dense = _dense(family, dtype)
    src = tmp_path / "dense"
    src.mkdir()
    state = {k: v.detach().cpu().contiguous() for k, v in dense.state_dict().items()}
    names = sorted(state)
    st.save_file({k: state[k] for k in names[::2]}, str(src / "model-00001-of-00002.safetensors"))     # two files
    st.save_file({k: state[k] for k in names[1::2]}, str(src / "model-00002-of-00002.safetensors"))
    (src / "config.json").write_text(json.dumps(M.config_dict(family)))
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(src), dtype=dtype, residual_length=32, weight_bits=4, weight_group=group,
                                                   weight_kernel_max_tokens=33)
    assert type(loaded) is M.classes()[family]
    want = _model(family, dtype, group)
    _same_state(loaded, want)
    mods = _quant_modules(loaded)
    assert len(mods) == 14 and all(m.kernel_max_tokens == 33 and m.group == group for m in mods.values())
    for name, m in mods.items():                                       # ... which is QuantLinear.from_linear of the dense model's module
        ref = wquant.QuantLinear.from_linear(dict(dense.named_modules())[name], group)
        for a, b in zip(m.triple, ref.triple):
            assert torch.equal(a, b), name
        assert (m.bias is None) == (ref.bias is None) and (m.bias is None or torch.equal(m.bias, ref.bias))
    # save_quantized -> from_pretrained: bit-identical, recognised by its tag, keywords not needed
    dst = tmp_path / "packed"
    loaded.save_quantized(str(dst))
    d = json.loads((dst / "config.json").read_text())
    assert (d["kivi_weight_bits"], d["kivi_weight_group"], d["kivi_weight_layout"]) == (4, group, wquant.LAYOUT)
    assert {k: v for k, v in d.items() if not k.startswith("kivi_weight")} == M.config_dict(family)
    packed = st.load_file(str(dst / "model.safetensors"))
    assert not any(k.endswith("_proj.weight") for k in packed) and "model.layers.1.self_attn.o_proj.qweight" in packed
    assert packed["model.layers.0.mlp.down_proj.scales"].dtype == torch.int16
    again = LlamaForCausalLM_KIVI.from_pretrained(str(dst), dtype=dtype, residual_length=32)
    assert type(again) is M.classes()[family]
    _same_state(again, loaded)
    d["kivi_weight_layout"] = "WT5"
    (dst / "config.json").write_text(json.dumps(d))
    with pytest.raises(ValueError, match="WT5"):
        LlamaForCausalLM_KIVI.from_pretrained(str(dst), dtype=dtype, residual_length=32)
    # a weight whose fp16 image is infinite is refused with the layer's name
    if dtype == torch.bfloat16:
        bad = dict(state)
        w = bad["model.layers.1.self_attn.k_proj.weight"].clone()
        w[0, 0] = 7e4
        bad["model.layers.1.self_attn.k_proj.weight"] = w
        for f in src.glob("*.safetensors"):
            f.unlink()
        st.save_file(bad, str(src / "model.safetensors"))
        with pytest.raises(ValueError, match="layers.1.self_attn.k_proj"):
            LlamaForCausalLM_KIVI.from_pretrained(str(src), dtype=dtype, residual_length=32, weight_bits=4, weight_group=group)


def _forced_logits(model, ids, forced):
    logits, past = model(ids)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past)
        out.append(logits)
    return out


@pytest.mark.parametrize("family,dtype,group", CASES, ids=IDS)
def test_logits_against_the_fake_quant_twin(family, dtype, group):
    model = _model(family, dtype, group)
    twin = M.fake_quant_twin(family, model)
    assert not any(k.endswith("qweight") for k in twin.state_dict())
    ids = M.prompts(4, 2, T0)
    forced = torch.randint(1, M.VOCAB, (STEPS, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    a, b = _forced_logits(model, ids, forced), _forced_logits(twin, ids, forced)
    bar = 1e-2 if dtype == torch.float16 else 5e-2
    worst = 0.0
    for s, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all() and x.dtype == y.dtype
        rms = y.float().pow(2).mean().sqrt().item()
        d = (x.float() - y.float()).abs().max().item() / rms
        worst = max(worst, d)
        assert d <= bar, (s, d)
    print(f"{family} {dtype} g{group}: worst |4-bit kernels - fake-quant twin| / rms over the prompt pass and {STEPS} steps = {worst:.3g}")


@pytest.mark.parametrize("family,dtype,group", CASES, ids=IDS)
def test_generate_graphed_and_continuous(family, dtype, group):
    import test_admit_gpu as AD
    model = _model(family, dtype, group, ALWAYS)
    assert all(m.kernel_max_tokens == ALWAYS for m in _quant_modules(model).values())
    ids = M.prompts(3, 2, T0)
    eager = model.generate(ids, STEPS)
    graphed = model.generate_graphed(ids, STEPS)
    assert torch.equal(eager, graphed)
    eager_steps, captures, replays = model.graphs.stats
    assert model.graphs.whole and captures >= 1 and replays >= STEPS - 2 * captures - 4, model.graphs.stats
    assert eager.shape == (2, T0 + STEPS) and int(eager.min()) >= 0 and int(eager.max()) < M.VOCAB
    model.release_graphs()
    g = torch.Generator().manual_seed(9)
    lens, limits = [21, 5, 33, 47, 12], [4, 30, 9, 12, 6]
    prompts = [torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in lens]
    want, landed = AD._restate(model, prompts, limits, 3)
    out = model.generate_continuous(prompts, limits, 3)
    assert [o.tolist() for o in out] == want and len(landed) > 3
    out = model.generate_continuous(prompts, limits, 3, graphed=True)
    assert [o.tolist() for o in out] == want
    model.release_graphs()
