"""GPU: sparse models with 4-bit experts through the public interface.  tests/tiny_moe_w4_models.py: the
Mixtral-like model in fp16 (G = 128) and bf16 (G = 64) with expert_bits=4 alone, the Qwen3-MoE-like one (one dense layer) with
expert_bits=4 and weight_bits=4 together.

Loading   from_pretrained(expert_bits=4) from a checkpoint under HF's per-expert names and under the fused names of transformers 5
          equals QuantExperts.from_dense of the dense model, buffer for buffer; no dense expert parameter is among
          named_parameters(); save_quantized then from_pretrained round-trips bit-identically and re-quantises nothing; a
          checkpoint that holds one expert's tensor twice and lacks another's is refused.
Logits    per step against the fake-quant twin -- the same class with dense experts holding the dequantised weights, on the torch
          loop --: 1e-2 of the rms in fp16, 5e-2 in bf16 (DESIGN.md section 30's bars).
Decoding  generate repeats itself; generate_continuous (eager: admission into living caches, left-padded batches) equals the
          restated policy of tests/test_admit_gpu.py.  (The graphed forms refuse such a model: tests/test_moe_w4_cpu.py.)"""
import functools
import json

import pytest
import torch

import tiny_moe_w4_models as M

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
T0, STEPS = 70, 12
MODEL_CASES = [("mixtral", F16, 128, None), ("mixtral", BF16, 64, None), ("qwen3_moe", F16, 64, 4)]
MODEL_IDS = ["mixtral-fp16-g128", "mixtral-bf16-g64", "qwen3_moe-fp16-g64-w4"]


@functools.lru_cache(maxsize=None)
def _dense(family, dtype):
    return M.build_dense(family, 50 + len(family), dtype)


@functools.lru_cache(maxsize=None)
def _model(family, dtype, group, weight_bits):
    return M.quantised(family, _dense(family, dtype), group, weight_bits)


def _quant_experts(model):
    from kivi_amd.moe import QuantExperts
    return {n: m for n, m in model.named_modules() if isinstance(m, QuantExperts)}


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("family,dtype,group,weight_bits", MODEL_CASES, ids=MODEL_IDS)
def test_module_tree_and_bytes(family, dtype, group, weight_bits):
    from kivi_amd import moe, wquant
    model = _model(family, dtype, group, weight_bits)
    mods = _quant_experts(model)
    assert len(mods) == (2 if family == "mixtral" else 1)
    assert not any(p.dim() == 3 for _, p in model.named_parameters())             # no dense expert parameter
    assert not any(n.endswith(("experts.gate_up_proj", "experts.down_proj")) for n, _ in model.named_parameters())
    lib = wquant._lib.load()
    for name, m in mods.items():
        E, H, I = m.num_experts, m.hidden, m.intermediate
        got = sum(b.numel() * b.element_size() for b in m.buffers())
        assert got == E * (lib.kivi_w4_bytes(2 * I, H, group) + lib.kivi_w4_bytes(H, I, group)), name
        assert all(b.is_cuda for b in m.buffers()) and m.group == group
    layer = model.model.layers[1]
    assert type(layer.mlp) is moe.SparseMoeBlock and layer.mlp.expert_bits == 4
    assert type(layer.self_attn.q_proj) is (torch.nn.Linear if weight_bits is None else wquant.QuantLinear)
    if family == "qwen3_moe":
        assert type(model.model.layers[0].mlp) is wquant.QuantMLP


@pytest.mark.parametrize("spelling", ["per-expert", "fused"])
@pytest.mark.parametrize("family,dtype,group,weight_bits", MODEL_CASES, ids=MODEL_IDS)
def test_from_pretrained_packs_the_experts_and_save_quantized_round_trips(family, dtype, group, weight_bits, spelling, tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd import wquant
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    from kivi_amd.moe import QuantExperts
    dense = _dense(family, dtype)
    src = tmp_path / "dense"
    src.mkdir()
    state = {k: v.detach().cpu().contiguous() for k, v in dense.state_dict().items()}
    if spelling == "per-expert":
        state = M.hf_names(state, family)
        assert not any(k.endswith("gate_up_proj") for k in state)
    else:
        assert "model.layers.1.mlp.experts.gate_up_proj" in state
    names = sorted(state)
    st.save_file({k: state[k] for k in names[::2]}, str(src / "model-00001-of-00002.safetensors"))     # two files
    st.save_file({k: state[k] for k in names[1::2]}, str(src / "model-00002-of-00002.safetensors"))
    (src / "config.json").write_text(json.dumps(M.config_dict(family)))
    kw = dict(weight_bits=weight_bits, weight_group=group) if weight_bits else {}
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(src), dtype=dtype, residual_length=32, expert_bits=4, expert_group=group, **kw)
    assert type(loaded) is M.classes()[family]
    _same_state(loaded, _model(family, dtype, group, weight_bits))
    mods = _quant_experts(loaded)
    assert mods and not any(p.dim() == 3 for _, p in loaded.named_parameters())
    for name, m in mods.items():                                        # ... which is from_dense of the dense model's stacks
        d = dict(dense.named_modules())[name]
        ref = QuantExperts.from_dense(d.gate_up_proj.data, d.down_proj.data, group)
        for (k, a), b in zip(m.state_dict().items(), ref.state_dict().values()):
            assert torch.equal(a, b), (name, k)
    if spelling == "fused":
        return
    # save_quantized -> from_pretrained: bit-identical, recognised by its tag, keywords not needed
    dst = tmp_path / "packed"
    loaded.save_quantized(str(dst))
    d = json.loads((dst / "config.json").read_text())
    assert (d["kivi_expert_bits"], d["kivi_expert_group"], d["kivi_weight_layout"]) == (4, group, wquant.LAYOUT)
    assert ("kivi_weight_bits" in d) == (weight_bits is not None)
    assert {k: v for k, v in d.items() if not k.startswith(("kivi_weight", "kivi_expert"))} == M.config_dict(family)
    packed = st.load_file(str(dst / "model.safetensors"))
    assert not any(k.endswith(("experts.gate_up_proj", "experts.down_proj")) for k in packed)
    assert packed["model.layers.1.mlp.experts.gate_up_proj.qweight"].dtype == torch.int32
    assert packed["model.layers.1.mlp.experts.down_proj.scales"].dtype == torch.int16
    again = LlamaForCausalLM_KIVI.from_pretrained(str(dst), dtype=dtype, residual_length=32)
    assert type(again) is M.classes()[family] and again.config.kivi_expert_bits == 4 and again.config.kivi_expert_group == group
    _same_state(again, loaded)


def _forced_logits(model, ids, forced):
    logits, past = model(ids)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past)
        out.append(logits)
    return out


@pytest.mark.parametrize("family,dtype,group,weight_bits", MODEL_CASES, ids=MODEL_IDS)
def test_logits_against_the_fake_quant_twin_and_decoding(family, dtype, group, weight_bits):
    model = _model(family, dtype, group, weight_bits)
    twin = M.fake_quant_twin(family, model)
    assert not any(k.endswith("qweight") for k in twin.state_dict()) and not twin.model.layers[1].mlp.kernel
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
    print(f"{family} {dtype} g{group} weight_bits={weight_bits}: worst |4-bit experts - fake-quant twin| / rms over the prompt pass "
          f"and {STEPS} steps = {worst:.3g}")
    out = model.generate(ids, STEPS)
    assert out.shape == (2, T0 + STEPS) and int(out.min()) >= 0 and int(out.max()) < M.VOCAB and torch.equal(out[:, :T0], ids)
    assert torch.equal(out, model.generate(ids, STEPS))                    # two runs: the same tokens


@pytest.mark.parametrize("family,dtype,group,weight_bits", MODEL_CASES, ids=MODEL_IDS)
def test_generate_continuous_equals_the_restated_policy(family, dtype, group, weight_bits):
    import test_admit_gpu as AD
    model = _model(family, dtype, group, weight_bits)
    g = torch.Generator().manual_seed(9)
    lens, limits = [21, 5, 33, 47, 12], [4, 30, 9, 12, 6]
    prompts = [torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in lens]
    want, landed = AD._restate(model, prompts, limits, 3)
    out = model.generate_continuous(prompts, limits, 3)
    assert [o.tolist() for o in out] == want and len(landed) > 3
    assert model.graphs is None


def test_a_checkpoint_that_repeats_one_expert_and_lacks_another_is_refused(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    family, dtype = "mixtral", F16
    state = M.hf_names({k: v.detach().cpu().contiguous() for k, v in _dense(family, dtype).state_dict().items()}, family)
    twice, lacking = "model.layers.1.block_sparse_moe.experts.2.w3.weight", "model.layers.1.block_sparse_moe.experts.5.w3.weight"
    del state[lacking]
    st.save_file(state, str(tmp_path / "model-00001-of-00002.safetensors"))
    st.save_file({twice: state[twice]}, str(tmp_path / "model-00002-of-00002.safetensors"))      # as many pieces as a whole stack
    (tmp_path / "config.json").write_text(json.dumps(M.config_dict(family)))
    with pytest.raises(KeyError, match="layers.1.mlp.experts.gate_up_proj"):
        LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), dtype=dtype, residual_length=32, expert_bits=4)
