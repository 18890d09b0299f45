"""No GPU: 4-bit experts (kivi_amd/moe.py QuantExperts) everywhere but on the device.

1. The ABI version is still 3.
2. Configuration: the default namespace and module tree are what they were; weight_bits=4 alone leaves `_Experts`; the state-dict
   names and shapes under expert_bits=4; dtype casts leave the integer buffers alone; the raises, those of the graphed entry
   points (before anything runs) and of a dtype the packed experts do not serve among them.
3. The torch path on the CPU: a QuantExperts filled through wquant.quantize_ref + from_ref, and SparseMoeBlock.forward in fp32
   bit-equal to experts_torch over the dequantised stacks."""
import pytest
import torch


def test_the_abi_version_stays_3():
    from kivi_amd import _lib
    assert _lib.load().kivi_abi_version() == 3 == _lib.ABI_VERSION


# ------------------------------------------------------------------------------------------------ configuration
def _cfg(**kw):
    d = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=384, vocab_size=64,
             head_dim=64, model_type="qwen3_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=128, mlp_only_layers=[0],
             norm_topk_prob=True)
    d.update(kw)
    return d


def _mixtral():
    return dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=128, vocab_size=64,
                head_dim=64, model_type="mixtral", num_local_experts=4, num_experts_per_tok=2)


def test_the_default_namespace_and_module_tree_are_unchanged():
    from kivi_amd import moe
    from kivi_amd.llama import MixtralForCausalLM_KIVI, Qwen3MoeForCausalLM_KIVI, make_config
    plain = make_config(_cfg())
    none = make_config(_cfg(), expert_bits=None, expert_group=64)
    assert vars(plain) == vars(none) and not any(k.startswith("kivi_expert") for k in vars(plain)) and "kivi_hf_config" not in vars(plain)
    a, b = Qwen3MoeForCausalLM_KIVI(plain), Qwen3MoeForCausalLM_KIVI(none)
    assert list(a.state_dict()) == list(b.state_dict()) and [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
    assert type(a.model.layers[1].mlp.experts) is moe._Experts
    assert "model.layers.1.mlp.experts.gate_up_proj" in a.state_dict() and "model.layers.1.mlp.experts.down_proj" in a.state_dict()
    assert not any(k.endswith(("qweight", "scales", "mins")) for k in a.state_dict())
    block = moe.SparseMoeBlock(256, 128, 4, 2)
    assert type(block.experts) is moe._Experts and block.kernel_max_tokens == moe.KERNEL_MAX_TOKENS and block.expert_bits is None
    mix = MixtralForCausalLM_KIVI(make_config(_mixtral()))
    assert all(type(layer.mlp.experts) is moe._Experts for layer in mix.model.layers)


def test_weight_bits_alone_leaves_the_experts_dense():
    from kivi_amd import moe, wquant
    from kivi_amd.llama import Qwen3MoeForCausalLM_KIVI, make_config
    cfg = make_config(_cfg(), weight_bits=4)
    assert not any(k.startswith("kivi_expert") for k in vars(cfg))
    model = Qwen3MoeForCausalLM_KIVI(cfg)
    assert type(model.model.layers[0].mlp) is wquant.QuantMLP and type(model.model.layers[1].mlp.experts) is moe._Experts
    assert model.model.layers[1].mlp.experts.gate_up_proj.dtype == torch.float32


@pytest.mark.parametrize("weight_bits", [None, 4])
def test_state_dict_names_and_shapes_under_expert_bits(weight_bits):
    from kivi_amd import moe, wquant
    from kivi_amd.llama import MLP, MixtralForCausalLM_KIVI, Qwen3MoeForCausalLM_KIVI, make_config
    cfg = make_config(_cfg(), expert_bits=4, expert_group=64, weight_bits=weight_bits)
    assert (cfg.kivi_expert_bits, cfg.kivi_expert_group) == (4, 64)
    assert hasattr(cfg, "kivi_weight_bits") == (weight_bits is not None) and cfg.kivi_hf_config == _cfg()
    model = Qwen3MoeForCausalLM_KIVI(cfg)
    assert type(model.model.layers[0].mlp) is (MLP if weight_bits is None else wquant.QuantMLP)
    assert type(model.model.layers[0].self_attn.q_proj) is (torch.nn.Linear if weight_bits is None else wquant.QuantLinear)
    block = model.model.layers[1].mlp
    assert type(block) is moe.SparseMoeBlock and type(block.experts) is moe.QuantExperts and block.expert_bits == 4
    assert (block.experts.num_experts, block.experts.hidden, block.experts.intermediate, block.experts.group) == (4, 256, 128, 64)
    state = model.state_dict()
    pre = "model.layers.1.mlp.experts."
    want = {"gate_up_proj.qweight": ((4, 16, 2, 256), torch.int32), "gate_up_proj.scales": ((4, 16, 4, 16), torch.int16),
            "gate_up_proj.mins": ((4, 16, 4, 16), torch.int16), "down_proj.qweight": ((4, 16, 1, 256), torch.int32),
            "down_proj.scales": ((4, 16, 2, 16), torch.int16), "down_proj.mins": ((4, 16, 2, 16), torch.int16)}
    assert sorted(k[len(pre):] for k in state if k.startswith(pre)) == sorted(want)
    for k, (shape, dtype) in want.items():
        assert tuple(state[pre + k].shape) == shape and state[pre + k].dtype == dtype, k
    assert "model.layers.1.mlp.gate.weight" in state
    assert not any(p.dim() == 3 for _, p in model.named_parameters())          # no dense expert parameter
    assert [n for n, _ in block.named_parameters()] == ["gate.weight"]
    # Mixtral: every layer sparse
    mix = MixtralForCausalLM_KIVI(make_config(_mixtral(), expert_bits=4))
    assert all(type(layer.mlp.experts) is moe.QuantExperts and layer.mlp.experts.group == 128 for layer in mix.model.layers)


def test_casts_leave_the_integer_buffers_alone():
    from kivi_amd import moe
    block = moe.SparseMoeBlock(256, 128, 4, 2, expert_bits=4, expert_group=128)
    g = torch.Generator().manual_seed(2)
    for stack in (block.experts.gate_up_proj, block.experts.down_proj):
        stack.qweight.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, stack.qweight.shape, generator=g, dtype=torch.int64).to(torch.int32))
        stack.scales.copy_(torch.randint(-2 ** 15, 2 ** 15 - 1, stack.scales.shape, generator=g, dtype=torch.int64).to(torch.int16))
        stack.mins.copy_(torch.randint(-2 ** 15, 2 ** 15 - 1, stack.mins.shape, generator=g, dtype=torch.int64).to(torch.int16))
    before = {k: v.clone() for k, v in block.experts.state_dict().items()}
    assert len(before) == 6
    for cast in (lambda m: m.bfloat16(), lambda m: m.half(), lambda m: m.to(torch.bfloat16), lambda m: m.float()):
        m = cast(block)
        for k, v in m.experts.state_dict().items():
            assert v.dtype == before[k].dtype and torch.equal(v, before[k]), k
    assert block.gate.weight.dtype == torch.float32


def test_the_raises_name_the_field():
    from kivi_amd import moe
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen3MoeForCausalLM_KIVI, make_config
    with pytest.raises(ValueError, match="hidden_size"):
        moe.SparseMoeBlock(192, 128, 4, 2, expert_bits=4)
    with pytest.raises(ValueError, match="intermediate_size"):
        moe.SparseMoeBlock(256, 96, 4, 2, expert_bits=4)
    with pytest.raises(ValueError, match="expert_group"):
        moe.SparseMoeBlock(256, 128, 4, 2, expert_bits=4, expert_group=32)
    with pytest.raises(ValueError, match="expert_bits"):
        moe.SparseMoeBlock(256, 128, 4, 2, expert_bits=2)
    for bad in (2, 3, 8, "4", 0):
        with pytest.raises(ValueError, match="expert_bits"):
            make_config(_cfg(), expert_bits=bad)
    with pytest.raises(ValueError, match="expert_group"):
        make_config(_cfg(), expert_bits=4, expert_group=32)
    dense = {k: v for k, v in _cfg().items() if k not in ("num_experts", "num_experts_per_tok", "moe_intermediate_size",
                                                          "mlp_only_layers", "norm_topk_prob", "model_type")}
    with pytest.raises(ValueError, match="expert_bits"):                    # a config without experts
        make_config(dense, expert_bits=4)
    with pytest.raises(ValueError, match="intermediate_size"):              # the model's constructor reaches the same refusal
        Qwen3MoeForCausalLM_KIVI(make_config(_cfg(moe_intermediate_size=96), expert_bits=4))
    with pytest.raises(ValueError, match="expert_bits"):                    # save_quantized with neither keyword
        LlamaForCausalLM_KIVI(make_config(dense)).save_quantized("unused")


def test_graphed_entry_points_refuse_before_anything_runs(monkeypatch):
    from kivi_amd.llama import Qwen3MoeForCausalLM_KIVI, make_config
    model = Qwen3MoeForCausalLM_KIVI(make_config(_cfg(), expert_bits=4)).eval()

    def never(*a, **k):
        raise AssertionError("a pass of the model ran before the refusal")
    monkeypatch.setattr(model, "forward", never)
    monkeypatch.setattr(model, "_hidden", never)
    monkeypatch.setattr(torch.cuda, "graph", never)
    ids = torch.ones((2, 5), dtype=torch.long)
    for call in (lambda: model.generate_graphed(ids, 4), lambda: model.decode_graphed(ids[:, :1], [], 5, 2),
                 lambda: model.prepare_graphs(2, "cpu", whole=True),
                 lambda: model.generate_continuous([[1, 2, 3], [4, 5]], [3, 3], 2, graphed=True)):
        with pytest.raises(ValueError, match="expert_bits=4"):
            call()
    assert model.graphs is None


def test_a_dtype_the_packed_experts_do_not_serve_is_named(tmp_path):
    import json
    from kivi_amd import moe
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    q = moe.QuantExperts(2, 128, 128, 64)
    with pytest.raises(ValueError, match="float32"):
        q.pack_expert_(0, "down", torch.zeros(128, 128), "experts.0.down")
    (tmp_path / "config.json").write_text(json.dumps(_cfg()))
    with pytest.raises(ValueError, match="float32"):
        LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu", dtype=torch.float32, expert_bits=4)


# ------------------------------------------------------------------------------------------------ the torch path on the CPU
@pytest.mark.parametrize("group", [64, 128])
@pytest.mark.parametrize("E,K,H,I", [(8, 2, 128, 128), (12, 4, 256, 384)])
def test_the_block_on_the_cpu_equals_experts_torch_over_the_dequantised_stacks(E, K, H, I, group):
    from kivi_amd import moe, wquant
    torch.manual_seed(E + H + group)
    block = moe.SparseMoeBlock(H, I, E, K, norm_topk=True, expert_bits=4, expert_group=group).eval()
    gate_up = torch.randn(E, 2 * I, H) * 0.08
    down = torch.randn(E, H, I) * 0.08
    down[1] = 0.0                                                           # an all-zero expert: scale 0 everywhere
    gate_up[2, :, :group] = 0.25                                            # constant groups
    q = block.experts
    for e in range(E):
        q.load_ref_(e, "gate", *wquant.quantize_ref(gate_up[e, :I], group))
        q.load_ref_(e, "up", *wquant.quantize_ref(gate_up[e, I:], group))
        q.load_ref_(e, "down", *wquant.quantize_ref(down[e], group))
    # gate and up packed separately are the (2 I, H) matrix packed whole; from_dense does the same off the GPU
    whole = moe.QuantExperts.from_dense(gate_up, down, group)
    for a, b in zip((*q.gate_up_proj.triple, *q.down_proj.triple), (*whole.gate_up_proj.triple, *whole.down_proj.triple)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for e in (0, E - 1):
        ref = wquant.from_ref(*wquant.quantize_ref(gate_up[e], group), group)
        for a, b in zip(q.slab(e, "gate_up"), ref):
            assert torch.equal(a, b)
    dq_gu = torch.stack([q.dequant_expert(e, torch.float32)[0] for e in range(E)])
    dq_dn = torch.stack([q.dequant_expert(e, torch.float32)[1] for e in range(E)])
    assert tuple(dq_gu.shape) == (E, 2 * I, H) and tuple(dq_dn.shape) == (E, H, I) and dq_gu.dtype == torch.float32
    assert bool((dq_dn[1] == 0).all()) and bool((dq_gu[2, :, :group] == 0.25).all())
    step = (gate_up[0].half().float().reshape(2 * I, H // group, group).amax(-1) -
            gate_up[0].half().float().reshape(2 * I, H // group, group).amin(-1)) / 15
    err = (dq_gu[0] - gate_up[0]).abs().reshape(2 * I, H // group, group).amax(-1)
    assert bool((err <= 0.51 * step + 1e-3 * gate_up[0].abs().max()).all())    # half a step plus fp16 roundings of scale and mn
    with torch.no_grad():
        x = torch.randn(3, 7, H)
        got = block(x)
        x2 = x.reshape(21, H)
        plan = moe.route_torch(torch.nn.functional.linear(x2, block.gate.weight), K, True, False)
        want = moe.experts_torch(x2, plan, dq_gu, dq_dn)
    assert got.dtype == torch.float32 and torch.isfinite(got).all() and torch.equal(got.view(21, H), want)
    assert torch.equal(moe.experts_w4_torch(x2, plan, q), want)
