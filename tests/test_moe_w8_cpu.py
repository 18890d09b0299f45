"""CPU: the FP8 expert block without a GPU.
  - the buffers of Fp8Experts: shapes, dtypes, names; casts leave the scale bits alone;
  - quantize_expert_ equals w8_ref.quantize_ref bit for bit per matrix, stacked gate_up equals gate and up apart;
  - experts_w8_torch in fp32 against the fp64 restatement on the represented weights (tests/moe_w8_ref.py);
  - the loader: per-expert, fused and Mixtral spellings, the halves over files in both orders, a 16-bit directory with the flag, a
    missing scale; every refusal by name; save_quantized round-trips to identical bytes under the stated names and config block;
  - the C entry: symbol, signature, and every KIVI_EINVAL / KIVI_EALIGN with fake pointers (nothing is enqueued);
  - tests/moe_w8_plan_main.cpp built with -fsanitize=address,undefined and run."""
import json
import os
import shutil
import subprocess

import pytest
import torch

import moe_ref
import moe_w8_ref as W
import tiny_moe_fp8_models as T
import w8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 16, 0x110
P = 0x10000          # a fake, 16-byte aligned pointer: a refused call never follows it
FP8 = torch.float8_e4m3fn


def _lib():
    from kivi_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------------------------- the module
def test_buffers_names_shapes_and_casts():
    from kivi_amd import moe
    m = moe.Fp8Experts(4, 256, 384)
    sd = m.state_dict()
    assert sorted(sd) == ["down_proj", "down_proj_scale_inv", "gate_up_proj", "gate_up_proj_scale_inv"] and not list(m.parameters())
    assert tuple(sd["gate_up_proj"].shape) == (4, 768, 256) and sd["gate_up_proj"].dtype == torch.uint8
    assert tuple(sd["gate_up_proj_scale_inv"].shape) == (4, 6, 2) and sd["gate_up_proj_scale_inv"].dtype == torch.int32
    assert tuple(sd["down_proj"].shape) == (4, 256, 384) and sd["down_proj"].dtype == torch.uint8
    assert tuple(sd["down_proj_scale_inv"].shape) == (4, 2, 3) and sd["down_proj_scale_inv"].dtype == torch.int32
    gu, gus, dn, dns = W.random_experts(4, 256, 384, 3)
    for e in range(4):
        m.load_expert_(e, "gate", gu[e, :384].view(FP8), gus[e, :3]).load_expert_(e, "up", gu[e, 384:].view(FP8), gus[e, 3:])
        m.load_expert_(e, "down", dn[e].view(FP8), dns[e])
    assert torch.equal(m.gate_up_proj, gu) and torch.equal(m.down_proj, dn)
    assert torch.equal(m.gate_up_proj_scale_inv.view(torch.float32), gus) and torch.equal(m.down_proj_scale_inv.view(torch.float32), dns)
    for cast in (lambda t: t.half(), lambda t: t.bfloat16(), lambda t: t.to(torch.float64), lambda t: t.float()):
        c = cast(moe.Fp8Experts(4, 256, 384).load_expert_(1, "gate_up", gu[1].view(FP8), gus[1]))
        assert c.gate_up_proj_scale_inv.dtype == torch.int32 and torch.equal(c.gate_up_proj_scale_inv[1].view(torch.float32), gus[1])
        assert c.gate_up_proj.dtype == torch.uint8 and torch.equal(c.gate_up_proj[1], gu[1])
    # a per-tensor scalar is expanded to the grid
    m.load_expert_(2, "down", scale=torch.tensor(0.25))
    assert torch.equal(m.down_proj_scale_inv[2].view(torch.float32), torch.full((2, 3), 0.25))
    # dequant_expert off the GPU: wfp8.dequant_torch, the represented weight rounded to fp32 and then to the dtype
    g32, d32 = m.dequant_expert(1, torch.float32)
    assert torch.equal(g32, R.represented(gu[1], gus[1]).float()) and torch.equal(d32, R.represented(dn[1], dns[1]).float())
    outs = (torch.empty((768, 256), dtype=torch.float16), torch.empty((256, 384), dtype=torch.float16))
    got = m.dequant_expert(1, torch.float16, outs)
    assert got[0] is outs[0] and torch.equal(outs[0], R.represented(gu[1], gus[1]).float().half())
    block = moe.SparseMoeBlock(256, 384, 4, 2, expert_fp8=True)
    assert isinstance(block.experts, moe.Fp8Experts) and block.expert_fp8 and block.kernel_max_tokens == moe.FP8_KERNEL_MAX_TOKENS
    assert sorted(k for k in block.state_dict()) == ["experts.down_proj", "experts.down_proj_scale_inv", "experts.gate_up_proj",
                                                     "experts.gate_up_proj_scale_inv", "gate.weight"]
    assert not block.uses_kernel(torch.zeros((3, 256), dtype=torch.float16))       # off the GPU: the loop


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_quantize_expert_equals_the_reference_quantiser(dtype):
    from kivi_amd import moe
    E, H, I = 2, 256, 128
    g = torch.Generator().manual_seed(5)
    gate_up = (torch.randn((E, 2 * I, H), generator=g) * 0.05).to(dtype)
    down = (torch.randn((E, H, I), generator=g) * 0.05).to(dtype)
    gate_up[1, I:I + 128, :128] = 0                                                  # an all-zero block: scale 1
    m = moe.Fp8Experts.from_dense(gate_up, down)
    apart = moe.Fp8Experts(E, H, I)
    for e in range(E):
        apart.quantize_expert_(e, "gate", gate_up[e, :I]).quantize_expert_(e, "up", gate_up[e, I:]).quantize_expert_(e, "down", down[e])
        for part, w in (("gate_up", gate_up[e]), ("gate", gate_up[e, :I]), ("up", gate_up[e, I:]), ("down", down[e])):
            codes, inv = R.quantize_ref(w)
            got_codes, got_bits = m.slab(e, part)
            assert torch.equal(got_codes, codes) and torch.equal(got_bits.view(torch.float32), inv), (e, part)
    for k, v in m.state_dict().items():
        assert torch.equal(v, apart.state_dict()[k]), k
    assert float(m.slab(1, "up")[1].view(torch.float32)[0, 0]) == 1.0


@pytest.mark.parametrize("E,K,H,I,N", [(8, 2, 256, 128, 37), (12, 4, 384, 256, 9)])
def test_the_eager_loop_in_fp32_against_the_fp64_restatement(E, K, H, I, N):
    """fp32 rounds a sum of n terms with a relative error near sqrt(n) * 2^-24 (n <= H + I = 640: 1.5e-6) of the terms' magnitude,
    which cancellation makes at most some tens of the result's rms: 1e-4 of the rms is two orders above what a correct loop gives
    and four below what a wrong block scale (order one) gives."""
    from kivi_amd import moe
    gu, gus, dn, dns = W.random_experts(E, H, I, 11)
    m = moe.Fp8Experts(E, H, I)
    for e in range(E):
        m.load_expert_(e, "gate_up", gu[e].view(FP8), gus[e]).load_expert_(e, "down", dn[e].view(FP8), dns[e])
    g = torch.Generator().manual_seed(N)
    x = torch.randn((N, H), generator=g)
    plan = moe.route_torch(torch.randn((N, E), generator=g), K, True, False)
    got = moe.experts_w8_torch(x, plan, m)
    ref, a_max = W.experts_w8_ref(x, plan.idx.long(), plan.w, gu, gus, dn, dns)
    assert got.dtype == torch.float32 and a_max < 65504 / 16 and float(ref.abs().max()) < 65504 / 16
    worst = float((got.double() - ref).abs().max() / ref.pow(2).mean().sqrt())
    assert worst <= 1e-4, worst
    stacks = W.represented_stacks(gu, gus, dn, dns)                                  # the same reference through moe_ref's statement
    assert torch.allclose(moe_ref.experts_ref(x, plan.idx.long(), plan.w, *stacks), ref, rtol=0, atol=1e-9)
    # the block, off the GPU: the same loop behind the router
    block = moe.SparseMoeBlock(H, I, E, K, expert_fp8=True)
    block.experts.load_state_dict(m.state_dict())
    y = block(x.view(1, N, H))
    plan2 = moe.route_torch(torch.nn.functional.linear(x, block.gate.weight), K, True, False)
    assert torch.equal(y.view(N, H), moe.experts_w8_torch(x, plan2, block.experts))


def test_the_gpu_tests_inputs_stay_inside_a_sixteenth_of_fp16():
    """The largest of tests/test_moe_w8_gpu.py's cases, in fp64 on the CPU: H = 640, I = 384, every token to one expert."""
    from kivi_amd import moe
    E, K, H, I, N = 8, 2, 640, 384, 64
    bufs = W.random_experts(E, H, I, 7 + H + I + E)
    lg = moe_ref.crafted_logits(moe_ref.crafted_assignment(N, E, K, "one", 16), E, 200 + N + E, torch.float16)
    x = torch.randn((N, H), generator=torch.Generator().manual_seed(N + E + I)).half()
    plan = moe.route_torch(lg, K, True, False)
    ref, a_max = W.experts_w8_ref(x, plan.idx.long(), plan.w, *bufs)
    assert a_max < 65504 / 16 and float(ref.abs().max()) < 65504 / 16 and float(ref.pow(2).mean().sqrt()) > 0.05


def test_module_refusals_by_name():
    from kivi_amd import moe
    with pytest.raises(ValueError, match="intermediate_size to be a positive multiple of 128, got 96"):
        moe.Fp8Experts(4, 256, 96)
    with pytest.raises(ValueError, match="hidden_size to be a positive multiple of 128, got 192"):
        moe.SparseMoeBlock(192, 128, 4, 2, expert_fp8=True)
    with pytest.raises(ValueError, match="expert_fp8 and expert_bits=4"):
        moe.SparseMoeBlock(256, 128, 4, 2, expert_bits=4, expert_fp8=True)
    m = moe.Fp8Experts(4, 256, 128)
    nan = torch.zeros((128, 256), dtype=torch.uint8)
    nan[3, 5] = 0xFF
    with pytest.raises(ValueError, match="experts.1.gate.weight: the FP8 weight holds a NaN byte"):
        m.load_expert_(1, "gate", nan.view(FP8), name="experts.1.gate.weight")
    with pytest.raises(ValueError, match="s_inv: a scale is not finite"):
        m.load_expert_(1, "gate", scale=torch.tensor([[1.0, float("inf")]]), name="s_inv")
    with pytest.raises(ValueError, match="s_inv: fp32 scales are needed"):
        m.load_expert_(1, "gate", scale=torch.ones((1, 2), dtype=torch.uint8), name="s_inv")
    with pytest.raises(ValueError, match=r"s_inv: shape \(2, 2\) does not fit"):
        m.load_expert_(1, "gate", scale=torch.ones((2, 2)), name="s_inv")
    with pytest.raises(ValueError, match=r"w: shape \(256, 128\) does not fit the gate matrix \(128, 256\)"):
        m.load_expert_(1, "gate", torch.zeros((256, 128), dtype=FP8), name="w")
    with pytest.raises(ValueError, match="w: expert 4 outside"):
        m.load_expert_(4, "down", torch.zeros((256, 128), dtype=FP8), name="w")
    with pytest.raises(ValueError, match="part has to be"):
        m.load_expert_(0, "w1", torch.zeros((256, 128), dtype=FP8))
    with pytest.raises(ValueError, match="w: the weight is not finite"):
        m.quantize_expert_(0, "down", torch.full((256, 128), float("nan")), "w")
    with pytest.raises(ValueError, match=r"w: shape \(128, 128\)"):
        m.quantize_expert_(0, "down", torch.zeros((128, 128)), "w")
    with pytest.raises(Exception, match="GPU"):
        moe.experts_w8(torch.zeros((2, 256), dtype=torch.float16), moe.route_torch(torch.zeros((2, 4)), 2), m)


# ------------------------------------------------------------------------------------------------------------- make_config
def test_make_config_flag_and_its_refusals():
    from kivi_amd.llama import make_config
    from kivi_amd.moe import Fp8Experts
    d = T.config_dict("qwen3_moe")
    assert not hasattr(make_config(d), "kivi_fp8_experts")
    cfg = make_config(d, fp8_experts=True)
    assert cfg.kivi_fp8_experts is True and not hasattr(cfg, "kivi_fp8_weights") and cfg.kivi_hf_config == d
    both = make_config(d, fp8_experts=True, fp8_weights=True)
    assert both.kivi_fp8_experts and both.kivi_fp8_weights
    with pytest.raises(ValueError, match="fp8_experts and expert_bits=4"):
        make_config(d, fp8_experts=True, expert_bits=4)
    with pytest.raises(ValueError, match="fp8_experts together with weight_bits=4"):
        make_config(d, fp8_experts=True, weight_bits=4)
    dense = {k: v for k, v in d.items() if k not in ("num_experts", "num_experts_per_tok", "moe_intermediate_size", "mlp_only_layers")}
    with pytest.raises(ValueError, match="fp8_experts: the config has no experts"):
        make_config(dict(dense, model_type="qwen3"), fp8_experts=True)
    with pytest.raises(ValueError, match="intermediate_size to be a positive multiple of 128, got 96"):
        T.classes()["qwen3_moe"](make_config(dict(d, moe_intermediate_size=96), fp8_experts=True))
    model = T.classes()["mixtral"](make_config(T.config_dict("mixtral"), fp8_experts=True))
    assert all(isinstance(layer.mlp.experts, Fp8Experts) for layer in model.model.layers)
    model._refuse_capture("generate_graphed")                                        # no refusal: the block has a capturable form


# ------------------------------------------------------------------------------------------------------------------ loader
DTYPE = torch.float16


def _load(path, **kw):
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    return LlamaForCausalLM_KIVI.from_pretrained(str(path), device="cpu", dtype=DTYPE, **kw)


def _fp8_expert_state(state: dict, family: str, spelling: str) -> dict:
    """A dense state_dict -> the checkpoint of it with FP8 experts (tests/w8_ref.quantize_ref per matrix): `per_expert` under the
    family's per-expert names, `fused` under transformers 5's stacked names."""
    out = {}
    if spelling == "fused":
        for k, v in state.items():
            if k.endswith((".experts.gate_up_proj", ".experts.down_proj")):
                I = v.shape[2] if k.endswith("down_proj") else v.shape[1] // 2
                qs = [[R.quantize_ref(m) for m in ((v[e],) if k.endswith("down_proj") else (v[e, :I], v[e, I:]))] for e in range(v.shape[0])]
                out[k] = torch.stack([torch.cat([c for c, _ in q]) for q in qs]).view(FP8)
                out[k + "_scale_inv"] = torch.stack([torch.cat([s for _, s in q]) for q in qs])
            else:
                out[k] = v
        return out
    for k, v in T.hf_names(state, family).items():
        if ".experts." in k:
            codes, inv = R.quantize_ref(v)
            out[k] = codes.view(FP8)
            out[k[: -len("weight")] + "weight_scale_inv"] = inv
        else:
            out[k] = v
    return out


def _expected_buffers(state: dict) -> dict:
    """name -> the bytes / scale bits the model's Fp8Experts must hold for the dense `state`."""
    want = {}
    for k, v in state.items():
        if k.endswith((".experts.gate_up_proj", ".experts.down_proj")):
            I = v.shape[1] // 2
            parts = (lambda e: (v[e],)) if k.endswith("down_proj") else (lambda e: (v[e, :I], v[e, I:]))
            qs = [[R.quantize_ref(m) for m in parts(e)] for e in range(v.shape[0])]
            want[k] = torch.stack([torch.cat([c for c, _ in q]) for q in qs])
            want[k + "_scale_inv"] = torch.stack([torch.cat([s for _, s in q]) for q in qs]).view(torch.int32)
    return want


def _assert_experts(model, state):
    sd, want = model.state_dict(), _expected_buffers(state)
    assert len(want) == 4 * sum(k.endswith("experts.down_proj") for k in state)
    for k, v in want.items():
        assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k
    for k, v in state.items():
        if ".experts." not in k:
            assert torch.equal(sd[k], v), k


@pytest.mark.parametrize("family,spelling", [("qwen3_moe", "per_expert"), ("mixtral", "per_expert"), ("qwen3_moe", "fused"),
                                             ("mixtral", "fused")])
def test_fp8_expert_checkpoints_load_as_they_are(tmp_path, family, spelling):
    from kivi_amd.moe import Fp8Experts
    state = T.dense_state(family, 3)
    ckpt = _fp8_expert_state(state, family, spelling)
    if spelling == "per_expert":
        name = ("model.layers.1.block_sparse_moe.experts.7.w3.weight_scale_inv" if family == "mixtral"
                else "model.layers.1.mlp.experts.15.up_proj.weight_scale_inv")
        assert name in ckpt and ckpt[name].dtype == torch.float32 and ckpt[name[: -len("_scale_inv")]].dtype == FP8
    else:
        assert ckpt["model.layers.1.mlp.experts.gate_up_proj"].dtype == FP8 and "model.layers.1.mlp.experts.down_proj_scale_inv" in ckpt
    dense = [k[: -len(".weight")] for k in state if k.endswith("_proj.weight")]       # the linears stay 16-bit
    R.write_fp8_dir(str(tmp_path), T.config_dict(family), ckpt, quant=dict(modules_to_not_convert=dense))
    model = _load(tmp_path, fp8_experts=True)
    assert type(model) is T.classes()[family] and model.config.kivi_fp8_experts
    assert isinstance(model.model.layers[1].mlp.experts, Fp8Experts)
    _assert_experts(model, state)


@pytest.mark.parametrize("order", ["weights_first", "scales_first"])
def test_the_halves_of_a_pair_come_from_different_files_in_either_order(tmp_path, order):
    state = T.dense_state("qwen3_moe", 4)
    ckpt = _fp8_expert_state(state, "qwen3_moe", "per_expert")
    scales = [k for k in ckpt if ".experts." in k and k.endswith("_scale_inv")]
    others = [k for k in ckpt if k not in scales]
    files = [others, scales] if order == "weights_first" else [scales, others]
    dense = [k[: -len(".weight")] for k in state if k.endswith("_proj.weight")]
    R.write_fp8_dir(str(tmp_path), T.config_dict("qwen3_moe"), ckpt, quant=dict(modules_to_not_convert=dense), files=files)
    _assert_experts(_load(tmp_path, fp8_experts=True), state)


@pytest.mark.parametrize("family", ["qwen3_moe", "mixtral"])
def test_a_16_bit_directory_with_the_flag_is_quantised(tmp_path, family):
    from safetensors.torch import save_file
    state = T.dense_state(family, 5)
    save_file(T.hf_names(state, family), str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(T.config_dict(family)))
    model = _load(tmp_path, fp8_experts=True)
    assert not hasattr(model.config, "kivi_fp8_weights")
    _assert_experts(model, state)
    fused = tmp_path / "fused"
    fused.mkdir()
    save_file(state, str(fused / "model.safetensors"))
    (fused / "config.json").write_text(json.dumps(T.config_dict(family)))
    _assert_experts(_load(fused, fp8_experts=True), state)


def _write(tmp_path, ckpt, state, **quant):
    dense = [k[: -len(".weight")] for k in state if k.endswith("_proj.weight")]
    R.write_fp8_dir(str(tmp_path), T.config_dict("qwen3_moe"), ckpt, quant=dict(modules_to_not_convert=dense, **quant))


def test_a_missing_half_leaves_its_key_owed(tmp_path):
    state = T.dense_state("qwen3_moe", 6)
    ckpt = _fp8_expert_state(state, "qwen3_moe", "per_expert")
    del ckpt["model.layers.1.mlp.experts.9.down_proj.weight_scale_inv"]
    _write(tmp_path, ckpt, state)
    with pytest.raises(KeyError, match=r"model\.layers\.1\.mlp\.experts\.down_proj_scale_inv"):
        _load(tmp_path, fp8_experts=True)


def test_without_the_flag_fp8_experts_are_refused_with_a_pointer(tmp_path):
    state = T.dense_state("qwen3_moe", 6)
    _write(tmp_path, _fp8_expert_state(state, "qwen3_moe", "per_expert"), state)
    with pytest.raises(ValueError, match=r"FP8 experts are not served \(the attention projections and the dense MLP layers are\).*"
                                         r"fp8_experts=True"):
        _load(tmp_path)


def _break(ckpt, what):
    name = "model.layers.1.mlp.experts.3.gate_proj.weight"
    if what == "nan":
        b = ckpt[name].view(torch.uint8).clone()
        b[0, 0] = 0x7F
        ckpt[name] = b.view(FP8)
    elif what == "inf":
        ckpt[name + "_scale_inv"] = torch.full_like(ckpt[name + "_scale_inv"], float("inf"))
    elif what == "ue8m0":
        ckpt[name + "_scale_inv"] = torch.ones_like(ckpt[name + "_scale_inv"]).to(torch.uint8)
    elif what == "block":
        ckpt[name + "_scale_inv"] = torch.ones((2, 4))
    elif what == "shape":
        ckpt[name] = torch.zeros((128, 128), dtype=FP8)
    elif what == "index":
        ckpt["model.layers.1.mlp.experts.16.gate_proj.weight"] = ckpt.pop(name)
        return "model.layers.1.mlp.experts.16.gate_proj.weight"
    elif what == "e5m2":
        ckpt[name] = torch.zeros((128, 256), dtype=torch.float8_e5m2)
    elif what == "uint8":
        ckpt[name] = ckpt[name].view(torch.uint8)
    return name


@pytest.mark.parametrize("what,match", [("nan", "NaN byte"), ("inf", "a scale is not finite"), ("ue8m0", "fp32 scales are needed"),
                                        ("block", r"shape \(2, 4\) does not fit the \[128, 128\] block grid"),
                                        ("shape", r"shape \(128, 128\) does not fit the gate matrix"), ("index", "expert 16 outside"),
                                        ("e5m2", "only e4m3"), ("uint8", "float8_e4m3fn")])
def test_loader_refusals_by_tensor_name(tmp_path, what, match):
    state = T.dense_state("qwen3_moe", 6)
    ckpt = _fp8_expert_state(state, "qwen3_moe", "per_expert")
    name = _break(ckpt, what)
    _write(tmp_path, ckpt, state)
    with pytest.raises(ValueError, match=match) as err:
        _load(tmp_path, fp8_experts=True)
    assert name.rsplit(".", 1)[0] in str(err.value)


@pytest.mark.parametrize("quant,match", [(dict(scale_fmt="ue8m0"), "ue8m0"), (dict(weight_block_size=[64, 64]), "weight_block_size")])
def test_config_refusals(tmp_path, quant, match):
    state = T.dense_state("qwen3_moe", 6)
    _write(tmp_path, _fp8_expert_state(state, "qwen3_moe", "per_expert"), state, **quant)
    with pytest.raises(ValueError, match=match):
        _load(tmp_path, fp8_experts=True)


def test_fused_refusals(tmp_path):
    state = T.dense_state("qwen3_moe", 6)
    ckpt = _fp8_expert_state(state, "qwen3_moe", "fused")
    ckpt["model.layers.1.mlp.experts.down_proj_scale_inv"] = torch.ones((16, 2, 2))
    _write(tmp_path, ckpt, state)
    with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.experts\.down_proj_scale_inv: shape \(2, 2\)"):
        _load(tmp_path, fp8_experts=True)


@pytest.mark.parametrize("family,both", [("qwen3_moe", False), ("mixtral", False), ("qwen3_moe", True)])
def test_save_quantized_round_trips_to_identical_bytes(tmp_path, family, both):
    from safetensors import safe_open
    from safetensors.torch import save_file
    from kivi_amd import wfp8
    state = T.dense_state(family, 8)
    src = tmp_path / "src"
    src.mkdir()
    save_file(state, str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps(T.config_dict(family)))
    model = _load(src, fp8_experts=True, fp8_weights=both)
    out = tmp_path / "out"
    model.save_quantized(str(out))
    cfg = json.load(open(out / "config.json"))
    q = cfg.pop("quantization_config")
    assert cfg == T.config_dict(family) and not any(k.startswith("kivi_") for k in cfg)
    assert {k: q[k] for k in R.QUANT_CONFIG} == R.QUANT_CONFIG
    attention = [f"model.layers.{i}.self_attn.{p}_proj" for i in range(2) for p in "qkvo"]
    assert ("lm_head" in q["modules_to_not_convert"]) and all((a in q["modules_to_not_convert"]) != both for a in attention)
    with safe_open(str(out / "model.safetensors"), "pt") as fh:
        names = {k: fh.get_tensor(k) for k in fh.keys()}
    E = 8 if family == "mixtral" else 16
    for e in range(E):
        for proj, rows in (("gate_proj", (128, 256)), ("up_proj", (128, 256)), ("down_proj", (256, 128))):
            base = f"model.layers.1.mlp.experts.{e}.{proj}"
            assert names[base + ".weight"].dtype == FP8 and tuple(names[base + ".weight"].shape) == rows
            assert names[base + ".weight_scale_inv"].dtype == torch.float32
            assert tuple(names[base + ".weight_scale_inv"].shape) == (rows[0] // 128, rows[1] // 128)
    assert not any(k.endswith(("experts.gate_up_proj", "experts.down_proj", "proj_scale_inv")) and ".experts." in k and
                   k.split(".")[-2] == "experts" for k in names)
    back = _load(out, fp8_experts=True)
    assert back.config.kivi_fp8_experts and back.config.kivi_fp8_weights           # the directory is an FP8 checkpoint
    a, b = model.state_dict(), back.state_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert sum(isinstance(m, wfp8.Fp8Linear) for m in back.modules()) == sum(isinstance(m, wfp8.Fp8Linear) for m in model.modules())
    with pytest.raises(ValueError, match="fp8_experts=True"):
        _load(out)


# ----------------------------------------------------------------------------------------------------------------- C entry
def test_entry_exists_and_the_abi_version_stays_3():
    _l, lib = _lib()
    assert lib.kivi_abi_version() == 3 == _l.ABI_VERSION
    assert "kivi_moe_experts_w8" in _l.SIGNATURES and len(_l.SIGNATURES["kivi_moe_experts_w8"][1]) == 22 and hasattr(lib, "kivi_moe_experts_w8")
    header = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert "int kivi_moe_experts_w8(const void* x, int64_t x_stride, int dtype, int N, int H, int I, int E, int top_k, const void* w," in header
    assert "#define KIVI_ABI_VERSION 3" in header


def _args(**kw):
    a = dict(x=P, x_stride=256, dtype=F16, N=4, H=256, I=128, E=8, top_k=2, w=P, pairs=P, pos=P, tiles=P, n_tiles=P, gate_up=P,
             gate_up_scale=P, down=P, down_scale=P, out=P, out_stride=256, workspace=P, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return list(a.values())


REFUSALS = [
    (dict(dtype=32), -1), (dict(N=0), -1), (dict(E=0), -1), (dict(E=300), -1), (dict(top_k=0), -1), (dict(top_k=9), -1),
    (dict(H=192, x_stride=192, out_stride=192), -1), (dict(I=96), -1), (dict(I=64), -1), (dict(H=0), -1), (dict(I=0), -1),
    (dict(H=160, x_stride=160, out_stride=160), -1), (dict(x_stride=248), -1), (dict(out_stride=252), -1),
    (dict(workspace_bytes=8 * 128 * 2 + 8 * 256 * 4 - 1), -1), (dict(x=None), -1), (dict(w=None), -1), (dict(pairs=None), -1),
    (dict(pos=None), -1), (dict(tiles=None), -1), (dict(n_tiles=None), -1), (dict(gate_up=None), -1), (dict(gate_up_scale=None), -1),
    (dict(down=None), -1), (dict(down_scale=None), -1), (dict(out=None), -1), (dict(workspace=None), -1), (dict(x=P + 8), -2),
    (dict(gate_up=P + 2), -2), (dict(down=P + 4), -2), (dict(workspace=P + 8), -2), (dict(out=P + 4), -2), (dict(x_stride=260), -2),
    (dict(out_stride=258), -2), (dict(w=P + 2), -2), (dict(pos=P + 1), -2), (dict(gate_up_scale=P + 2), -2), (dict(down_scale=P + 1), -2),
]


@pytest.mark.parametrize("change,rc", REFUSALS, ids=[str(c) for c, _ in REFUSALS])
def test_entry_refuses_before_anything_is_enqueued(change, rc):
    _l, lib = _lib()
    assert lib.kivi_moe_experts_w8(*_args(**change)) == rc, lib.kivi_last_error()
    assert b"kivi_moe_experts_w8" in lib.kivi_last_error()


def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "moe_w8_plan")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "moe_w8_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "moe w8 plan ok" and run.stderr == "", run.stdout + run.stderr
