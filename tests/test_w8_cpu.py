"""No GPU: the FP8 weight path (kivi_amd/wfp8.py) everywhere but on the device.

1. The entries exist with their signatures, the ABI version is still 3, and every refusal of kivi_w8_dequant / kivi_w8_linear /
   kivi_w8_gate_up is reached with fake pointers: a refused call enqueues nothing, so no device is needed.
2. tests/w8_plan_main.cpp, a stand-alone program over kivi_amd/csrc/kivi_w8_plan.h, built with -fsanitize=address,undefined and run
   as a child process.
3. The format in torch: the byte table of tests/w8_ref.py against torch's float8_e4m3fn, the quantiser against its restatement and
   against a fixture minted from transformers' Fp8Quantize, dequant_torch against the fp64 contract, the skip rule.
4. Fp8Linear's state-dict names and dtype casts, make_config plumbing, the module trees.
5. The loader on the CPU: pre-quantised directories (split files in either order, per-tensor scales, modules_to_not_convert, an FP8
   pair for a dense module), the refusals by name, the missing scale, and the save_quantized round trip."""
import json
import os
import shutil
import subprocess

import pytest
import torch

import w8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 16, 0x110
P = 0x10000          # a fake, 16-byte aligned pointer: a refused call never follows it


def _lib():
    from kivi_amd import _lib
    return _lib, _lib.load()


def test_entries_exist_and_the_abi_version_stays_3():
    _l, lib = _lib()
    assert lib.kivi_abi_version() == 3 == _l.ABI_VERSION
    for name, n_args in (("kivi_w8_dequant", 8), ("kivi_w8_linear", 12), ("kivi_w8_gate_up", 13), ("kivi_w8_bytes", 2)):
        assert name in _l.SIGNATURES and len(_l.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    for name in ("kivi_w8_dequant(", "kivi_w8_linear(", "kivi_w8_gate_up(", "kivi_w8_bytes(", "#define KIVI_ABI_VERSION 3"):
        assert name in header
    assert lib.kivi_w8_bytes(4096, 4096) == 4096 * 4096 + 4 * 32 * 32
    assert lib.kivi_w8_bytes(144, 384) == 144 * 384 + 4 * 2 * 3
    assert lib.kivi_w8_bytes(24, 128) == -1 and lib.kivi_w8_bytes(16, 192) == -1 and lib.kivi_w8_bytes(0, 128) == -1


def _dequant_args(**kw):
    a = dict(weight=P, scale_inv=P, O=32, K=256, dtype=F16, out=P, out_stride=256, stream=None)
    a.update(kw)
    return list(a.values())


def _linear_args(**kw):
    a = dict(x=P, x_stride=256, dtype=F16, N=4, O=32, K=256, weight=P, scale_inv=P, bias=None, y=P, y_stride=32, stream=None)
    a.update(kw)
    return list(a.values())


def _gate_up_args(**kw):
    a = dict(x=P, x_stride=256, dtype=F16, N=4, I=32, K=256, gw=P, gs=P, uw=P, us=P, y=P, y_stride=32, stream=None)
    a.update(kw)
    return list(a.values())


SHAPE_REFUSALS = [(dict(dtype=32), -1), (dict(dtype=0), -1), (dict(K=192), -1), (dict(K=64), -1), (dict(K=0), -1), (dict(K=-128), -1)]
DEQUANT_REFUSALS = SHAPE_REFUSALS + [
    (dict(O=24), -1), (dict(O=0), -1), (dict(out_stride=248), -1), (dict(out=None), -1), (dict(weight=None), -1),
    (dict(scale_inv=None), -1), (dict(out=P + 8), -2), (dict(weight=P + 8), -2), (dict(scale_inv=P + 2), -2), (dict(out_stride=260), -2)]
LINEAR_REFUSALS = SHAPE_REFUSALS + [
    (dict(O=24, y_stride=24), -1), (dict(O=0), -1), (dict(N=0), -1), (dict(N=-3), -1), (dict(N=2 ** 26, O=32), -1),
    (dict(N=2 ** 19, O=4096, y_stride=4096), -1), (dict(x_stride=248), -1), (dict(y_stride=28), -1), (dict(x=None), -1),
    (dict(weight=None), -1), (dict(scale_inv=None), -1), (dict(y=None), -1), (dict(x=P + 8), -2), (dict(weight=P + 8), -2),
    (dict(scale_inv=P + 2), -2), (dict(y=P + 4), -2), (dict(bias=P + 1), -2), (dict(x_stride=260), -2), (dict(y_stride=34), -2)]
GATE_UP_REFUSALS = SHAPE_REFUSALS + [
    (dict(I=24, y_stride=24), -1), (dict(N=0), -1), (dict(N=2 ** 26), -1), (dict(x_stride=248), -1), (dict(y_stride=16), -1),
    (dict(x=None), -1), (dict(gw=None), -1), (dict(gs=None), -1), (dict(uw=None), -1), (dict(us=None), -1), (dict(y=None), -1),
    (dict(uw=P + 8), -2), (dict(us=P + 2), -2), (dict(gs=P + 1), -2), (dict(y=P + 2), -2), (dict(x_stride=260), -2),
    (dict(y_stride=34), -2)]


def _refused(entry, args, rc):
    _l, lib = _lib()
    assert getattr(lib, entry)(*args) == rc, lib.kivi_last_error()
    assert entry.encode() in lib.kivi_last_error()


@pytest.mark.parametrize("change,rc", DEQUANT_REFUSALS, ids=[str(c) for c, _ in DEQUANT_REFUSALS])
def test_dequant_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w8_dequant", _dequant_args(**change), rc)


@pytest.mark.parametrize("change,rc", LINEAR_REFUSALS, ids=[str(c) for c, _ in LINEAR_REFUSALS])
def test_linear_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w8_linear", _linear_args(**change), rc)


@pytest.mark.parametrize("change,rc", GATE_UP_REFUSALS, ids=[str(c) for c, _ in GATE_UP_REFUSALS])
def test_gate_up_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w8_gate_up", _gate_up_args(**change), rc)


def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "w8_plan")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "w8_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "w8 plan ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ the format in torch
def test_the_byte_table_is_torchs_float8_e4m3fn():
    every = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    torchs = every.view(torch.float8_e4m3fn).to(torch.float64)
    finite = ~torch.isnan(R.E4M3)
    assert [b for b in range(256) if not finite[b]] == list(R.NAN_BYTES) and torch.equal(torch.isnan(torchs), ~finite)
    assert torch.equal(torchs[finite], R.E4M3[finite]) and R.E4M3.abs()[finite].max() == 448.0 == R.FP8_MAX
    # every finite value is exact in fp16 and in bf16: the reason the kernels convert at scale 1 and lose nothing
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(R.E4M3[finite].to(dtype).double(), R.E4M3[finite])
    assert R.FINITE_BYTES.numel() == 254
    # ... and the module's torch dequantiser at scale 1 is the table: an O x K weight holding every finite byte, one scale block
    from kivi_amd import wfp8
    weight = R.FINITE_BYTES.repeat(9)[:16 * 128].reshape(16, 128)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        assert torch.equal(wfp8.dequant_torch(weight, torch.ones((1, 1)), dtype).double(), R.E4M3[weight.long()])
    with pytest.raises(ValueError, match="NaN byte"):
        wfp8.as_bytes(every, "w")


def _weights(kind, O, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((O, K), generator=g) * 0.05
    if kind == "zero_block":
        w[:128, 128:256] = 0
    elif kind == "outlier":
        w[3, 200] = 5.0
    return w.to(dtype)


@pytest.mark.parametrize("kind,O,K", [("normal", 256, 384), ("zero_block", 256, 384), ("outlier", 128, 256), ("normal", 144, 384),
                                      ("zero_block", 48, 256)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_the_quantiser_is_its_restatement_and_fits_the_contract(kind, O, K, dtype):
    from kivi_amd import wfp8
    w = _weights(kind, O, K, dtype, O + K)
    codes, inv = wfp8.quantize(w)
    rc, ri = R.quantize_ref(w)
    assert codes.dtype == torch.uint8 and inv.dtype == torch.float32 and tuple(inv.shape) == R.grid(O, K) == wfp8.scale_shape(O, K)
    assert torch.equal(codes, rc) and torch.equal(inv.view(torch.int32), ri.view(torch.int32))
    assert not bool(((codes & 0x7F) == 0x7F).any())
    # the block maximum lands on +-448, and the represented weight is within half a step of e4m3 at the top binade (2^-4 relative
    # to the block maximum) of the weight
    wt, w64 = R.represented(codes, inv), w.double()
    bound = R.expand(inv.double(), O, K) * 448.0 * 2.0 ** -4
    assert bool(((wt - w64).abs() <= bound * (1 + 1e-6)).all())
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(wfp8.dequant_torch(codes, inv, dt), wt.float().to(dt))
    with pytest.raises(ValueError, match="not finite"):
        bad = w.clone()
        bad[0, 0] = float("inf")
        wfp8.quantize(bad, "w")


def test_the_quantiser_against_a_fixture_of_transformers_fp8quantize():
    """tests/golden/fp8_block_144x384.safetensors: a bf16 weight (blocks of different magnitude, one outlier, an all-zero partial
    block), and what transformers 5.15's Fp8Quantize made of it at weight_block_size [128, 128] (its rows padded with zeros to 256 for
    that call, which wants whole blocks, and the first 144 rows of the codes kept)."""
    from safetensors.torch import load_file
    from kivi_amd import wfp8
    t = load_file(os.path.join(ROOT, "tests", "golden", "fp8_block_144x384.safetensors"))
    w, codes, inv = t["input"], t["weight"].view(torch.uint8), t["weight_scale_inv"]
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (144, 384) and tuple(inv.shape) == (2, 3) and float(inv[1, 2]) == 1.0
    for got in (R.quantize_ref(w), wfp8.quantize(w)):
        assert torch.equal(got[0], codes) and torch.equal(got[1].view(torch.int32), inv.view(torch.int32))


def test_the_skip_rule_is_transformers():
    from kivi_amd import wfp8
    names = ["lm_head", "model.layers.1.self_attn.q_proj", "model.layers.11.self_attn.q_proj", "model.layers.0.mlp.down_proj",
             "model.layers.0.mlp.gate_proj"]
    for patterns in (None, [], ["lm_head"], ["model.layers.1"], ["q_proj"], ["model\\.layers\\.\\d+\\.mlp"], ["mlp.down_proj", "lm_head"],
                     ["model.layers.1.self_attn.q_proj"]):
        for n in names:
            assert wfp8.should_convert(n, patterns) == R.should_convert_ref(n, patterns or None), (n, patterns)
    assert not wfp8.should_convert("model.layers.11.self_attn.q_proj", ["model.layers.1"])        # the rule's prefix match
    assert wfp8.should_convert("model.layers.0.mlp.gate_proj", ["mlp.down_proj"]) and wfp8.should_convert(None, ["lm_head"])


# ------------------------------------------------------------------------------------------------ modules and configuration
def _cfg(**kw):
    d = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=384, vocab_size=64,
             head_dim=64)
    d.update(kw)
    return d


def test_fp8_linear_state_dict_names_and_dtype_casts():
    from kivi_amd import wfp8
    lin = wfp8.Fp8Linear(256, 144, bias=True)
    assert sorted(lin.state_dict()) == ["bias", "weight", "weight_scale_inv"]
    assert sorted(wfp8.Fp8Linear(256, 48).state_dict()) == ["weight", "weight_scale_inv"]
    assert tuple(lin.weight.shape) == (144, 256) and lin.weight.dtype == torch.uint8
    assert tuple(lin.weight_scale_inv.shape) == (2, 2) and lin.weight_scale_inv.dtype == torch.int32
    g = torch.Generator().manual_seed(2)
    lin.weight.copy_(R.random_bytes((144, 256), 3))
    lin.weight_scale_inv.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (2, 2), generator=g, dtype=torch.int64).to(torch.int32))
    before = {k: v.clone() for k, v in lin.state_dict().items()}
    for cast in (lambda m: m.bfloat16(), lambda m: m.half(), lambda m: m.to(torch.bfloat16), lambda m: m.float()):
        m = cast(lin)
        for name in ("weight", "weight_scale_inv"):
            assert torch.equal(getattr(m, name), before[name]) and getattr(m, name).dtype == before[name].dtype, name
    assert lin.bias.dtype == torch.float32
    mlp = wfp8.Fp8MLP(256, 384)
    assert sorted(mlp.state_dict()) == sorted(f"{p}_proj.{b}" for p in ("gate", "up", "down") for b in ("weight", "weight_scale_inv"))
    for o, k in ((24, 128), (16, 192), (16, 64), (0, 128)):
        assert not wfp8.usable(o, k)
        with pytest.raises(ValueError):
            wfp8.Fp8Linear(k, o)
    with pytest.raises(Exception, match="GPU"):                 # no CPU path, no fallback
        wfp8.Fp8Linear(128, 16)(torch.zeros((2, 128), dtype=torch.float16))
    # load_ refuses by name
    with pytest.raises(ValueError, match="q_proj.weight.*NaN"):
        bad = R.random_bytes((144, 256), 4)
        bad[7, 9] = 0xFF
        lin.load_(weight_fp8=bad.view(torch.float8_e4m3fn), name="q_proj.weight")
    with pytest.raises(ValueError, match="q_proj.weight_scale_inv.*not finite"):
        lin.load_(scale=torch.tensor([[1.0, float("inf")], [1.0, 1.0]]), name="q_proj.weight_scale_inv")
    with pytest.raises(ValueError, match="block grid"):
        lin.load_(scale=torch.ones((2, 3)), name="s")


def test_make_config_plumbing():
    from kivi_amd import wfp8, wquant
    from kivi_amd.llama import MLP, LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, make_config
    plain = make_config(_cfg())
    assert not hasattr(plain, "kivi_fp8_weights") and vars(plain) == vars(make_config(_cfg(), fp8_weights=False, weight_kernel_max_tokens=5))
    with pytest.raises(ValueError, match="fp8_weights"):
        make_config(_cfg(), fp8_weights=True, weight_bits=4)
    moe = _cfg(model_type="qwen3_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=128)
    with pytest.raises(ValueError, match="fp8_weights together with expert_bits"):
        make_config(moe, fp8_weights=True, expert_bits=4)
    cfg = make_config(_cfg(), fp8_weights=True, weight_kernel_max_tokens=7)
    assert cfg.kivi_fp8_weights is True and cfg.kivi_weight_kernel_max_tokens == 7 and not hasattr(cfg, "kivi_weight_bits")
    model = LlamaForCausalLM_KIVI(cfg)
    for layer in model.model.layers:
        att = layer.self_attn
        for lin, (o, k) in ((att.q_proj, (256, 256)), (att.k_proj, (128, 256)), (att.v_proj, (128, 256)), (att.o_proj, (256, 256))):
            assert type(lin) is wfp8.Fp8Linear and (lin.out_features, lin.in_features) == (o, k)
            assert lin.kernel_max_tokens == 7 and lin.bias is None
        assert type(layer.mlp) is wfp8.Fp8MLP and layer.mlp.down_proj.in_features == 384
    assert type(model.lm_head) is torch.nn.Linear and type(model.model.embed_tokens) is torch.nn.Embedding
    sd = model.state_dict()
    assert sd["model.layers.1.mlp.up_proj.weight"].dtype == torch.uint8 and "model.layers.0.self_attn.k_proj.weight_scale_inv" in sd
    q2 = Qwen2ForCausalLM_KIVI(make_config(_cfg(), fp8_weights=True))
    att = q2.model.layers[0].self_attn
    assert type(att.q_proj) is wfp8.Fp8Linear and att.q_proj.bias is not None and att.v_proj.bias is not None
    assert type(att.o_proj) is wfp8.Fp8Linear and att.o_proj.bias is None and att.q_proj.kernel_max_tokens == wfp8.KERNEL_MAX_TOKENS
    # a shape the kernels do not serve stays an nn.Linear, projection by projection: with hidden 192 (no multiple of 128) q / k / v
    # reduce over 192 and stay dense, o_proj reduces over 4 * 64 = 256 into 192 = 12 * 16 rows and is FP8; the MLP stays whole
    odd = LlamaForCausalLM_KIVI(make_config(_cfg(hidden_size=192, head_dim=64, intermediate_size=256), fp8_weights=True))
    att = odd.model.layers[0].self_attn
    assert type(att.q_proj) is torch.nn.Linear and type(att.v_proj) is torch.nn.Linear and type(att.o_proj) is wfp8.Fp8Linear
    assert type(odd.model.layers[0].mlp) is MLP and type(odd.model.layers[0].mlp.down_proj) is torch.nn.Linear
    # a checkpoint's modules_to_not_convert leaves modules dense by name; one projection of an MLP keeps the whole MLP dense
    skip = LlamaForCausalLM_KIVI(make_config(_cfg(), fp8_weights=True, fp8_skip_modules=["lm_head", "model.layers.0.self_attn.q_proj",
                                                                                        "layers.1.mlp.up_proj"]))
    l0, l1 = skip.model.layers
    assert type(l0.self_attn.q_proj) is torch.nn.Linear and type(l0.self_attn.k_proj) is wfp8.Fp8Linear
    assert type(l1.self_attn.q_proj) is wfp8.Fp8Linear and type(l0.mlp) is wfp8.Fp8MLP and type(l1.mlp) is MLP
    # the 4-bit factory is what it was
    assert type(LlamaForCausalLM_KIVI(make_config(_cfg(), weight_bits=4)).model.layers[0].mlp) is wquant.QuantMLP


def test_sparse_models_take_fp8_in_attention_and_dense_layers_only():
    from kivi_amd import wfp8
    from kivi_amd.llama import Qwen3MoeForCausalLM_KIVI, make_config
    from kivi_amd.moe import SparseMoeBlock
    d = _cfg(model_type="qwen3_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=128, mlp_only_layers=[0],
             norm_topk_prob=True)
    model = Qwen3MoeForCausalLM_KIVI(make_config(d, fp8_weights=True))
    assert type(model.model.layers[0].mlp) is wfp8.Fp8MLP and type(model.model.layers[1].mlp) is SparseMoeBlock
    assert model.model.layers[1].mlp.experts.gate_up_proj.dtype == torch.float32
    assert all(type(layer.self_attn.q_proj) is wfp8.Fp8Linear for layer in model.model.layers)


def test_lora_targets_an_fp8_linear():
    from kivi_amd import wfp8
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    model = LlamaForCausalLM_KIVI(make_config(_cfg(), fp8_weights=True))
    lset = model.enable_lora(2, 8, ("q_proj", "gate_proj"))
    assert len(lset.modules) == 4 and all(type(m) is wfp8.Fp8Linear for m in lset.modules.values())


# ------------------------------------------------------------------------------------------------ the loader
DTYPE = torch.bfloat16


@pytest.fixture(scope="module")
def dense_state():
    """The 16-bit state_dict of a tiny Llama, bf16."""
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    torch.manual_seed(11)
    model = LlamaForCausalLM_KIVI(make_config(_cfg()))
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.0625)
    return {k: v.detach().to(DTYPE) for k, v in model.state_dict().items()}


def _load(path, **kw):
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    return LlamaForCausalLM_KIVI.from_pretrained(str(path), device="cpu", dtype=DTYPE, **kw)


def _assert_holds(model, state):
    """Every tensor of the FP8 state `state` is in the model bit for bit: bytes as bytes, scales as bits."""
    sd = model.state_dict()
    assert sorted(sd) == sorted(state)
    for k, v in state.items():
        if v.dtype == torch.float8_e4m3fn:
            assert sd[k].dtype == torch.uint8 and torch.equal(sd[k], v.view(torch.uint8)), k
        elif k.endswith("weight_scale_inv"):
            assert sd[k].dtype == torch.int32 and torch.equal(sd[k], v.view(torch.int32)), k
        else:
            assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k


@pytest.mark.parametrize("order", ["scales_first", "weights_first", "one_file"])
def test_a_prequantised_directory_fills_the_model_bit_for_bit(tmp_path, dense_state, order):
    from kivi_amd import wfp8
    state = R.fp8_state(dense_state)
    assert sum(v.dtype == torch.float8_e4m3fn for v in state.values()) == 14
    scales = [k for k in state if k.endswith("weight_scale_inv")]
    rest = [k for k in state if not k.endswith("weight_scale_inv")]
    files = None if order == "one_file" else [scales, rest] if order == "scales_first" else [rest, scales]
    R.write_fp8_dir(str(tmp_path), _cfg(), state, files=files)
    model = _load(tmp_path)
    assert model.config.kivi_fp8_weights and type(model.model.layers[0].self_attn.q_proj) is wfp8.Fp8Linear
    _assert_holds(model, state)
    # ... and the true weight is back to within e4m3's half step: the silent failure was max |w| = 448 for a weight of 0.0625 sigma
    lin = model.model.layers[1].mlp.down_proj
    w = dense_state["model.layers.1.mlp.down_proj.weight"].double()
    got = lin.dequant(torch.float32).double()
    assert float(got.abs().max()) < 1.0 and float((got - w).abs().max()) <= float(w.abs().max()) * 2.0 ** -4 * 1.01
    # a 16-bit directory with fp8_weights=True gives the same buffers
    from safetensors.torch import save_file
    d16 = tmp_path / "dense"
    os.makedirs(d16)
    json.dump(_cfg(), open(d16 / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in dense_state.items()}, str(d16 / "model.safetensors"))
    _assert_holds(_load(d16, fp8_weights=True), state)


def test_a_per_tensor_scalar_is_expanded(tmp_path, dense_state):
    state = {}
    for k, v in dense_state.items():
        if k.endswith("_proj.weight"):
            s = 448.0 / v.float().abs().max()
            state[k] = (v.float() * s).clamp(-448, 448).to(torch.float8_e4m3fn)
            state[k[:-6] + "weight_scale_inv"] = (1.0 / s).reshape(())
        else:
            state[k] = v
    R.write_fp8_dir(str(tmp_path), _cfg(), state, quant=dict(weight_block_size=None))
    model = _load(tmp_path)
    for name in ("model.layers.0.self_attn.k_proj", "model.layers.1.mlp.gate_proj"):
        lin = dict(model.named_modules())[name]
        assert torch.equal(lin.weight, state[name + ".weight"].view(torch.uint8))
        want = state[name + ".weight_scale_inv"].reshape(1, 1).expand(lin.scale.shape)
        assert torch.equal(lin.scale.view(torch.int32), want.contiguous().view(torch.int32))


def test_modules_to_not_convert_and_an_fp8_pair_for_a_dense_module(tmp_path, dense_state):
    from kivi_amd import wfp8
    q0, k1 = "model.layers.0.self_attn.q_proj", "model.layers.1.self_attn.k_proj"
    state = R.fp8_state(dense_state, keep_dense=(q0 + ".weight",))          # q0 is 16-bit in the file, k1 FP8 in the file ...
    scales = [k for k in state if k.endswith("weight_scale_inv")]
    rest = [k for k in state if not k.endswith("weight_scale_inv")]
    for files in ([rest, scales], [scales, rest]):
        shutil.rmtree(tmp_path, ignore_errors=True)
        R.write_fp8_dir(str(tmp_path), _cfg(), state, quant=dict(modules_to_not_convert=["lm_head", q0, k1]), files=files)
        model = _load(tmp_path)                                              # ... and both are built dense
        mods = dict(model.named_modules())
        assert type(mods[q0]) is torch.nn.Linear and type(mods[k1]) is torch.nn.Linear
        assert type(mods["model.layers.1.self_attn.q_proj"]) is wfp8.Fp8Linear
        assert torch.equal(mods[q0].weight.data, dense_state[q0 + ".weight"])
        codes, inv = state[k1 + ".weight"].view(torch.uint8), state[k1 + ".weight_scale_inv"]
        assert mods[k1].weight.dtype == DTYPE and torch.equal(mods[k1].weight.data, R.represented(codes, inv).float().to(DTYPE))


def test_a_missing_scale_is_a_keyerror_from_finish(tmp_path, dense_state):
    state = R.fp8_state(dense_state)
    gone = "model.layers.1.self_attn.v_proj.weight_scale_inv"
    R.write_fp8_dir(str(tmp_path / "a"), _cfg(), {k: v for k, v in state.items() if k != gone})
    with pytest.raises(KeyError, match="v_proj.weight_scale_inv"):
        _load(tmp_path / "a")
    # ... and where the module is dense, its weight stays owed until the scale has come
    R.write_fp8_dir(str(tmp_path / "b"), _cfg(), {k: v for k, v in state.items() if k != gone},
                    quant=dict(modules_to_not_convert=["model.layers.1.self_attn.v_proj"]))
    with pytest.raises(KeyError, match="model.layers.1.self_attn.v_proj.weight"):
        _load(tmp_path / "b")


def test_a_stranded_half_and_a_uint8_weight_are_refused_by_name(tmp_path, dense_state):
    """A weight_scale_inv beside a 16-bit weight of a dense module fills no key and would wait for ever: finish() names it.  FP8
    bytes stored as uint8 would be copied into a dense parameter unscaled: refused where they arrive."""
    k1 = "model.layers.1.self_attn.k_proj"
    state = R.fp8_state(dense_state, keep_dense=(k1 + ".weight",))
    state[k1 + ".weight_scale_inv"] = torch.ones((1, 2))
    R.write_fp8_dir(str(tmp_path / "a"), _cfg(), state, quant=dict(modules_to_not_convert=[k1]))
    with pytest.raises(ValueError, match="k_proj.weight_scale_inv.*other half never came"):
        _load(tmp_path / "a")
    state = R.fp8_state(dense_state)
    state[k1 + ".weight"] = state[k1 + ".weight"].view(torch.uint8)
    R.write_fp8_dir(str(tmp_path / "b"), _cfg(), state, quant=dict(modules_to_not_convert=[k1]))
    with pytest.raises(ValueError, match="k_proj.weight: a uint8 weight"):
        _load(tmp_path / "b")


def test_a_callers_skip_list_is_joined_with_the_checkpoints(tmp_path, dense_state):
    q0, k1 = "model.layers.0.self_attn.q_proj", "model.layers.1.self_attn.k_proj"
    R.write_fp8_dir(str(tmp_path), _cfg(), R.fp8_state(dense_state), quant=dict(modules_to_not_convert=["lm_head", q0]))
    model = _load(tmp_path, fp8_skip_modules=[k1])
    mods = dict(model.named_modules())
    assert type(mods[q0]) is torch.nn.Linear and type(mods[k1]) is torch.nn.Linear
    assert model.config.kivi_fp8_skip == [k1, "lm_head", q0]


def _refusal_cases():
    def nan_byte(state):
        w = state["model.layers.0.mlp.up_proj.weight"].view(torch.uint8).clone()
        w[5, 5] = 0x7F
        state["model.layers.0.mlp.up_proj.weight"] = w.view(torch.float8_e4m3fn)
    def stray_scale(state):
        state["model.norm.weight_scale_inv"] = torch.ones((1, 2))
    def input_scale(state):
        state["model.layers.0.mlp.up_proj.input_scale"] = torch.ones(())
    return [("nan_byte", nan_byte, {}, "up_proj.weight.*NaN byte"), ("ue8m0", None, dict(scale_fmt="ue8m0"), "ue8m0"),
            ("static", None, dict(activation_scheme="static"), "static"), ("block64", None, dict(weight_block_size=[64, 64]),
                                                                          "weight_block_size"),
            ("e5m2", None, dict(fmt="e5m2"), "e4m3"), ("stray_scale", stray_scale, {}, "model.norm.weight_scale_inv"),
            ("input_scale", input_scale, {}, "up_proj.input_scale.*static activation")]


@pytest.mark.parametrize("case", _refusal_cases(), ids=[c[0] for c in _refusal_cases()])
def test_what_is_not_served_is_refused_by_name(tmp_path, dense_state, case):
    _, change, quant, match = case
    state = R.fp8_state(dense_state)
    if change is not None:
        change(state)
    R.write_fp8_dir(str(tmp_path), _cfg(), state, quant=quant)
    with pytest.raises(ValueError, match=match):
        _load(tmp_path)


@pytest.mark.parametrize("name", ["model.layers.1.mlp.experts.0.gate_proj.weight_scale_inv", "model.layers.1.mlp.experts.gate_up_proj_scale_inv",
                                  "model.layers.1.mlp.experts.2.down_proj.weight"])
def test_fp8_experts_are_refused(tmp_path, name):
    d = _cfg(model_type="qwen3_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=128, mlp_only_layers=[0],
             norm_topk_prob=True)
    t = torch.zeros((256, 128), dtype=torch.float8_e4m3fn) if name.endswith(".weight") else torch.ones((2, 1))
    R.write_fp8_dir(str(tmp_path), d, {name: t})
    with pytest.raises(ValueError, match="FP8 experts are not served"):
        _load(tmp_path)


def test_save_quantized_round_trip(tmp_path, dense_state):
    from safetensors.torch import load_file, save_file
    d16 = tmp_path / "dense"
    os.makedirs(d16)
    json.dump(_cfg(rms_norm_eps=1e-6), open(d16 / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in dense_state.items()}, str(d16 / "model.safetensors"))
    model = _load(d16, fp8_weights=True)
    out = tmp_path / "fp8"
    model.save_quantized(str(out))
    written = json.load(open(out / "config.json"))
    assert written["quantization_config"] == dict(quant_method="fp8", fmt="e4m3", activation_scheme="dynamic", weight_block_size=[128, 128],
                                                  scale_fmt="float", modules_to_not_convert=["lm_head"])
    assert written["rms_norm_eps"] == 1e-6 and not any(k.startswith("kivi_") for k in written)
    files = load_file(str(out / "model.safetensors"))
    assert files["model.layers.0.self_attn.o_proj.weight"].dtype == torch.float8_e4m3fn
    assert files["model.layers.0.self_attn.o_proj.weight_scale_inv"].dtype == torch.float32
    assert files["lm_head.weight"].dtype == DTYPE
    again = _load(out)
    a, b = model.state_dict(), again.state_dict()
    assert list(a) == list(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    assert [type(m) for m in model.modules()] == [type(m) for m in again.modules()]
