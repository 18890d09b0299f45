"""No GPU: the 4-bit weight path (kivi_amd/wquant.py) everywhere but on the device.

1. The entries exist with their signatures, the ABI version is still 3, and every refusal of kivi_w4_pack / kivi_w4_dequant /
   kivi_w4_linear / kivi_w4_gate_up is reached with fake pointers: a refused call enqueues nothing, so no device is needed.
2. tests/w4_plan_main.cpp, a stand-alone program over kivi_amd/csrc/kivi_w4_plan.h (layout, wave runs, grids, token passes, the
   refusals), built with -fsanitize=address,undefined and run as a child process.
3. The layout in torch: to_ref / from_ref invert each other on random triples, from_ref of the oracle's pack of a small weight puts
   every code where the word / bit formula restated in tests/w4_ref.py says, dequant_torch equals the fp64 statement rounded.
4. make_config plumbing, the refusal of other widths, QuantLinear's state-dict names, dtype casts leaving scales / mins alone, and
   the default configuration building exactly the module tree it built before."""
import os
import shutil
import subprocess

import pytest
import torch

import w4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 16, 0x110
P = 0x10000          # a fake, 16-byte aligned pointer: a refused call never follows it


def _lib():
    from kivi_amd import _lib
    return _lib, _lib.load()


def test_entries_exist_and_the_abi_version_stays_3():
    _l, lib = _lib()
    assert lib.kivi_abi_version() == 3 == _l.ABI_VERSION
    for name, n_args in (("kivi_w4_pack", 10), ("kivi_w4_dequant", 10), ("kivi_w4_linear", 14), ("kivi_w4_gate_up", 16),
                         ("kivi_w4_bytes", 3)):
        assert name in _l.SIGNATURES and len(_l.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    for name in ("kivi_w4_pack(", "kivi_w4_dequant(", "kivi_w4_linear(", "kivi_w4_gate_up(", "kivi_w4_bytes(", "#define KIVI_ABI_VERSION 3"):
        assert name in header
    assert lib.kivi_w4_bytes(4096, 4096, 128) == 4096 * 4096 // 2 + 4 * 4096 * 32
    assert lib.kivi_w4_bytes(48, 384, 64) == 48 * 384 // 2 + 4 * 48 * 6
    assert lib.kivi_w4_bytes(24, 128, 64) == -1 and lib.kivi_w4_bytes(16, 192, 64) == -1 and lib.kivi_w4_bytes(16, 128, 32) == -1


def _pack_args(**kw):
    a = dict(w=P, w_stride=256, dtype=F16, O=32, K=256, group=64, qweight=P, scales=P, mins=P, stream=None)
    a.update(kw)
    return list(a.values())


def _dequant_args(**kw):
    a = dict(qweight=P, scales=P, mins=P, O=32, K=256, group=64, dtype=F16, out=P, out_stride=256, stream=None)
    a.update(kw)
    return list(a.values())


def _linear_args(**kw):
    a = dict(x=P, x_stride=256, dtype=F16, N=4, O=32, K=256, group=64, qweight=P, scales=P, mins=P, bias=None, y=P, y_stride=32,
             stream=None)
    a.update(kw)
    return list(a.values())


def _gate_up_args(**kw):
    a = dict(x=P, x_stride=256, dtype=F16, N=4, I=32, K=256, group=64, gq=P, gs=P, gm=P, uq=P, us=P, um=P, y=P, y_stride=32, stream=None)
    a.update(kw)
    return list(a.values())


SHAPE_REFUSALS = [(dict(dtype=32), -1), (dict(dtype=0), -1), (dict(K=192), -1), (dict(K=64), -1), (dict(K=0), -1), (dict(group=32), -1),
                  (dict(group=256), -1), (dict(group=0), -1)]
PACK_REFUSALS = SHAPE_REFUSALS + [
    (dict(O=24), -1), (dict(O=0), -1), (dict(w_stride=248), -1), (dict(w=None), -1), (dict(qweight=None), -1), (dict(scales=None), -1),
    (dict(mins=None), -1), (dict(w=P + 8), -2), (dict(qweight=P + 4), -2), (dict(scales=P + 2), -2), (dict(mins=P + 4), -2),
    (dict(w_stride=260), -2)]
DEQUANT_REFUSALS = SHAPE_REFUSALS + [
    (dict(O=24), -1), (dict(O=0), -1), (dict(out_stride=248), -1), (dict(out=None), -1), (dict(qweight=None), -1),
    (dict(scales=None), -1), (dict(mins=None), -1), (dict(out=P + 8), -2), (dict(qweight=P + 8), -2), (dict(scales=P + 4), -2),
    (dict(out_stride=260), -2)]
LINEAR_REFUSALS = SHAPE_REFUSALS + [
    (dict(O=24, y_stride=24), -1), (dict(O=0), -1), (dict(N=0), -1), (dict(N=-3), -1), (dict(N=2 ** 26, O=32), -1),
    (dict(N=2 ** 19, O=4096, y_stride=4096), -1), (dict(x_stride=248), -1), (dict(y_stride=28), -1), (dict(x=None), -1),
    (dict(qweight=None), -1), (dict(scales=None), -1), (dict(mins=None), -1), (dict(y=None), -1), (dict(x=P + 8), -2),
    (dict(qweight=P + 8), -2), (dict(scales=P + 4), -2), (dict(mins=P + 2), -2), (dict(y=P + 4), -2), (dict(bias=P + 1), -2),
    (dict(x_stride=260), -2), (dict(y_stride=34), -2)]
GATE_UP_REFUSALS = SHAPE_REFUSALS + [
    (dict(I=24, y_stride=24), -1), (dict(N=0), -1), (dict(N=2 ** 26), -1), (dict(x_stride=248), -1), (dict(y_stride=16), -1),
    (dict(x=None), -1), (dict(gq=None), -1), (dict(gs=None), -1), (dict(gm=None), -1), (dict(uq=None), -1), (dict(us=None), -1),
    (dict(um=None), -1), (dict(y=None), -1), (dict(uq=P + 8), -2), (dict(us=P + 4), -2), (dict(um=P + 2), -2), (dict(y=P + 2), -2),
    (dict(x_stride=260), -2), (dict(y_stride=34), -2)]


def _refused(entry, args, rc):
    _l, lib = _lib()
    assert getattr(lib, entry)(*args) == rc, lib.kivi_last_error()
    assert entry.encode() in lib.kivi_last_error()


@pytest.mark.parametrize("change,rc", PACK_REFUSALS, ids=[str(c) for c, _ in PACK_REFUSALS])
def test_pack_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w4_pack", _pack_args(**change), rc)


@pytest.mark.parametrize("change,rc", DEQUANT_REFUSALS, ids=[str(c) for c, _ in DEQUANT_REFUSALS])
def test_dequant_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w4_dequant", _dequant_args(**change), rc)


@pytest.mark.parametrize("change,rc", LINEAR_REFUSALS, ids=[str(c) for c, _ in LINEAR_REFUSALS])
def test_linear_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w4_linear", _linear_args(**change), rc)


@pytest.mark.parametrize("change,rc", GATE_UP_REFUSALS, ids=[str(c) for c, _ in GATE_UP_REFUSALS])
def test_gate_up_refuses_before_anything_is_enqueued(change, rc):
    _refused("kivi_w4_gate_up", _gate_up_args(**change), rc)


def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "w4_plan")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "w4_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "w4 plan ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ the layout in torch
def _random_triple(O, K, G, seed):
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(-2 ** 31, 2 ** 31 - 1, (O, K // 8), generator=g, dtype=torch.int64).to(torch.int32)
    scale = torch.randint(-2 ** 15, 2 ** 15 - 1, (O, K // G), generator=g, dtype=torch.int64).to(torch.int16).view(torch.float16)
    mn = torch.randint(-2 ** 15, 2 ** 15 - 1, (O, K // G), generator=g, dtype=torch.int64).to(torch.int16).view(torch.float16)
    return code, scale, mn


@pytest.mark.parametrize("O,K,G", [(16, 128, 64), (16, 128, 128), (48, 384, 64), (32, 896, 128)])
def test_to_ref_and_from_ref_invert_each_other(O, K, G):
    from kivi_amd import wquant
    code, scale, mn = _random_triple(O, K, G, O + K + G)
    q, s, m = wquant.from_ref(code, scale, mn, G)
    assert (tuple(q.shape), tuple(s.shape), tuple(m.shape)) == wquant.shapes(O, K, G)
    assert q.dtype == torch.int32 and s.dtype == torch.int16 and m.dtype == torch.int16
    c2, s2, m2 = wquant.to_ref(q, s, m)
    assert torch.equal(c2, code) and torch.equal(s2.view(torch.int16), scale.view(torch.int16))
    assert torch.equal(m2.view(torch.int16), mn.view(torch.int16))
    g = torch.Generator().manual_seed(1)                    # ... and the reverse, from a random device triple
    q = torch.randint(-2 ** 31, 2 ** 31 - 1, q.shape, generator=g, dtype=torch.int64).to(torch.int32)
    s = torch.randint(-2 ** 15, 2 ** 15 - 1, s.shape, generator=g, dtype=torch.int64).to(torch.int16)
    q2, s2, m2 = wquant.from_ref(*wquant.to_ref(q, s, m), G)
    assert torch.equal(q2, q) and torch.equal(s2, s) and torch.equal(m2, m)


@pytest.mark.parametrize("G", [64, 128])
def test_from_ref_of_the_oracles_pack_follows_the_documented_formula(G):
    from kivi_amd import wquant
    O, K = 32, 384
    w = R.weights("outlier", O, K, G, torch.float16, 7)
    code, scale, mn = R.oracle_triple(w, G)
    q, s, m = wquant.from_ref(code, scale, mn, G)
    flat, sflat, mflat = q.reshape(-1).to(torch.int64) & 0xFFFFFFFF, s.reshape(-1), m.reshape(-1)
    codes = R.codes_of(code)
    assert int(codes.max()) == 15 and int(codes.min()) == 0
    for o in range(O):
        for k in range(K):
            word, bit = R.word_bit(o, k, K)
            assert (int(flat[word]) >> bit) & 15 == int(codes[o, k]), (o, k)
        for g in range(K // G):
            h = R.sm_half(o, g, K, G)
            assert int(sflat[h]) == int(scale.view(torch.int16)[o, g]) and int(mflat[h]) == int(mn.view(torch.int16)[o, g]), (o, g)
    # the torch statement of the quantiser agrees with the oracle on this weight, and dequant_torch with the fp64 contract
    c2, s2, m2 = wquant.quantize_ref(w, G)
    assert torch.equal(c2, code) and torch.equal(s2, scale) and torch.equal(m2, mn)
    wt = R.represented(code, scale, mn, G)
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(wquant.dequant_torch(q, s, m, dtype), wt.float().to(dtype))


def test_usable_and_shapes():
    from kivi_amd import wquant
    assert wquant.usable(16, 128, 64) and wquant.usable(4096, 11008, 128) and wquant.usable(1024, 4096)
    for o, k, g in ((24, 128, 64), (16, 192, 64), (16, 64, 64), (16, 128, 32), (0, 128, 64), (16, 128, 256)):
        assert not wquant.usable(o, k, g)
        with pytest.raises(ValueError):
            wquant.shapes(o, k, g)
    assert wquant.shapes(48, 384, 64) == ((3, 3, 256), (3, 6, 16), (3, 6, 16))
    x = torch.zeros((2, 128), dtype=torch.float16)
    lin = wquant.QuantLinear(128, 16)
    with pytest.raises(Exception, match="GPU"):                 # no CPU path, no fallback
        lin(x)
    with pytest.raises(Exception, match="GPU"):
        wquant.pack(torch.zeros((16, 128), dtype=torch.float16))


# ------------------------------------------------------------------------------------------------ modules and configuration
def _cfg(**kw):
    d = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=384, vocab_size=64,
             head_dim=64)
    d.update(kw)
    return d


def test_quant_linear_state_dict_names_and_dtype_casts():
    from kivi_amd import wquant
    lin = wquant.QuantLinear(256, 48, bias=True, group=64)
    assert sorted(lin.state_dict()) == ["bias", "mins", "qweight", "scales"]
    assert sorted(wquant.QuantLinear(256, 48).state_dict()) == ["mins", "qweight", "scales"]
    assert tuple(lin.qweight.shape) == (3, 2, 256) and tuple(lin.scales.shape) == (3, 4, 16) and lin.scales.dtype == torch.int16
    g = torch.Generator().manual_seed(2)
    lin.scales.copy_(torch.randint(-2 ** 15, 2 ** 15 - 1, lin.scales.shape, generator=g, dtype=torch.int64).to(torch.int16))
    lin.mins.copy_(torch.randint(-2 ** 15, 2 ** 15 - 1, lin.mins.shape, generator=g, dtype=torch.int64).to(torch.int16))
    lin.qweight.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=g, dtype=torch.int64).to(torch.int32))
    before = {k: v.clone() for k, v in lin.state_dict().items()}
    for cast in (lambda m: m.bfloat16(), lambda m: m.half(), lambda m: m.to(torch.bfloat16), lambda m: m.float()):
        m = cast(lin)
        for name in ("qweight", "scales", "mins"):
            assert torch.equal(getattr(m, name), before[name]) and getattr(m, name).dtype == before[name].dtype, name
    assert lin.bias.dtype == torch.float32
    mlp = wquant.QuantMLP(256, 384, 128)
    assert sorted(mlp.state_dict()) == sorted(f"{p}_proj.{b}" for p in ("gate", "up", "down") for b in ("qweight", "scales", "mins"))


def test_make_config_plumbing_and_the_refusal_of_other_widths():
    from kivi_amd import wquant
    from kivi_amd.llama import MLP, LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, make_config
    for bad in (3, 2, 8, 16, "4", 0):
        with pytest.raises(ValueError, match="weight_bits"):
            make_config(_cfg(), weight_bits=bad)
    with pytest.raises(ValueError, match="weight_group"):
        make_config(_cfg(), weight_bits=4, weight_group=32)
    cfg = make_config(_cfg(), weight_bits=4, weight_group=64, weight_kernel_max_tokens=7)
    assert (cfg.kivi_weight_bits, cfg.kivi_weight_group, cfg.kivi_weight_kernel_max_tokens) == (4, 64, 7)
    model = LlamaForCausalLM_KIVI(cfg)
    for layer in model.model.layers:
        att = layer.self_attn
        for lin, (o, k) in ((att.q_proj, (256, 256)), (att.k_proj, (128, 256)), (att.v_proj, (128, 256)), (att.o_proj, (256, 256))):
            assert type(lin) is wquant.QuantLinear and (lin.out_features, lin.in_features, lin.group) == (o, k, 64)
            assert lin.kernel_max_tokens == 7 and lin.bias is None
        assert type(layer.mlp) is wquant.QuantMLP and layer.mlp.down_proj.in_features == 384
    assert type(model.lm_head) is torch.nn.Linear and type(model.model.embed_tokens) is torch.nn.Embedding
    assert not any(k.endswith("_proj.weight") for k in model.state_dict())
    assert "model.layers.1.mlp.up_proj.scales" in model.state_dict() and "model.layers.0.self_attn.k_proj.qweight" in model.state_dict()
    # Qwen2's biases ride on the quantised projections; o_proj carries none
    q2 = Qwen2ForCausalLM_KIVI(make_config(_cfg(), weight_bits=4))
    att = q2.model.layers[0].self_attn
    assert type(att.q_proj) is wquant.QuantLinear and att.q_proj.bias is not None and att.v_proj.bias is not None
    assert type(att.o_proj) is wquant.QuantLinear and att.o_proj.bias is None and att.q_proj.kernel_max_tokens == wquant.KERNEL_MAX_TOKENS
    # a shape the kernels do not serve stays an nn.Linear, projection by projection: with hidden 192 (no multiple of 128) q / k / v
    # reduce over 192 and stay dense, o_proj reduces over 4 * 64 = 256 into 192 = 12 * 16 rows and is quantised; the MLP stays whole
    odd = LlamaForCausalLM_KIVI(make_config(_cfg(hidden_size=192, head_dim=64, intermediate_size=256), weight_bits=4))
    att = odd.model.layers[0].self_attn
    assert type(att.q_proj) is torch.nn.Linear and type(att.v_proj) is torch.nn.Linear and type(att.o_proj) is wquant.QuantLinear
    assert type(odd.model.layers[0].mlp) is MLP and type(odd.model.layers[0].mlp.down_proj) is torch.nn.Linear


def test_sparse_models_quantise_attention_and_dense_layers_only():
    from kivi_amd import wquant
    from kivi_amd.llama import Qwen3MoeForCausalLM_KIVI, make_config
    from kivi_amd.moe import SparseMoeBlock
    d = _cfg(model_type="qwen3_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=128, mlp_only_layers=[0],
             norm_topk_prob=True)
    model = Qwen3MoeForCausalLM_KIVI(make_config(d, weight_bits=4))
    assert type(model.model.layers[0].mlp) is wquant.QuantMLP and type(model.model.layers[1].mlp) is SparseMoeBlock
    assert model.model.layers[1].mlp.experts.gate_up_proj.dtype == torch.float32
    assert all(type(layer.self_attn.q_proj) is wquant.QuantLinear for layer in model.model.layers)


def test_the_default_config_builds_the_module_tree_it_built_before():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, make_config
    plain, none = make_config(_cfg()), make_config(_cfg(), weight_bits=None, weight_group=64, weight_kernel_max_tokens=5)
    assert vars(plain) == vars(none) and not any(k.startswith("kivi_weight") for k in vars(plain))
    for cls in (LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI):
        a, b = cls(plain), cls(none)
        assert list(a.state_dict()) == list(b.state_dict())
        assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
        assert not any(k.endswith(("qweight", "scales", "mins")) for k in a.state_dict())
        names = set(a.state_dict())
        for i in range(2):
            for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                      "mlp.down_proj"):
                assert f"model.layers.{i}.{n}.weight" in names
        assert all(type(m) is not __import__("kivi_amd.wquant", fromlist=["QuantLinear"]).QuantLinear for m in a.modules())


def test_save_quantized_needs_a_quantised_model(tmp_path):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    with pytest.raises(ValueError, match="weight_bits"):
        LlamaForCausalLM_KIVI(make_config(_cfg())).save_quantized(str(tmp_path))
