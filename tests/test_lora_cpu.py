"""No GPU: per-request LoRA adapters (kivi_amd/lora.py) everywhere but on the device.

1. The entries exist with their signatures, the ABI version is still 3, and every refusal of kivi_lora_shrink / kivi_lora_expand is
   reached with fake pointers: a refused call enqueues nothing, so no device is needed.
2. tests/lora_plan_main.cpp, a stand-alone program over kivi_amd/csrc/kivi_lora_plan.h that walks every block, wave and lane of both
   launches over buffers of exactly the stated sizes, built with -fsanitize=address,undefined and run as a child process.
3. apply_torch against the fp64 statement (tests/lora_ref.py) within its bound; rows of slot -1 and a zero B (PEFT's
   initialisation) leave y bit-unchanged; the same r = 5 adapter in tables of rank 8 and 64 gives the same bits.
4. LoraAdapter.from_peft on directories the test writes: names, the fp32 -> dtype cast, both scale rules, every refusal with its
   field or key in the message.  LoraSet.load / unload, nbytes.
5. enable_lora leaves the module names and state_dict() keys what they were; `adapters=` is checked by every entry point before a
   pass runs."""
import json
import os
import shutil
import subprocess

import pytest
import torch

import lora_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 16, 0x110
P = 0x10000          # a fake, 16-byte aligned pointer: a refused call never follows it


def _lib():
    from kivi_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------------ the C entries
def test_entries_exist_and_the_abi_version_stays_3():
    _l, lib = _lib()
    assert lib.kivi_abi_version() == 3 == _l.ABI_VERSION
    for name, n_args in (("kivi_lora_shrink", 13), ("kivi_lora_expand", 14)):
        assert name in _l.SIGNATURES and len(_l.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    for name in ("kivi_lora_shrink(", "kivi_lora_expand(", "#define KIVI_ABI_VERSION 3"):
        assert name in header
    from kivi_amd import build
    assert "kivi_lora.hip" in build.SOURCES


def _shrink_args(**kw):
    a = dict(x=P, x_stride=64, dtype=F16, N=15, Q=5, K=64, slots=P, S=3, R=16, ranks=P, A=P, t=P, stream=None)
    a.update(kw)
    return list(a.values())


def _expand_args(**kw):
    a = dict(t=P, slots=P, S=3, R=16, ranks=P, scale=P, B=P, y=P, y_stride=64, dtype=F16, N=15, Q=5, O=64, stream=None)
    a.update(kw)
    return list(a.values())


SHRINK_REFUSALS = [
    (dict(dtype=32), -1), (dict(dtype=0), -1), (dict(N=0), -1), (dict(Q=0), -1), (dict(N=16), -1), (dict(N=2 ** 31, Q=1), -1),
    (dict(K=0), -1), (dict(K=12, x_stride=16), -1), (dict(K=-8), -1), (dict(S=0), -1), (dict(R=0), -1), (dict(R=4), -1), (dict(R=24), -1),
    (dict(R=128), -1), (dict(x_stride=56), -1), (dict(x=None), -1), (dict(slots=None), -1), (dict(ranks=None), -1), (dict(A=None), -1),
    (dict(t=None), -1), (dict(x=P + 8), -2), (dict(A=P + 2), -2), (dict(x_stride=68), -2), (dict(slots=P + 2), -2),
    (dict(ranks=P + 1), -2), (dict(t=P + 2), -2),
]
EXPAND_REFUSALS = [
    (dict(dtype=32), -1), (dict(N=0), -1), (dict(Q=0), -1), (dict(N=16), -1), (dict(O=0), -1), (dict(O=12, y_stride=16), -1),
    (dict(O=512 * 65535 + 8, y_stride=512 * 65535 + 8), -1), (dict(S=0), -1), (dict(R=12), -1), (dict(R=0), -1), (dict(y_stride=62), -1),
    (dict(t=None), -1), (dict(slots=None), -1), (dict(ranks=None), -1), (dict(scale=None), -1), (dict(B=None), -1), (dict(y=None), -1),
    (dict(B=P + 8), -2), (dict(y=P + 2), -2), (dict(y_stride=65), -2), (dict(scale=P + 2), -2), (dict(t=P + 1), -2),
    (dict(slots=P + 2), -2), (dict(ranks=P + 2), -2),
]


@pytest.mark.parametrize("change,rc", SHRINK_REFUSALS, ids=[str(c) for c, _ in SHRINK_REFUSALS])
def test_shrink_refuses_before_anything_is_enqueued(change, rc):
    _l, lib = _lib()
    assert lib.kivi_lora_shrink(*_shrink_args(**change)) == rc, lib.kivi_last_error()
    assert b"kivi_lora_shrink" in lib.kivi_last_error()


@pytest.mark.parametrize("change,rc", EXPAND_REFUSALS, ids=[str(c) for c, _ in EXPAND_REFUSALS])
def test_expand_refuses_before_anything_is_enqueued(change, rc):
    _l, lib = _lib()
    assert lib.kivi_lora_expand(*_expand_args(**change)) == rc, lib.kivi_last_error()
    assert b"kivi_lora_expand" in lib.kivi_last_error()


def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "lora_plan")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "lora_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "lora plan ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ apply_torch
def _case(dtype, K, O, Rk, ranks, Bt, Q, seed):
    A, B, scale, rk = R.tables(len(ranks), Rk, K, O, ranks, dtype, "cpu", seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((Bt, Q, K), generator=g).to(dtype)
    y = torch.randn((Bt, Q, O), generator=g).to(dtype)
    return A, B, scale, rk, x, y


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,O,Rk,ranks", [(24, 8, 8, (1, 5, 8)), (256, 264, 64, (5, 8, 64)), (1032, 8, 8, (8, 1, 5))])
def test_apply_torch_against_the_fp64_statement(dtype, K, O, Rk, ranks):
    from kivi_amd import lora
    worst = 0.0
    for Bt, Q, slots in ((1, 1, [1]), (3, 5, [2, -1, 0]), (17, 1, [0, 1, 2, -1, 1, 1, 0, -1, 2, 0, 0, 1, -1, 2, 2, 1, 0])):
        A, B, scale, rk, x, y0 = _case(dtype, K, O, Rk, ranks, Bt, Q, K + O + Bt)
        y = lora.apply_torch(y0.clone(), x, A, B, scale.tolist(), rk.tolist(), slots)
        y64, mag = R.statement64(y0, x, A, B, scale, slots)
        worst = max(worst, R.worst_ratio(y, y0, y64, mag, K, Rk, dtype))
        for b, s in enumerate(slots):
            if s < 0:
                assert torch.equal(y[b], y0[b]), b                      # the base model's rows: bit-unchanged
            else:
                assert not torch.equal(y[b], y0[b]), b
        none = lora.apply_torch(y0.clone(), x, A, B, scale.tolist(), rk.tolist(), [-1] * Bt)
        assert torch.equal(none, y0)
    print(f"{dtype} K={K} O={O} R={Rk}: worst |apply_torch - fp64| / bound = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_zero_B_leaves_y_bit_unchanged_and_the_table_rank_does_not_matter(dtype):
    from kivi_amd import lora
    K, O, Bt, Q = 256, 264, 3, 5
    A, B, scale, rk, x, y0 = _case(dtype, K, O, 8, (5, 5, 5), Bt, Q, 3)
    zero = lora.apply_torch(y0.clone(), x, A, torch.zeros_like(B), scale.tolist(), rk.tolist(), [0, 1, 2])
    assert torch.equal(zero, y0)                                        # PEFT initialises B with zeros: the adapter is the base model
    A64, B64 = torch.zeros((3, 64, K), dtype=dtype), torch.zeros((3, O, 64), dtype=dtype)
    A64[:, :8], B64[:, :, :8] = A, B
    small = lora.apply_torch(y0.clone(), x, A, B, scale.tolist(), rk.tolist(), [0, -1, 2])
    large = lora.apply_torch(y0.clone(), x, A64, B64, scale.tolist(), rk.tolist(), [0, -1, 2])
    assert torch.equal(small, large) and not torch.equal(small, y0)


# ------------------------------------------------------------------------------------------------ PEFT directories
def _write_peft(path, tensors, **cfg):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    base = dict(peft_type="LORA", r=4, lora_alpha=8, target_modules=["q_proj", "v_proj"], bias="none", use_dora=False,
                use_rslora=False, fan_in_fan_out=False, modules_to_save=None, rank_pattern={}, alpha_pattern={})
    base.update(cfg)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(base, f)
    save_file({k: v.contiguous() for k, v in tensors.items()}, os.path.join(path, "adapter_model.safetensors"))
    return str(path)


def _peft_tensors(r=4, K=64, O=32, layers=2, mods=("q_proj", "v_proj"), dtype=torch.float32):
    g = torch.Generator().manual_seed(7)
    t = {}
    for i in range(layers):
        for m in mods:
            base = f"base_model.model.model.layers.{i}.self_attn.{m}"
            t[base + ".lora_A.weight"] = torch.randn((r, K), generator=g).to(dtype)
            t[base + ".lora_B.weight"] = torch.randn((O, r), generator=g).to(dtype)
    return t


def test_from_peft_reads_names_shapes_and_both_scale_rules(tmp_path):
    from kivi_amd.lora import LoraAdapter
    t = _peft_tensors()
    ad = LoraAdapter.from_peft(_write_peft(tmp_path / "a", t))
    assert sorted(ad.tensors) == [f"model.layers.{i}.self_attn.{m}" for i in range(2) for m in ("q_proj", "v_proj")]
    a, b = ad.tensors["model.layers.1.self_attn.v_proj"]
    assert torch.equal(a, t["base_model.model.model.layers.1.self_attn.v_proj.lora_A.weight"]) and tuple(b.shape) == (32, 4)
    assert (ad.r, ad.alpha, ad.rslora, ad.scale) == (4, 8.0, False, 2.0)
    rs = LoraAdapter.from_peft(_write_peft(tmp_path / "b", t, use_rslora=True, lora_alpha=6))
    assert rs.rslora and rs.scale == 6 / 4 ** 0.5 == 3.0


REFUSED_CONFIGS = [(dict(use_dora=True), "use_dora"), (dict(bias="all"), "bias"), (dict(bias="lora_only"), "bias"),
                   (dict(modules_to_save=["lm_head"]), "modules_to_save"), (dict(rank_pattern={"q_proj": 8}), "rank_pattern"),
                   (dict(alpha_pattern={"q_proj": 4}), "alpha_pattern"), (dict(fan_in_fan_out=True), "fan_in_fan_out")]


@pytest.mark.parametrize("cfg,field", REFUSED_CONFIGS, ids=[f for _, f in REFUSED_CONFIGS])
def test_from_peft_refuses_what_is_out_of_scope_by_field(cfg, field, tmp_path):
    from kivi_amd.lora import LoraAdapter
    with pytest.raises(ValueError, match=field):
        LoraAdapter.from_peft(_write_peft(tmp_path / "a", _peft_tensors(), **cfg))


def test_from_peft_refuses_keys_by_name(tmp_path):
    from kivi_amd.lora import LoraAdapter
    t = _peft_tensors()
    lone = dict(t)
    lone.pop("base_model.model.model.layers.1.self_attn.q_proj.lora_B.weight")
    with pytest.raises(ValueError, match=r"layers\.1\.self_attn\.q_proj\.lora_B"):
        LoraAdapter.from_peft(_write_peft(tmp_path / "a", lone))
    lone = dict(t)
    lone.pop("base_model.model.model.layers.0.self_attn.v_proj.lora_A.weight")
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.v_proj\.lora_A"):
        LoraAdapter.from_peft(_write_peft(tmp_path / "b", lone))
    for i, key in enumerate(("base_model.model.model.embed_tokens.lora_A.weight", "base_model.model.lm_head.lora_B.weight",
                             "base_model.model.model.layers.0.mlp.gate.lora_A.weight",
                             "base_model.model.model.layers.0.mlp.experts.3.down_proj.lora_A.weight",
                             "base_model.model.model.layers.0.block_sparse_moe.experts.1.w1.lora_B.weight")):
        bad = dict(t)
        bad[key] = torch.zeros((4, 64))
        with pytest.raises(ValueError, match=key.rsplit(".", 3)[1]):
            LoraAdapter.from_peft(_write_peft(tmp_path / f"k{i}", bad))
    bad = dict(t)
    bad["base_model.model.model.layers.0.self_attn.q_proj.lora_magnitude_vector"] = torch.zeros(32)
    with pytest.raises(ValueError, match="lora_magnitude_vector"):
        LoraAdapter.from_peft(_write_peft(tmp_path / "m", bad))


# ------------------------------------------------------------------------------------------------ the set, on a CPU model
def _cfg(**kw):
    d = dict(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=160, vocab_size=64,
             head_dim=16)
    d.update(kw)
    return d


def _model(dtype=torch.float32, **kw):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    torch.manual_seed(0)
    return LlamaForCausalLM_KIVI(make_config(_cfg(**kw))).to(dtype).eval()


def test_enable_lora_keeps_the_module_tree_and_the_state_dict():
    from kivi_amd import lora
    model = _model()
    names, keys = [n for n, _ in model.named_modules()], list(model.state_dict())
    buffers = [n for n, _ in model.named_buffers()]
    lset = model.enable_lora(3, 16, lora.TARGETS)
    assert isinstance(lset, lora.LoraSet) and model.lora is lset and lset.active is None
    assert [n for n, _ in model.named_modules()] == names and list(model.state_dict()) == keys
    assert [n for n, _ in model.named_buffers()] == buffers
    assert len(lset.modules) == 2 * 7 and all(len(m._forward_hooks) == 1 for m in lset.modules.values())
    # S R (K + O) 2 bytes per target, 8 S for scale and ranks: q, o 64 -> 64; k, v 64 -> 32; gate, up 64 -> 160; down 160 -> 64
    per_layer = 2 * (64 + 64) + 2 * (64 + 32) + 2 * (64 + 160) + (160 + 64)
    assert lset.nbytes == 2 * 3 * 16 * per_layer * 4 + 8 * 3            # (the CPU model is fp32: 4 bytes an element)
    model.disable_lora()
    assert model.lora is None and all(not m._forward_hooks for m in lset.modules.values())
    assert [n for n, _ in model.named_modules()] == names and list(model.state_dict()) == keys
    default = model.enable_lora(2, 8)
    assert sorted({n.rsplit(".", 1)[1] for n in default.modules}) == ["q_proj", "v_proj"]
    for bad in (dict(max_adapters=0), dict(max_rank=12), dict(target_modules=("lm_head",)), dict(target_modules=("experts",)),
                dict(target_modules=())):
        kw = dict(max_adapters=2, max_rank=8, target_modules=("q_proj",))
        kw.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            model.enable_lora(**kw)


def test_load_casts_once_checks_shapes_and_unload_zeroes(tmp_path):
    from kivi_amd import lora
    model = _model(torch.bfloat16)
    lset = model.enable_lora(2, 8, ("q_proj", "v_proj"))
    t = {}
    g = torch.Generator().manual_seed(1)
    for i in range(2):
        for m, O in (("q_proj", 64), ("v_proj", 32)):
            base = f"base_model.model.model.layers.{i}.self_attn.{m}"
            t[base + ".lora_A.weight"] = torch.randn((5, 64), generator=g)
            t[base + ".lora_B.weight"] = torch.randn((O, 5), generator=g)
    ad = lora.LoraAdapter.from_peft(_write_peft(tmp_path / "a", t, r=5, lora_alpha=10))
    ptrs = {n: (lset.A[n].data_ptr(), lset.B[n].data_ptr()) for n in lset.modules}
    assert lset.load(ad) == 0 and lset.load(ad) == 1
    name = "model.layers.1.self_attn.v_proj"
    a32 = t[f"base_model.model.{name}.lora_A.weight"]
    assert torch.equal(lset.A[name][1, :5], a32.bfloat16()) and not torch.equal(lset.A[name][1, :5].float(), a32)   # rounded once
    assert bool((lset.A[name][1, 5:] == 0).all()) and bool((lset.B[name][1, :, 5:] == 0).all())
    assert lset.ranks.tolist() == [5, 5] and lset.scale.tolist() == [2.0, 2.0] and lset.ranks_host == [5, 5]
    assert ptrs == {n: (lset.A[n].data_ptr(), lset.B[n].data_ptr()) for n in lset.modules}      # in place: addresses never change
    with pytest.raises(ValueError, match="slots hold"):
        lset.load(ad)
    assert lset.load(ad, slot=1) == 1
    lset.unload(0)
    assert bool((lset.A[name][0] == 0).all()) and bool((lset.B[name][0] == 0).all()) and lset.ranks.tolist() == [0, 5]
    assert lset.scale.tolist() == [0.0, 2.0]
    big = lora.LoraAdapter({name: (torch.zeros(16, 64), torch.zeros(32, 16))}, 16, 16)
    with pytest.raises(ValueError, match="max_rank"):
        lset.load(big, 0)
    with pytest.raises(ValueError, match=r"layers\.1\.self_attn\.v_proj"):
        lset.load(lora.LoraAdapter({name: (torch.zeros(4, 64), torch.zeros(64, 4))}, 4, 8), 0)
    with pytest.raises(KeyError, match=r"layers\.0\.mlp\.down_proj"):
        lset.load(lora.LoraAdapter({"model.layers.0.mlp.down_proj": (torch.zeros(4, 160), torch.zeros(64, 4))}, 4, 8), 0)
    assert lset.ranks.tolist() == [0, 5]                                    # a refused load wrote nothing
    for bad in (-1, 2, True, 1.0):
        with pytest.raises(ValueError, match="slot"):
            lset.load(ad, slot=bad)


def test_the_hook_applies_the_binding_and_none_is_the_base_linear():
    """A target linear on the CPU: its hook runs apply_torch under a binding and returns at once without one."""
    from kivi_amd import lora
    model = _model(torch.bfloat16)
    lset = model.enable_lora(2, 8, ("q_proj",))
    lset.load(R.make_adapter(model, 5, 10.0, 2, ("q_proj",)), 0)
    q = model.model.layers[0].self_attn.q_proj
    x = torch.randn((3, 4, 64), generator=torch.Generator().manual_seed(3)).bfloat16()
    base = torch.nn.functional.linear(x, q.weight)
    assert torch.equal(q(x), base)
    binding = lora.RowBinding(3, "cpu", [0, None, 1])
    assert binding.host == [0, -1, 1] and binding.slots.tolist() == [0, -1, 1] and binding.key() == ("lora", 3, binding.slots.data_ptr())
    with lset.bound(binding):
        y = q(x)
    assert lset.active is None and torch.equal(q(x), base)
    assert torch.equal(y[1], base[1]) and torch.equal(y[2], base[2]) and not torch.equal(y[0], base[0])     # slot 1 is empty
    name = "model.layers.0.self_attn.q_proj"
    y64, mag = R.statement64(base, x, lset.A[name], lset.B[name], lset.scale, [0, -1, 1])
    assert R.worst_ratio(y, base, y64, mag, 64, 8, torch.bfloat16) <= 1.0
    binding.set_row(1, 0)
    binding.set_row(0, None)
    assert binding.host == [-1, 0, 1] and binding.slots.tolist() == [-1, 0, 1]
    with pytest.raises(ValueError, match="rows"):
        binding.bind([0, 1])
    with lset.bound(lora.RowBinding(2, "cpu", [0, 0])), pytest.raises(ValueError, match="3 rows"):
        q(x)


# ------------------------------------------------------------------------------------------------ adapters= of the entry points
BAD_ADAPTERS = ["0", 1.5, True, [0], [0, 3], [0, -2], [0, 1.0], (0, True)]


def _entry_points(model):
    ids = torch.zeros((2, 4), dtype=torch.long)
    return {
        "forward": lambda a: model.forward(ids, adapters=a),
        "score": lambda a: model.score(ids, adapters=a),
        "perplexity": lambda a: model.perplexity(ids, adapters=a),
        "generate": lambda a: model.generate(ids, 2, adapters=a),
        "generate_graphed": lambda a: model.generate_graphed(ids, 2, adapters=a),
        "decode_graphed": lambda a: model.decode_graphed(ids[:, :1], None, 4, 1, adapters=a),
        "generate_continuous": lambda a: model.generate_continuous([[1, 2], [3]], 2, 2, adapters=a),
        "admit_": lambda a: model.admit_(None, [0, 1], ids, torch.ones_like(ids), adapters=a),
    }


@pytest.mark.parametrize("entry", ["forward", "score", "perplexity", "generate", "generate_graphed", "decode_graphed",
                                   "generate_continuous", "admit_"])
def test_adapters_is_checked_before_a_pass_runs(entry):
    model = _model()
    with pytest.raises(ValueError, match="enable_lora"):
        _entry_points(model)[entry](0)                                  # no adapters without enable_lora
    model.enable_lora(3, 8)
    call = _entry_points(model)[entry]
    for bad in BAD_ADAPTERS:
        with pytest.raises(ValueError, match="adapters|slot"):
            call(bad)
    assert model.lora.active is None


def test_resolve_adapters_and_the_fan():
    from kivi_amd import lora
    assert lora.resolve_adapters(None, 3, 4) is None and lora.resolve_adapters([None, -1, None], 3, 4) is None
    assert lora.resolve_adapters(2, 3, 4) == [2, 2, 2] and lora.resolve_adapters([0, None, 3], 3, 4) == [0, -1, 3]
    assert lora.resolve_adapters((1, -1), 2, 2) == [1, -1]
    model = _model()
    model.enable_lora(4, 8)
    with lora.call_binding(model, [2, None], 2, fan=3) as b:
        assert b.host == [2, 2, 2, -1, -1, -1] and b.prompt.host == [2, -1] and model.lora.active is b
        assert b.for_rows(6) is b and b.for_rows(2) is b.prompt
        with lora.call_binding(model, None, 2):                         # an inner call without adapters keeps the outer binding
            assert model.lora.active is b
        with lora.call_binding(model, [None, None], 2):                 # an explicit base-model call does not
            assert model.lora.active is None
    assert model.lora.active is None
    with lora.call_binding(model, [1, 0], 2, kept=True) as k1:
        pass
    with lora.call_binding(model, [0, None], 2, kept=True) as k2:
        assert k2 is k1 and k2.host == [0, -1] and k2.slots.tolist() == [0, -1]      # rebound in place: the key stays
