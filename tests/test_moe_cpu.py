"""No GPU: the sparse expert block (kivi_amd/moe.py) everywhere but on the device.

1. The entries exist with their signatures, the ABI version is still 3, and every refusal of kivi_moe_route / kivi_moe_experts is
   reached with fake pointers: a refused call enqueues nothing, so no device is needed (the library loads without one).
2. tests/moe_plan_main.cpp, a stand-alone program over kivi_amd/csrc/kivi_moe_plan.h (tile bound against adversarial count vectors,
   grid and workspace sizes, the shape refusals), built with -fsanitize=address,undefined and run as a child process.
3. route_torch / experts_torch / SparseMoeBlock on the CPU in fp32 against transformers' MixtralSparseMoeBlock and
   Qwen3MoeSparseMoeBlock holding the same weights, and against the fp64 restatement tests/moe_ref.py: max |delta| <= 1e-5 of the
   reference's rms.  (The HF fp32 blocks themselves sit at 1.3-1.5e-6 of the fp64 restatement at E = 8 / K = 2 and E = 12 / K = 4,
   H = 64: the bar has about 7x room.)
4. The layer-kind rule against HF's Qwen3MoeDecoderLayer for decoder_sparse_step 1 and 2 with mlp_only_layers; the translation of
   checkpoint names for the three spellings (kivi_amd/loading.py); the refusal of shared experts."""
import os
import shutil
import subprocess

import pytest
import torch

import moe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
F16, BF16 = 16, 0x110


def _lib():
    from kivi_amd import _lib
    return _lib, _lib.load()


def test_entries_exist_and_the_abi_version_stays_3():
    _l, lib = _lib()
    assert lib.kivi_abi_version() == 3 == _l.ABI_VERSION
    for name, n_args in (("kivi_moe_route", 16), ("kivi_moe_experts", 20), ("kivi_moe_max_tiles", 3), ("kivi_moe_workspace_bytes", 5)):
        assert name in _l.SIGNATURES and len(_l.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    for name in ("kivi_moe_route(", "kivi_moe_experts(", "kivi_moe_max_tiles(", "kivi_moe_workspace_bytes(", "#define KIVI_ABI_VERSION 3"):
        assert name in header
    assert "#define KIVI_MOE_TOKEN_TILE 16" in header and _l.MOE_TOKEN_TILE == 16
    from kivi_amd import moe
    assert moe.TOKEN_TILE == 16 and moe.max_tiles(5, 8, 2) == lib.kivi_moe_max_tiles(5, 8, 2) == 8
    assert moe.max_tiles(1000, 128, 8) == lib.kivi_moe_max_tiles(1000, 128, 8) == 128 + 500
    assert lib.kivi_moe_workspace_bytes(5, 256, 96, 8, 2) == 10 * 96 * 2 + 10 * 256 * 4
    assert lib.kivi_moe_max_tiles(0, 8, 2) == -1 and lib.kivi_moe_workspace_bytes(5, 250, 96, 8, 2) == -1


P = 0x10000          # a fake, 16-byte aligned pointer: a refused call never follows it


def _route_args(**kw):
    a = dict(logits=P, row_stride=8, dtype=F16, N=4, E=8, top_k=2, flags=3, idx=P, w=P, counts=P, offsets=P, pairs=P, pos=P, tiles=P,
             n_tiles=P, stream=None)
    a.update(kw)
    return list(a.values())


def _experts_args(**kw):
    a = dict(x=P, x_stride=64, dtype=F16, N=4, H=64, I=96, E=8, top_k=2, w=P, pairs=P, pos=P, tiles=P, n_tiles=P, gate_up=P, down=P,
             out=P, out_stride=64, workspace=P, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return list(a.values())


ROUTE_REFUSALS = [
    (dict(dtype=32), -1), (dict(dtype=0), -1), (dict(N=0), -1), (dict(E=0), -1), (dict(E=257, row_stride=257), -1),
    (dict(top_k=0), -1), (dict(top_k=9), -1), (dict(E=64, row_stride=64, top_k=17), -1), (dict(N=2 ** 30, top_k=2), -1),
    (dict(flags=4), -1), (dict(row_stride=7), -1), (dict(logits=None), -1), (dict(idx=None), -1), (dict(w=None), -1),
    (dict(counts=None), -1), (dict(offsets=None), -1), (dict(pairs=None), -1), (dict(pos=None), -1), (dict(tiles=None), -1),
    (dict(n_tiles=None), -1), (dict(logits=P + 1), -2), (dict(idx=P + 2), -2), (dict(w=P + 2), -2), (dict(n_tiles=P + 1), -2),
]
EXPERTS_REFUSALS = [
    (dict(dtype=32), -1), (dict(N=0), -1), (dict(E=0), -1), (dict(E=300), -1), (dict(top_k=0), -1), (dict(top_k=9), -1),
    (dict(H=48, x_stride=48, out_stride=48), -1), (dict(I=80), -1), (dict(H=0), -1), (dict(I=0), -1), (dict(x_stride=56), -1),
    (dict(out_stride=60), -1), (dict(workspace_bytes=8 * 96 * 2 + 8 * 64 * 4 - 1), -1), (dict(x=None), -1), (dict(w=None), -1),
    (dict(pairs=None), -1), (dict(pos=None), -1), (dict(tiles=None), -1), (dict(n_tiles=None), -1), (dict(gate_up=None), -1),
    (dict(down=None), -1), (dict(out=None), -1), (dict(workspace=None), -1), (dict(x=P + 8), -2), (dict(gate_up=P + 2), -2),
    (dict(down=P + 4), -2), (dict(workspace=P + 8), -2), (dict(out=P + 4), -2), (dict(x_stride=68), -2), (dict(out_stride=66), -2),
    (dict(w=P + 2), -2), (dict(pos=P + 1), -2),
]


@pytest.mark.parametrize("change,rc", ROUTE_REFUSALS, ids=[str(c) for c, _ in ROUTE_REFUSALS])
def test_route_refuses_before_anything_is_enqueued(change, rc):
    _l, lib = _lib()
    assert lib.kivi_moe_route(*_route_args(**change)) == rc, lib.kivi_last_error()
    assert b"kivi_moe_route" in lib.kivi_last_error()


@pytest.mark.parametrize("change,rc", EXPERTS_REFUSALS, ids=[str(c) for c, _ in EXPERTS_REFUSALS])
def test_experts_refuses_before_anything_is_enqueued(change, rc):
    _l, lib = _lib()
    assert lib.kivi_moe_experts(*_experts_args(**change)) == rc, lib.kivi_last_error()
    assert b"kivi_moe_experts" in lib.kivi_last_error()


def test_python_checks_and_usable():
    from kivi_amd import moe
    lg = torch.zeros((4, 8), dtype=torch.float16)
    with pytest.raises(Exception, match="GPU"):
        moe.route(lg, 2)
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="top_k"):
            moe.route_torch(lg, bad)
    with pytest.raises(ValueError, match="logits"):
        moe.route_torch(lg[0], 2)
    x = torch.zeros((4, 64), dtype=torch.float16)
    assert not moe.usable(x, 8, 2, 64, 96)                                  # not on the GPU
    assert not moe.usable(x.float(), 8, 2, 64, 96)


def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "moe_plan")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "moe_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "moe plan ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ against transformers, in fp32
CASES = [("mixtral", 8, 2, True), ("qwen3_moe", 12, 4, True), ("qwen3_moe", 12, 4, False)]
H, I = 64, 96


def _hf_block(family, E, K, norm):
    tf = pytest.importorskip("transformers")
    if family == "mixtral":
        from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock
        cfg = tf.MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=K)
        return MixtralSparseMoeBlock(cfg)
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeSparseMoeBlock
    cfg = tf.Qwen3MoeConfig(hidden_size=H, moe_intermediate_size=I, num_experts=E, num_experts_per_tok=K, norm_topk_prob=norm)
    return Qwen3MoeSparseMoeBlock(cfg)


@pytest.mark.parametrize("family,E,K,norm", CASES)
def test_torch_path_equals_transformers_and_the_fp64_restatement(family, E, K, norm):
    from kivi_amd import moe
    torch.manual_seed(E + K)
    hf = _hf_block(family, E, K, norm).float().eval()
    ours = moe.SparseMoeBlock(H, I, E, K, norm_topk=norm, round_weights=family == "qwen3_moe").eval()
    with torch.no_grad():
        for p in ours.parameters():
            p.normal_(0.0, 0.2)
        hf.gate.weight.copy_(ours.gate.weight)
        hf.experts.gate_up_proj.copy_(ours.experts.gate_up_proj)
        hf.experts.down_proj.copy_(ours.experts.down_proj)
        x = torch.randn(3, 7, H)
        want = hf(x.clone())
        want = want[0] if isinstance(want, tuple) else want
        got = ours(x)
        x2 = x.reshape(-1, H)
        logits = torch.nn.functional.linear(x2, ours.gate.weight)
        plan = moe.route_torch(logits, K, norm, family == "qwen3_moe")
        idx64, w64 = R.route_ref(logits, K, norm, False)
        ref = R.experts_ref(x2, idx64, w64, ours.experts.gate_up_proj, ours.experts.down_proj)
    assert got.shape == x.shape and got.dtype == torch.float32
    assert torch.equal(plan.idx.long(), idx64) and plan.w.dtype == torch.float32
    assert ((plan.w.double() - w64).abs() <= 1e-6 * w64).all()
    R.check_plan(plan, idx64, moe.TOKEN_TILE)
    rms = ref.pow(2).mean().sqrt().item()
    d_hf = (got - want).abs().max().item() / rms
    d_ref = (got.reshape(-1, H).double() - ref).abs().max().item() / rms
    d_hf_ref = (want.reshape(-1, H).double() - ref).abs().max().item() / rms
    print(f"{family} E={E} K={K} norm={norm}: |ours - hf| = {d_hf:.3g}, |ours - fp64| = {d_ref:.3g}, |hf - fp64| = {d_hf_ref:.3g} (of rms)")
    assert d_hf <= BAR and d_ref <= BAR
    # experts_torch from the plan alone gives what the module gives
    assert torch.equal(moe.experts_torch(x2, plan, ours.experts.gate_up_proj, ours.experts.down_proj).view_as(got), got)


def test_route_torch_resolves_equal_logits_to_the_lower_expert():
    from kivi_amd import moe
    lg = R.tied_logits(9, 12, 3, torch.float32)
    plan = moe.route_torch(lg, 4, True, False)
    idx64, w64 = R.route_ref(lg, 4, True, False)
    assert torch.equal(plan.idx.long(), idx64) and plan.idx[0].tolist() == [0, 1, 2, 3] and plan.idx[1].tolist() == [0, 1, 2, 3]
    assert torch.allclose(plan.w.double(), w64, rtol=1e-6, atol=0) and torch.allclose(plan.w.sum(-1), torch.ones(9))
    half = moe.route_torch(lg.half(), 4, False, True)
    assert torch.equal(half.w, half.w.half().float()) and half.w.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ models
def _cfg(**kw):
    d = dict(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=6, intermediate_size=160, vocab_size=64,
             head_dim=16)
    d.update(kw)
    return d


@pytest.mark.parametrize("step,only", [(1, []), (1, [0, 4]), (2, []), (2, [1, 3])])
def test_layer_kinds_follow_hfs_rule(step, only):
    tf = pytest.importorskip("transformers")
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeDecoderLayer, Qwen3MoeSparseMoeBlock
    from kivi_amd.llama import MLP, Qwen3MoeForCausalLM_KIVI, layer_is_sparse, make_config
    from kivi_amd.moe import SparseMoeBlock
    d = _cfg(model_type="qwen3_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=32, decoder_sparse_step=step,
             mlp_only_layers=only, norm_topk_prob=True)
    cfg = make_config(d)
    assert (cfg.num_experts, cfg.num_experts_per_tok, cfg.moe_intermediate_size, cfg.norm_topk_prob) == (4, 2, 32, True)
    assert cfg.decoder_sparse_step == step and cfg.mlp_only_layers == only and cfg.kivi_moe_kernel and cfg.kivi_moe_kernel_max_tokens is None
    model = Qwen3MoeForCausalLM_KIVI(cfg)
    hf_cfg = tf.Qwen3MoeConfig(**{k: v for k, v in d.items() if k != "model_type"})
    for i, layer in enumerate(model.model.layers):
        hf_sparse = isinstance(Qwen3MoeDecoderLayer(hf_cfg, i).mlp, Qwen3MoeSparseMoeBlock)
        assert layer_is_sparse(cfg, i) == hf_sparse == isinstance(layer.mlp, SparseMoeBlock), i
        if hf_sparse:
            assert layer.mlp.round_weights and layer.mlp.norm_topk and tuple(layer.mlp.experts.gate_up_proj.shape) == (4, 64, 64)
        else:
            assert type(layer.mlp) is MLP and layer.mlp.gate_proj.out_features == 160


def test_a_config_without_experts_builds_the_dense_modules():
    from kivi_amd.llama import MLP, LlamaForCausalLM_KIVI, make_config
    cfg = make_config(_cfg())
    assert cfg.num_experts == 0
    model = LlamaForCausalLM_KIVI(cfg)
    assert all(type(layer.mlp) is MLP for layer in model.model.layers)
    assert not any("experts" in k for k in model.state_dict())


def test_mixtral_config_fields():
    from kivi_amd.llama import MixtralForCausalLM_KIVI, make_config
    from kivi_amd.moe import SparseMoeBlock
    cfg = make_config(_cfg(model_type="mixtral", num_local_experts=8, num_experts_per_tok=2, num_hidden_layers=2),
                      moe_kernel=False, moe_kernel_max_tokens=64)
    assert (cfg.num_experts, cfg.num_experts_per_tok, cfg.moe_intermediate_size, cfg.norm_topk_prob) == (8, 2, 160, True)
    assert not cfg.kivi_moe_kernel and cfg.kivi_moe_kernel_max_tokens == 64
    model = MixtralForCausalLM_KIVI(cfg)
    for layer in model.model.layers:
        assert isinstance(layer.mlp, SparseMoeBlock) and not layer.mlp.round_weights and layer.mlp.norm_topk
        assert not layer.mlp.kernel and layer.mlp.kernel_max_tokens == 64 and layer.self_attn.q_proj.bias is None


@pytest.mark.parametrize("field", ["shared_expert_intermediate_size", "n_shared_experts", "num_shared_experts"])
def test_shared_experts_are_refused_by_name(field):
    from kivi_amd.llama import make_config
    with pytest.raises(ValueError, match=field):
        make_config(_cfg(model_type="qwen2_moe", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=32, **{field: 128}))
    make_config(_cfg(num_experts=4, num_experts_per_tok=2, moe_intermediate_size=32, **{field: 0}))     # absent in effect


def _spell(state, spelling):
    """The model's state dict under another spelling of the sparse blocks' names."""
    out = {}
    for name, t in state.items():
        if ".mlp.experts." not in name and ".mlp.gate.weight" not in name:
            out[name] = t
            continue
        if spelling == "fused":
            out[name] = t
        elif name.endswith(".mlp.gate.weight"):
            out[name.replace(".mlp.", ".block_sparse_moe.") if spelling == "mixtral" else name] = t
        else:
            prefix = name[: name.index(".mlp.experts.")]
            mid = ".block_sparse_moe.experts." if spelling == "mixtral" else ".mlp.experts."
            g, u, dn = ("w1", "w3", "w2") if spelling == "mixtral" else ("gate_proj", "up_proj", "down_proj")
            for e in range(t.shape[0]):
                if name.endswith("gate_up_proj"):
                    inter = t.shape[1] // 2
                    out[f"{prefix}{mid}{e}.{g}.weight"] = t[e, :inter].clone()
                    out[f"{prefix}{mid}{e}.{u}.weight"] = t[e, inter:].clone()
                else:
                    out[f"{prefix}{mid}{e}.{dn}.weight"] = t[e].clone()
    return out


@pytest.mark.parametrize("spelling", ["mixtral", "qwen3_moe", "fused"])
def test_checkpoint_names_are_translated(spelling):
    from kivi_amd.llama import MixtralForCausalLM_KIVI, make_config
    from kivi_amd.loading import CheckpointLoader
    d = _cfg(model_type="mixtral", num_local_experts=4, num_experts_per_tok=2, num_hidden_layers=2, intermediate_size=32)
    torch.manual_seed(1)
    src = MixtralForCausalLM_KIVI(make_config(d))
    state = _spell({k: v.detach().clone() for k, v in src.state_dict().items()}, spelling)
    if spelling != "fused":
        assert not any(k.endswith("gate_up_proj") for k in state) and len(state) > len(src.state_dict())
    torch.manual_seed(2)
    dst = MixtralForCausalLM_KIVI(make_config(d))
    half = len(state) // 2                                      # two "files": the pieces of one parameter may come apart
    names = list(state)
    loader = CheckpointLoader(dst, torch.float32)
    for part in ({k: state[k] for k in names[:half]}, {k: state[k] for k in names[half:]}):
        loader.take(part)
    loader.finish()
    assert not loader.unexpected, loader.unexpected
    for (k, a), (_, b) in zip(sorted(src.state_dict().items()), sorted(dst.state_dict().items())):
        assert torch.equal(a, b), k
    # a checkpoint that lacks one expert's piece is reported
    if spelling != "fused":
        torch.manual_seed(3)
        short = CheckpointLoader(MixtralForCausalLM_KIVI(make_config(d)), torch.float32)
        part = dict(state)
        part.pop(next(k for k in part if ".experts.3." in k))
        short.take(part)
        with pytest.raises(KeyError, match="experts.gate_up_proj"):
            short.finish()
