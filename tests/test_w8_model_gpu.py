"""GPU: models with FP8 weights through the public interface.  tests/tiny_w4_models.py: a Llama-like, a
Qwen2-like with biases and a padded query-group ratio, the Mixtral-like with only its attention in FP8; fp16 and bf16 each.

Tree      the module tree, the bytes of every FP8 module (O K + 4 ceil(O / 128) K / 128) and what stays in the model dtype.
Loading   from_pretrained of a pre-quantised FP8 directory (written by tests/w8_ref.py's CPU quantiser, weights and scales in two
          files) and of the 16-bit directory with fp8_weights=True give identical buffers, those of quantising the dense model's
          modules; save_quantized then from_pretrained round-trips bit-identically.
Logits    per step against the fake-quant twin -- the same class with nn.Linears holding dequant() -- under the bar of
          tests/test_w4_model_gpu.py::test_logits_against_the_fake_quant_twin.  The prompt pass (140 tokens) runs the dequantise +
          F.linear path, the steps the kernels.  Asserted on every pass; the Mixtral-like model and its twin route every token to
          the same experts (_SharedRouting), since a router's choice is not continuous in its input.
Decoding  generate equals generate_graphed token for token from a whole-step capture; generate_continuous, eager and graphed, equals
          the restated policy of tests/test_admit_gpu.py -- with the kernel at every N, as the 4-bit model's test runs them.
LoRA      an adapter on q_proj and gate_proj over the FP8 llama: base rows are byte-identical to a pass without adapters, adapted
          rows meet the bar of tests/test_lora_model_gpu.py against the merged twin (dequant() + scale B A, rounded once)."""
import functools
import json

import pytest
import torch

import lora_ref as LR
import tiny_w4_models as M
import w8_ref as R

pytestmark = pytest.mark.gpu
T0, STEPS = 70, 24
CASES = [(f, d) for f in ("llama", "qwen2", "mixtral") for d in (torch.float16, torch.bfloat16)]
IDS = [f"{f}-{'fp16' if d == torch.float16 else 'bf16'}" for f, d in CASES]
ALWAYS = 1 << 20
PAIR = ("weight", "weight_scale_inv")


@functools.lru_cache(maxsize=None)
def _dense(family, dtype):
    return M.build_dense(family, 40 + len(family), dtype)


def _fp8_modules(model):
    from kivi_amd.wfp8 import Fp8Linear
    return {n: m for n, m in model.named_modules() if isinstance(m, Fp8Linear)}


@functools.lru_cache(maxsize=None)
def _model(family, dtype, kernel_max_tokens=None):
    """The FP8 model of the dense one: the same class built with fp8_weights=True, every Fp8Linear quantised from the dense model's
    nn.Linear (quantize_), everything else copied."""
    dense = _dense(family, dtype)
    model = M.classes()[family](M.config(family, fp8_weights=True, weight_kernel_max_tokens=kernel_max_tokens)).to(dtype).cuda().eval()
    src, rest = dict(dense.named_modules()), dict(dense.state_dict())
    for name, m in _fp8_modules(model).items():
        m.quantize_(src[name].weight.data, name + ".weight")
        rest.pop(name + ".weight")
    missing, unexpected = model.load_state_dict(rest, strict=False)
    assert not unexpected and all(k.rsplit(".", 1)[1] in PAIR for k in missing), (missing, unexpected)
    return model


def _twin(family, model, replace=None):
    """The same class with nn.Linears holding the FP8 model's dequantised weights (`replace`: name -> another weight)."""
    dtype = next(model.parameters()).dtype
    other = M.classes()[family](M.config(family)).to(dtype).cuda().eval()
    fp8 = _fp8_modules(model)
    state = {k: v for k, v in model.state_dict().items() if k.rsplit(".", 1)[0] not in fp8 or k.endswith(".bias")}
    for name, m in fp8.items():
        state[name + ".weight"] = m.dequant(dtype)
    state.update(replace or {})
    missing, unexpected = other.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return other


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_module_tree_and_bytes(family, dtype):
    from kivi_amd import wfp8
    from kivi_amd.moe import SparseMoeBlock
    model = _model(family, dtype)
    mods = _fp8_modules(model)
    assert len(mods) == 2 * (4 if family == "mixtral" else 7)
    for layer in model.model.layers:
        assert type(layer.mlp) is (SparseMoeBlock if family == "mixtral" else wfp8.Fp8MLP)
        assert type(layer.self_attn.q_proj) is wfp8.Fp8Linear and (layer.self_attn.q_proj.bias is not None) == (family == "qwen2")
        assert layer.self_attn.o_proj.bias is None
    for name, m in mods.items():
        O, K = m.out_features, m.in_features
        got = sum(b.numel() * b.element_size() for b in m.buffers())
        assert got == O * K + 4 * ((O + 127) // 128) * (K // 128) == wfp8._lib.load().kivi_w8_bytes(O, K), name
        assert m.weight.dtype == torch.uint8 and all(b.is_cuda for b in m.buffers()) and not any(p.dim() > 1 for p in m.parameters())
        assert not bool(((m.weight & 0x7F) == 0x7F).any()) and int((m.weight & 0x7F).max()) == 0x7E    # every block reaches +-448
    assert model.lm_head.weight.dtype == dtype and model.model.embed_tokens.weight.dtype == dtype
    if family == "mixtral":
        assert model.model.layers[0].mlp.experts.gate_up_proj.dtype == dtype


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_from_pretrained_of_both_directories_gives_the_same_buffers(family, dtype, tmp_path):
    import safetensors.torch as st
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    dense = _dense(family, dtype)
    state = {k: v.detach().cpu().contiguous() for k, v in dense.state_dict().items()}
    src = tmp_path / "dense"
    src.mkdir()
    st.save_file(state, str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps(M.config_dict(family)))
    from16 = LlamaForCausalLM_KIVI.from_pretrained(str(src), dtype=dtype, residual_length=32, fp8_weights=True, weight_kernel_max_tokens=33)
    assert type(from16) is M.classes()[family]
    want = _model(family, dtype)
    _same_state(from16, want)
    assert all(m.kernel_max_tokens == 33 for m in _fp8_modules(from16).values())
    # the pre-quantised directory: the CPU restatement's bytes, weights and scales in two files, the scales first
    fp8 = R.fp8_state(state)
    scales = [k for k in fp8 if k.endswith("weight_scale_inv")]
    assert len(scales) == len(_fp8_modules(want))
    pre = tmp_path / "fp8"
    R.write_fp8_dir(str(pre), M.config_dict(family), fp8, quant=dict(modules_to_not_convert=["lm_head"]),
                    files=[scales, [k for k in fp8 if k not in scales]])
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(pre), dtype=dtype, residual_length=32)
    assert type(loaded) is M.classes()[family]
    _same_state(loaded, want)
    for name, m in _fp8_modules(loaded).items():                       # the checkpoint's bytes are the device's bytes
        assert torch.equal(m.weight.cpu(), fp8[name + ".weight"].view(torch.uint8)), name
        assert torch.equal(m.weight_scale_inv.cpu(), fp8[name + ".weight_scale_inv"].view(torch.int32)), name
    # save_quantized -> from_pretrained: transformers' format, bit-identical, nothing re-quantised
    dst = tmp_path / "saved"
    loaded.save_quantized(str(dst))
    d = json.loads((dst / "config.json").read_text())
    q = d.pop("quantization_config")
    assert d == M.config_dict(family) and q["quant_method"] == "fp8" and q["weight_block_size"] == [128, 128]
    assert "lm_head" in q["modules_to_not_convert"] and not any(n.endswith("_proj") for n in q["modules_to_not_convert"])
    saved = st.load_file(str(dst / "model.safetensors"))
    assert saved["model.layers.1.self_attn.o_proj.weight"].dtype == torch.float8_e4m3fn
    assert saved["model.layers.1.self_attn.o_proj.weight_scale_inv"].dtype == torch.float32
    again = LlamaForCausalLM_KIVI.from_pretrained(str(dst), dtype=dtype, residual_length=32)
    _same_state(again, loaded)


def _forced_logits(model, ids, forced, **kw):
    logits, past = model(ids, **kw)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past, **kw)
        out.append(logits)
    return out


class _SharedRouting:
    """Both models of a comparison route every token of every sparse block to the SAME experts: the first model run (the twin)
    keeps the top-k of its own router logits, the second (the FP8 model) is given that choice.  A choice is imposed by lowering the
    logits of the other experts to -1e4 before kivi_amd.moe.route / route_torch see them: the chosen experts keep their own logits,
    so with weights normalised over the top-k (Mixtral's rule) every weight stays a continuous function of the model's own logits.
    The twin's choice is imposed on the twin as well, which settles a tie the same way in both.  `differ`: the tokens whose own
    choice was another than the one imposed."""

    def __init__(self, monkeypatch):
        import kivi_amd.moe as moe
        self.choices, self.replay, self.differ = [], None, 0
        for name in ("route", "route_torch"):
            monkeypatch.setattr(moe, name, functools.partial(self._call, getattr(moe, name)))

    def second_model(self):
        self.replay = list(self.choices)

    def _call(self, orig, logits, top_k, *args, **kw):
        idx = logits.float().topk(top_k, dim=-1).indices
        if self.replay is None:
            self.choices.append(idx)
        else:
            own, idx = idx, self.replay.pop(0)
            self.differ += int((own.sort(-1).values != idx.sort(-1).values).any(-1).sum())
        masked = torch.full_like(logits, -1e4).scatter(-1, idx, logits.gather(-1, idx))
        return orig(masked, top_k, *args, **kw)


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_logits_against_the_fake_quant_twin(family, dtype, monkeypatch):
    """The bar is the one of tests/test_w4_model_gpu.py::test_logits_against_the_fake_quant_twin, on every pass of every family:
    1e-2 of the rms in fp16, 5e-2 in bf16.  Measured on an MI355X: 0.0037 / 0.0040 (llama / qwen2, fp16) and 0.029 / 0.031 (bf16):
    the twin rounds every dequantised weight to the dtype, the kernels do not, so in bf16 the two differ by the rounding of 8-bit
    significands.
    The Mixtral-like model and its twin run under _SharedRouting.  A router's choice is no continuous function of its input: left to
    themselves the two models sent one token to different experts where its second and third router logits were one unit in the
    last place apart (2^-7 in fp16 at pass 8, 2^-5 in bf16 at pass 10), and that pass's logits were 0.11 / 0.23 of the rms apart
    with every other pass under 0.0061 / 0.042.  What the FP8 kernels do to the logits is continuous and is held to the bar on all
    25 passes (measured 0.0049 / 0.042); the number of tokens whose own choice differed from the twin's is printed (1 / 1)."""
    model = _model(family, dtype)
    twin = _twin(family, model)
    assert not any(k.endswith("weight_scale_inv") for k in twin.state_dict())
    ids = M.prompts(4, 2, T0)
    forced = torch.randint(1, M.VOCAB, (STEPS, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    shared = _SharedRouting(monkeypatch)
    b = _forced_logits(twin, ids, forced)
    shared.second_model()
    a = _forced_logits(model, ids, forced)
    sparse_calls = 2 * len(a) if family == "mixtral" else 0           # two sparse layers per pass
    assert len(shared.choices) == sparse_calls and shared.replay == []
    bar = 1e-2 if dtype == torch.float16 else 5e-2
    worst = 0.0
    for s, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all() and x.dtype == y.dtype
        rms = y.float().pow(2).mean().sqrt().item()
        d = (x.float() - y.float()).abs().max().item() / rms
        worst = max(worst, d)
        assert d <= bar, (s, d)
    print(f"{family} {dtype}: worst |FP8 kernels - fake-quant twin| / rms over the prompt pass and {STEPS} steps = {worst:.3g} (bar {bar})"
          + (f"; tokens whose own routing differed from the twin's: {shared.differ}" if sparse_calls else ""))


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_generate_graphed_and_continuous(family, dtype):
    import test_admit_gpu as AD
    model = _model(family, dtype, ALWAYS)
    assert all(m.kernel_max_tokens == ALWAYS for m in _fp8_modules(model).values())
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


def test_lora_over_an_fp8_llama():
    """The passes stay inside the residual window (16 prompt tokens + 14 steps <= residual_length = 32), as
    tests/test_lora_model_gpu.py::test_logits_against_the_merged_twin explains: its bar is for passes that read nothing back from
    the 2-bit cache."""
    family, dtype = "llama", torch.float16
    dense = _dense(family, dtype)
    model = _model(family, dtype)
    adapter = LR.make_adapter(dense, 4, 16.0, 21, ("q_proj", "gate_proj"))
    ids = M.prompts(5, 4, 16)
    forced = torch.randint(1, M.VOCAB, (14, 4, 1), generator=torch.Generator().manual_seed(6)).cuda()
    base = _forced_logits(model, ids, forced)
    lset = model.enable_lora(2, 8, ("q_proj", "gate_proj"))
    try:
        assert len(lset.modules) == 4 and lset.load(adapter) == 0
        mixed = _forced_logits(model, ids, forced, adapters=[0, None, 0, None])
        graphed = model.generate_graphed(ids, 6, adapters=[0, None, 0, None])
        assert torch.equal(graphed, model.generate(ids, 6, adapters=[0, None, 0, None]))
    finally:
        model.disable_lora()
    replace = {}
    for name, (a, b) in adapter.tensors.items():
        w = dict(model.named_modules())[name].dequant(dtype).float()
        replace[name + ".weight"] = (w + adapter.scale * (b.to(dtype).float().cuda() @ a.to(dtype).float().cuda())).to(dtype)
    twin = _twin(family, model, replace)
    want = _forced_logits(twin, ids, forced)
    bar, worst, moved = 1e-2, 0.0, float("inf")
    for s, (m, b, y) in enumerate(zip(mixed, base, want)):
        assert torch.equal(m[1], b[1]) and torch.equal(m[3], b[3]), s      # base rows: the bytes of a pass without adapters
        assert not torch.equal(m[0], b[0]) and not torch.equal(m[2], b[2]), s
        rms = y.float().pow(2).mean().sqrt().item()
        for row in (0, 2):
            worst = max(worst, (m[row].float() - y[row].float()).abs().max().item() / rms)
            moved = min(moved, (y[row].float() - b[row].float()).abs().max().item() / rms)
    print(f"FP8 llama fp16, LoRA r=4 on q_proj / gate_proj: worst |adapter path - merged twin| / rms over a 16-token prompt pass and "
          f"14 steps = {worst:.3g} (bar {bar}); the adapter moves the logits by at least {moved:.3g} of the rms")
    assert worst <= bar and moved > 3 * bar, (worst, moved)     # (or the comparison would prove nothing)
