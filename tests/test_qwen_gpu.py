"""GPU: kivi_qk_rope and the padded query groups through the public interface.

1. A Llama-shaped tiny model at ratio 4 with qk_kernel=True against the same weights with it off: prompt logits and the logits of
   40 decode steps bit-identical, generate() tokens identical -- the kernel changes the launch count and nothing else.
2. Qwen2 (ratio 7, q / k / v biases) and Qwen3 (ratio 5, head norms): generate, generate_graphed and generate_continuous run on
   KiviLayerCacheMF caches of nh_kv * 8 = 16 query heads; the graphed path captures the whole step and equals the eager one token
   for token (the relation tests/test_graph_gpu.py holds replayed steps to: the same bits); per-step logits against the same weights
   with qk_kernel=False (hook-state layout, torch chain) stay inside the band tests/test_padding_gpu.py:266 holds two forms of one
   model to: 1e-2 of the rms on the prompt pass, 5e-2 on the decode steps.
3. Qwen3 weights saved under HF's names and loaded by from_pretrained reproduce the constructed model's logits bit for bit.
Tiny models: tests/tiny_qk_models.py; a 70-token prompt, 40 steps across the K flush at 96."""
import json

import pytest
import torch

import tiny_qk_models as M
from helpers import same_bits

pytestmark = pytest.mark.gpu
T0, STEPS = 70, 40


def _classes():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, Qwen3ForCausalLM_KIVI
    return {"llama": LlamaForCausalLM_KIVI, "qwen2": Qwen2ForCausalLM_KIVI, "qwen3": Qwen3ForCausalLM_KIVI}


def _forced_logits(model, ids, forced):
    """Logits of the prompt pass and of every teacher-forced decode step, and the final caches."""
    logits, past = model(ids)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past)
        out.append(logits)
    return out, past


def test_llama_ratio4_kernel_changes_nothing_but_the_launch_count():
    from kivi_amd.attention import KiviLayerCacheMF
    cls = _classes()["llama"]
    on = M.build(cls, 4, 31, qk_kernel=True)
    off = M.twin(cls, on, 4)
    assert on.model.layers[0].self_attn.qk_kernel and not off.model.layers[0].self_attn.qk_kernel
    ids = M.prompts(1, 2, T0)
    forced = torch.randint(1, M.VOCAB, (STEPS, 2, 1), generator=torch.Generator().manual_seed(2)).cuda()
    a, pa = _forced_logits(on, ids, forced)
    b, pb = _forced_logits(off, ids, forced)
    for s, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), s
    for p, q in zip(pa, pb):
        assert isinstance(p.layer, KiviLayerCacheMF) and isinstance(q.layer, KiviLayerCacheMF) and p.layer.nh == q.layer.nh == 8
        for x, y in zip(p.layer.as_tuple()[:8], q.layer.as_tuple()[:8]):
            assert (x is None and y is None) or same_bits(x, y)
    assert torch.equal(on.generate(ids, STEPS), off.generate(ids, STEPS))
    assert torch.equal(on.generate_graphed(ids, 12), off.generate_graphed(ids, 12))
    on.release_graphs(), off.release_graphs()


FAMILIES = [("qwen2", 7), ("qwen3", 5)]


@pytest.mark.parametrize("family,ratio", FAMILIES)
def test_qwen_generates_on_padded_matrix_pipe_caches(family, ratio, monkeypatch):
    import kivi_amd.attention as A
    from kivi_amd.attention import KiviLayerCacheMF
    cls = _classes()[family]
    model = M.build(cls, ratio, 41 + ratio, qk_kernel=True)
    a0 = model.model.layers[0].self_attn
    assert a0.cache_heads == 16 and (a0.q_norm is not None) == (family == "qwen3") and (a0.q_proj.bias is not None) == (family == "qwen2")
    made = []
    make = A.make_layer_cache
    monkeypatch.setattr(A, "make_layer_cache", lambda *a, **k: made.append(make(*a, **k)) or made[-1])

    def all_padded():
        assert made and all(isinstance(c, KiviLayerCacheMF) and c.nh == 16 for c in made)
        made.clear()

    ids = M.prompts(3, 2, T0)
    eager = model.generate(ids, STEPS)
    all_padded()
    graphed = model.generate_graphed(ids, STEPS)
    all_padded()
    assert torch.equal(eager, graphed)
    eager_steps, captures, replays = model.graphs.stats
    assert model.graphs.whole and captures >= 1 and replays >= STEPS - 2 * captures - 4, model.graphs.stats
    assert eager.shape == (2, T0 + STEPS) and int(eager.min()) >= 0 and int(eager.max()) < M.VOCAB
    model.release_graphs()
    # continuous batching: against the scheduler's policy restated with the model's own calls (tests/test_admit_gpu.py)
    import test_admit_gpu as AD
    g = torch.Generator().manual_seed(9)
    lens, limits = [21, 5, 33, 47, 12], [4, 30, 9, 12, 6]
    prompts = [torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in lens]
    want, landed = AD._restate(model, prompts, limits, 3)
    made.clear()
    out = model.generate_continuous(prompts, limits, 3)
    all_padded()
    assert [o.tolist() for o in out] == want and len(landed) > 3
    out = model.generate_continuous(prompts, limits, 3, graphed=True)
    all_padded()
    assert [o.tolist() for o in out] == want
    model.release_graphs()


@pytest.mark.parametrize("family,ratio", FAMILIES)
def test_qwen_logits_against_the_hook_state_layout(family, ratio):
    from kivi_amd.attention import KiviLayerCache, KiviLayerCacheMF
    cls = _classes()[family]
    on = M.build(cls, ratio, 51 + ratio, qk_kernel=True)
    off = M.twin(cls, on, ratio, qk_kernel=False)
    ids = M.prompts(4, 2, T0)
    forced = torch.randint(1, M.VOCAB, (STEPS, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    a, pa = _forced_logits(on, ids, forced)
    b, pb = _forced_logits(off, ids, forced)
    assert all(isinstance(p.layer, KiviLayerCacheMF) and p.layer.nh == 16 for p in pa)
    assert all(type(p.layer) is KiviLayerCache for p in pb)
    worst = 0.0
    for s, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all()
        rms = y.float().pow(2).mean().sqrt().item()
        d = (x.float() - y.float()).abs().max().item() / rms
        worst = max(worst, d)
        assert d <= (1e-2 if s == 0 else 5e-2), (s, d)             # tests/test_padding_gpu.py:266
    print(f"{family}: worst |padded matrix-pipe - hook-state| / rms over {STEPS} steps = {worst:.3g}")
    assert pa[0].layer.kv_seq_len == pb[0].layer.kv_seq_len == T0 + STEPS and pa[0].layer.k_quant_len == 96


def test_qwen3_from_pretrained_reproduces_the_constructed_model(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen3ForCausalLM_KIVI
    model = M.build(Qwen3ForCausalLM_KIVI, 5, 61, qk_kernel=True)
    state = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    assert "model.layers.1.self_attn.q_norm.weight" in state and "model.layers.0.self_attn.k_norm.weight" in state
    st.save_file(state, str(tmp_path / "model.safetensors"))
    d = dict(model_type="qwen3", hidden_size=256, num_attention_heads=10, num_key_value_heads=2, num_hidden_layers=2,
             intermediate_size=512, vocab_size=M.VOCAB, head_dim=128, rms_norm_eps=1e-6)
    (tmp_path / "config.json").write_text(json.dumps(d))
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), residual_length=32)
    assert type(loaded) is Qwen3ForCausalLM_KIVI and loaded.model.layers[0].self_attn.qk_kernel
    for x, y in zip(model.model.layers, loaded.model.layers):     # the rotary frequencies are no part of a checkpoint: from_pretrained
        assert y.self_attn.inv_freq.dtype == torch.float32       # keeps them in fp32, .half() rounded the constructed model's
        x.self_attn.inv_freq = y.self_attn.inv_freq.clone()
    ids = M.prompts(6, 2, T0)
    forced = torch.randint(1, M.VOCAB, (8, 2, 1), generator=torch.Generator().manual_seed(7)).cuda()
    a, _ = _forced_logits(model, ids, forced)
    b, _ = _forced_logits(loaded, ids, forced)
    for s, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), s
