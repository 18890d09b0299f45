"""GPU: bf16 models through the public interface.

The tiny models of tests/tiny_qk_models.py rebuilt in bf16 -- Llama at ratio 4, Qwen2 at ratio 7, Qwen3 at ratio 5 with qk_kernel,
and a head_dim 64 Llama (the torch boundary on the GPU, the hook-state layout) -- from weights that are the same numbers in bf16,
fp16 and fp32 (tests/bf16_ref.shared_weights; tests/test_bf16_cpu.py asserts it).

1. Every cache a bf16 model makes holds fp16 members; the matrix-pipe caches have nh_kv * Rp query heads.
2. generate_graphed equals generate token for token on a 70-token prompt over 40 steps, across the K flush at 96, from a whole-step
   capture; also with a RowSampler and top_logprobs=3.  generate_continuous, eager and graphed, equals the restated policy of
   tests/test_admit_gpu.py.  checkpoint -> 5 steps -> restore_ -> the same 5 steps: bit-identical logits; rebase_ against its oracle.  Beam search, score()
   and perplexity() run and return finite values of the documented shapes.  from_pretrained(dtype=torch.bfloat16) reproduces the
   constructed model's logits bit for bit.
3. Accuracy against the dense reference -- the same weights in a .float() model, whose q / k / v take the torch boundary (held to
   fp64 by the CPU test) into the same fp16 cache code -- teacher-forced: (i) a 20-token prompt and 8 steps, all inside the residual
   window (nothing is quantised); (ii) 70 + 40 across the flush.  d16 = the worst max |logit - reference| / rms(reference) over the
   passes of the fp16 model, dbf the same of the bf16 model.  The bar on dbf is 8 * d16 -- the ratio of the formats' unit roundoffs
   -- in (i), and twice that in (ii), where a 2-bit code may flip; d16 is the constant D16 below, measured on an MI355X, not the
   value of the run."""
import functools
import json

import pytest
import torch

import bf16_ref as R
import tiny_qk_models as M
from helpers import same_bits

pytestmark = pytest.mark.gpu
T0, STEPS = 70, 40
BF, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
FAMILIES = {"llama": ("llama", 4, 128, {}), "qwen2": ("qwen2", 7, 128, dict(qk_kernel=True)),
            "qwen3": ("qwen3", 5, 128, dict(qk_kernel=True)), "llama64": ("llama", 2, 64, {})}
# d16 of the fp16 twins against the .float() reference, measured on an MI355X: {family: (case (i), case (ii))}
D16 = {"llama": (0.00373, 0.0855), "qwen2": (0.00281, 0.0448), "qwen3": (0.00600, 0.1475), "llama64": (0.00704, 0.2137)}
RATIO, FLIP_MARGIN = 8.0, 2.0


def _classes():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, Qwen3ForCausalLM_KIVI
    return {"llama": LlamaForCausalLM_KIVI, "qwen2": Qwen2ForCausalLM_KIVI, "qwen3": Qwen3ForCausalLM_KIVI}


@functools.lru_cache(maxsize=None)
def _models(family):
    """(bf16, fp16, fp32) models of one family over the same weights."""
    name, ratio, head_dim, kw = FAMILIES[family]
    return R.models(_classes()[name], ratio, 70 + ratio + head_dim, (BF, FP16, FP32), head_dim=head_dim, **kw)


def _forced_logits(model, ids, forced, past=None):
    logits, past = model(ids, past)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past)
        out.append(logits)
    return out, past


def _record_caches(monkeypatch):
    import kivi_amd.attention as A
    made, make = [], A.make_layer_cache
    monkeypatch.setattr(A, "make_layer_cache", lambda *a, **k: made.append(make(*a, **k)) or made[-1])
    return made


@pytest.mark.parametrize("family", list(FAMILIES))
def test_generation_paths_agree_on_fp16_caches(family, monkeypatch):
    from kivi_amd.attention import KiviLayerCache, KiviLayerCacheMF
    from kivi_amd.sampling import SamplingParams
    model = _models(family)[0]
    a0 = model.model.layers[0].self_attn
    assert model.lm_head.weight.dtype == BF and a0.q_proj.weight.dtype == BF
    made = _record_caches(monkeypatch)
    mf = family != "llama64"
    heads = {"llama": 8, "qwen2": 16, "qwen3": 16, "llama64": 4}[family]

    def caches_are_fp16():
        assert made
        for c in made:
            assert isinstance(c, KiviLayerCacheMF) == mf and (mf or type(c) is KiviLayerCache)
            assert c.k_res.dtype == FP16 and c.v_res.dtype == FP16
            assert all(t.dtype != BF and t.dtype != FP32 for t in c.as_tuple()[:8] if torch.is_tensor(t))
            if mf:
                assert c.nh == heads == a0.cache_heads
        made.clear()

    ids = M.prompts(3, 2, T0)
    logits, past = model(ids)
    assert logits.dtype == BF and tuple(logits.shape) == (2, 1, M.VOCAB) and torch.isfinite(logits).all()
    caches_are_fp16()
    eager = model.generate(ids, STEPS)
    caches_are_fp16()
    graphed = model.generate_graphed(ids, STEPS)
    caches_are_fp16()
    assert torch.equal(eager, graphed)
    assert eager.shape == (2, T0 + STEPS) and int(eager.min()) >= 0 and int(eager.max()) < M.VOCAB
    if mf:
        eager_steps, captures, replays = model.graphs.stats
        assert model.graphs.whole and captures >= 1 and replays >= STEPS - 2 * captures - 4, model.graphs.stats
    g = model.graphs
    assert g.boundary and g.x[0].dtype == BF and g.attn.dtype == FP16 and g.cos.dtype == FP32 and g.mask is None
    assert all(t.dtype == FP16 for qkv in g.qkv for t in qkv)
    model.release_graphs()
    # per-request sampling and top_logprobs=3, eager against graphed
    params = [SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=71), SamplingParams(do_sample=False)]
    a = model.generate(ids, STEPS, sampling=params, return_logprobs=True, top_logprobs=3)
    b = model.generate_graphed(ids, STEPS, sampling=params, return_logprobs=True, top_logprobs=3)
    model.release_graphs()
    assert len(a) == len(b) == 4 and tuple(a[2].shape) == (2, STEPS, 3) and a[1].dtype == FP32
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.is_floating_point() else x,
                                                  y.view(torch.int32) if y.is_floating_point() else y)
    assert torch.isfinite(a[1]).all() and (a[1] <= 0).all()


@pytest.mark.parametrize("family", ["llama", "qwen2", "qwen3"])
def test_continuous_batching_equals_the_restated_policy(family, monkeypatch):
    import test_admit_gpu as AD
    model = _models(family)[0]
    made = _record_caches(monkeypatch)
    g = torch.Generator().manual_seed(9)
    lens, limits = [21, 5, 33, 47, 12], [4, 30, 9, 12, 6]
    prompts = [torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in lens]
    want, landed = AD._restate(model, prompts, limits, 3)
    out = model.generate_continuous(prompts, limits, 3)
    assert [o.tolist() for o in out] == want and len(landed) > 3
    out = model.generate_continuous(prompts, limits, 3, graphed=True)
    assert [o.tolist() for o in out] == want
    model.release_graphs()
    assert made and all(c.k_res.dtype == FP16 for c in made)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_checkpoint_restore_beams_and_scores(family):
    model = _models(family)[0]
    ids = M.prompts(4, 2, T0)
    forced = torch.randint(1, M.VOCAB, (5, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    logits, past = model(ids)
    ck = model.checkpoint(past)
    first, past = _forced_logits(model, forced[0], forced[1:], past)
    past = model.restore_(past, ck)
    again, past = _forced_logits(model, forced[0], forced[1:], past)
    assert len(first) == 5
    for s, (x, y) in enumerate(zip(first, again)):
        assert x.dtype == BF and same_bits(x.float(), y.float()), s
    beams = model.generate(ids, 8, num_beams=2)
    assert tuple(beams.shape) == (2, T0 + 8) and beams.dtype == torch.int64 and int(beams.min()) >= 0 and int(beams.max()) < M.VOCAB
    assert torch.equal(beams[:, :T0], ids)
    lp, valid, _, rank, top_ids, top_lp = model.score(ids, first_chunk=T0 - 8, chunk_size=1, return_rank=True, top_logprobs=5)
    assert tuple(lp.shape) == (2, T0 - 1) and lp.dtype == FP32 and valid.all() and torch.isfinite(lp).all() and (lp <= 0).all()
    assert tuple(top_ids.shape) == (2, T0 - 1, 5) and torch.isfinite(top_lp).all() and (rank >= 0).all()
    hit = rank < 5
    assert torch.equal(top_ids.gather(-1, rank.clamp(max=4).long()[..., None])[..., 0][hit], ids[:, 1:][hit])
    per_row, overall = model.perplexity(ids)
    assert tuple(per_row.shape) == (2,) and torch.isfinite(per_row).all() and torch.isfinite(overall) and overall.item() > 1.0


def test_rebase_of_a_bf16_models_caches():
    """rebase_(32) of caches at L = 84 whose rows all start with at least 32 pads, then 20 steps with the shortened mask, against
    caches rebuilt through the sliced-tuple oracle of tests/test_rebase_gpu.py: the same tokens."""
    import test_rebase_gpu as RB
    from kivi_amd.llama import left_pad
    from test_admit_gpu import _feed, _greedy
    model = _models("llama")[0]
    g = torch.Generator().manual_seed(1)
    ids, mask = left_pad([torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in (20, 14, 7)], 0, "cuda", length=52)
    gen = model.generate(ids, 33, attention_mask=mask)[:, 52:]
    lg, past, mask = _feed(model, ids, mask, gen[:, :32])
    assert past[0][-1] == 84 and mask.shape == (3, 84) and model.rebase_quantum(past) == 32 and model.rebase_limit(past) == 52
    want_past = RB._oracle_pasts(past, 32)
    caches = [p.layer for p in past]
    past2 = model.rebase_(past, 32)
    assert [p.layer for p in past2] == caches and past2[0][-1] == 52 and all(c.k_res.dtype == FP16 for c in caches)
    got = _greedy(model, lg, past2, mask[:, 32:], 20)
    want = _greedy(model, lg, want_past, mask[:, 32:], 20)
    assert torch.equal(got, want) and torch.equal(got[:, 0], gen[:, 32])


def test_left_padded_prompts_with_the_prefill_kernel_and_the_decode_lead():
    """The options that hand the attention a lead in place of a mask (DESIGN.md sections 20, 21) on a bf16 model: the padded
    graphed decode, per-row positions in fp32 tables, equals the eager one."""
    from kivi_amd.llama import LlamaForCausalLM_KIVI, left_pad
    model = R.models(LlamaForCausalLM_KIVI, 4, 91, (BF,), prefill_kernel=True, decode_lead=True)[0]
    g = torch.Generator().manual_seed(2)
    ids, mask = left_pad([torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in (T0, 41, 9)], 0, "cuda")
    eager = model.generate(ids, STEPS, attention_mask=mask)
    graphed = model.generate_graphed(ids, STEPS, attention_mask=mask)
    assert torch.equal(eager, graphed) and tuple(eager.shape) == (3, T0 + STEPS)
    gr = model.graphs
    assert gr.whole and gr.padded and gr.lead is not None and gr.mask.dtype == FP16 and gr.cos.dtype == FP32 and gr.cos.shape[0] == 3
    model.release_graphs()


def test_from_pretrained_bf16_reproduces_the_constructed_model(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen3ForCausalLM_KIVI
    model = _models("qwen3")[0]
    state = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    assert all(v.dtype == BF for v in state.values() if v.is_floating_point())
    st.save_file(state, str(tmp_path / "model.safetensors"))
    d = dict(model_type="qwen3", hidden_size=256, num_attention_heads=10, num_key_value_heads=2, num_hidden_layers=2,
             intermediate_size=512, vocab_size=M.VOCAB, head_dim=128, rms_norm_eps=1e-6)
    (tmp_path / "config.json").write_text(json.dumps(d))
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), dtype=BF, residual_length=32)
    assert type(loaded) is Qwen3ForCausalLM_KIVI and loaded.lm_head.weight.dtype == BF
    assert loaded.model.layers[0].self_attn.qk_kernel and loaded.model.layers[0].self_attn.q_norm.weight.dtype == BF
    ids = M.prompts(6, 2, T0)
    forced = torch.randint(1, M.VOCAB, (8, 2, 1), generator=torch.Generator().manual_seed(7)).cuda()
    a, _ = _forced_logits(model, ids, forced)
    b, _ = _forced_logits(loaded, ids, forced)
    for s, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == BF and same_bits(x.float(), y.float()), s


def _drift(family, T, steps, seed):
    """(d16, dbf): the worst max |logit - reference| / rms(reference) over the prompt pass and `steps` teacher-forced steps."""
    bf, f16, f32 = _models(family)
    ids = M.prompts(seed, 2, T)
    forced = torch.randint(1, M.VOCAB, (steps, 2, 1), generator=torch.Generator().manual_seed(seed + 1)).cuda()
    ref, pr = _forced_logits(f32, ids, forced)
    out = []
    for m in (f16, bf):
        got, pm = _forced_logits(m, ids, forced)
        worst = 0.0
        for x, r in zip(got, ref):
            assert torch.isfinite(x).all() and r.dtype == FP32
            worst = max(worst, ((x.float() - r).abs().max() / r.pow(2).mean().sqrt()).item())
        out.append(worst)
        assert pm[0].layer.kv_seq_len == pr[0].layer.kv_seq_len == T + steps and pm[0].layer.k_res.dtype == pr[0].layer.k_res.dtype == FP16
    return out[0], out[1], pr[0].layer


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bf16_stays_within_eight_fp16_errors_of_the_dense_reference(family):
    d16, dbf, layer = _drift(family, 20, 8, 11)                         # (i) inside the residual window: nothing is quantised
    assert layer.kv_seq_len == 28 and getattr(layer, "k_quant_len", 0) == 0
    bar = RATIO * D16[family][0]
    print(f"{family} (i) 20 + 8: d16 = {d16:.4g} (recorded {D16[family][0]:.4g}), dbf = {dbf:.4g}, bar = {bar:.4g}")
    d16b, dbfb, layer = _drift(family, T0, STEPS, 13)                   # (ii) across the K flush at 96
    assert layer.kv_seq_len == T0 + STEPS and getattr(layer, "k_quant_len", 96) == 96
    barb = RATIO * FLIP_MARGIN * D16[family][1]
    print(f"{family} (ii) {T0} + {STEPS}: d16 = {d16b:.4g} (recorded {D16[family][1]:.4g}), dbf = {dbfb:.4g}, bar = {barb:.4g}")
    assert dbf <= bar, (dbf, bar)
    assert dbfb <= barb, (dbfb, barb)
