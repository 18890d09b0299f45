"""GPU: per-request LoRA adapters through the models (kivi_amd/lora.py).

The tiny llama and qwen2 of tests/tiny_w4_models.py (2 layers, hidden 256), dense and weight_bits=4, fp16 and bf16, with adapters
~ N(0, 0.05) of r = 4 and r = 16 on all seven targets in slots 0 and 1 of a set of three.
  * adapters=None and all-None lists give the parent's logits and tokens bit for bit, eager and graphed;
  * in a mixed batch [0, None, 1, 0] the None row equals the base model's row and row 0 equals row 0 of [0, 0, 0, 0], bit for bit;
  * per-step logits against a merged twin (W + scale B A formed in fp32, rounded once) at the bars of tests/test_w4_model_gpu.py, 1e-2
    of the rms in fp16 and 5e-2 in bf16 -- dense models only, a packed weight cannot absorb the update --, with the adapter moving
    the logits by more than ten times the bar; on passes that read nothing back from the 2-bit cache (the test's docstring);
  * generate_graphed gives generate's tokens, and another request mix replays the graphs that exist;
  * num_beams=2 and num_return_sequences=2 run with per-prompt slots;
  * generate_continuous, five requests over three slots at batch 2, eager and graphed, equals the policy restated from
    forward(adapters=) and admit_(adapters=) as tests/test_admit_gpu.py restates it, with as many graph builds as without adapters;
  * score(adapters=) equals the teacher-forced log-probabilities of forward(adapters=)."""
import functools
import itertools

import pytest
import torch

import lora_ref as R
import tiny_w4_models as M

pytestmark = pytest.mark.gpu
ALL7 = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
CASES = list(itertools.product(("llama", "qwen2"), (None, 4), (torch.float16, torch.bfloat16)))
IDS = [f"{f}-{'w4' if b else 'dense'}-{'fp16' if d == torch.float16 else 'bf16'}" for f, b, d in CASES]
DENSE = [(c, i) for c, i in zip(CASES, IDS) if c[1] is None]
T0, STEPS, LONG = 70, 12, 520


@functools.lru_cache(maxsize=None)
def _dense(family, dtype):
    return M.build_dense(family, 50 + len(family), dtype)


@functools.lru_cache(maxsize=None)
def _adapters(family):
    dense = _dense(family, torch.float16)
    return R.make_adapter(dense, 4, 8.0, 21, ALL7), R.make_adapter(dense, 16, 32.0, 22, ALL7)


@functools.lru_cache(maxsize=None)
def _model(family, bits, dtype):
    """The model with its LoraSet: slot 0 the r = 4 adapter, slot 1 the r = 16 adapter, slot 2 empty."""
    dense = _dense(family, dtype)
    model = dense if bits is None else M.quantised(family, dense, 128)
    lset = model.enable_lora(3, 16, ALL7)
    for slot, ad in enumerate(_adapters(family)):
        assert lset.load(ad) == slot
    return model


def _merged_twin(family, dtype, adapter):
    """A dense model of the same class whose target weights are round(W + scale B A), the update formed in fp32."""
    dense = _dense(family, dtype)
    twin = M.classes()[family](M.config(family)).to(dtype).cuda().eval()
    state = {k: v.clone() for k, v in dense.state_dict().items()}
    for name, (a, b) in adapter.tensors.items():
        a, b = a.to(dtype).float().cuda(), b.to(dtype).float().cuda()          # the values the tables hold
        state[name + ".weight"] = (state[name + ".weight"].float() + adapter.scale * (b @ a)).to(dtype)
    twin.load_state_dict(state)
    return twin


def _forced_logits(model, ids, forced, **kw):
    logits, past = model(ids, **kw)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past, **kw)
        out.append(logits)
    return out


@pytest.mark.parametrize("family,bits,dtype", CASES, ids=IDS)
def test_none_is_the_parent_bit_for_bit(family, bits, dtype):
    model = _model(family, bits, dtype)
    ids = M.prompts(3, 2, 40)
    lset = model.lora
    model.disable_lora()                                                # the parent: no hook anywhere
    want_logits = model(ids, last_token_only=False)[0]
    want, want_graphed = model.generate(ids, STEPS), model.generate_graphed(ids, STEPS)
    model.release_graphs()
    model.lora = lset.attach()
    for adapters in (None, [None, None], [-1, None]):
        assert torch.equal(model(ids, last_token_only=False, adapters=adapters)[0], want_logits)
        assert torch.equal(model.generate(ids, STEPS, adapters=adapters), want)
        assert torch.equal(model.generate_graphed(ids, STEPS, adapters=adapters), want_graphed)
    assert model.graphs.lora_key is None
    model.release_graphs()


@pytest.mark.parametrize("family,bits,dtype", CASES, ids=IDS)
def test_mixed_batch_rows_are_their_own(family, bits, dtype):
    model = _model(family, bits, dtype)
    ids = M.prompts(5, 4, 12)                                           # the prompt pass takes the launches too
    forced = torch.randint(1, M.VOCAB, (3, 4, 1), generator=torch.Generator().manual_seed(6)).cuda()
    base = _forced_logits(model, ids, forced)
    mixed = _forced_logits(model, ids, forced, adapters=[0, None, 1, 0])
    same = _forced_logits(model, ids, forced, adapters=[0, 0, 0, 0])
    one = _forced_logits(model, ids, forced, adapters=0)
    for s, (b, m, z, o) in enumerate(zip(base, mixed, same, one)):
        assert torch.equal(m[1], b[1]), s                               # the None row: the base model's bytes
        assert torch.equal(m[0], z[0]) and torch.equal(m[3], z[3]), s   # rows of slot 0: whatever the other rows run
        assert torch.equal(z, o), s
        assert not torch.equal(m[0], b[0]) and not torch.equal(m[2], b[2]) and not torch.equal(m[2], z[2]), s
    assert model.lora.active is None


@pytest.mark.parametrize("family,bits,dtype", [c for c, _ in DENSE], ids=[i for _, i in DENSE])
def test_logits_against_the_merged_twin(family, bits, dtype):
    """The passes stay inside the residual window (16 prompt tokens + 14 steps <= residual_length = 32), so no token of the compared
    steps is read back from the 2-bit cache: the twin rounds W + scale B A to the dtype, the adapter path rounds the base linear's
    output and the sum, so nearly every element of k and v differs in its last bit between the two, and the 2-bit quantiser turns a
    last-bit difference near a code boundary into a third of the group's range.  Measured with quantised tokens under the steps (70
    and 33 prompt tokens): 0.035-0.054 of the rms in fp16 and 0.06-0.26 in bf16, for the launches AND for apply_torch, which agree
    with each other to 0-0.0025 (fp16) / 0-0.025 (bf16) on the same passes -- the distance is the quantiser's, not the adapter
    path's.  The prompt pass attends in the dtype before anything is quantised, so a 520-token pass (1040 tokens: apply_torch) is
    compared too, on the logits a step has: the last position's, as tests/test_w4_model_gpu.py compares its prompt pass.  (Over all
    2 x 520 positions the maximum of so many more bf16 logits reached 0.0553 of the rms on the Llama-like model, fp16 stayed under
    1e-2; the bar is the one for a step's logits.)"""
    model = _model(family, bits, dtype)
    from kivi_amd import lora
    assert 2 * LONG > lora.LORA_KERNEL_MAX_TOKENS >= 2 * 16
    ids = M.prompts(4, 2, 16)                                           # 32 tokens: the launches, as in the steps
    forced = torch.randint(1, M.VOCAB, (14, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    long_ids = M.prompts(4, 2, LONG)                                    # 1040 tokens, past LORA_KERNEL_MAX_TOKENS: apply_torch
    bar = 1e-2 if dtype == torch.float16 else 5e-2
    base = _forced_logits(model, ids, forced) + [model(long_ids)[0]]
    for slot, adapter in enumerate(_adapters(family)):
        twin = _merged_twin(family, dtype, adapter)
        got = _forced_logits(model, ids, forced, adapters=slot) + [model(long_ids, adapters=slot)[0]]
        want = _forced_logits(twin, ids, forced) + [twin(long_ids)[0]]
        worst, moved = 0.0, float("inf")
        for s, (x, y, b) in enumerate(zip(got, want, base)):
            assert torch.isfinite(x).all() and x.dtype == y.dtype
            rms = y.float().pow(2).mean().sqrt().item()
            d = (x.float() - y.float()).abs().max().item() / rms
            worst, moved = max(worst, d), min(moved, (y.float() - b.float()).abs().max().item() / rms)
            assert d <= bar, (slot, s, d)
        print(f"{family} {dtype} r={adapter.r}: worst |adapter path - merged twin| / rms over a 16-token prompt pass, 14 steps and a {LONG}-token prompt pass = "
              f"{worst:.3g} (bar {bar}); the adapter moves the logits by at least {moved:.3g} of the rms")
        assert moved > 10 * bar, (slot, moved)                          # or the comparison would prove nothing
        del twin


@pytest.mark.parametrize("family,bits,dtype", CASES, ids=IDS)
def test_generate_graphed_equals_generate_and_a_new_mix_replays(family, bits, dtype):
    import kivi_amd.graph as G
    model = _model(family, bits, dtype)
    model.release_graphs()
    ids = M.prompts(7, 3, 33)
    built = []
    init = G.DecodeGraphs.__init__

    def counting(self, *a, **kw):
        built.append(1)
        init(self, *a, **kw)
    G.DecodeGraphs.__init__ = counting
    try:
        for adapters in ([0, None, 1], [1, 1, None], 0):
            eager = model.generate(ids, STEPS, adapters=adapters)
            graphed = model.generate_graphed(ids, STEPS, adapters=adapters)
            assert torch.equal(eager, graphed), adapters
            assert model.graphs.lora_key is not None and eager.shape == (3, 33 + STEPS)
        assert len(built) == 1                                          # three request mixes, one set of graphs
        base = model.generate(ids, STEPS)
        assert not torch.equal(eager, base)
    finally:
        G.DecodeGraphs.__init__ = init
        model.release_graphs()


@pytest.mark.parametrize("family,bits,dtype", [CASES[0], CASES[7]], ids=[IDS[0], IDS[7]])
def test_beams_and_samples_expand_a_requests_slot(family, bits, dtype):
    from kivi_amd.sampling import SamplingParams
    model = _model(family, bits, dtype)
    ids = M.prompts(8, 2, 20)
    beams = model.generate(ids, 6, num_beams=2, adapters=[1, None])
    assert beams.shape == (2, 26)
    alone = model.generate(ids, 6, num_beams=2)
    assert torch.equal(beams[1], alone[1])                              # the None request: the base model's beams
    two = model.generate(ids, 6, num_beams=2, num_return_sequences=2, adapters=[0, 1])
    assert two.shape == (4, 26)
    params = SamplingParams(do_sample=True, temperature=0.8, top_k=20, seed=3)
    drawn = model.generate(ids, 6, sampling=params, num_return_sequences=2, adapters=[None, 1])
    plain = model.generate(ids, 6, sampling=params, num_return_sequences=2)
    assert drawn.shape == (4, 26) and torch.equal(drawn[:2], plain[:2])
    assert model.lora.active is None


def _restate(model, prompts, limits, batch, slots, pad=0):
    """The policy of kivi_amd/serving.py written out from forward(padding_mask=, adapters=), admit_(adapters=) and argmax, as
    tests/test_admit_gpu.py restates it without adapters: a row runs its request's slot, an idle row the base model."""
    from kivi_amd.llama import left_pad
    N, B, L = len(prompts), min(batch, len(prompts)), max(len(p) for p in prompts)
    ids, mask = left_pad(prompts[:B], pad, "cuda", length=L)
    lg, past = model(ids, padding_mask=mask, adapters=slots[:B])
    tok = lg.argmax(-1)
    req, out, nxt = list(range(B)), [[] for _ in range(N)], B

    def emit(b, t):
        r = req[b]
        out[r].append(t)
        if len(out[r]) == limits[r]:
            req[b] = None
    while True:
        for b, t in enumerate(tok[:, 0].tolist()):
            if req[b] is not None:
                emit(b, t)
        while nxt < N and None in req:
            free = [b for b in range(B) if req[b] is None][: N - nxt]
            new = list(range(nxt, nxt + len(free)))
            nxt += len(free)
            nids, nmask = left_pad([prompts[r] for r in new], pad, "cuda", length=L)
            lg, past = model.admit_(past, free, nids, nmask, adapters=[slots[r] for r in new])
            mask[free] = nmask
            first = lg.argmax(-1)
            tok[free] = first
            for b, r, t in zip(free, new, first[:, 0].tolist()):
                req[b] = r
                emit(b, t)
        if all(r is None for r in req):
            return out
        for b in range(B):
            if req[b] is None:
                tok[b] = pad
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(tok, past, padding_mask=mask, adapters=[None if req[b] is None else slots[req[b]] for b in range(B)])
        tok = lg.argmax(-1)
        L += 1


@pytest.mark.parametrize("family,bits,dtype", [CASES[1], CASES[2], CASES[4], CASES[7]], ids=[IDS[1], IDS[2], IDS[4], IDS[7]])
def test_generate_continuous_over_three_slots(family, bits, dtype):
    import kivi_amd.graph as G
    model = _model(family, bits, dtype)
    model.release_graphs()
    g = torch.Generator().manual_seed(9)
    lens, limits, slots = [21, 5, 33, 47, 12], [4, 14, 9, 12, 6], [0, 2, None, 1, 0]
    model.lora.load(_adapters(family)[1], 2)                            # three slots in use
    prompts = [torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in lens]
    built = []
    init = G.DecodeGraphs.__init__

    def counting(self, *a, **kw):
        built.append(1)
        init(self, *a, **kw)
    G.DecodeGraphs.__init__ = counting
    try:
        want = _restate(model, prompts, limits, 2, slots)
        assert [len(w) for w in want] == limits
        out = model.generate_continuous(prompts, limits, 2, adapters=slots)
        assert [o.tolist() for o in out] == want
        plain = model.generate_continuous(prompts, limits, 2, graphed=True)
        model.release_graphs()
        without = len(built)
        out = model.generate_continuous(prompts, limits, 2, graphed=True, adapters=slots)
        assert [o.tolist() for o in out] == want
        assert len(built) - without == without                          # admissions replay: no more graph builds than without adapters
        assert [o.tolist() for o in plain] != want
    finally:
        G.DecodeGraphs.__init__ = init
        model.release_graphs()
        model.lora.unload(2)
    assert model.lora.active is None


@pytest.mark.parametrize("family,bits,dtype", [CASES[0], CASES[3], CASES[5], CASES[6]], ids=[IDS[0], IDS[3], IDS[5], IDS[6]])
def test_score_is_the_teacher_forced_logprob_of_forward(family, bits, dtype):
    from kivi_amd.scoring import reference_token_logprobs
    model = _model(family, bits, dtype)
    ids = M.prompts(11, 3, 50)
    adapters = [1, None, 0]
    lp, valid, _ = model.score(ids, adapters=adapters)
    lg, _ = model(ids, last_token_only=False, adapters=adapters)
    rlp, rlse, _ = reference_token_logprobs(lg[:, :-1], ids[:, 1:])
    xt = lg[:, :-1].double().cpu().gather(-1, ids[:, 1:].cpu().unsqueeze(-1)).squeeze(-1)
    bar = 2.0 ** -19 * torch.maximum(torch.maximum(torch.ones_like(rlse), rlse.abs()), xt.abs())    # tests/test_score_gpu.py's BAR
    assert bool(valid.all()) and ((lp.cpu().double() - rlp).abs() <= bar).all()
    base, _, _ = model.score(ids)
    assert torch.equal(base[1], lp[1]) and not torch.equal(base[0], lp[0])
    ppl = model.perplexity(ids, adapters=adapters)[0]
    assert torch.allclose(ppl.cpu(), torch.exp(-lp.double().mean(-1)).cpu(), rtol=1e-12, atol=0)
