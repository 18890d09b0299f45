"""GPU: continuous batching -- kivi_cache_admit, KiviCacheBase.admit_, LlamaForCausalLM_KIVI.admit_, generate_continuous
(DESIGN.md section 16).  Every comparison is bit for bit.

5. Bytes: rows of a fresh prompt-pass cache admitted into a destination that was prefilled at T0 and decoded to L (ring phase moved
   and wrapped, K flushes, a super-block crossed, stores grown by reserve()): the 9-tuple members and range words of the admitted
   rows are the source's, every other row of every tensor the cache holds is unchanged, lengths / data pointers / the native
   descriptor stay, a checkpoint taken before is refused.  Both layouts, 2-bit at nh / nh_kv 1 and 4, 4-bit matrix-pipe at 4.
6. Steps: after admitting 3 rows to rows [2, 0, 1], 40 decode steps on source and destination with the inputs permuted accordingly
   give equal outputs in every step and equal caches at the end; one case goes on with a 5-token extend.
7. Model, all rows replaced: after admit_ into caches at L = 84 the continuation equals generate() on the new prompts alone --
   eagerly, and through two decode_graphed calls around the admission with ONE capture and a RowSampler whose rows were set_row'd.
8. Model, one row replaced: the other rows go on as if nothing happened; the admitted row's caches are those of its prompt alone.
9. generate_continuous against a restatement of its policy, against generate() on the initial batch, graphed against eager, with
   EOS, with per-request sampling; a request's draws do not depend on the row it lands in (at the sampler).
"""
import pytest
import torch

from helpers import make_kv, same_bits
from test_extend_gpu import _model
from test_sample_gpu import _layouts

pytestmark = pytest.mark.gpu
D, R = 128, 32


# ------------------------------------------------------------------ layer level
def _layer(layout, bits, ratio, B, cap, nh_kv=2):
    from kivi_amd.attention import KiviConfig, KiviLayerCache, make_layer_cache
    cfg = KiviConfig(bits, bits, 32, R)
    if layout == "hook":
        return KiviLayerCache(cfg, B, nh_kv, D, cap, "cuda")
    lc = make_layer_cache(cfg, B, nh_kv, D, cap, "cuda", num_heads=nh_kv * ratio)
    assert lc.layout == "mfma"
    return lc


def _prefilled(layout, bits, ratio, B, T, seed, nh_kv=2):
    lc = _layer(layout, bits, ratio, B, T + 8, nh_kv)
    lc.prefill(make_kv(seed, B, nh_kv, T, D).cuda(), make_kv(seed + 1, B, nh_kv, T, D, "outlier").cuda())
    return lc


def _step_inputs(seed, B, nh, nh_kv):
    return (make_kv(seed, B, nh, 1, D).cuda(), make_kv(seed + 1, B, nh_kv, 1, D, "outlier").cuda(),
            make_kv(seed + 2, B, nh_kv, 1, D).cuda())


def _decode_to(lc, L, ratio, seed):
    from kivi_amd.attention import kivi_attention_decode
    while lc.kv_seq_len < L:
        q, k, v = _step_inputs(seed + 3 * lc.kv_seq_len, lc.B, lc.nh_kv * ratio, lc.nh_kv)
        kivi_attention_decode(q, k, v, lc)
    return lc


def _range_words(lc):
    from kivi_amd.quant import mfma
    return [mfma.range_flags(lc.kt), mfma.range_flags(lc.vt)] if hasattr(lc, "kt") else []


def _held(lc):
    """Every tensor the cache object holds that has a row per batch row (scratch rows and range words included)."""
    out = {n: t for n, t in lc.__dict__.items() if torch.is_tensor(t) and t.dim() and t.shape[0] == lc.B}
    out.update({f"range{i}": t for i, t in enumerate(_range_words(lc))})
    return out


def _same_member(x, y):
    return (x is None and y is None) or (x is not None and y is not None and same_bits(x, y))


def _admit_and_check(dst, src, rows):
    lengths = tuple(getattr(dst, n) for n in ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len"))
    before = {n: t.clone() for n, t in _held(dst).items()}
    ptrs = {n: t.data_ptr() for n, t in _held(dst).items()}
    nat, ck = dst._native, dst.checkpoint()
    want, want_range = src.as_tuple(), [t.clone() for t in _range_words(src)]
    assert dst.admit_(torch.tensor(rows, device="cuda", dtype=torch.int32 if len(rows) == 1 else torch.int64), src) is dst
    got = dst.as_tuple()
    assert got[8] == want[8] == lengths[5]
    for i, (x, y) in enumerate(zip(got[:8], want[:8])):
        assert _same_member(None if x is None else x[rows], y), i
    for x, y in zip(_range_words(dst), want_range):
        assert torch.equal(x[rows], y)
    others = [b for b in range(dst.B) if b not in rows]
    for n, t in _held(dst).items():
        assert t.data_ptr() == ptrs[n], n
        assert torch.equal(t[others].view(torch.uint8), before[n][others].view(torch.uint8)), n
    assert lengths == tuple(getattr(dst, n) for n in ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len"))
    assert dst._native is nat
    with pytest.raises(ValueError, match="stale"):
        dst.restore_(ck)
    for x, y in zip(src.as_tuple()[:8], want[:8]):       # the source is only read
        assert _same_member(x, y)


LAYOUTS = [("mfma", 2, 1), ("mfma", 2, 4), ("hook", 2, 1), ("hook", 2, 4), ("mfma", 4, 4)]


@pytest.mark.parametrize("T0,L", [(9, 20), (40, 45), (40, 64), (40, 110), (500, 530)])
@pytest.mark.parametrize("layout,bits,ratio", LAYOUTS)
def test_admitted_bytes(layout, bits, ratio, T0, L):
    dst = _decode_to(_prefilled(layout, bits, ratio, 3, T0, 1), L, ratio, 100)
    assert dst.kv_seq_len == L and (dst._native is not None or layout == "hook")
    if layout == "mfma" and L > R:
        assert dst.v_res_start == (L - max(T0, R)) % (R + 1)                       # the ring has moved (and wrapped at (40, 110))
    twins = [dst.clone(), dst.clone()]
    for d in twins:                                                                # the native descriptor a step would have built
        d._desc(d.nh, "cuda") if layout == "mfma" else d._native_desc(d.nh_kv * ratio)
    _admit_and_check(dst, _prefilled(layout, bits, ratio, 1, L, 7), [1])
    _admit_and_check(twins[0], _prefilled(layout, bits, ratio, 2, L, 9), [2, 0])
    src = _decode_to(_prefilled(layout, bits, ratio, 2, L - 3, 11), L, ratio, 200)  # a source that has decoded itself
    if layout == "mfma" and L - 3 >= R:
        assert src.v_res_start == 3
    _admit_and_check(twins[1], src, [0, 2])


@pytest.mark.parametrize("layout,bits,ratio,extend", [("mfma", 2, 1, False), ("mfma", 2, 4, True), ("hook", 2, 1, False),
                                                      ("hook", 2, 4, False), ("mfma", 4, 4, False)])
def test_steps_after_admission(layout, bits, ratio, extend):
    from kivi_amd.attention import kivi_attention_decode, kivi_attention_extend
    rows, L, nh_kv = [2, 0, 1], 110, 2
    nh = nh_kv * ratio
    dst = _decode_to(_prefilled(layout, bits, ratio, 3, 40, 1), L, ratio, 100)
    src = _prefilled(layout, bits, ratio, 3, L, 5)
    dst.admit_(rows, src)
    inv = torch.tensor(rows, device="cuda")

    def to_dst(x):
        y = torch.empty_like(x)
        y[inv] = x                                                                 # destination row rows[i] is source row i
        return y
    for s in range(40):                                                            # a K flush at 128, a V flush in every step
        q, k, v = _step_inputs(1000 + 3 * s, 3, nh, nh_kv)
        a = kivi_attention_decode(q, k, v, src)
        b = kivi_attention_decode(to_dst(q), to_dst(k), to_dst(v), dst)
        assert same_bits(b[inv], a), s
    assert src.kv_seq_len == dst.kv_seq_len == L + 40 and dst.k_quant_len == 128
    if extend:
        q, k, v = (make_kv(77 + i, 3, h, 5, D).cuda() for i, h in enumerate((nh, nh_kv, nh_kv)))
        a = kivi_attention_extend(q, k, v, src)
        b = kivi_attention_extend(to_dst(q), to_dst(k), to_dst(v), dst)
        assert same_bits(b[inv], a)
    ta, tb = src.as_tuple(), dst.as_tuple()
    assert ta[8] == tb[8]
    for i, (x, y) in enumerate(zip(ta[:8], tb[:8])):
        assert _same_member(y if y is None else y[inv], x), i
    for x, y in zip(_range_words(src), _range_words(dst)):
        assert torch.equal(y[inv], x)


# ------------------------------------------------------------------ model level
def _prompts(seed, lens):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, 320, (n,), generator=g).tolist() for n in lens]


def _feed(model, ids, mask, toks):
    """forward(padding_mask=) over the prompt, then the given tokens one by one -> (logits after the last one, caches, mask)."""
    lg, past = model(ids, padding_mask=mask)
    for s in range(toks.shape[1]):
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(toks[:, s: s + 1], past, padding_mask=mask)
    return lg, past, mask


def _greedy(model, lg, past, mask, n):
    out = []
    for s in range(n):
        tok = lg.argmax(-1)
        out.append(tok)
        if s < n - 1:
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
            lg, past = model(tok, past, padding_mask=mask)
    return torch.cat(out, 1)


def _living(model):
    """A padded batch of 3 (47, 40 and 7 tokens) generated for 37 steps: (caches at L = 84, their 2D mask, the tokens)."""
    from kivi_amd.llama import left_pad
    ids, mask = left_pad(_prompts(1, [47, 40, 7]), 0, "cuda")
    gen = model.generate(ids, 37, attention_mask=mask)[:, 47:]
    _, past, mask = _feed(model, ids, mask, gen)
    assert past[0][-1] == 84 and mask.shape == (3, 84)
    return past, mask, gen


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_all_rows_replaced(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    _layouts(monkeypatch, layout)
    model = _model(4, 51)
    past, _, _ = _living(model)
    assert getattr(past[0].layer, "layout", "hook") == layout
    new_ids, new_mask = left_pad(_prompts(2, [84, 30, 3]), 0, "cuda", length=84)       # a prompt of exactly L tokens: no pad
    caches = [p.layer for p in past]
    lg, past2 = model.admit_(past, [0, 1, 2], new_ids, new_mask)
    assert lg.shape == (3, 1, 320) and [p.layer for p in past2] == caches and past2[0][-1] == 84
    want = model.generate(new_ids, 40, attention_mask=new_mask)[:, 84:]
    assert torch.equal(_greedy(model, lg, past2, new_mask, 40), want)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_all_rows_replaced_graphed(layout, monkeypatch):
    """Two decode_graphed calls around the admission: the same DecodeGraphs, one capture in all, a RowSampler re-bound by set_row."""
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler, SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 52)
    first = [SamplingParams(temperature=0.8, top_k=40, seed=61), SamplingParams(do_sample=False), SamplingParams(top_k=0, seed=62)]
    second = [SamplingParams(temperature=1.3, top_k=0, top_p=0.9, seed=63), SamplingParams(temperature=0.7, top_k=20, seed=64),
              SamplingParams(do_sample=False)]
    ids, mask = left_pad(_prompts(1, [47, 40, 7]), 0, "cuda")
    new_ids, new_mask = left_pad(_prompts(2, [84, 30, 3]), 0, "cuda", length=84)
    one = torch.ones((3, 1), dtype=mask.dtype, device="cuda")
    model.release_graphs()
    rs = RowSampler(first, "cuda")
    lg, past = model(ids, padding_mask=mask)
    a = model.decode_graphed(rs(lg), past, 47, 37, attention_mask=torch.cat([mask, one], 1), sampling=rs)
    assert torch.equal(a, model.generate(ids, 37, attention_mask=mask, sampling=RowSampler(first, "cuda"))[:, 47:])
    graphs, stats1 = model.graphs, model.graphs.stats
    lg, past = model.admit_(past, [0, 1, 2], new_ids, new_mask)
    for b, p in enumerate(second):
        rs.set_row(b, p)
    b_ = model.decode_graphed(rs(lg), past, 84, 40, attention_mask=torch.cat([new_mask, one], 1), sampling=rs)
    assert torch.equal(b_, model.generate(new_ids, 40, attention_mask=new_mask, sampling=RowSampler(second, "cuda"))[:, 84:])
    assert model.graphs is graphs and graphs.sampler_key == rs.key()
    if layout == "mfma":
        assert stats1 == (1, 1, 36) and model.graphs.stats == (1, 1, 76)           # the admission replays what was captured


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_one_row_replaced(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    _layouts(monkeypatch, layout)
    model = _model(1, 53)
    past, mask, _ = _living(model)
    twin = [p.layer.clone().as_tuple() for p in past]                              # the run without admission
    tok = torch.tensor([[11], [12], [13]], device="cuda")
    step_mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
    lg_t, twin = model(tok, twin, padding_mask=step_mask)
    untouched = _greedy(model, lg_t, twin, step_mask, 12)
    new_ids, new_mask = left_pad(_prompts(3, [30]), 0, "cuda", length=84)
    lg, past2 = model.admit_(past, [1], new_ids, new_mask)
    alone_lg, alone = model(new_ids, padding_mask=new_mask)                        # the prompt run alone
    assert same_bits(lg, alone_lg)
    for p, q in zip(past2, alone):
        tp, tq = p.layer.as_tuple(), q.layer.as_tuple()
        for i, (x, y) in enumerate(zip(tp[:8], tq[:8])):
            assert _same_member(x if x is None else x[1:2], y), i
        for x, y in zip(_range_words(p.layer), _range_words(q.layer)):
            assert torch.equal(x[1:2], y)
    # rows 0 and 2 go on as in the run without admission: they are fed the same token, row 1 its own first token
    tok[1] = lg.argmax(-1)[0]
    step_mask[1, :84] = new_mask[0]
    lg_a, past2 = model(tok, past2, padding_mask=step_mask)
    got = _greedy(model, lg_a, past2, step_mask, 12)
    assert torch.equal(got[[0, 2]], untouched[[0, 2]])


# ------------------------------------------------------------------ the scheduler
def _restate(model, prompts, limits, batch, eos=None, pad=0, params=None):
    """The policy of kivi_amd/serving.py written out from forward(padding_mask=), admit_, argmax and RowSampler.
    -> (tokens per request, the row every request landed in)."""
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler
    N, B, L = len(prompts), min(batch, len(prompts)), max(len(p) for p in prompts)

    def draw(lg, reqs):
        return lg.argmax(-1) if params is None else RowSampler([params[r] for r in reqs], "cuda")(lg)
    ids, mask = left_pad(prompts[:B], pad, "cuda", length=L)
    lg, past = model(ids, padding_mask=mask)
    rs = None if params is None else RowSampler(params[:B], "cuda")
    tok = lg.argmax(-1) if rs is None else rs(lg)
    req, out, landed, nxt = list(range(B)), [[] for _ in range(N)], {r: r for r in range(B)}, B

    def emit(b, t):
        r = req[b]
        out[r].append(t)
        if len(out[r]) == limits[r] or t == eos:
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
            lg, past = model.admit_(past, free, nids, nmask)
            mask[free] = nmask
            first = draw(lg, new)                                                  # draw 0 of each request's own seed
            tok[free] = first
            for b, r, t in zip(free, new, first[:, 0].tolist()):
                req[b], landed[r] = r, b
                if rs is not None:
                    rs.set_row(b, params[r], draw_index=1)
                emit(b, t)
        if all(r is None for r in req):
            return out, landed
        for b in range(B):
            if req[b] is None:
                tok[b] = pad
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(tok, past, padding_mask=mask)
        tok = lg.argmax(-1) if rs is None else rs(lg)
        L += 1


LENS, LIMITS = [21, 5, 33, 47, 12, 8, 26], [4, 30, 9, 12, 1, 25, 6]


def _check_outputs(out, limits, eos=None):
    assert len(out) == len(limits)
    for o, m in zip(out, limits):
        assert o.dtype == torch.int64 and o.dim() == 1 and 1 <= o.numel() <= m
        o = o.tolist()
        if eos is not None and eos in o:
            assert o.index(eos) == len(o) - 1                                      # it stops at its first EOS
        else:
            assert len(o) == m


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_greedy(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    _layouts(monkeypatch, layout)
    model = _model(4, 54)
    prompts = _prompts(4, LENS)
    out = model.generate_continuous(prompts, LIMITS, 3)
    _check_outputs(out, LIMITS)
    want, landed = _restate(model, prompts, LIMITS, 3)
    assert [o.tolist() for o in out] == want
    # request 0 ends after 4 tokens (row 0 -> request 3), request 2 after 9 (row 2 -> request 4, whose single token ends it at
    # once -> request 5 at the same length), request 3 after 12 more (row 0 -> request 6)
    assert landed == {0: 0, 1: 1, 2: 2, 3: 0, 4: 2, 5: 2, 6: 0}
    # requests 0 to 2: generate() on the initial padded batch, truncated at their ends
    ids, mask = left_pad(prompts[:3], 0, "cuda", length=47)
    gen = model.generate(ids, 30, attention_mask=mask)[:, 47:]
    for r in range(3):
        assert out[r].tolist() == gen[r, : LIMITS[r]].tolist(), r
    graphed = model.generate_continuous(prompts, LIMITS, 3, graphed=True)
    assert [o.tolist() for o in graphed] == want
    # an int for every request, more rows than requests
    few = model.generate_continuous(prompts[:2], 5, 4)
    ids2, mask2 = left_pad(prompts[:2], 0, "cuda")
    assert [o.tolist() for o in few] == model.generate(ids2, 5, attention_mask=mask2)[:, ids2.shape[1]:].tolist()
    # EOS: a token some request generated
    eos = want[1][7]
    out_e = model.generate_continuous(prompts, LIMITS, 3, eos_token_id=eos, pad_token_id=0)
    _check_outputs(out_e, LIMITS, eos)
    want_e, _ = _restate(model, prompts, LIMITS, 3, eos=eos)
    assert [o.tolist() for o in out_e] == want_e and len(out_e[1]) <= 8
    for r in range(3):                                                             # the initial batch, truncated at its EOS
        g = gen[r, : LIMITS[r]].tolist()
        assert out_e[r].tolist() == (g[: g.index(eos) + 1] if eos in g else g), r
    graphed = model.generate_continuous(prompts, LIMITS, 3, eos_token_id=eos, pad_token_id=0, graphed=True)
    assert [o.tolist() for o in graphed] == want_e


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_sampling(layout, monkeypatch):
    from kivi_amd.sampling import SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 55)
    prompts = _prompts(5, LENS)
    params = [SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=71), SamplingParams(do_sample=False),
              SamplingParams(temperature=1.4, top_k=0, min_p=0.02, seed=72), SamplingParams(temperature=0.9, top_k=30, seed=73),
              SamplingParams(seed=74), SamplingParams(do_sample=False), SamplingParams(temperature=1.1, top_k=0, top_p=0.8, seed=75)]
    out = model.generate_continuous(prompts, LIMITS, 3, sampling=params)
    _check_outputs(out, LIMITS)
    want, _ = _restate(model, prompts, LIMITS, 3, params=params)
    assert [o.tolist() for o in out] == want
    graphed = model.generate_continuous(prompts, LIMITS, 3, sampling=params, graphed=True)
    assert [o.tolist() for o in graphed] == want
    greedy = model.generate_continuous(prompts, LIMITS, 3)
    assert out[1].tolist() == greedy[1].tolist()                                   # a greedy request among sampled ones
    assert [o.tolist() for o in out] != [o.tolist() for o in greedy]


def test_a_requests_draws_do_not_depend_on_its_row():
    """The sampler side of an admission, given the logits: whichever row a request lands in and whatever the batch around it
    draws, token i of the request is draw i of its own seed with stream 0 -- what a RowSampler of the request alone draws."""
    from kivi_amd.sampling import RowSampler, SamplingParams
    V, n = 320, 12
    g = torch.Generator().manual_seed(6)
    p = SamplingParams(temperature=0.9, top_k=30, top_p=0.95, seed=0xC0FFEE)
    mine = (torch.randn((n, V), generator=g) * 3).half().cuda()                    # the request's logits, one row per token
    alone = RowSampler(p, "cuda")
    want = [int(alone(mine[i: i + 1])) for i in range(n)]
    seqs = []
    for row, B, fill, busy in ((0, 3, 0, 5), (2, 3, 1, 0), (1, 4, 2, 17)):
        others = [SamplingParams(do_sample=bool((i + fill) % 3), temperature=0.5 + 0.3 * i, seed=1000 * fill + i) for i in range(B)]
        rs = RowSampler(others, "cuda")
        batch = (torch.randn((B, V), generator=g) * 3).half().cuda()
        for _ in range(busy):                                                      # the batch has been drawing for a while
            rs(batch)
        first = int(RowSampler([p], "cuda")(mine[:1]))                             # the admission: draw 0 from the prompt logits
        rs.set_row(row, p, draw_index=1)
        toks = [first]
        for i in range(1, n):
            batch[row] = mine[i]
            toks.append(int(rs(batch)[row]))
        seqs.append(toks)
        assert rs.draw_index[row].item() == n
    assert seqs[0] == seqs[1] == seqs[2] == want and len(set(want)) > 3
