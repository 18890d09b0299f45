"""GPU: rebase of a living cache -- kivi_mf_store_shift, KiviCacheBase.rebase_, LlamaForCausalLM_KIVI.rebase_,
generate_continuous(compact=).  Every comparison is bit for bit; B = 3 and nh_kv = 2 at the layer level.

a. Bytes: a cache prefilled at T0 and decoded to L, then rebase_(drop), against the ORACLE: a second cache prefilled from the same
   K / V tensors with the first `drop` tokens cut off and decoded with the same step inputs.  The 9-tuple members, the range words,
   the lengths (all but v_res_start: the oracle's window started elsewhere) and, on the matrix-pipe layout, the whole stores over
   the common super-blocks; data pointers stay, a checkpoint taken before is refused as stale.  One case has a row whose DROPPED
   tokens hold a K and a V scale >= 256: the range words come out as the oracle's, not the old ones.
b. Steps: 40 decode steps and a 5-token extend on the rebased cache and on the oracle: equal outputs in every step, equal caches
   at the end (a K flush and a V block boundary fall inside the steps).
c. Sliced tuple: the rebased cache equals from_tuple of its own earlier 9-tuple with every token axis sliced by `drop`.
d. Model: rebase_(32) of caches at L = 84 whose rows all start with at least 32 pads, then 20 steps with the shortened mask, against
   caches rebuilt through the sliced-tuple oracle; the same through decode_graphed before and after the rebase.
e. generate_continuous(compact=32) against a restatement of the policy whose rebase goes through the sliced-tuple oracle.
"""
import pytest
import torch

from helpers import make_kv, same_bits
from test_admit_gpu import _check_outputs, _feed, _greedy, _prompts, _range_words, _same_member, _step_inputs
from test_admit_gpu import _restate as _restate_plain
from test_extend_gpu import _model
from test_sample_gpu import _layouts

pytestmark = pytest.mark.gpu
D, B, NH_KV = 128, 3, 2
LENGTHS = ("k_quant_len", "k_res_len", "v_quant_len", "v_res_len", "kv_seq_len")       # (v_res_start: the ring phase is the cache's own)


# ------------------------------------------------------------------ layer level
def _layer(layout, bits, ratio, R, cap):
    from kivi_amd.attention import KiviConfig, KiviLayerCache, make_layer_cache
    cfg = KiviConfig(bits, bits, 32, R)
    if layout == "hook":
        return KiviLayerCache(cfg, B, NH_KV, D, cap, "cuda")
    lc = make_layer_cache(cfg, B, NH_KV, D, cap, "cuda", num_heads=NH_KV * ratio)
    assert lc.layout == "mfma"
    return lc


def _steps(lc, ratio, first, n, seed=100):
    """Decode steps first .. first + n - 1 of a fixed input sequence (the same for a cache and its oracle) -> the outputs."""
    from kivi_amd.attention import kivi_attention_decode
    out = []
    for s in range(first, first + n):
        q, k, v = _step_inputs(seed + 3 * s, B, NH_KV * ratio, NH_KV)
        out.append(kivi_attention_decode(q, k, v, lc).clone())
    return out


def _pair(layout, bits, ratio, R, T0, L, drop, big=False):
    """-> (the cache at L, not yet rebased; the oracle at L - drop)."""
    k, v = make_kv(1, B, NH_KV, T0, D).cuda(), make_kv(2, B, NH_KV, T0, D, "outlier").cuda()
    if big:                                              # row 1: a K group and a V token among the dropped ones with a scale >= 256
        k[1, :, 5, 3] = 20000.0                          # (range / 3 at 2 bits, / 15 at 4 bits)
        v[1, :, 7, 40] = -30000.0
    lc, oracle = _layer(layout, bits, ratio, R, T0 + 8), _layer(layout, bits, ratio, R, T0 - drop + 8)
    lc.prefill(k, v)
    oracle.prefill(k[:, :, drop:], v[:, :, drop:])
    for c in (lc, oracle):
        _steps(c, ratio, 0, L - T0)
    assert lc.kv_seq_len == L and oracle.kv_seq_len == L - drop
    return lc, oracle


def _buffers(lc):
    return {n: getattr(lc, n) for n in lc._BUFFERS}


def _same_cache(a, b, stores=True):
    ta, tb = a.as_tuple(), b.as_tuple()
    assert ta[8] == tb[8]
    for i, (x, y) in enumerate(zip(ta[:8], tb[:8])):
        assert _same_member(x, y), i
    for i, (x, y) in enumerate(zip(_range_words(a), _range_words(b))):
        assert torch.equal(x, y), (i, x.tolist(), y.tolist())
    assert [getattr(a, n) for n in LENGTHS] == [getattr(b, n) for n in LENGTHS]
    if stores and hasattr(a, "kt"):                      # vacated blocks are zero, as in a store they were never written to
        n = min(a.n_sb, b.n_sb)
        assert torch.equal(a.kt[:, :, :n], b.kt[:, :, :n]) and torch.equal(a.vt[:, :, :n], b.vt[:, :, :n])


def _sliced(t, drop, kf, g=32):
    """A 9-tuple (members cloned) with every token axis cut by `drop` tokens from the front."""
    kc, kfull, ks, km, vc, vfull, vs, vm, n = [x.clone() if torch.is_tensor(x) else x for x in t]
    if kc is not None:
        kc, ks, km = (None,) * 3 if kc.shape[-1] * kf == drop else (kc[..., drop // kf:], ks[..., drop // g:], km[..., drop // g:])
    if vc is not None:
        vc, vs, vm = (None,) * 3 if vc.shape[2] == drop else (vc[:, :, drop:], vs[:, :, drop:], vm[:, :, drop:])
    return (kc, kfull, ks, km, vc, vfull, vs, vm, n - drop)


def _from_sliced(lc, drop):
    """The sliced-tuple oracle: a new cache from_tuple of lc's 9-tuple without its first `drop` tokens."""
    t = _sliced(tuple(lc.as_tuple()), drop, 32 // lc.cfg.k_bits)
    if hasattr(lc, "kt"):
        return type(lc).from_tuple(lc.cfg, t, lc.cap, lc.nh)
    return type(lc).from_tuple(lc.cfg, t, lc.cap)


LAYOUTS = [("mfma", 2, 1), ("mfma", 2, 4), ("mfma", 4, 4), ("hook", 2, 1), ("hook", 2, 4)]
SHAPES = [(40, 64, 32),          # V kept = 0, K kept = 32
          (40, 110, 32),         # one block; the in-flight depth exceeds the shift
          (300, 330, 256),       # K half-super-block boundary
          (500, 530, 480),       # 15 blocks
          (600, 650, 512),       # exactly one super-block
          (600, 650, 544),       # 17 blocks, crossing
          (1100, 1130, 1056)]    # 33 blocks, three super-blocks
CASES = [(lay, bits, ratio, 32, *s) for lay, bits, ratio in LAYOUTS for s in SHAPES] + \
    [("mfma", 2, 4, 64, 350, 360, 256), ("mfma", 2, 1, 128, 480, 490, 256)]           # a K flush within 40 steps of L at these R


@pytest.mark.parametrize("layout,bits,ratio,R,T0,L,drop", CASES)
def test_rebased_bytes_steps_and_sliced_tuple(layout, bits, ratio, R, T0, L, drop):
    from kivi_amd.attention import kivi_attention_extend
    lc, oracle = _pair(layout, bits, ratio, R, T0, L, drop)
    assert lc.rebase_quantum == R and lc.rebase_limit >= drop
    ptrs = {n: t.data_ptr() for n, t in _buffers(lc).items()}
    start, cap, ck = lc.v_res_start, lc.cap, lc.checkpoint()
    sliced = _from_sliced(lc, drop)
    # a. bytes
    assert lc.rebase_(drop) is lc
    _same_cache(lc, oracle)
    assert ptrs == {n: t.data_ptr() for n, t in _buffers(lc).items()} and (lc.v_res_start, lc.cap) == (start, cap)
    with pytest.raises(ValueError, match="stale"):
        lc.restore_(ck)
    # c. the sliced tuple (its stores were written by the relayout, tail slots of a partial V block included: members and words)
    _same_cache(lc, sliced, stores=False)
    # b. steps
    kq, vq = lc.k_quant_len, lc.v_quant_len
    for s, (x, y) in enumerate(zip(_steps(lc, ratio, L - T0, 40), _steps(oracle, ratio, L - T0, 40))):
        assert same_bits(x, y), s
    assert lc.k_quant_len > kq and lc.v_quant_len == vq + 40 and vq // 32 != lc.v_quant_len // 32     # a K flush, a V block boundary
    q, k, v = (make_kv(77 + i, B, h, 5, D).cuda() for i, h in enumerate((NH_KV * ratio, NH_KV, NH_KV)))
    assert same_bits(kivi_attention_extend(q, k, v, lc), kivi_attention_extend(q, k, v, oracle))
    _same_cache(lc, oracle)


@pytest.mark.parametrize("layout,bits,ratio", [("mfma", 2, 1), ("mfma", 2, 4), ("mfma", 4, 4)])
def test_range_words_are_recomputed_from_the_kept_scales(layout, bits, ratio):
    from kivi_amd.quant import mfma
    lc, oracle = _pair(layout, bits, ratio, 32, 300, 330, 256, big=True)
    for st in (lc.kt, lc.vt):                            # the dropped tokens left their mark on row 1 alone
        assert mfma.range_big(st).any(1).tolist() == [False, True, False]
    for st in (oracle.kt, oracle.vt):
        assert not mfma.range_big(st).any()
    lc.rebase_(256)
    _same_cache(lc, oracle)
    for st in (lc.kt, lc.vt):
        assert not mfma.range_big(st).any() and (mfma.range_flags(st) != 0).all()
    for x, y in zip(_steps(lc, ratio, 30, 3), _steps(oracle, ratio, 30, 3)):
        assert same_bits(x, y)


@pytest.mark.parametrize("layout,bits,ratio", [("mfma", 2, 1), ("mfma", 4, 4)])
def test_nothing_kept_leaves_zero_words_and_zero_blocks(layout, bits, ratio):
    from kivi_amd.quant import mfma
    lc, oracle = _pair(layout, bits, ratio, 32, 40, 64, 32)
    lc.rebase_(32)                                       # V kept = 0
    assert lc.v_quant_len == 0 and not mfma.range_flags(lc.vt).any() and not lc.vt.any()
    assert (mfma.range_flags(lc.kt) != 0).all()
    lc.rebase_(0)
    _same_cache(lc, oracle)


# ------------------------------------------------------------------ model level
def _oracle_pasts(past, drop):
    return [_from_sliced(p.layer, drop).as_tuple() for p in past]


def _at_84(model):
    """A batch of 3 (20, 14 and 7 tokens) left-padded to 52 (32, 38 and 45 leading pads) and generated for 32 steps, to L = 84:
    (ids, prompt mask, the 33 tokens generate() picks)."""
    from kivi_amd.llama import left_pad
    ids, mask = left_pad(_prompts(1, [20, 14, 7]), 0, "cuda", length=52)
    return ids, mask, model.generate(ids, 33, attention_mask=mask)[:, 52:]


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_rebase_eager(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 61)
    ids, mask, gen = _at_84(model)
    lg, past, mask = _feed(model, ids, mask, gen[:, :32])
    assert past[0][-1] == 84 and mask.shape == (3, 84) and getattr(past[0].layer, "layout", "hook") == layout
    assert int(mask.sum(-1).max()) == 84 - 32 and model.rebase_quantum(past) == 32 and model.rebase_limit(past) == 52
    want_past = _oracle_pasts(past, 32)
    caches = [p.layer for p in past]
    past2 = model.rebase_(past, 32)
    assert [p.layer for p in past2] == caches and past2[0][-1] == 52
    got = _greedy(model, lg, past2, mask[:, 32:], 20)
    want = _greedy(model, lg, want_past, mask[:, 32:], 20)
    assert torch.equal(got, want)
    assert torch.equal(got[:, 0], gen[:, 32])                                      # (the token the unrebased run picks next)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_rebase_graphed(layout, monkeypatch):
    """decode_graphed before and after the rebase: the tokens of the eager run, at most one capture more than without the rebase."""
    _layouts(monkeypatch, layout)
    model = _model(4, 62)
    ids, mask, gen = _at_84(model)
    one = torch.ones((3, 1), dtype=mask.dtype, device="cuda")
    lg, past, mask84 = _feed(model, ids, mask, gen[:, :32])
    eager = _greedy(model, lg, model.rebase_(past, 32), mask84[:, 32:], 20)

    def graphed(drop):
        model.release_graphs()
        lg, past = model(ids, padding_mask=mask)
        a = model.decode_graphed(lg.argmax(-1), past, 52, 32, attention_mask=torch.cat([mask, one], 1))
        assert torch.equal(a, gen[:, :32])
        past = model.rebase_(past, drop)
        b = model.decode_graphed(model.graphs.tok.clone(), past, 84 - drop, 20, attention_mask=torch.cat([mask84[:, drop:], one], 1))
        return b, model.graphs.stats
    without, stats0 = graphed(0)
    got, stats = graphed(32)
    assert torch.equal(got, eager) and torch.equal(got[:, 0], gen[:, 32]) and torch.equal(without[:, 0], gen[:, 32])
    if layout == "mfma":                                 # (eager steps, captures, replays): 52 steps in both runs
        assert stats[1] <= stats0[1] + 1 and stats[0] + stats[2] == stats0[0] + stats0[2] == 52


# ------------------------------------------------------------------ the scheduler
def _restate(model, prompts, limits, batch, compact, eos=None, pad=0, params=None):
    """The policy of kivi_amd/serving.py with compact= written out from forward(padding_mask=), admit_, argmax and RowSampler; the
    rebase goes through the sliced-tuple oracle (new caches from the sliced 9-tuples), not through rebase_.
    -> (tokens per request, the (L, drop) of every rebase, L at the end)."""
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler
    N, nb, L = len(prompts), min(batch, len(prompts)), max(len(p) for p in prompts)

    def draw(lg, reqs):
        return lg.argmax(-1) if params is None else RowSampler([params[r] for r in reqs], "cuda")(lg)
    ids, mask = left_pad(prompts[:nb], pad, "cuda", length=L)
    lg, past = model(ids, padding_mask=mask)
    rs = None if params is None else RowSampler(params[:nb], "cuda")
    tok = lg.argmax(-1) if rs is None else rs(lg)
    req, out, nxt, drops = list(range(nb)), [[] for _ in range(N)], nb, []
    lead = [L - len(prompts[r]) for r in range(nb)]

    def emit(b, t):
        r = req[b]
        out[r].append(t)
        if len(out[r]) == limits[r] or t == eos:
            req[b] = None
    while True:
        for b, t in enumerate(tok[:, 0].tolist()):
            if req[b] is not None:
                emit(b, t)
        live = [lead[b] for b in range(nb) if req[b] is not None]
        room = min(min(live) if live else L, L - max([len(p) for p in prompts[nxt:]], default=0),
                   min(past[0].layer.k_quant_len, past[0].layer.v_quant_len))
        drop = room // 32 * 32
        if drop >= compact:
            past = _oracle_pasts(past, drop)
            mask = mask[:, drop:]
            drops.append((L, drop))
            L -= drop
            lead = [n - drop for n in lead]
        while nxt < N and None in req:
            free = [b for b in range(nb) if req[b] is None][: N - nxt]
            new = list(range(nxt, nxt + len(free)))
            nxt += len(free)
            nids, nmask = left_pad([prompts[r] for r in new], pad, "cuda", length=L)
            lg, past = model.admit_(past, free, nids, nmask)
            mask[free] = nmask
            first = draw(lg, new)
            tok[free] = first
            for b, r, t in zip(free, new, first[:, 0].tolist()):
                req[b], lead[b] = r, L - len(prompts[r])
                if rs is not None:
                    rs.set_row(b, params[r], draw_index=1)
                emit(b, t)
        if all(r is None for r in req):
            return out, drops, L
        for b in range(nb):
            if req[b] is None:
                tok[b] = pad
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(tok, past, padding_mask=mask)
        tok = lg.argmax(-1) if rs is None else rs(lg)
        L += 1


LENS, LIMITS = [66, 12, 9, 8, 30, 7, 11, 6, 9, 5], [3, 20, 24, 12, 26, 10, 9, 12, 1, 6]


def _watch(model, monkeypatch):
    """Counters on the model: the kv length after every rebase_, the kv length every eager step starts from."""
    rebases, steps = [], []
    rebase_, forward_ = model.rebase_, model._forward

    def counted(past, drop):
        out = rebase_(past, drop)
        rebases.append((out[0][-1] + drop, drop))
        return out

    def stepped(ids, past=None, *a, **k):
        if past is not None:
            steps.append(past[0].layer.kv_seq_len)
        return forward_(ids, past, *a, **k)
    monkeypatch.setattr(model, "rebase_", counted)
    monkeypatch.setattr(model, "_forward", stepped)
    return rebases, steps


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_compact_greedy(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 63)
    prompts = _prompts(6, LENS)
    want, drops, L_end = _restate(model, prompts, LIMITS, 3, 32)
    assert drops == [(68, 32), (72, 32)]                                           # what the lengths of this queue give
    rebases, steps = _watch(model, monkeypatch)
    out = model.generate_continuous(prompts, LIMITS, 3, compact=32)
    _check_outputs(out, LIMITS)
    assert [o.tolist() for o in out] == want
    assert rebases == drops and steps[-1] + 1 == L_end == 41
    del rebases[:], steps[:]
    graphed = model.generate_continuous(prompts, LIMITS, 3, compact=32, graphed=True)
    assert [o.tolist() for o in graphed] == want and rebases == drops
    # compact=None: the existing behaviour, and a longer cache at the end
    del rebases[:], steps[:]
    plain = model.generate_continuous(prompts, LIMITS, 3, compact=None)
    assert rebases == [] and steps[-1] + 1 == 105 > L_end
    assert [o.tolist() for o in plain] == _restate_plain(model, prompts, LIMITS, 3)[0]
    # EOS: a token some request generated
    eos = want[2][9]
    out_e = model.generate_continuous(prompts, LIMITS, 3, eos_token_id=eos, pad_token_id=0, compact=32)
    _check_outputs(out_e, LIMITS, eos)
    want_e, drops_e, _ = _restate(model, prompts, LIMITS, 3, 32, eos=eos)
    assert [o.tolist() for o in out_e] == want_e and len(out_e[2]) <= 10 and drops_e
    graphed = model.generate_continuous(prompts, LIMITS, 3, eos_token_id=eos, pad_token_id=0, compact=32, graphed=True)
    assert [o.tolist() for o in graphed] == want_e


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_compact_sampling(layout, monkeypatch):
    from kivi_amd.sampling import SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 64)
    prompts = _prompts(7, LENS)
    params = [SamplingParams(temperature=0.8 + 0.05 * r, top_k=(0, 40, 25)[r % 3], top_p=(0.9, 1.0)[r % 2], seed=80 + r) if r % 4 else
              SamplingParams(do_sample=False) for r in range(len(LENS))]
    want, drops, _ = _restate(model, prompts, LIMITS, 3, 32, params=params)
    assert len(drops) >= 2
    out = model.generate_continuous(prompts, LIMITS, 3, sampling=params, compact=32)
    _check_outputs(out, LIMITS)
    assert [o.tolist() for o in out] == want
    graphed = model.generate_continuous(prompts, LIMITS, 3, sampling=params, compact=32, graphed=True)
    assert [o.tolist() for o in graphed] == want
