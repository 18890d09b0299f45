"""GPU: beam search over the quantised KV cache (kivi_cache_reorder, reorder_ / index_select, generate(num_beams=...)).

1. reorder_ is exact against an independent construction on both layouts: cache A shares a prompt per group, takes different
   decode-step tokens per row (across a K flush, a V window flush, a 512-token super-block boundary and a capacity growth), then
   reorder_(idx, group, from_token=prompt length); cache B is fed row idx[b]'s inputs from the start.  Every 9-tuple member, the
   range words and the next decode step are bit-identical.  The same with from_token = 0, different prompts and group = B.
2. index_select (the fork) equals a cache prefilled on the repeated inputs; _reorder_cache equals index_select of the members.
3. generate(num_beams=4): every returned sequence replayed teacher-forced in a batch of the same shape gives back its score bit for
   bit (the fp32 sum of log_softmax of its tokens / len ** length_penalty) -- wrong if any row continued from the wrong history;
   also for a left-padded batch and for a second turn (the caller's caches stay as they were).
Tiny random-weight models as in tests/test_extend_gpu.py."""
import pytest
import torch

from helpers import make_kv, same_bits
from test_extend_gpu import _model

pytestmark = pytest.mark.gpu
D = 128


def _layer(layout, bits, ratio, g, R, B, nh_kv, cap):
    from kivi_amd.attention import KiviConfig, KiviLayerCache, make_layer_cache
    cfg = KiviConfig(bits, bits, g, R)
    if layout == "hook":
        return KiviLayerCache(cfg, B, nh_kv, D, cap, "cuda")
    layer = make_layer_cache(cfg, B, nh_kv, D, cap, "cuda", num_heads=nh_kv * ratio)
    assert layer.layout == "mfma"
    return layer


def _same_state(a, b):
    ta, tb = a.as_tuple(), b.as_tuple()
    for x, y in zip(ta[:8], tb[:8]):
        assert (x is None and y is None) or (x is not None and y is not None and same_bits(x, y))
    assert ta[8] == tb[8]
    if getattr(a, "layout", "") == "mfma":
        from kivi_amd.quant import mfma
        for sa, sb in ((a.kt, b.kt), (a.vt, b.vt)):
            assert torch.equal(mfma.range_flags(sa), mfma.range_flags(sb))


def _steps(layer, n, rows, nh, nh_kv, seed):
    """n decode steps; row b takes the inputs of source row rows[b] (a (B,) index into per-source streams)."""
    from kivi_amd.attention import kivi_attention_decode
    S = int(rows.max()) + 1
    out = None
    for s in range(n):
        q = make_kv(seed + 3 * s, S, nh, 1, D).cuda()[rows]
        k = make_kv(seed + 3 * s + 1, S, nh_kv, 1, D).cuda()[rows]
        v = make_kv(seed + 3 * s + 2, S, nh_kv, 1, D).cuda()[rows]
        out = kivi_attention_decode(q, k, v, layer)
    return out


SHAPES = [("mfma", 2, 1, 32, 32), ("mfma", 2, 4, 32, 32), ("mfma", 2, 8, 32, 32), ("mfma", 4, 1, 32, 32), ("mfma", 4, 4, 32, 32),
          ("hook", 2, 1, 32, 32), ("hook", 4, 1, 64, 64)]


@pytest.mark.parametrize("layout,bits,ratio,g,R", SHAPES)
def test_reorder_from_fork_is_exact(layout, bits, ratio, g, R):
    B, G, nh_kv, T0, n = 8, 4, 2, 490, 40          # K flushes at 502 / 534 (R 32), V flushes every step, 512 crossed, cap grows
    nh = nh_kv * ratio
    idx = torch.tensor([1, 0, 2, 2, 4, 4, 7, 5], device="cuda")   # swap, identity, duplicate | identity, duplicate, chain
    prompt_k, prompt_v = make_kv(1, B // G, nh_kv, T0, D).cuda(), make_kv(2, B // G, nh_kv, T0, D).cuda()
    groups = torch.arange(B, device="cuda") // G
    a = _layer(layout, bits, ratio, g, R, B, nh_kv, T0 + 8)
    a.prefill(prompt_k[groups], prompt_v[groups])
    _steps(a, n, torch.arange(B, device="cuda"), nh, nh_kv, 100)
    a.reorder_(idx, group=G, from_token=T0)
    b = _layer(layout, bits, ratio, g, R, B, nh_kv, T0 + 8)
    b.prefill(prompt_k[groups], prompt_v[groups])
    _steps(b, n, idx, nh, nh_kv, 100)
    _same_state(a, b)
    rows = torch.arange(B, device="cuda")
    assert same_bits(_steps(a, 1, rows, nh, nh_kv, 900), _steps(b, 1, rows, nh, nh_kv, 900))
    _same_state(a, b)


@pytest.mark.parametrize("layout,bits,ratio,g,R", [SHAPES[0], SHAPES[4], SHAPES[5], SHAPES[6]])
def test_reorder_whole_rows_any_permutation(layout, bits, ratio, g, R):
    B, nh_kv, T0, n = 8, 2, 530, 20
    nh = nh_kv * ratio
    idx = torch.tensor([3, 0, 7, 2, 4, 4, 1, 6], device="cuda", dtype=torch.int32)
    pk, pv = make_kv(5, B, nh_kv, T0, D).cuda(), make_kv(6, B, nh_kv, T0, D).cuda()
    a = _layer(layout, bits, ratio, g, R, B, nh_kv, T0 + 8)
    a.prefill(pk, pv)
    _steps(a, n, torch.arange(B, device="cuda"), nh, nh_kv, 300)
    a.reorder_(idx)                                   # group = B, from_token = 0
    b = _layer(layout, bits, ratio, g, R, B, nh_kv, T0 + 8)
    b.prefill(pk[idx.long()], pv[idx.long()])
    _steps(b, n, idx.long(), nh, nh_kv, 300)
    _same_state(a, b)
    rows = torch.arange(B, device="cuda")
    assert same_bits(_steps(a, 1, rows, nh, nh_kv, 950), _steps(b, 1, rows, nh, nh_kv, 950))


@pytest.mark.parametrize("layout,bits,ratio,g,R", [SHAPES[1], SHAPES[5]])
def test_fork_and_reorder_cache(layout, bits, ratio, g, R):
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    nh_kv, T0 = 2, 300
    pk, pv = make_kv(7, 2, nh_kv, T0, D).cuda(), make_kv(8, 2, nh_kv, T0, D).cuda()
    src = _layer(layout, bits, ratio, g, R, 2, nh_kv, T0 + 8)
    src.prefill(pk, pv)
    _steps(src, 5, torch.arange(2, device="cuda"), nh_kv * ratio, nh_kv, 500)
    fork = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1], device="cuda")
    a = src.index_select(fork)
    b = _layer(layout, bits, ratio, g, R, 8, nh_kv, T0 + 8)
    b.prefill(pk[fork], pv[fork])
    _steps(b, 5, fork, nh_kv * ratio, nh_kv, 500)
    _same_state(a, b)
    # _reorder_cache: fresh tuples equal to index_select of the old members along dim 0
    before = [x.clone() if x is not None else None for x in a.as_tuple()[:8]]
    beam_idx = torch.tensor([2, 2, 0, 1, 7, 4, 5, 5], device="cuda")
    (t,) = LlamaForCausalLM_KIVI._reorder_cache([a.as_tuple()], beam_idx)
    for x, y in zip(t[:8], before):
        assert (x is None and y is None) or same_bits(x, y.index_select(0, beam_idx))


# ------------------------------------------------------------------ the model
def _replay(model, input_ids, seqs, nb, past=None, mask=None):
    """Teacher-forced replay of returned sequences (B * nb rows, request-major) in a batch of the search's shape: the per-token
    fp32 log_softmax of every row's own tokens, (B * nb, L)."""
    from kivi_amd.llama import padding_key_row, padding_position_ids, padding_prompt_mask
    B, T = input_ids.shape
    past_len = model._past_len(past)
    if past is not None:
        past = [p.layer.clone().as_tuple() for p in past]
    L = seqs.shape[1] - T
    row = pos = None
    if mask is not None:
        row = padding_key_row(mask, past_len + T + L)
        m = padding_prompt_mask(mask) if past_len == 0 else row[..., : past_len + T].expand(-1, -1, T, -1)
        logits, pasts = model._forward(input_ids, past, m, padding_position_ids(mask, T), True, True)
        pos = mask.long().sum(-1, keepdim=True).repeat_interleave(nb, 0)
        row = row.repeat_interleave(nb, 0)
    else:
        logits, pasts = model.forward(input_ids, past)
    caches = [p.layer.index_select(torch.arange(B, device="cuda").repeat_interleave(nb)) for p in pasts]
    lps = [torch.log_softmax(logits[:, -1].float(), -1).repeat_interleave(nb, 0)]
    for s in range(L - 1):
        tok = seqs[:, T + s: T + s + 1]
        pasts = [c.as_tuple() for c in caches]
        if row is None:
            logits, _ = model.forward(tok, pasts)
        else:
            logits, _ = model._forward(tok, pasts, row[..., : past_len + T + s + 1], pos, True, True)
            pos = pos + 1
        lps.append(torch.log_softmax(logits[:, -1].float(), -1))
    return torch.stack([lp.gather(1, seqs[:, T + i: T + i + 1])[:, 0] for i, lp in enumerate(lps)], 1)


def _check_scores(seqs, scores, lps, T, eos, lp):
    for r in range(seqs.shape[0]):
        gen = seqs[r, T:].tolist()
        n = gen.index(eos) + 1 if eos is not None and eos in gen else len(gen)
        acc = torch.zeros((), dtype=torch.float32, device="cuda")
        for i in range(n):
            acc = acc + lps[r, i]
        assert same_bits((acc / (n ** lp)).reshape(1), scores[r].reshape(1)), (r, float(acc / n ** lp), float(scores[r]))


@pytest.mark.parametrize("nkv", [1, 4])
def test_generate_beams_scores_replay(nkv, monkeypatch):
    import kivi_amd.attention as A
    import kivi_amd.cache_mf as CM
    model = _model(nkv, 11)
    ids = torch.randint(0, 320, (2, 37), device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    layouts = ["mfma", "hook"]
    for layout in layouts:
        with monkeypatch.context() as m:
            if layout == "hook":
                m.setattr(CM, "supported", lambda *a, **k: False)
                m.setattr(A, "_mf_supported", lambda *a, **k: False)
            assert torch.equal(model.generate(ids, 6, num_beams=1), model.generate(ids, 6))
            for eos, lp in ((None, 1.0), (7, 2.0)):
                kw = {} if eos is None else dict(eos_token_id=eos, pad_token_id=0)
                if eos is not None:         # an EOS the model actually produces: the second token of the best beam without one
                    s0 = model.generate(ids, 6, num_beams=4)
                    eos = kw["eos_token_id"] = int(s0[0, 38])
                seqs, scores = model.generate(ids, 30, num_beams=4, num_return_sequences=4, length_penalty=lp, return_scores=True, **kw)
                p0 = model(ids)[1][0].layer
                assert getattr(p0, "layout", "hook") == layout
                _check_scores(seqs, scores, _replay(model, ids, seqs, 4), 37, eos, lp)


def test_generate_beams_padded_and_second_turn():
    from kivi_amd.llama import left_pad
    model = _model(4, 12)
    ids, mask = left_pad([list(range(3, 40)), list(range(50, 71))], pad_token_id=0, device="cuda")
    seqs, scores = model.generate(ids, 12, attention_mask=mask, num_beams=4, num_return_sequences=4, return_scores=True)
    _check_scores(seqs, scores, _replay(model, ids, seqs, 4, mask=mask), ids.shape[1], None, 1.0)
    # second turn over the caller's caches (greedy first turn), which stay as they were
    _, past = model(ids, padding_mask=mask)
    before = [p.layer.clone() for p in past]
    ids2 = torch.randint(0, 320, (2, 9), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    mask2 = torch.cat([mask, torch.ones_like(ids2)], 1)
    seqs, scores = model.generate(ids2, 10, past_key_values=past, attention_mask=mask2, num_beams=4, num_return_sequences=4,
                                  return_scores=True)
    for p, c in zip(past, before):
        _same_state(p.layer, c)
    _check_scores(seqs, scores, _replay(model, ids2, seqs, 4, past=past, mask=mask2), 9, None, 1.0)
