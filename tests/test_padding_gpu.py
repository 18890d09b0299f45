"""GPU: batches of prompts with different lengths (left padding, HF's 2D attention mask).

1. kivi_mf_extend_layer with one broadcast key-mask row per batch row (mask_sq = 0) is bit-identical to the same mask built out,
   output and cache; the hook-state extend takes the same expanded view;
2. the model (forward(padding_mask=...) logits, generate(attention_mask=...) tokens) on both cache layouts against an explicit
   composition of the per-layer calls (kivi_attention_prefill / _extend / _decode) with the HF masks and positions spelled out
   here: bit-identical -- for one turn and for a padded second turn extended onto padded caches;
3. graphed decode (whole-step graph on the matrix-pipe layout, dense-only graph on the hook-state layout) equals eager decode token
   for token, across K and window flushes and a growth of the caches;
4. a mask without a pad changes nothing; the unpadded row of a padded batch matches the same prompt run alone.
Tiny random-weight models (hidden 512, 2 layers, vocab 320) as in tests/test_extend_gpu.py."""
import pytest
import torch

from helpers import same_bits
from test_extend_gpu import _assert_same_state, _chunk, _model, _setup

pytestmark = pytest.mark.gpu
MIN16 = torch.finfo(torch.float16).min
D = 128


def _row(B, total, pads):
    row = torch.zeros((B, 1, 1, total), dtype=torch.float16, device="cuda")
    for b, p in enumerate(pads):
        row[b, ..., :p] = MIN16
    return row


# ------------------------------------------------------------------ 1. the kernel boundary
@pytest.mark.parametrize("bits,ratio", [(2, 1), (2, 4), (4, 1)])
@pytest.mark.parametrize("Q", [5, 37])
def test_extend_broadcast_mask_bit_identical(bits, ratio, Q):
    from kivi_amd.attention import kivi_attention_extend
    B, nh_kv, R, T0 = 2, 2, 32, 130
    layer, _ = _setup(bits, ratio, R, T0, "randn", B, nh_kv)
    other = layer.clone()
    q, kn, vn = _chunk(Q, B, nh_kv * ratio, nh_kv, "randn")
    row = _row(B, T0 + Q, [40, 3])
    row[1, ..., 90:97] = MIN16                        # a hole in the history, not only a prefix
    view = row.expand(B, 1, Q, T0 + Q)
    assert view.stride(2) == 0
    a = kivi_attention_extend(q, kn, vn, layer, attention_mask=view)
    b = kivi_attention_extend(q, kn, vn, other, attention_mask=view.contiguous())
    assert same_bits(a, b)
    _assert_same_state(layer, other)


def test_hook_state_extend_takes_the_expanded_view():
    from kivi_amd.attention import KiviConfig, KiviLayerCache, kivi_attention_extend
    from helpers import make_kv
    B, nh_kv, R, T0, Q = 2, 2, 32, 70, 9
    cfg = KiviConfig(2, 2, 32, R)
    layer = KiviLayerCache(cfg, B, nh_kv, D, T0 + 8, "cuda")
    layer.prefill(make_kv(1, B, nh_kv, T0, D).cuda(), make_kv(2, B, nh_kv, T0, D).cuda())
    other = layer.clone()
    q, kn, vn = _chunk(Q, B, nh_kv, nh_kv, "randn")
    view = _row(B, T0 + Q, [33, 0]).expand(B, 1, Q, T0 + Q)
    assert same_bits(kivi_attention_extend(q, kn, vn, layer, attention_mask=view),
                     kivi_attention_extend(q, kn, vn, other, attention_mask=view.contiguous()))


# ------------------------------------------------------------------ 2. the model against an explicit composition
def _prompts(seed, lengths, vocab=320):
    g = torch.Generator().manual_seed(seed)
    from kivi_amd.llama import left_pad
    return left_pad([torch.randint(1, vocab, (n,), generator=g) for n in lengths], pad_token_id=0, device="cuda")


def _hf_masks(mask, past_len, T):
    """HF's additive 4D mask (causal + padding, finfo(fp16).min) of a pass of T tokens after `past_len` cached ones, and HF's
    position ids (cumsum - 1, pads at 1), written out element by element."""
    B, L = mask.shape
    m = mask.cpu()
    m4 = torch.zeros((B, 1, T, L), dtype=torch.float16)
    pos = torch.zeros((B, L), dtype=torch.long)
    for b in range(B):
        c = 0
        for j in range(L):
            c += int(m[b, j])
            pos[b, j] = c - 1 if m[b, j] else 1
        for i in range(T):
            for j in range(L):
                if j > past_len + i or not m[b, j]:
                    m4[b, 0, i, j] = MIN16
    return m4.cuda(), pos[:, L - T:].cuda()


def _compose(model, ids, m4, pos, caches):
    """One pass of the model from its per-layer calls; `caches[i]` None = the prompt pass (a cache is made)."""
    from kivi_amd.attention import kivi_attention_decode, kivi_attention_extend, kivi_attention_prefill, make_layer_cache
    x = model.model.embed_tokens(ids)
    B, T, _ = x.shape
    for i, layer in enumerate(model.model.layers):
        a = layer.self_attn
        nh, nkv = a.num_heads, a.num_key_value_heads
        h = layer.input_layernorm(x)
        q = a.q_proj(h).view(B, T, nh, D).transpose(1, 2)
        k = a.k_proj(h).view(B, T, nkv, D).transpose(1, 2)
        v = a.v_proj(h).view(B, T, nkv, D).transpose(1, 2)
        freqs = pos[:, :, None].float() * a.inv_freq[None, None, :].float()
        emb = torch.cat((freqs, freqs), dim=-1)
        cos, sin = emb.cos()[:, None].half(), emb.sin()[:, None].half()
        rot = lambda t: torch.cat((-t[..., D // 2:], t[..., : D // 2]), dim=-1)     # noqa: E731
        q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
        if caches[i] is None:
            caches[i] = make_layer_cache(a.kivi, B, nkv, D, a._capacity(T), "cuda", num_heads=nh)
            o = kivi_attention_prefill(q, k, v, caches[i], m4)
        elif T > 1:
            o = kivi_attention_extend(q, k, v, caches[i], m4)
        else:
            o = kivi_attention_decode(q, k, v, caches[i], m4)
        x = x + a.o_proj(o.transpose(1, 2).reshape(B, T, nh * D))
        x = x + layer.mlp(layer.post_attention_layernorm(x))
    return model.lm_head(model.model.norm(x[:, -1:]))


def _compose_generate(model, ids, mask, n, caches):
    """Greedy decoding by _compose: (tokens (B, n), logits of every pass)."""
    past = 0 if caches[0] is None else caches[0].kv_seq_len
    m4, pos = _hf_masks(mask, past, ids.shape[1])
    logits = [_compose(model, ids, m4, pos, caches)]
    toks = []
    for _ in range(n):
        tok = logits[-1].argmax(-1)
        toks.append(tok)
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        m4, pos = _hf_masks(mask, caches[0].kv_seq_len, 1)
        logits.append(_compose(model, tok, m4, pos, caches))
    return torch.cat(toks, 1), logits


def _model_steps(model, ids, mask, toks, pasts=None):
    """forward(padding_mask=...) over the prompt, then the given tokens one by one: the logits of every pass and the caches."""
    lg, pasts = model(ids, pasts, padding_mask=mask)
    logits = [lg]
    for s in range(toks.shape[1]):
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, pasts = model(toks[:, s:s + 1], pasts, padding_mask=mask)
        logits.append(lg)
    return logits, pasts


def _layouts(monkeypatch):
    import kivi_amd.attention as A
    import kivi_amd.cache_mf as CM

    yield "mfma"
    with monkeypatch.context() as m:
        m.setattr(CM, "supported", lambda *a, **k: False)
        m.setattr(A, "_mf_supported", lambda *a, **k: False)
        yield "hook"


@pytest.mark.parametrize("nkv", [1, 4])
def test_padded_generate_matches_composition(nkv, monkeypatch):
    model = _model(nkv, 5)
    ids, mask = _prompts(1, [47, 40, 7])                 # 0, 7 and 40 pads
    n = 6
    for layout in _layouts(monkeypatch):
        toks, ref_logits = _compose_generate(model, ids, mask, n, [None, None])
        gen = model.generate(ids, n, attention_mask=mask)
        assert torch.equal(gen[:, ids.shape[1]:], toks), layout
        logits, pasts = _model_steps(model, ids, mask, toks)
        assert getattr(pasts[0].layer, "layout", "hook") == layout
        for a, b in zip(logits, ref_logits):
            assert torch.isfinite(a).all() and same_bits(a, b), layout


@pytest.mark.parametrize("nkv", [1, 4])
def test_padded_second_turn_matches_composition(nkv, monkeypatch):
    model = _model(nkv, 6)
    ids1, m1 = _prompts(2, [47, 40, 7])
    ids2, m2 = _prompts(3, [5, 29, 12])
    mask = torch.cat([m1, m2], 1)
    n = 5
    for layout in _layouts(monkeypatch):
        caches = [None, None]
        m4, pos = _hf_masks(m1, 0, ids1.shape[1])
        _compose(model, ids1, m4, pos, caches)
        toks, ref_logits = _compose_generate(model, ids2, mask, n, caches)
        _, pasts = model(ids1, padding_mask=m1)
        gen = model.generate(ids2, n, past_key_values=pasts, attention_mask=mask)
        assert torch.equal(gen[:, ids2.shape[1]:], toks), layout
        _, pasts = model(ids1, padding_mask=m1)
        logits, pasts = _model_steps(model, ids2, mask, toks, pasts)
        for a, b in zip(logits, ref_logits):
            assert torch.isfinite(a).all() and same_bits(a, b), layout
        assert getattr(pasts[0].layer, "layout", "hook") == layout
        for p, c in zip(pasts, caches):
            assert p[-1] == c.kv_seq_len == ids1.shape[1] + ids2.shape[1] + n


# ------------------------------------------------------------------ 3. graphed decode under padding
@pytest.mark.parametrize("nkv,lengths,n", [(1, [47, 40, 7], 40), (4, [470, 500, 33], 50)])
def test_padded_graphed_equals_eager(nkv, lengths, n, monkeypatch):
    """n = 40 after 47 tokens crosses K flushes (R = 32) and moves the value window every step; 500 + 50 tokens outgrow the caches
    made for the prompt (544 tokens: the stores and the mask buffer are reallocated, the graph is captured again)."""
    model = _model(nkv, 7)
    ids, mask = _prompts(4, lengths)
    for layout in _layouts(monkeypatch):
        eager = model.generate(ids, n, attention_mask=mask)
        graphed = model.generate_graphed(ids, n, attention_mask=mask)
        assert torch.equal(graphed, eager), layout
        if layout == "mfma":
            eager_steps, captures, replays = model.graphs.stats
            assert replays > 0 and captures >= (2 if max(lengths) + n > 544 else 1)


def test_mask_buffer_grows_between_calls_on_one_model(monkeypatch):
    """The static mask buffer of the graphed step is as wide as the stores: prompts of one super-block, then of two (a wider buffer
    at another address, in the graphs that exist), then of one again -- every call equals eager decoding, and on the matrix-pipe
    layout every call captures its step and replays it."""
    model = _model(1, 11)
    small, big = _prompts(7, [20, 9]), _prompts(8, [530, 40])
    for layout in _layouts(monkeypatch):
        for ids, mask in (small, big, small):
            graphed = model.generate_graphed(ids, 6, attention_mask=mask)
            eager_steps, captures, replays = model.graphs.stats or (0, 0, 0)
            assert torch.equal(graphed, model.generate(ids, 6, attention_mask=mask)), (layout, ids.shape)
            if layout == "mfma":
                assert captures >= 1 and replays >= 1, (layout, ids.shape)


# ------------------------------------------------------------------ 4. no change without a pad; the unpadded row
def test_all_ones_mask_changes_nothing(monkeypatch):
    model = _model(1, 8)
    ids1 = torch.randint(0, 320, (2, 45), device="cuda")
    ids2 = torch.randint(0, 320, (2, 23), device="cuda")
    ones1 = torch.ones_like(ids1)
    for layout in _layouts(monkeypatch):
        assert torch.equal(model.generate(ids1, 8), model.generate(ids1, 8, attention_mask=ones1)), layout
        assert torch.equal(model.generate_graphed(ids1, 8), model.generate_graphed(ids1, 8, attention_mask=ones1)), layout
        _, pa = model(ids1)
        _, pb = model(ids1, padding_mask=ones1)
        ga = model.generate(ids2, 6, past_key_values=pa)
        gb = model.generate(ids2, 6, past_key_values=pb, attention_mask=torch.ones((2, 68), dtype=torch.long, device="cuda"))
        assert torch.equal(ga, gb), layout
        for x, y in zip(pa, pb):
            if layout == "mfma":
                _assert_same_state(x.layer, y.layer)
            else:
                ta, tb = x.layer.as_tuple(), y.layer.as_tuple()
                assert all((s is None and t is None) or same_bits(s, t) for s, t in zip(ta[:8], tb[:8])) and ta[8] == tb[8]


@pytest.mark.parametrize("nkv", [1, 4])
def test_unpadded_row_matches_alone(nkv):
    """Row 0 (no pad) of a padded batch against the same prompt run alone.  Through the same masked prompt pass (HF's 4D mask, all
    causal for this row) it is bit-identical, logits of every pass.  Without a mask the prompt pass is SDPA with is_causal=True,
    which rounds differently from SDPA with attn_mask (about an ulp): the prompt logits stay within 1e-2 of their rms, and the
    decode steps, which quantise keys and values that differ by that rounding into 2-bit codes, within 5e-2 (measured: at most
    2.5e-2; a batch of one and a batch of three give bit-identical rows without a mask, so the dense GEMMs play no part here)."""
    model = _model(nkv, 9)
    ids, mask = _prompts(5, [47, 40, 7])
    toks = model.generate(ids, 6, attention_mask=mask)[:, ids.shape[1]:]
    batch, _ = _model_steps(model, ids, mask, toks)
    ref_toks, masked = _compose_generate(model, ids[:1], torch.ones_like(mask[:1]), 6, [None, None])
    assert torch.equal(ref_toks, toks[:1])
    for a, b in zip(batch, masked):
        assert same_bits(a[:1], b)
    alone, _ = _model_steps(model, ids[:1], mask[:1], toks[:1])
    for s, (a, b) in enumerate(zip(batch, alone)):
        ref = b[0].float()
        rms = ref.pow(2).mean().sqrt().item()
        assert (a[0].float() - ref).abs().max().item() <= (1e-2 if s == 0 else 5e-2) * rms, s


def test_eos_rows_emit_pad_and_stop():
    model = _model(1, 10)
    ids, mask = _prompts(6, [20, 13])
    free = model.generate(ids, 12, attention_mask=mask)[:, ids.shape[1]:]
    eos = int(free[0, 2])                                   # row 0 produces it at step 2 (or earlier)
    gen = model.generate(ids, 12, attention_mask=mask, eos_token_id=eos, pad_token_id=319)[:, ids.shape[1]:]
    for b in range(2):
        hit = (free[b] == eos).nonzero()
        stop = int(hit[0]) if len(hit) else None
        got = gen[b].tolist()
        if stop is None:
            assert got == free[b, : len(got)].tolist()
        else:
            assert got[: stop + 1] == free[b, : stop + 1].tolist() and all(t == 319 for t in got[stop + 1:])
    finished = [int((free[b] == eos).nonzero()[0]) if (free[b] == eos).any() else 12 for b in range(2)]
    assert gen.shape[1] == min(12, max(finished) + 1)
