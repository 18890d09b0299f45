"""GPU: query groups padded to a ratio the matrix-pipe layout serves -- a KiviLayerCacheMF built with
nh_kv * Rp query heads, fed q with Rp - R zero heads per kv head by kivi_qk_rope.

1. Inertness: a decode step (one-launch row form, two-launch form) and an extend of Q = 5 from clones of one cache, once with zero
   pad heads and once with the pad heads overwritten by random finite queries: the real heads' outputs and the whole cache (9-tuple,
   range words) are bit-identical -- nothing couples the heads of a group.
2. Parity: ratios 2, 3, 5, 6, 7 at 2 bits and 2, 3 at 4 bits -- a 70-token prompt (two packed groups + 6 residual tokens), 40 decode
   steps across a K flush, and one case from 500 across the 512-token super-block -- against tests/torch_ref64.decode_step at the
   bars tests/test_mfma_gpu.py holds ratios 4 and 8 to: the rows the softmax consumes within gemv_close(rtol=1e-3, ulps=1), the
   output within gemv_close(rtol=3e-3, ulps=1) end to end; the 9-tuple bit-identical to a hook-state KiviLayerCache fed the same
   keys and values.
3. One case each through the model: a left-padded batch with decode_lead=True, a checkpoint / restore_ round trip, an admit_ into a
   living padded cache."""
import pytest
import torch

import tiny_qk_models as M
import torch_ref64 as T64
from helpers import gemv_close, make_kv, same_bits
from test_extend_gpu import _assert_same_state

pytestmark = pytest.mark.gpu
D, G, RES, B, NKV = 128, 32, 32, 2, 2


def _padded_cache(bits, ratio, T0):
    from kivi_amd.attention import KiviConfig, KiviLayerCacheMF
    from kivi_amd.cache_mf import padded_heads
    cfg = KiviConfig(bits, bits, G, RES)
    nhp = padded_heads(cfg, D, NKV * ratio, NKV)
    assert nhp is not None and nhp > NKV * ratio
    k0, v0 = make_kv(1, B, NKV, T0, D).cuda(), make_kv(2, B, NKV, T0, D).cuda()
    layer = KiviLayerCacheMF(cfg, B, NKV, D, T0 + 8, "cuda", num_heads=nhp)          # small capacity: the cache must grow
    layer.prefill(k0, v0)
    return cfg, layer, nhp // NKV, k0, v0


def _pad(q, ratio, rp, fill=None):
    """(B, nh_kv * R, Q, D) -> (B, nh_kv * Rp, Q, D) as kivi_qk_rope lays it out; `fill`: what the pad heads hold (default zeros)."""
    Q = q.shape[2]
    out = torch.zeros((B, NKV, rp, Q, D), dtype=q.dtype, device=q.device) if fill is None else fill.clone().view(B, NKV, rp, Q, D)
    out[:, :, :ratio] = q.view(B, NKV, ratio, Q, D)
    return out.view(B, NKV * rp, Q, D)


def _real(x, ratio, rp):
    return x.view(B, NKV, rp, *x.shape[2:])[:, :, :ratio].reshape(B, NKV * ratio, *x.shape[2:])


# ------------------------------------------------------------------ 1. inertness
@pytest.mark.parametrize("form", ["row", "split", "extend"])
@pytest.mark.parametrize("bits,ratio", [(2, 2), (2, 3), (2, 5), (2, 7), (4, 3)])
def test_pad_heads_are_inert(bits, ratio, form):
    from kivi_amd import _lib
    from kivi_amd.attention import kivi_attention_decode, kivi_attention_extend
    _, zero, rp, _, _ = _padded_cache(bits, ratio, 70)
    if form != "extend":
        zero.flags = _lib.GQA_FORCE_ROW if form == "row" else _lib.GQA_FORCE_SPLIT
    noisy = zero.clone()
    noisy.flags = zero.flags
    Q = 5 if form == "extend" else 1
    for s in range(1 if form == "extend" else 4):
        q = make_kv(100 + s, B, NKV * ratio, Q, D).cuda()
        kn, vn = make_kv(200 + s, B, NKV, Q, D).cuda(), make_kv(300 + s, B, NKV, Q, D).cuda()
        fill = (make_kv(400 + s, B, NKV * rp, Q, D).float() * 5).half().cuda()
        qz, qn = _pad(q, ratio, rp), _pad(q, ratio, rp, fill)
        assert torch.isfinite(qn).all() and not same_bits(qz, qn)
        step = kivi_attention_extend if form == "extend" else kivi_attention_decode
        a, b = step(qz, kn, vn, zero), step(qn, kn, vn, noisy)
        assert same_bits(_real(a, ratio, rp), _real(b, ratio, rp)), (form, s)
        assert torch.isfinite(b).all()
        _assert_same_state(zero, noisy)


# ------------------------------------------------------------------ 2. parity
PARITY = [(2, 2, 70), (2, 3, 70), (2, 5, 70), (2, 6, 70), (2, 7, 70), (4, 2, 70), (4, 3, 70), (2, 7, 500)]


@pytest.mark.parametrize("form", ["row", "split"])
@pytest.mark.parametrize("bits,ratio,T0", PARITY)
def test_padded_decode_matches_the_fp64_reference(bits, ratio, T0, form):
    from kivi_amd import _lib
    from kivi_amd.attention import KiviLayerCache, kivi_attention_decode
    cfg, layer, rp, k0, v0 = _padded_cache(bits, ratio, T0)
    layer.flags = (_lib.GQA_FORCE_ROW | _lib.GQA_DUMP_SCORES) if form == "row" else _lib.GQA_FORCE_SPLIT
    hook = KiviLayerCache(cfg, B, NKV, D, T0 + 8, "cuda")
    hook.prefill(k0, v0)
    past = T64.prefill_cache(k0, v0, bits, bits, G, RES)
    for x, y in zip(layer.as_tuple()[:8], hook.as_tuple()[:8]):
        assert (x is None and y is None) or same_bits(x, y)
    nh, flushed = NKV * ratio, False
    for s in range(40):
        q = make_kv(100 + s, B, nh, 1, D).cuda()
        kn, vn = make_kv(200 + s, B, NKV, 1, D).cuda(), make_kv(300 + s, B, NKV, 1, D).cuda()
        n = T0 + s + 1
        layer._native and layer._native[4][0].fill_(float("nan"))            # (a stale row must not pass for this step's)
        before = layer.k_quant_len
        out = _real(kivi_attention_decode(_pad(q, ratio, rp), kn, vn, layer), ratio, rp)
        flushed |= layer.k_quant_len > before
        kivi_attention_decode(q, kn, vn, hook)
        ref, past, pre = T64.decode_step(q, kn, vn, past, bits, bits, G, RES)
        x_gpu = _real(layer._native[4][0][:B, : NKV * rp, :, :n], ratio, rp)  # the rows the softmax consumed (dumped / the split form's)
        ok, ra = gemv_close(x_gpu, pre, rtol=1e-3, ulps=1)
        assert ok, ("scores", s, ra)
        ok, rb = gemv_close(out, ref, rtol=3e-3, ulps=1)
        assert ok, ("output", s, rb)
    assert flushed and layer.kv_seq_len == T0 + 40
    if T0 == 500:
        assert layer.n_sb >= 2 and layer.k_quant_len == 512                                  # K has filled the first super-block
    ta, tb = layer.as_tuple(), hook.as_tuple()
    for x, y, z in zip(ta[:8], tb[:8], past[:8]):
        assert (x is None and y is None) or (same_bits(x, y) and same_bits(x, z))
    assert ta[8] == tb[8] == past[8]


# ------------------------------------------------------------------ 3. through the model
def _models(ratio, seed, **kw):
    from kivi_amd.llama import Qwen2ForCausalLM_KIVI
    return M.build(Qwen2ForCausalLM_KIVI, ratio, seed, qk_kernel=True, **kw)


def _assert_padded(pasts, heads):
    from kivi_amd.attention import KiviLayerCacheMF
    for p in pasts:
        assert isinstance(p.layer, KiviLayerCacheMF) and p.layer.nh == heads


def test_left_padded_batch_with_decode_lead():
    """decode_lead=True on a padded ratio-7 model: every decode step hands the 16-head caches the rows' leads; against the same
    weights without the option the prompt pass is the same and the decode logits stay inside the band tests/test_padding_gpu.py:266
    gives two roundings of one prompt (5e-2 of the rms); graphed decode equals eager token for token."""
    from kivi_amd.llama import Qwen2ForCausalLM_KIVI, left_pad
    on = _models(7, 21, decode_lead=True)
    off = M.twin(Qwen2ForCausalLM_KIVI, on, 7, qk_kernel=True)
    g = torch.Generator().manual_seed(4)
    ids, mask = left_pad([torch.randint(1, M.VOCAB, (n,), generator=g) for n in (70, 9)], pad_token_id=0, device="cuda")
    leads = []
    la, pa = on(ids, padding_mask=mask)
    lb, pb = off(ids, padding_mask=mask)
    _assert_padded(pa, 16)
    assert same_bits(la, lb)
    for p in pa:
        step = p.layer.decode_step
        p.layer.decode_step = lambda *a, _step=step, **k: leads.append(k.get("lead")) or _step(*a, **k)
    m = mask
    for s in range(6):
        tok = lb.argmax(-1)
        m = torch.cat([m, torch.ones_like(m[:, :1])], 1)
        la, pa = on(tok, pa, padding_mask=m)
        lb, pb = off(tok, pb, padding_mask=m)
        rms = lb.float().pow(2).mean().sqrt().item()
        assert (la.float() - lb.float()).abs().max().item() <= 5e-2 * rms, s
    assert len(leads) == 12 and all(ld is not None and ld.tolist() == [0, 61] for ld in leads)
    assert torch.equal(on.generate(ids, 8, attention_mask=mask), on.generate_graphed(ids, 8, attention_mask=mask))
    on.release_graphs()


def test_checkpoint_restore_round_trip():
    model = _models(5, 22, max_cache_len=256)
    ids = M.prompts(5, B, 70)
    logits, past = model(ids)
    _assert_padded(past, 16)
    toks = [logits.argmax(-1)]
    for s in range(3):
        logits, past = model(toks[-1], past)
        toks.append(logits.argmax(-1))
    ck = model.checkpoint(past)
    kept = [p.layer.clone() for p in past]
    want = []
    t = toks[-1]
    for s in range(30):                               # across the K flush at 96
        logits, past = model(t, past)
        want.append(logits)
        t = logits.argmax(-1)
    past = model.restore_(past, ck)
    for p, k in zip(past, kept):
        _assert_same_state(p.layer, k)
    t = toks[-1]
    for s in range(30):
        logits, past = model(t, past)
        assert same_bits(logits, want[s]), s
        t = logits.argmax(-1)


def test_admit_into_a_living_padded_cache():
    """Row 1 of a living batch is taken over by a new prompt left-padded to the caches' length.  Right after the admission the row's
    cache is, bit for bit, the cache the prompt makes in a batch of its own, and row 0's is what it was; both rows then decode
    across a K flush inside the band tests/test_padding_gpu.py:266 gives a row of a padded batch against the same row alone."""
    from kivi_amd.llama import left_pad
    model = _models(7, 23)
    L = 70
    g = torch.Generator().manual_seed(6)
    ids = M.prompts(7, B, L)
    new, new_mask = left_pad([torch.randint(1, M.VOCAB, (40,), generator=g)], pad_token_id=0, device="cuda", length=L)
    logits, past = model(ids)
    _assert_padded(past, 16)
    before = [p.layer.clone().as_tuple() for p in past]
    alone_logits, alone = model(ids[:1])
    fresh_logits, fresh = model(new, padding_mask=new_mask)
    got, past = model.admit_(past, [1], new, new_mask)
    assert same_bits(got, fresh_logits)
    _assert_padded(past, 16)
    for p, f, c in zip(past, fresh, before):
        for x, y, z in zip(p.layer.as_tuple()[:8], f.layer.as_tuple()[:8], c[:8]):
            assert (x is None and y is None) or (same_bits(x[1:], y) and same_bits(x[:1], z[:1]))
    mask = torch.cat([torch.ones_like(new_mask), new_mask], 0)
    tok = torch.cat([logits[:1].argmax(-1), got.argmax(-1)], 0)
    for s in range(30):
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        logits, past = model(tok, past, padding_mask=mask)
        alone_logits, alone = model(tok[:1], alone)
        fresh_logits, fresh = model(tok[1:], fresh, padding_mask=mask[1:])
        assert torch.isfinite(logits).all()
        for a, b in ((logits[:1], alone_logits), (logits[1:], fresh_logits)):
            rms = b.float().pow(2).mean().sqrt().item()
            assert (a.float() - b.float()).abs().max().item() <= 5e-2 * rms, s
        tok = logits.argmax(-1)
    assert past[0].layer.k_quant_len == 96
